"""The per-pixel value bar (tests/value_bar.py) shown to bite, on the CPU with the oracle
alone: on every input set of tests/test_gpu_path_values.py and both kernels

* a straightforward float32 NumPy evaluation (absolute-frame offsets, every operation
  rounded to fp32, fp64 accumulation) passes ``assert_terms_close``;
* the oracle map with ONE class of particles scaled by 1 + 1e-3 is rejected, for each
  class in turn (the gathered, wide and wave-walked classes included);
* the global-peak bar of tests/test_gpu_parity.py accepts the wide class scaled by 1.2 on
  ``test_wide_particles``' own inputs -- the gap the per-pixel bar closes.
"""
import numpy as np
import pytest

import value_bar as vb


@pytest.mark.parametrize("kernel", vb.KERNELS)
@pytest.mark.parametrize("size", [vb.SIZE2D, vb.SIZE2D_NONSQUARE], ids=["256x256", "192x256"])
def test_f32_evaluation_passes_2d(oracle, kernel, size):
    s = vb.mixed_set(oracle, kernel)
    ref = vb.reference2d(oracle, kernel, size)
    for a, r, E, by_class in ((s["a"], ref["r1"], ref["E1"], ref["by_class1"]),
                              (s["a0"], ref["r0"], ref["E0"], ref["by_class0"])):
        g, cnt = vb.eval_f32_2d(s, a, kernel, size)
        want, _ = oracle.project_scatter(s["u"], s["v"], s["h"], np.ones(a.size), None, size,
                                         vb.CHUNK, *vb.EXT2D, kernel="indicator")
        assert np.array_equal(cnt, want)  # the evaluation sums over the exact neighbour sets
        worst = vb.assert_terms_close(g, r, E, by_class)
        assert worst > 0.0  # it is an fp32 evaluation, not the oracle again
        # the fixed-point term is small beside the bar wherever the bar is not 0
        assert vb.assert_terms_close(g, r, E, by_class, floor=ref["F1"]) <= worst


@pytest.mark.parametrize("kernel", vb.KERNELS)
def test_scaled_class_is_rejected_2d(oracle, kernel):
    s = vb.mixed_set(oracle, kernel)
    ref = vb.reference2d(oracle, kernel)
    for k, name in enumerate(s["names"]):
        bad = ref["r1"] + 1e-3 * vb.class_map2d(oracle, s, s["a"], kernel, k)
        with pytest.raises(AssertionError, match="worst err/E"):
            vb.assert_terms_close(bad, ref["r1"], ref["E1"], ref["by_class1"])
        with pytest.raises(AssertionError, match="worst err/E"):  # the fixed-point bar too
            vb.assert_terms_close(bad, ref["r1"], ref["E1"], ref["by_class1"], floor=ref["F1"])


@pytest.mark.parametrize("kernel", vb.KERNELS)
def test_f32_evaluation_passes_and_scaled_class_is_rejected_cube(oracle, kernel):
    s = vb.cube_set(oracle, kernel)
    ref = vb.reference3d(oracle, kernel)
    g, cnt = vb.eval_f32_3d(s, kernel)
    want = oracle.project3d(s["x"], s["y"], s["z"], s["h"], np.ones(s["h"].size), vb.SIZE3D,
                            vb.EXT3D, kernel="indicator")
    assert np.array_equal(cnt, want)
    assert vb.assert_terms_close(g, ref["r"], ref["E"], ref["by_class"]) > 0.0
    for k, name in enumerate(s["names"]):
        bad = ref["r"] + 1e-3 * vb.class_map3d(oracle, s, kernel, k)
        with pytest.raises(AssertionError, match="worst err/E"):
            vb.assert_terms_close(bad, ref["r"], ref["E"], ref["by_class"])


@pytest.mark.parametrize("kernel", vb.KERNELS)
def test_stamps(oracle, kernel):
    """Every stamp: the NumPy reference equals the oracle, the fp32 evaluation passes the
    particle's own term, a 1e-3 error does not wherever the stamp shows its core."""
    for path, h_px, *_ in vb.STAMP_PATHS:
        for where in vb.STAMP_POSITIONS:
            u, v, h, a = vb.stamp_particle(oracle, kernel, h_px, where)
            r, E = vb.stamp_reference(oracle, kernel, u, v, h, a)
            assert np.count_nonzero(r) > 0, (path, where)
            one = dict(u=np.array([u]), v=np.array([v]), h=np.array([h]))
            want, _ = oracle.project_scatter(one["u"], one["v"], one["h"], [a], None, vb.SIZE2D,
                                             vb.CHUNK, *vb.EXT2D, kernel=kernel)
            assert np.array_equal(r != 0, want != 0)
            np.testing.assert_allclose(r, want, rtol=1e-12, atol=1e-13)  # a W(0) = 1.25
            g, _ = vb.eval_f32_2d(one, [a], kernel)
            vb.assert_terms_close(g, r, E)
            if where != "outside":  # (there a small disc shows only its tail, W < 0.1 W(0))
                with pytest.raises(AssertionError, match="worst err/E"):
                    vb.assert_terms_close(r * (1 + 1e-3), r, E)


def test_report_names_pixel_and_class(oracle):
    s = vb.mixed_set(oracle, "cubic")
    ref = vb.reference2d(oracle, "cubic")
    k = s["names"].index("h40-120")
    bad = ref["r1"] + 1e-3 * vb.class_map2d(oracle, s, s["a"], "cubic", k)
    with pytest.raises(AssertionError, match=r"at pixel \(\d+, \d+\).*dominated by class"):
        vb.assert_terms_close(bad, ref["r1"], ref["E1"], ref["by_class1"])
    zero = np.zeros((4, 4))
    with pytest.raises(AssertionError, match="are not 0"):
        vb.assert_terms_close(np.full_like(zero, 1e-30), zero, zero)
    assert vb.assert_terms_close(zero, zero, zero) == 0.0


def test_global_peak_bar_accepts_a_wrong_wide_class(oracle):
    """test_wide_particles' own inputs (tests/test_gpu_parity.py): its 40 wide particles
    scaled by 1.2 in the oracle map pass ``assert_map_close``.  The per-pixel bar rejects
    the same map."""
    from test_gpu_parity import assert_map_close
    rng = np.random.default_rng(5)
    n = 3000
    pos = np.asarray(rng.uniform(-1, 1, (n, 3)), np.float32).astype(np.float64)
    h = np.asarray(rng.uniform(0.0025, 0.01, n), np.float32).astype(np.float64)
    h[:40] = np.asarray(rng.uniform(0.3, 2.0, 40), np.float32)
    h[40:400] = np.asarray(rng.uniform(0.01, 0.06, 360), np.float32)
    A = np.asarray(rng.uniform(0.5, 1.5, n), np.float32).astype(np.float64)
    G, ext = 2048, (-1.0, 1.0, -1.0, 1.0)
    ref, _ = oracle.project_scatter(pos[:, 0], pos[:, 1], h, A, None, (G, G), 32, *ext)
    wide, _ = oracle.project_scatter(pos[:40, 0], pos[:40, 1], h[:40], A[:40], None, (G, G), 32,
                                     *ext)
    bad = ref + 0.2 * wide
    assert_map_close(bad, ref)  # the gap
    e = vb.term_bound(oracle, "cubic", h, A, vb.pitch2d((G, G), ext))
    E, _ = oracle.project_scatter(pos[:, 0], pos[:, 1], h, e, None, (G, G), 32, *ext,
                                  kernel="indicator")
    with pytest.raises(AssertionError, match="worst err/E"):
        vb.assert_terms_close(bad, ref, E)
