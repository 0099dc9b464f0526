"""The per-pixel value bar (tests/value_bar.py) shown to bite, on the CPU with the oracle
alone: on every input set of tests/test_gpu_path_values.py and both kernels

* a straightforward float32 NumPy evaluation (absolute-frame offsets, every operation
  rounded to fp32, fp64 accumulation) passes ``assert_terms_close``;
* the oracle map with ONE class of particles scaled by 1 + 1e-3 is rejected, for each
  class in turn (the gathered, wide and wave-walked classes included);
* the global-peak bar of tests/test_gpu_parity.py accepts the wide class scaled by 1.2 on
  ``test_wide_particles``' own inputs -- the gap the per-pixel bar closes.

At the offset windows (value_bar.WINDOWS: zoom maps far from the origin, the same bar)

* a float32 evaluation in LOCAL frames -- the device's arithmetic -- passes at every window;
* the absolute-frame evaluation fl32(u) - fl32(X) is rejected wherever u or X is off the
  fp32 lattice: the raw fp64 set on ``box`` and ``far_negative``, any set on ``box_offgrid``;
* the edge forms' dead zone taken from the local frames' bound passes, and
  taken from max |corner| for the wide class alone is rejected;
* every class scaled by 1 + 1e-3 is rejected on ``box``.

At the pass seams (value_bar.STRIPS and the pass / ratio rules, for tests/test_gpu_seams.py)

* the local-frame evaluation reproduces the oracle's neighbour counts on both strips and
  passes the unchanged bar; the absolute-frame one is rejected on ``strip_offgrid``;
* every class scaled by 1 + 1e-3 is rejected under the pass rule's widest bar as well;
* the mixed set evaluated in batches, re-rounded to fp32 between them, passes with the rule;
* an fp32 quotient passes the ratio rule, whose excluded share stays within its cap;
* the seam set is what the GPU cases rely on, asserted from the reference alone.
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


# ------------------------------------------------- offset windows (value_bar.WINDOWS)
def _window_evaluations(oracle, kernel, window):
    """The local-frame fp32 evaluation of the window's mixed set (amplitudes a): plain, with
    every record's dead zone from mgl, and with the wide class's from mg = max |corner|."""
    def make():
        s = vb.mixed_set(oracle, kernel, window)
        ext = vb.window_ext(window)
        mg, mgl = vb.frame_bounds(vb.SIZE2D, ext)
        tau_l = vb.dead_zone_tau(mgl, s["h"])
        wide = s["cls"] == s["names"].index("h40-120")
        tau_g = np.where(wide, vb.dead_zone_tau(mg, s["h"]), tau_l)
        assert np.all(tau_g[wide] > 0)  # the dead zone is on (tau < 2^-4) for every wide h
        (plain, dead_l, dead_g), cnt = vb.eval_f32_local_2d(s, s["a"], kernel, vb.SIZE2D, ext,
                                                           taus=(None, tau_l, tau_g))
        return dict(plain=plain, dead_l=dead_l, dead_g=dead_g, cnt=cnt)
    return vb._cached(("window_evals", kernel, window), make)


@pytest.mark.parametrize("kernel", vb.KERNELS)
@pytest.mark.parametrize("window", vb.WINDOW_NAMES)
def test_window_local_frame_passes(oracle, kernel, window):
    """The device's arithmetic (local frames) stays inside the bar at every window: the
    inputs chosen keep a correct implementation inside a bar that has no |corner| term."""
    ref = vb.reference2d(oracle, kernel, window=window)
    ev = _window_evaluations(oracle, kernel, window)
    assert np.array_equal(ev["cnt"], ref["cnt"])
    worst = vb.assert_terms_close(ev["plain"], ref["r1"], ref["E1"], ref["by_class1"])
    assert worst > 0.0
    print(f"VALUE_BAR cpu local frame {window} {kernel}: worst err/E = {worst:.3f}")


@pytest.mark.parametrize("kernel", vb.KERNELS)
@pytest.mark.parametrize("window,raw", [("box", True), ("box_offgrid", False),
                                        ("far_negative", True)],
                         ids=["box", "box_offgrid", "far_negative"])
def test_window_absolute_frame_is_rejected(oracle, kernel, window, raw):
    """eval_f32_2d forms fl32(u) - fl32(X) in absolute coordinates; the bar must catch it
    wherever that arithmetic loses something, i.e. wherever u or X is off the fp32 lattice.

    ``box`` and ``far_negative`` (corners exact in fp32) with the RAW fp64 set, the inputs of
    the fp64 entry points: fl32(u) moves a position by up to half the lattice step, 1/16
    pitch near 67 and 1/8 pitch near -1000, where a local frame formed from the fp64 value
    keeps it -- the local-frame evaluation of the same raw set passes the same bar (with
    F64_INPUT_ULPS for the rounding of h and a, which both evaluations do).
    ``box_offgrid`` with the fp32 set: the positions are exact, the corners X round to the
    lattice near 67 (2^-17, 1/8 pitch) and are off by up to 1/16 pitch.

    (The fp32 set on ``box`` cannot show this: the pitch 2^-14 is a whole multiple of the
    lattice 2^-17 and x_min lies on it, so every corner and every fp32 position is exact and
    the absolute frame carries no error there at all.)"""
    s = vb.mixed_set(oracle, kernel, window, raw)
    ref = vb.reference2d(oracle, kernel, window=window, raw=raw)
    ext = vb.window_ext(window)
    (loc,), cnt = vb.eval_f32_local_2d(s, s["a"], kernel, vb.SIZE2D, ext)
    assert np.array_equal(cnt, ref["cnt"])
    worst = vb.assert_terms_close(loc, ref["r1"], ref["E1"], ref["by_class1"])
    print(f"VALUE_BAR cpu local frame {window} raw={raw} {kernel}: worst err/E = {worst:.3f}")
    g, cnt = vb.eval_f32_2d(s, s["a"], kernel, vb.SIZE2D, ext)
    assert np.array_equal(cnt, ref["cnt"])
    with pytest.raises(AssertionError, match="worst err/E") as bad:
        vb.assert_terms_close(g, ref["r1"], ref["E1"], ref["by_class1"])
    print(f"VALUE_BAR cpu absolute frame {window} raw={raw} {kernel}: rejected, "
          + str(bad.value).split(" at pixel")[0])


@pytest.mark.parametrize("kernel", vb.KERNELS)
@pytest.mark.parametrize("window", vb.WINDOW_NAMES)
def test_window_dead_zone_frame(oracle, kernel, window):
    """The edge forms' dead zone tau = band / (2 thr) + 2^-20: taken from the local frames'
    bound mgl (128 pitches) it stays inside the bar; taken from mg = max |corner| for the
    wide class alone -- what a wide path that keeps prep_record's absolute-frame band
    evaluates -- it is rejected, and the report names that class."""
    ref = vb.reference2d(oracle, kernel, window=window)
    ev = _window_evaluations(oracle, kernel, window)
    worst = vb.assert_terms_close(ev["dead_l"], ref["r1"], ref["E1"], ref["by_class1"])
    print(f"VALUE_BAR cpu dead zone mgl {window} {kernel}: worst err/E = {worst:.3f}")
    with pytest.raises(AssertionError, match="worst err/E.*dominated by class h40-120"):
        vb.assert_terms_close(ev["dead_g"], ref["r1"], ref["E1"], ref["by_class1"])


@pytest.mark.parametrize("kernel", vb.KERNELS)
def test_window_scaled_class_is_rejected(oracle, kernel):
    s = vb.mixed_set(oracle, kernel, "box")
    ref = vb.reference2d(oracle, kernel, window="box")
    for k, name in enumerate(s["names"]):
        bad = ref["r1"] + 1e-3 * vb.class_map2d(oracle, s, s["a"], kernel, k,
                                                ext=vb.window_ext("box"))
        with pytest.raises(AssertionError, match="worst err/E"):
            vb.assert_terms_close(bad, ref["r1"], ref["E1"], ref["by_class1"])
        with pytest.raises(AssertionError, match="worst err/E"):  # the fixed-point bar too
            vb.assert_terms_close(bad, ref["r1"], ref["E1"], ref["by_class1"], floor=ref["F1"])


def test_window_sets_keep_their_local_positions(oracle):
    """The windows' sets are the default set's draws: the same classes, h in pitches and
    equal-peak amplitudes, fp32-representable; the raw set is not rounded."""
    base = vb.mixed_set(oracle, "cubic")
    for window in vb.WINDOW_NAMES:
        ext = vb.window_ext(window)
        pitch = vb.pitch2d(vb.SIZE2D, ext)
        s, raw = vb.mixed_set(oracle, "cubic", window), vb.mixed_set(oracle, "cubic", window, True)
        assert np.array_equal(s["cls"], base["cls"])
        for key in ("u", "v", "h", "a", "a0"):
            assert np.array_equal(s[key], vb.f32(s[key])), key
        assert np.any(raw["u"] != vb.f32(raw["u"])) and np.any(raw["h"] != vb.f32(raw["h"]))
        np.testing.assert_allclose(s["h"] / pitch, base["h"] / vb.PITCH2D, rtol=3e-7)
        lu = (raw["u"] - ext[0]) / ((ext[1] - ext[0]) / 256)
        np.testing.assert_allclose(lu, (base["u"] + 1.0) / vb.PITCH2D, atol=1e-4)  # pitches
        peak = s["a"] * vb.w0(oracle, "cubic", s["h"])
        assert 0.49 < peak.min() and peak.max() < 1.51


def test_window_stamps(oracle):
    """The stamps at every window: reference equals the oracle, the local-frame evaluation
    passes the particle's own term."""
    kernel = "wendland_c2"
    for window in vb.WINDOW_NAMES:
        ext = vb.window_ext(window)
        for path, h_px, *_ in vb.STAMP_PATHS:
            for where in vb.STAMP_POSITIONS:
                u, v, h, a = vb.stamp_particle(oracle, kernel, h_px, where, window)
                assert (u, v, h, a) == tuple(float(vb.f32(t)) for t in (u, v, h, a))
                r, E = vb.stamp_reference(oracle, kernel, u, v, h, a, vb.SIZE2D, ext)
                assert np.count_nonzero(r) > 0, (window, path, where)
                one = dict(u=np.array([u]), v=np.array([v]), h=np.array([h]))
                want, _ = oracle.project_scatter(one["u"], one["v"], one["h"], [a], None,
                                                 vb.SIZE2D, vb.CHUNK, *ext, kernel=kernel)
                assert np.array_equal(r != 0, want != 0)
                np.testing.assert_allclose(r, want, rtol=1e-9, atol=1e-10)
                (g,), _ = vb.eval_f32_local_2d(one, [a], kernel, vb.SIZE2D, ext)
                vb.assert_terms_close(g, r, E)


def test_f64_input_term():
    """F64_INPUT_ULPS bounds the effect of rounding h and a to fp32 on a W(r, h), measured
    on the fp64 kernel itself at the worst roundings (relative 2^-24 each)."""
    q = np.linspace(0.0, 2.0, 4001)
    for kernel in vb.KERNELS:
        h, a = 0.37, 1.3
        w_0 = a * vb.kernel_f64(kernel, np.zeros(1), np.array([h]))[0]
        for sh in (-1.0, 1.0):
            for sa in (-1.0, 1.0):
                hh, aa = h * (1 + sh * vb.U24), a * (1 + sa * vb.U24)
                d = np.abs(aa * vb.kernel_f64(kernel, q * h, hh)
                           - a * vb.kernel_f64(kernel, q * h, h))
                assert d.max() <= vb.F64_INPUT_ULPS * vb.U24 * w_0
                if sh != sa:  # (opposite signs add up at q = 0: the count is not slack)
                    assert d.max() >= 3.9 * vb.U24 * w_0


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


# ------------------------------------------------- pass seams (value_bar.STRIPS, the rules)
# What tests/test_gpu_seams.py relies on, shown on the CPU from the references alone: the
# strip's seam set keeps a correct implementation inside the unchanged bar, the bar still
# bites there and with the pass rule's extra, and the ratio rule holds for an fp32 quotient.
STRIP_PASSES, MIXED_PASSES = 6, 4  # the most passes the GPU cases take on either set


def _strip_evaluations(oracle, kernel, name):
    """The local-frame fp32 evaluation of the strip's two maps and the neighbour counts,
    cropped as the references are."""
    def make():
        s = vb.strip_set(oracle, kernel, name)
        ext = vb.strip_ext(name)
        (g1,), cnt = vb.eval_f32_local_2d(s, s["a"], kernel, vb.STRIP_SIZE, ext)
        (g0,), _ = vb.eval_f32_local_2d(s, s["a0"], kernel, vb.STRIP_SIZE, ext)
        return dict(g0=vb.strip_crop(g0), g1=vb.strip_crop(g1), cnt=vb.strip_crop(cnt))
    return vb._cached(("strip_evals", kernel, name), make)


@pytest.mark.parametrize("kernel", vb.KERNELS)
@pytest.mark.parametrize("name", vb.STRIP_NAMES)
def test_strip_local_frame_passes(oracle, kernel, name):
    ref = vb.strip_reference(oracle, kernel, name)
    ev = _strip_evaluations(oracle, kernel, name)
    assert np.array_equal(ev["cnt"], ref["cnt"])
    w1 = vb.assert_terms_close(ev["g1"], ref["r1"], ref["E1"], ref["by_class1"])
    w0 = vb.assert_terms_close(ev["g0"], ref["r0"], ref["E0"], ref["by_class0"])
    assert min(w0, w1) > 0.0
    print(f"VALUE_BAR cpu local frame {name} {kernel}: worst err/E = {max(w0, w1):.3f}")


@pytest.mark.parametrize("kernel", vb.KERNELS)
def test_strip_absolute_frame_is_rejected(oracle, kernel):
    """On ``strip_offgrid`` the corners X round to the fp32 lattice near 256 (2^-16 .. 2^-15,
    1/16 .. 1/32 of a pitch): fl32(u) - fl32(X) is rejected.  (``strip_grid`` cannot show it:
    every corner k 2^-10 <= 256.5 and every fp32 position is exact.)"""
    name = "strip_offgrid"
    s = vb.strip_set(oracle, kernel, name)
    ref = vb.strip_reference(oracle, kernel, name)
    g, cnt = vb.eval_f32_2d(s, s["a"], kernel, vb.STRIP_SIZE, vb.strip_ext(name))
    assert np.array_equal(vb.strip_crop(cnt), ref["cnt"])
    with pytest.raises(AssertionError, match="worst err/E") as bad:
        vb.assert_terms_close(vb.strip_crop(g), ref["r1"], ref["E1"], ref["by_class1"])
    print(f"VALUE_BAR cpu absolute frame {name} {kernel}: rejected, "
          + str(bad.value).split(" at pixel")[0])


@pytest.mark.parametrize("kernel", vb.KERNELS)
@pytest.mark.parametrize("name", vb.STRIP_NAMES)
def test_strip_scaled_class_is_rejected(oracle, kernel, name):
    """Each class scaled by 1 + 1e-3, under the plain bar and under the pass rule's widest
    (STRIP_PASSES passes, with the fixed-point floor)."""
    s = vb.strip_set(oracle, kernel, name)
    ref = vb.strip_reference(oracle, kernel, name)
    wide = vb.with_passes(ref["E1"], ref["S1"], STRIP_PASSES)
    assert np.all(wide >= ref["E1"]) and np.any(wide > ref["E1"])
    for k, cname in enumerate(s["names"]):
        one = vb.strip_crop(vb.class_map2d(oracle, s, s["a"], kernel, k, vb.STRIP_SIZE,
                                           vb.strip_ext(name)))
        bad = ref["r1"] + 1e-3 * one
        with pytest.raises(AssertionError, match="worst err/E"):
            vb.assert_terms_close(bad, ref["r1"], ref["E1"], ref["by_class1"])
        with pytest.raises(AssertionError, match="worst err/E") as rej:
            vb.assert_terms_close(bad, ref["r1"], wide, ref["by_class1"], floor=ref["F1"])
        print(f"VALUE_BAR cpu scaled {cname} {name} {kernel} P={STRIP_PASSES}: rejected, "
              + str(rej.value).split(" at pixel")[0])


@pytest.mark.parametrize("kernel", vb.KERNELS)
def test_mixed_scaled_class_is_rejected_under_the_pass_rule(oracle, kernel):
    s = vb.mixed_set(oracle, kernel)
    ref = vb.reference2d(oracle, kernel)
    wide = vb.with_passes(ref["E1"], ref["S1"], MIXED_PASSES + 1)  # (+ 1: a caller's accumulate)
    for k, cname in enumerate(s["names"]):
        bad = ref["r1"] + 1e-3 * vb.class_map2d(oracle, s, s["a"], kernel, k)
        with pytest.raises(AssertionError, match="worst err/E"):
            vb.assert_terms_close(bad, ref["r1"], wide, ref["by_class1"], floor=ref["F1"])


@pytest.mark.parametrize("kernel", vb.KERNELS)
def test_pass_rule_is_the_bar_with_extra_ulps(oracle, kernel):
    """with_passes(E, S, P) is bar2d with extra_ulps = 3 (P - 1): term_bound is linear."""
    s = vb.mixed_set(oracle, kernel)
    ref = vb.reference2d(oracle, kernel)
    assert vb.pass_ulps(1) == 0.0 and vb.pass_ulps(4) == 9.0
    E, _ = vb.bar2d(oracle, s, s["a"], kernel, extra_ulps=vb.pass_ulps(MIXED_PASSES))
    np.testing.assert_allclose(vb.with_passes(ref["E1"], ref["S1"], MIXED_PASSES), E, rtol=1e-12)
    assert np.array_equal(ref["S1"] == 0, ref["E1"] == 0)


@pytest.mark.parametrize("kernel", vb.KERNELS)
def test_mixed_set_in_batches_passes(oracle, kernel):
    """The mixed set evaluated in MIXED_PASSES array-order batches, the map re-rounded to
    fp32 after each (what accumulating passes store): inside the pass rule's bar."""
    s = vb.mixed_set(oracle, kernel)
    ref = vb.reference2d(oracle, kernel)
    n = s["h"].size
    edges = np.linspace(0, n, MIXED_PASSES + 1).astype(int)
    g = np.zeros(vb.SIZE2D)
    for a, b in zip(edges[:-1], edges[1:]):
        part = {k: s[k][a:b] for k in ("u", "v", "h")}
        gb, _ = vb.eval_f32_2d(part, s["a"][a:b], kernel)
        g = vb.f32(g + gb)
    E = vb.with_passes(ref["E1"], ref["S1"], MIXED_PASSES)
    worst = vb.assert_terms_close(g, ref["r1"], E, ref["by_class1"])
    assert worst > 0.0
    print(f"VALUE_BAR cpu {MIXED_PASSES} batches {kernel}: worst err/E = {worst:.3f}")


def _quotient_f32(g0, g1):
    g0, g1 = np.asarray(g0, np.float32), np.asarray(g1, np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(g1 != 0, g0 / g1, np.float32(0.0)).astype(np.float64)


@pytest.mark.parametrize("kernel", vb.KERNELS)
@pytest.mark.parametrize("name", vb.STRIP_NAMES)
def test_ratio_rule_strip(oracle, kernel, name):
    """The fp32 quotient of the fp32-stored local-frame maps passes the ratio rule; the
    pixels it leaves out are within the cap; a quotient off by 1e-3 is rejected."""
    ref = vb.strip_reference(oracle, kernel, name)
    ev = _strip_evaluations(oracle, kernel, name)
    q = _quotient_f32(ev["g0"], ev["g1"])
    share = vb.ratio_tail_share(ref["r1"], ref["E1"])
    assert 0.0 < share <= vb.RATIO_TAIL_SHARE
    worst = vb.assert_ratio_close(q, ref["r0"], ref["r1"], ref["E0"], ref["E1"])
    assert worst > 0.0
    print(f"VALUE_BAR cpu ratio {name} {kernel}: worst err/E = {worst:.3f}, "
          f"tail share {share:.2%}")
    wide0, wide1 = (vb.with_passes(ref["E" + k], ref["S" + k], STRIP_PASSES) for k in "01")
    assert vb.ratio_tail_share(ref["r1"], wide1) <= vb.RATIO_TAIL_SHARE
    with pytest.raises(AssertionError, match="worst err/E"):
        vb.assert_ratio_close(q * (1 + 1e-3), ref["r0"], ref["r1"], wide0, wide1)
    with pytest.raises(AssertionError, match="are not 0"):
        vb.assert_ratio_close(q + (ref["r1"] == 0), ref["r0"], ref["r1"], ref["E0"], ref["E1"])


@pytest.mark.parametrize("kernel", vb.KERNELS)
def test_ratio_rule_mixed_set(oracle, kernel):
    """On the 256^2 mixed set (the batched ratio cases): the tail share, with the pass
    rule's widest bar, and the oracle's own quotient under the rule."""
    ref = vb.reference2d(oracle, kernel)
    wide0, wide1 = (vb.with_passes(ref["E" + k], ref["S" + k], MIXED_PASSES) for k in "01")
    assert vb.ratio_tail_share(ref["r1"], wide1) <= vb.RATIO_TAIL_SHARE
    q = _quotient_f32(ref["r0"], ref["r1"])
    vb.assert_ratio_close(q, ref["r0"], ref["r1"], ref["E0"], ref["E1"])
    with pytest.raises(AssertionError, match="worst err/E"):
        vb.assert_ratio_close(q * (1 + 1e-3), ref["r0"], ref["r1"], wide0, wide1)


@pytest.mark.parametrize("raw", [False, True], ids=["fp32", "raw"])
@pytest.mark.parametrize("kernel", vb.KERNELS)
@pytest.mark.parametrize("name", vb.STRIP_NAMES)
def test_strip_set_is_what_the_gpu_cases_rely_on(oracle, kernel, name, raw):
    s = vb.strip_set(oracle, kernel, name, raw)
    ext = vb.strip_ext(name)
    nx, ny = vb.STRIP_SIZE
    seam, tile = vb.STRIP_SEAM, 64
    assert (nx + tile - 1) // tile == 4104 and (ny + tile - 1) // tile == 1 and seam == 4096 * tile
    psx, psy = (ext[1] - ext[0]) / nx, (ext[3] - ext[2]) / nx
    assert abs(psx / psy - 1.0) < 1e-12  # square pixels
    for key in ("u", "v", "h", "a", "a0"):
        assert np.array_equal(s[key], vb.f32(s[key])) != raw, key
    peak = s["a"] * vb.w0(oracle, kernel, s["h"])
    assert 0.49 < peak.min() and peak.max() < 1.51
    # every class has particles whose pixels lie on both sides of the seam (the fp64 test
    # on rows seam - 1 and seam, the nearest column)
    Y = ext[2] + np.arange(ny) * psy
    dy2 = np.min((s["v"][:, None] - Y[None, :]) ** 2, axis=1)
    below = (s["u"] - (ext[0] + (seam - 1) * psx)) ** 2 + dy2 < (2 * s["h"]) ** 2
    above = (s["u"] - (ext[0] + seam * psx)) ** 2 + dy2 < (2 * s["h"]) ** 2
    for k, cname in enumerate(s["names"]):
        assert np.count_nonzero(below & above & (s["cls"] == k)) >= 1, cname
    # the wide class: > STRIP_WIDE_TILES tiles in each window, the other classes never
    lo = np.floor((s["u"] - 2 * s["h"] - ext[0]) / psx).astype(int) + 1  # first / last row met
    hi = np.ceil((s["u"] + 2 * s["h"] - ext[0]) / psx).astype(int) - 1
    assert lo.min() >= vb.STRIP_LO + tile
    t0 = seam // tile - np.minimum(lo, seam) // tile          # tiles below the seam
    t1 = np.minimum(hi, nx - 1) // tile + 1 - seam // tile    # tiles from the seam on
    wide = s["cls"] == s["names"].index(vb.STRIP_WIDE[0])
    limit = int(vb.STRIP_WIDE_TILES)
    assert np.count_nonzero(wide & (t0 > limit) & (t1 > limit)) >= 8
    assert np.all((np.maximum(hi, lo) // tile - lo // tile + 1)[~wide] <= limit)
    # both windows hold pixels next to the seam
    ref = vb.strip_reference(oracle, kernel, name, raw)
    k = seam - vb.STRIP_LO
    for m in (ref["r0"], ref["r1"], ref["cnt"]):
        assert m[k - 1].any() and m[k].any()
    assert ref["cnt"].shape == (nx - vb.STRIP_LO, ny)
