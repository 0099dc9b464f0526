"""Column-integrated kernels (ids 3 and 4) on the GPU: asp_kernel_eval against the closed
forms, the reference's own maps (G13 / G14), the native deposit against the plug-in path,
every deposit path's values under the per-pixel bar of tests/column_ref.py against the
fp64 restatement of the reference, the other entry points, and what the feature is for:
a map whose sum times the pixel area is sum a.

References are computed once per module and shared.  Every case prints its worst err/E
(``pytest -s``).
"""
import numpy as np
import pytest

from conftest import golden

import column_ref as cr
import value_bar as vb
from test_gpu_parity import assert_map_close, g3
from test_gpu_path_values import THRESHOLDS, _dev, _host, _knobs

pytestmark = pytest.mark.gpu

NATIVE = {"cubic_column": "cubic_spline_column_kernel",
          "wendland_c2_column": "wendland_c2_column_kernel"}
GOLDEN = {"cubic_column": "g13_cubic_column.npz", "wendland_c2_column": "g14_wendland_c2_column.npz"}


def _native(kernel):
    from asp_amd.tools import projections
    return getattr(projections, NATIVE[kernel])


def _report(label, worst):
    print(f"COLUMN_BAR {label}: worst err/E = {worst:.3f}")


_refs = {}


def _reference(oracle, kernel, window=None, raw=False):
    """The mixed set with the column kernel's equal-peak amplitudes, the fp64 restatement
    of its two maps (a0 = a T, a1 = a) and their bars; computed once."""
    key = (kernel, window, raw)
    if key not in _refs:
        s = cr.mixed_set(kernel, window, raw)
        ext = vb.window_ext(window)
        extra = vb.F64_INPUT_ULPS if raw else 0.0
        r = cr.scatter_f64(s["u"], s["v"], s["h"], np.stack([s["a0"], s["a"]]), vb.SIZE2D,
                           vb.CHUNK, *ext, kernel=kernel)
        ref = dict(s=s, ext=ext, r0=r[0], r1=r[1])
        for k, a in (("0", s["a0"]), ("1", s["a"])):
            ref["E" + k] = cr.bar2d(oracle, s["u"], s["v"], s["h"], a, kernel, ext=ext,
                                    extra_ulps=extra)
            ref["F" + k] = cr.fixed_point_term(kernel, s["h"], a)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _refs[key] = ref
    return _refs[key]


# ----------------------------------------------------------------- asp_kernel_eval
@pytest.mark.parametrize("kernel", cr.KERNELS)
def test_kernel_eval(gpu, kernel):
    one = np.float64(1.0)
    qs = np.concatenate([np.random.default_rng(30).uniform(0.0, 2.0, 2000),
                         [0.0, 0.5, np.nextafter(one, 0), 1.0, np.nextafter(one, 2), 1.5,
                          np.nextafter(2.0, 0), 2.0, 3.0]])
    hs = np.array([0.5, 1.0, 2.7])
    qq, hh = np.meshgrid(qs, hs, indexing="ij")
    rng = np.random.default_rng(1)
    r = np.concatenate([(qq * hh).ravel(), rng.uniform(0.0, 5.0, 10000)])
    h = np.concatenate([hh.ravel(), rng.uniform(0.05, 3.0, 10000)])
    w = _native(kernel)(r, h)
    want = cr.column_kernel(kernel, r, h)
    err = np.abs(w - want) / cr.w0(kernel, h)
    print(f"COLUMN kernel_eval {kernel}: worst |W - closed form| / W(0) = {err.max():.3e}")
    assert err.max() <= 2.0 ** -40
    assert np.all(w[r >= 2.0 * h] == 0.0)
    assert np.count_nonzero(r >= 2.0 * h) > 1000
    # h <= 0 as for ids 0 and 1: h = 0 gives 0
    assert np.all(_native(kernel)(np.array([0.0, 1.0]), np.zeros(2)) == 0.0)


# ------------------------------------------------------------ the reference's maps
@pytest.mark.parametrize("kernel", cr.KERNELS)
def test_golden(gpu, kernel):
    from asp_amd.tools.projections import create_image
    pos, h, A, size, cs, ext, _ = g3()
    img = create_image(pos, h, A, size, cs, 2, *ext, kernel_func=_native(kernel))
    assert_map_close(img, golden(GOLDEN[kernel])["img"])


@pytest.mark.parametrize("kernel", cr.KERNELS)
def test_native_against_plugin(gpu, oracle, kernel):
    """The same map through the native id and through the kernel_func plug-in with the
    closed-form NumPy callable (which itself reproduces the reference's map)."""
    from asp_amd.tools.projections import create_image
    pos, h, A, size, cs, ext, _ = g3()
    plug = create_image(pos, h, A, size, cs, 2, *ext, kernel_func=cr.CALLABLES[kernel])
    ref = golden(GOLDEN[kernel])["img"]
    np.testing.assert_allclose(plug, ref, rtol=1e-12, atol=1e-12 * np.abs(ref).max())
    img = create_image(pos, h, A, size, cs, 2, *ext, kernel_func=_native(kernel))
    E = cr.bar2d(oracle, pos[:, 0], pos[:, 1], h, A, kernel, size, ext, cs)
    _report(f"native vs plug-in {kernel}", vb.assert_terms_close(img, plug, E))


# ------------------------------------------------------------------------ mixed set
@pytest.mark.parametrize("thresholds", list(THRESHOLDS))
@pytest.mark.parametrize("deterministic", [False, True], ids=["fp64", "deterministic"])
@pytest.mark.parametrize("kernel", cr.KERNELS)
def test_mixed_set(gpu, oracle, monkeypatch, kernel, deterministic, thresholds):
    from asp_amd.device import project2d, stats
    _knobs(monkeypatch, THRESHOLDS[thresholds], vb.WIDE_TILES)
    ref = _reference(oracle, kernel)
    s = ref["s"]
    u, v, h, a, a0 = _dev(s["u"], s["v"], s["h"], s["a"], s["a0"])
    kw = dict(image_size=vb.SIZE2D, extent=vb.EXT2D, chunk_size=vb.CHUNK, kernel=kernel,
              deterministic=deterministic)

    def paths_ran():
        st = stats(0)
        assert st["wide"] > 0, st                                        # k_wide
        assert (st["large"] == 0) == (thresholds == "sweep_all"), st     # k_gather
        assert st["records"] > st["large"] and st["merges"] > 0, st      # k_deposit (packed 3x3)

    label = f"mixed {kernel} {'fix' if deterministic else 'f64'} {thresholds}"
    g, _ = project2d(u, v, h, a, **kw)
    paths_ran()
    _report(label + " one map", vb.assert_terms_close(
        _host(g), ref["r1"], ref["E1"], floor=ref["F1"] if deterministic else 0.0))
    g0, g1 = project2d(u, v, h, a0, a, **kw)
    paths_ran()
    w0 = vb.assert_terms_close(_host(g0), ref["r0"], ref["E0"],
                               floor=ref["F0"] if deterministic else 0.0)
    w1 = vb.assert_terms_close(_host(g1), ref["r1"], ref["E1"],
                               floor=ref["F1"] if deterministic else 0.0)
    _report(label + " two maps", max(w0, w1))
    assert _host(g).min() >= 0.0 and _host(g1).min() >= 0.0   # a >= 0: no negative pixel


# --------------------------------------------------------------------------- stamps
@pytest.mark.parametrize("where", vb.STAMP_POSITIONS)
@pytest.mark.parametrize("path", vb.STAMP_PATHS, ids=[p[0] for p in vb.STAMP_PATHS])
@pytest.mark.parametrize("kernel", cr.KERNELS)
def test_stamp(gpu, monkeypatch, kernel, path, where):
    from asp_amd.device import project2d, stats
    name, h_px, gmin, garea, wide_tiles, expect = path
    _knobs(monkeypatch, (gmin, garea), wide_tiles)
    u, v, h, a = vb.stamp_particle(cr.W0, kernel, h_px, where)
    r, E = cr.stamp_reference(kernel, u, v, h, a)
    assert np.count_nonzero(r) > 0
    g, _ = project2d(*_dev([u], [v], [h], [a]), image_size=vb.SIZE2D, extent=vb.EXT2D,
                     chunk_size=vb.CHUNK, kernel=kernel)
    st = stats(0)
    if expect == "wide":
        assert st["wide"] == 1, st
    else:
        assert st["wide"] == 0 and st["records"] > 0, st
        assert (st["large"] > 0) == (expect == "large"), st
    g = _host(g)
    if where == "corner":  # (u, v) is the corner of pixel (128, 128): q = 0, f = 1
        assert r[128, 128] == pytest.approx(a * cr.w0(kernel, h)[0], rel=1e-14)
        assert r[128, 128] == r.max() and g[128, 128] == g.max()
    _report(f"stamp {kernel} {name} {where}", vb.assert_terms_close(g, r, E))


@pytest.mark.parametrize("kernel", cr.KERNELS)
def test_identical_particles_on_a_corner(gpu, kernel):
    """4096 identical particles on one pixel corner, fixed point: that pixel's sum is
    n max|c| max f, the bound the per-tile scale is chosen for (max f = 1)."""
    from asp_amd.device import project2d
    n = 4096
    u, v, h, a = vb.stamp_particle(cr.W0, kernel, 3.0, "corner")
    r, E = cr.stamp_reference(kernel, u, v, h, a)
    F = cr.fixed_point_term(kernel, np.full(n, h), np.full(n, a))
    g, _ = project2d(*_dev(np.full(n, u), np.full(n, v), np.full(n, h), np.full(n, a)),
                     image_size=vb.SIZE2D, extent=vb.EXT2D, chunk_size=vb.CHUNK, kernel=kernel,
                     deterministic=True)
    g = _host(g)
    assert g[128, 128] == g.max() and abs(g[128, 128] - n * r[128, 128]) <= n * E[128, 128] + F
    _report(f"4096 on a corner {kernel}", vb.assert_terms_close(g, n * r, n * E, floor=F))


# ------------------------------------------------------------- other entry points
@pytest.mark.parametrize("kernel", cr.KERNELS)
def test_props_and_sph(gpu, oracle, monkeypatch, kernel):
    """asp_project2d_props (4 maps from one binning: the EXT passes) and asp_project2d_sph
    (coefficients fl32(A m / rho), formed in fp64 and rounded once)."""
    from asp_amd.device import project2d_props
    _knobs(monkeypatch, None, vb.WIDE_TILES)
    ref = _reference(oracle, kernel)
    s = ref["s"]
    rng = np.random.default_rng(22)
    p3 = vb.f32(s["a"] * (s["T"] - 2.0))  # mixed signs
    u, v, h = _dev(s["u"], s["v"], s["h"])
    kw = dict(image_size=vb.SIZE2D, extent=vb.EXT2D, chunk_size=vb.CHUNK, kernel=kernel)
    outs = project2d_props(u, v, h, _dev(s["a"], s["a0"], p3, s["a"]), **kw)
    r3 = cr.scatter_f64(s["u"], s["v"], s["h"], p3, vb.SIZE2D, vb.CHUNK, *vb.EXT2D, kernel=kernel)
    E3 = cr.bar2d(oracle, s["u"], s["v"], s["h"], p3, kernel)
    worst = max(vb.assert_terms_close(_host(o), r, E) for o, r, E in
                zip(outs, (ref["r1"], ref["r0"], r3, ref["r1"]),
                    (ref["E1"], ref["E0"], E3, ref["E1"])))
    _report(f"props {kernel}", worst)
    # sph: the plain projection of the coefficients w = fl32(a m / rho)
    m = vb.f32(rng.uniform(0.5, 2.0, s["a"].size))
    rho = vb.f32(rng.uniform(0.5, 2.0, s["a"].size))
    w = vb.f32(s["a"] * (m / rho))
    rw = cr.scatter_f64(s["u"], s["v"], s["h"], w, vb.SIZE2D, vb.CHUNK, *vb.EXT2D, kernel=kernel)
    Ew = cr.bar2d(oracle, s["u"], s["v"], s["h"], w, kernel)
    out, = project2d_props(u, v, h, _dev(s["a"]), mass=_dev(m)[0], density=_dev(rho)[0], **kw)
    _report(f"sph {kernel}", vb.assert_terms_close(_host(out), rw, Ew))


@pytest.mark.parametrize("kernel", cr.KERNELS)
def test_raw_f64(gpu, oracle, monkeypatch, kernel):
    """asp_project2d_f64 on raw fp64 arrays: the bar plus value_bar.F64_INPUT_ULPS."""
    from asp_amd.device import project2d_f64
    _knobs(monkeypatch, None, vb.WIDE_TILES)
    ref = _reference(oracle, kernel, raw=True)
    s = ref["s"]
    pos = np.stack([s["u"], s["v"], np.zeros(s["u"].size)], axis=1)
    g0, g1 = project2d_f64(pos, np.array(s["h"]), np.array(s["a0"]), np.array(s["a"]),
                           projection_axis=2, image_size=vb.SIZE2D, extent=vb.EXT2D,
                           chunk_size=vb.CHUNK, kernel=kernel)
    w0 = vb.assert_terms_close(g0, ref["r0"], ref["E0"])
    w1 = vb.assert_terms_close(g1, ref["r1"], ref["E1"])
    _report(f"raw f64 {kernel}", max(w0, w1))


@pytest.mark.parametrize("kernel", cr.KERNELS)
def test_rows(gpu, oracle, monkeypatch, kernel):
    from asp_amd.device import project2d
    _knobs(monkeypatch, None, vb.WIDE_TILES)
    rows = (100, 171)
    ref = _reference(oracle, kernel)
    s = ref["s"]
    u, v, h, a, a0 = _dev(s["u"], s["v"], s["h"], s["a"], s["a0"])
    g0, g1 = project2d(u, v, h, a0, a, rows=rows, image_size=vb.SIZE2D, extent=vb.EXT2D,
                       chunk_size=vb.CHUNK, kernel=kernel)
    cut = lambda m: m[rows[0]:rows[1]]  # noqa: E731
    w0 = vb.assert_terms_close(_host(g0), cut(ref["r0"]), cut(ref["E0"]))
    w1 = vb.assert_terms_close(_host(g1), cut(ref["r1"]), cut(ref["E1"]))
    _report(f"rows {rows} {kernel}", max(w0, w1))


@pytest.mark.parametrize("kernel", cr.KERNELS)
def test_offset_window(gpu, oracle, monkeypatch, kernel):
    from asp_amd.device import project2d
    _knobs(monkeypatch, None, vb.WIDE_TILES)
    ref = _reference(oracle, kernel, window="box")
    s = ref["s"]
    u, v, h, a, a0 = _dev(s["u"], s["v"], s["h"], s["a"], s["a0"])
    g0, g1 = project2d(u, v, h, a0, a, image_size=vb.SIZE2D, extent=ref["ext"],
                       chunk_size=vb.CHUNK, kernel=kernel)
    w0 = vb.assert_terms_close(_host(g0), ref["r0"], ref["E0"])
    w1 = vb.assert_terms_close(_host(g1), ref["r1"], ref["E1"])
    _report(f"window box {kernel}", max(w0, w1))


@pytest.mark.parametrize("kernel", cr.KERNELS)
def test_periodic_image(gpu, oracle, kernel):
    """create_periodic_image = the plain column projection of the staged set (the oracle's
    restatement of asp_stage_particles: every periodic image, fp32)."""
    from asp_amd.tools.projections import create_periodic_image
    rng = np.random.default_rng(3)
    L, n, G = 4.0, 1500, 96
    pos = rng.uniform(0.0, L, (n, 3))
    pos[0] = [0.01, 2.0, 2.0]  # hugs the x = 0 face: deposits on both sides
    h = rng.uniform(0.02, 0.12, n)
    A = rng.uniform(0.5, 2.0, n)
    c = np.array([2.5, 1.0, 0.0])
    img = create_periodic_image(pos, h, A, (G, G), 16, 2, L, c, kernel_func=_native(kernel))
    u, v, hh, a = (t.astype(np.float64) for t in oracle.stage_particles(
        pos, h, [A], 2, L=L, centre=c, shift="centre", images=True))
    assert u.size > n
    r = cr.scatter_f64(u, v, hh, a, (G, G), 16, 0.0, L, 0.0, L, kernel=kernel)
    E = cr.bar2d(oracle, u, v, hh, a, kernel, (G, G), (0.0, L, 0.0, L), 16)
    _report(f"periodic {kernel}", vb.assert_terms_close(img, r, E))


# ---------------------------------------------------------------- mass conservation
@pytest.mark.parametrize("kernel", cr.KERNELS)
def test_mass_conservation(gpu, oracle, kernel):
    """sum(map) x pixel area = sum a for footprints inside the window: what a column
    density is.  h >= 8 px: the exact kernel's lattice sum over pixel corners is then
    within 1e-7 of 1 (2 - 4e-6 at 4 px), so 1e-6 sum a is a condition on the inputs, which
    the fp64 restatement is asserted to meet first.  The 3-D-normalised kernel on the
    same inputs misses by more than 10 %."""
    from asp_amd.device import project2d
    rng = np.random.default_rng(40)
    n, pitch = 200, vb.PITCH2D
    hp = rng.uniform(8.0, 12.0, n)
    lo, hi = 2.0 * hp + 1.0, 256.0 - (2.0 * hp + 1.0)
    u = vb.f32(-1.0 + (lo + (hi - lo) * rng.uniform(0.0, 1.0, n)) * pitch)
    v = vb.f32(-1.0 + (lo + (hi - lo) * rng.uniform(0.0, 1.0, n)) * pitch)
    h = vb.f32(hp * pitch)
    a = vb.f32(rng.uniform(0.5, 1.5, n))
    total = a.sum()
    r = cr.scatter_f64(u, v, h, a, vb.SIZE2D, vb.CHUNK, *vb.EXT2D, kernel=kernel)
    assert abs(r.sum() * pitch ** 2 - total) <= 1e-6 * total
    E = cr.bar2d(oracle, u, v, h, a, kernel)
    kw = dict(image_size=vb.SIZE2D, extent=vb.EXT2D, chunk_size=vb.CHUNK)
    g, _ = project2d(*_dev(u, v, h, a), kernel=kernel, **kw)
    g = _host(g)
    miss = abs(g.sum() * pitch ** 2 - total)
    print(f"COLUMN mass {kernel}: |sum img pitch^2 - sum a| / sum a = {miss / total:.3e} "
          f"(bar {(E.sum() * pitch ** 2 + 1e-6 * total) / total:.3e})")
    assert miss <= E.sum() * pitch ** 2 + 1e-6 * total
    assert g.min() >= 0.0
    g3d, _ = project2d(*_dev(u, v, h, a), kernel=cr.BASE[kernel], **kw)
    assert abs(_host(g3d).sum() * pitch ** 2 - total) > 0.1 * total


# ------------------------------------------------------------------------- the cube
def test_cube_rejects_column_kernels(gpu):
    from asp_amd import _lib
    x = np.zeros(1, np.float32)
    out = np.zeros((4, 4, 4), np.float32)
    P = _lib.ptr
    for kid in (_lib.ASP_KERNEL_CUBIC_SPLINE_COLUMN, _lib.ASP_KERNEL_WENDLAND_C2_COLUMN):
        rc = _lib.lib().asp_project3d(P(x), P(x), P(x), P(np.ones(1, np.float32)),
                                      P(np.ones(1, np.float32)), 1, -1.0, 1.0, -1.0, 1.0, -1.0,
                                      1.0, 4, 4, 4, 0, 4, kid, 0, P(out), 0, None)
        assert rc == _lib.ASP_ERR_INVALID
        with pytest.raises(ValueError, match="no 3-D form"):
            _lib.check(rc)
    assert not out.any()
