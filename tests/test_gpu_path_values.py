"""Per-path VALUES of every deposit path, 2-D map and cube, against the oracle with the
per-pixel bar of tests/value_bar.py (DESIGN.md §5 "Bars").

The neighbour sets are pinned bit-exactly elsewhere through the indicator kernel, which
takes the exact decision through code of its own.  The values of the gathered deposit
(k_gather), the wide path (k_wide), the EXT coefficient passes and the cube's
edge-continuous plane walk come from the packed fp32 forms, and under the global-peak bar
of tests/test_gpu_parity.py a large-h particle's whole contribution lies below the
tolerance.  Here every particle's own peak is O(1) (equal-peak amplitudes), the bar is
per pixel, and each parametrisation asserts through ``stats()`` or its forcing knob that
the path it names ran.  Every case prints its worst err/E (``pytest -s``).
"""
import numpy as np
import pytest

import value_bar as vb

pytestmark = pytest.mark.gpu

SWEEP_ALL = ("65", str(1 << 30))
GATHER_ALL = ("5", "6")
THRESHOLDS = {"default": None, "sweep_all": SWEEP_ALL, "gather_all": GATHER_ALL}


def _dev(*arrs):
    import torch
    return [torch.tensor(np.asarray(a), dtype=torch.float32, device="cuda") for a in arrs]


def _host(t):
    return t.cpu().numpy().astype(np.float64)


def _knobs(monkeypatch, thresholds, wide_tiles):
    for name in ("ASP_GATHER_MIN", "ASP_GATHER_AREA"):
        monkeypatch.delenv(name, raising=False)
    if thresholds is not None:
        monkeypatch.setenv("ASP_GATHER_MIN", thresholds[0])
        monkeypatch.setenv("ASP_GATHER_AREA", thresholds[1])
    monkeypatch.setenv("ASP_WIDE_TILES", wide_tiles)


def _report(label, worst):
    print(f"VALUE_BAR {label}: worst err/E = {worst:.3f}")


# ------------------------------------------------------------------ mixed set, 2-D
@pytest.mark.parametrize("thresholds", list(THRESHOLDS))
@pytest.mark.parametrize("deterministic", [False, True], ids=["fp64", "deterministic"])
@pytest.mark.parametrize("kernel", vb.KERNELS)
def test_mixed_set_2d(gpu, oracle, monkeypatch, kernel, deterministic, thresholds):
    from asp_amd.device import project2d, stats
    _knobs(monkeypatch, THRESHOLDS[thresholds], vb.WIDE_TILES)
    s = vb.mixed_set(oracle, kernel)
    ref = vb.reference2d(oracle, kernel)
    u, v, h, a, a0 = _dev(s["u"], s["v"], s["h"], s["a"], s["a0"])
    kw = dict(image_size=vb.SIZE2D, extent=vb.EXT2D, chunk_size=vb.CHUNK, kernel=kernel,
              deterministic=deterministic)

    def paths_ran():
        st = stats(0)
        assert st["wide"] > 0, st
        assert (st["large"] == 0) == (thresholds == "sweep_all"), st
        assert st["merges"] > 0, st  # the clump's tile is split over several items

    label = f"2d {kernel} {'fix' if deterministic else 'f64'} {thresholds}"
    g, _ = project2d(u, v, h, a, **kw)
    paths_ran()
    w = vb.assert_terms_close(_host(g), ref["r1"], ref["E1"], ref["by_class1"],
                              floor=ref["F1"] if deterministic else 0.0)
    _report(label + " one map", w)
    g0, g1 = project2d(u, v, h, a0, a, **kw)
    paths_ran()
    w0 = vb.assert_terms_close(_host(g0), ref["r0"], ref["E0"], ref["by_class0"],
                               floor=ref["F0"] if deterministic else 0.0)
    w1 = vb.assert_terms_close(_host(g1), ref["r1"], ref["E1"], ref["by_class1"],
                               floor=ref["F1"] if deterministic else 0.0)
    _report(label + " two maps", max(w0, w1))


# ------------------------------------------------------------------------- stamps
@pytest.mark.parametrize("where", vb.STAMP_POSITIONS)
@pytest.mark.parametrize("path", vb.STAMP_PATHS, ids=[p[0] for p in vb.STAMP_PATHS])
@pytest.mark.parametrize("kernel", vb.KERNELS)
def test_stamp(gpu, oracle, monkeypatch, kernel, path, where):
    """One particle per map against a W(r, h) in fp64 NumPy at every pixel: E is that
    particle's own term, so a failure names the path."""
    from asp_amd.device import project2d, stats
    name, h_px, gmin, garea, wide_tiles, expect = path
    _knobs(monkeypatch, (gmin, garea), wide_tiles)
    u, v, h, a = vb.stamp_particle(oracle, kernel, h_px, where)
    r, E = vb.stamp_reference(oracle, kernel, u, v, h, a)
    assert np.count_nonzero(r) > 0
    g, _ = project2d(*_dev([u], [v], [h], [a]), image_size=vb.SIZE2D, extent=vb.EXT2D,
                     chunk_size=vb.CHUNK, kernel=kernel)
    st = stats(0)
    if expect == "wide":
        assert st["wide"] == 1, st
    else:
        assert st["wide"] == 0 and st["records"] > 0, st
        assert (st["large"] > 0) == (expect == "large"), st
    w = vb.assert_terms_close(_host(g), r, E, {name: E})
    _report(f"stamp {kernel} {name} {where}", w)


# -------------------------------------------------------------------- props passes
@pytest.mark.parametrize("kernel", vb.KERNELS)
def test_props_passes(gpu, oracle, monkeypatch, kernel):
    """k = 4 properties from one binning: maps 2 and 3 come from the EXT coefficient passes
    of k_deposit and k_gather (and of the wide path), each against the oracle."""
    from asp_amd.device import project2d_props, stats
    _knobs(monkeypatch, None, vb.WIDE_TILES)
    s = vb.mixed_set(oracle, kernel)
    ref = vb.reference2d(oracle, kernel)
    rng = np.random.default_rng(22)
    # property 2: an independent factor; property 3: mixed signs (T - 2 in [-1, 1])
    props = [s["a"], s["a0"], vb.f32(s["a"] * rng.uniform(0.5, 1.5, s["a"].size)),
             vb.f32(s["a"] * (s["T"] - 2.0))]
    u, v, h = _dev(s["u"], s["v"], s["h"])
    outs = project2d_props(u, v, h, _dev(*props), image_size=vb.SIZE2D, extent=vb.EXT2D,
                           chunk_size=vb.CHUNK, kernel=kernel)
    st = stats(0)
    assert st["wide"] > 0 and st["large"] > 0 and st["merges"] > 0, st
    for k, (p, o) in enumerate(zip(props, outs)):
        if k < 2:
            r, E, by_class = ((ref["r1"], ref["E1"], ref["by_class1"]) if k == 0 else
                              (ref["r0"], ref["E0"], ref["by_class0"]))
        else:
            r, _ = oracle.project_scatter(s["u"], s["v"], s["h"], p, None, vb.SIZE2D, vb.CHUNK,
                                          *vb.EXT2D, kernel=kernel)
            E, by_class = vb.bar2d(oracle, s, p, kernel)
        w = vb.assert_terms_close(_host(o), r, E, by_class)
        _report(f"props {kernel} map {k}", w)


# ---------------------------------------------------------------------- non-square
def test_mixed_set_nonsquare(gpu, oracle, monkeypatch):
    """192 x 256: the reference's nx quirk changes the v pitch and the chunk cull cuts the
    discs, so the gather forms take decisions again."""
    from asp_amd.device import project2d, stats
    _knobs(monkeypatch, None, vb.WIDE_TILES)
    kernel, size = "cubic", vb.SIZE2D_NONSQUARE
    s = vb.mixed_set(oracle, kernel)
    ref = vb.reference2d(oracle, kernel, size)
    u, v, h, a, a0 = _dev(s["u"], s["v"], s["h"], s["a"], s["a0"])
    g0, g1 = project2d(u, v, h, a0, a, image_size=size, extent=vb.EXT2D, chunk_size=vb.CHUNK,
                       kernel=kernel)
    st = stats(0)
    assert st["wide"] > 0 and st["large"] > 0 and st["merges"] > 0, st
    w0 = vb.assert_terms_close(_host(g0), ref["r0"], ref["E0"], ref["by_class0"])
    w1 = vb.assert_terms_close(_host(g1), ref["r1"], ref["E1"], ref["by_class1"])
    _report("2d cubic 192x256", max(w0, w1))


# ---------------------------------------------------------------------------- cube
@pytest.mark.parametrize("lane_cols", [None, "0", "100000"],
                         ids=["default", "wave_walk", "lane_per_record"])
@pytest.mark.parametrize("kernel", vb.KERNELS)
def test_cube(gpu, oracle, monkeypatch, kernel, lane_cols):
    """ASP_CUBE_LANE_COLS = 0 walks every record with a wave, 100000 deposits every record
    lane-per-record; the default mixes them by box size."""
    from asp_amd.device import project3d
    monkeypatch.delenv("ASP_CUBE_LANE_COLS", raising=False)
    if lane_cols is not None:
        monkeypatch.setenv("ASP_CUBE_LANE_COLS", lane_cols)
    s = vb.cube_set(oracle, kernel)
    ref = vb.reference3d(oracle, kernel)
    x, y, z, h, a = _dev(s["x"], s["y"], s["z"], s["h"], s["a"])
    g = project3d(x, y, z, h, a, cube_size=vb.SIZE3D, extent=vb.EXT3D, kernel=kernel)
    w = vb.assert_terms_close(_host(g), ref["r"], ref["E"], ref["by_class"])
    _report(f"cube {kernel} lane_cols={lane_cols}", w)


def test_cube_planes_slab(gpu, oracle):
    from asp_amd.device import project3d
    kernel, planes = "wendland_c2", (21, 45)
    s = vb.cube_set(oracle, kernel)
    x, y, z, h, a = _dev(s["x"], s["y"], s["z"], s["h"], s["a"])
    g = project3d(x, y, z, h, a, cube_size=vb.SIZE3D, extent=vb.EXT3D, kernel=kernel,
                  planes=planes)
    r = oracle.project3d(s["x"], s["y"], s["z"], s["h"], s["a"], vb.SIZE3D, vb.EXT3D,
                         kernel=kernel, planes=planes)
    E, by_class = vb.bar3d(oracle, s, kernel, planes=planes)
    full = vb.reference3d(oracle, kernel)
    assert np.array_equal(r, full["r"][:, :, planes[0]:planes[1]])  # the oracle's own planes
    w = vb.assert_terms_close(_host(g), r, E, by_class)
    _report(f"cube {kernel} planes={planes}", w)


@pytest.mark.parametrize("lane_cols", ["0", "100000"], ids=["wave_walk", "lane_per_record"])
@pytest.mark.parametrize("kernel", vb.KERNELS)
def test_cube_stamp_exact_ties(gpu, oracle, monkeypatch, kernel, lane_cols):
    """One particle on a voxel corner with 2h a whole number of z pitches (1/16, exact in
    binary): the voxels k +- 2h / pz of its column lie at exactly r = 2h, which the
    reference excludes (strict <) and the edge-continuous plane walk evaluates.  They must
    be exactly 0 (value_bar's first assertion), the others within the particle's term."""
    from asp_amd.device import project3d
    monkeypatch.setenv("ASP_CUBE_LANE_COLS", lane_cols)
    worst = 0.0
    for planes2h in range(3, 10):
        h = planes2h * (4.0 / 64) / 2
        s = dict(x=np.array([0.0]), y=np.array([0.0]), z=np.array([0.0]), h=vb.f32([h]),
                 cls=np.array([0]), names=[f"2h={planes2h}pz"])
        s["a"] = vb.f32(1.25 / vb.w0(oracle, kernel, s["h"]))
        r = oracle.project3d(s["x"], s["y"], s["z"], s["h"], s["a"], vb.SIZE3D, vb.EXT3D,
                             kernel=kernel)
        assert r[24, 20, 32] != 0 and r[24, 20, 32 + planes2h] == 0
        assert r[24, 20, 32 + planes2h - 1] != 0
        E, by_class = vb.bar3d(oracle, s, kernel)
        g = project3d(*_dev(s["x"], s["y"], s["z"], s["h"], s["a"]), cube_size=vb.SIZE3D,
                      extent=vb.EXT3D, kernel=kernel)
        worst = max(worst, vb.assert_terms_close(_host(g), r, E, by_class))
    _report(f"cube stamp {kernel} lane_cols={lane_cols}", worst)


# ---------------------------------------------------------------- offset windows
# The same sets at zoom windows far from the origin (value_bar.WINDOWS):
# |corner| is 1e5 .. 1e7 pixel pitches, the bar is unchanged -- it has no |corner| term.
# Every case also runs the indicator kernel through the same path selection and compares
# its neighbour counts with the oracle's bit-exactly: the candidate boxes grow by 2 .. 8
# pixels per side at these |u| / pitch, and a grown box must change no neighbour set.
def _mixed_kw(window, kernel, size=vb.SIZE2D, **more):
    return dict(image_size=size, extent=vb.window_ext(window), chunk_size=vb.CHUNK,
                kernel=kernel, **more)


def _mixed_paths_ran(large=True):
    from asp_amd.device import stats
    st = stats(0)
    assert st["wide"] > 0, st
    assert (st["large"] > 0) == large, st
    assert st["merges"] > 0, st  # the clump's tile is split over several items


def _counts_exact(window, s, cnt, **kw):
    from asp_amd.device import project2d
    u, v, h = _dev(s["u"], s["v"], s["h"])
    ones = _dev(np.ones(s["h"].size))[0]
    c, _ = project2d(u, v, h, ones, **_mixed_kw(window, "indicator", **kw))
    assert np.array_equal(_host(c), cnt), f"{window}: neighbour counts differ from the oracle"


@pytest.mark.parametrize("thresholds", list(THRESHOLDS))
@pytest.mark.parametrize("kernel", vb.KERNELS)
@pytest.mark.parametrize("window", vb.WINDOW_NAMES)
def test_window_mixed_set(gpu, oracle, monkeypatch, window, kernel, thresholds):
    from asp_amd.device import project2d
    _knobs(monkeypatch, THRESHOLDS[thresholds], vb.WIDE_TILES)
    s = vb.mixed_set(oracle, kernel, window)
    ref = vb.reference2d(oracle, kernel, window=window)
    u, v, h, a, a0 = _dev(s["u"], s["v"], s["h"], s["a"], s["a0"])
    g0, g1 = project2d(u, v, h, a0, a, **_mixed_kw(window, kernel))
    _mixed_paths_ran(large=thresholds != "sweep_all")
    _counts_exact(window, s, ref["cnt"])
    _mixed_paths_ran(large=thresholds != "sweep_all")  # (the indicator's run as well)
    w0 = vb.assert_terms_close(_host(g0), ref["r0"], ref["E0"], ref["by_class0"])
    w1 = vb.assert_terms_close(_host(g1), ref["r1"], ref["E1"], ref["by_class1"])
    _report(f"window {window} {kernel} f64 {thresholds} two maps", max(w0, w1))


@pytest.mark.parametrize("where", vb.STAMP_POSITIONS)
@pytest.mark.parametrize("path", vb.STAMP_PATHS, ids=[p[0] for p in vb.STAMP_PATHS])
@pytest.mark.parametrize("kernel", vb.KERNELS)
@pytest.mark.parametrize("window", vb.WINDOW_NAMES)
def test_window_stamp(gpu, oracle, monkeypatch, window, kernel, path, where):
    """test_stamp at the window.  There the candidate-box margin is 2 - 8 px, so a stamp's
    box may be binned larger than at the origin (a ``small3`` box need not stay <= 3 x 3:
    nothing here asserts that it did); the stream each path's knobs select is asserted as
    in test_stamp."""
    from asp_amd.device import project2d, stats
    name, h_px, gmin, garea, wide_tiles, expect = path
    _knobs(monkeypatch, (gmin, garea), wide_tiles)
    ext = vb.window_ext(window)
    u, v, h, a = vb.stamp_particle(oracle, kernel, h_px, where, window)
    r, E = vb.stamp_reference(oracle, kernel, u, v, h, a, vb.SIZE2D, ext)
    assert np.count_nonzero(r) > 0
    kw = dict(image_size=vb.SIZE2D, extent=ext, chunk_size=vb.CHUNK)
    g, _ = project2d(*_dev([u], [v], [h], [a]), kernel=kernel, **kw)
    st = stats(0)
    if expect == "wide":
        assert st["wide"] == 1, st
    else:
        assert st["wide"] == 0 and st["records"] > 0, st
        assert (st["large"] > 0) == (expect == "large"), st
    c, _ = project2d(*_dev([u], [v], [h], [1.0]), kernel="indicator", **kw)
    assert np.array_equal(_host(c), (r != 0).astype(np.float64))
    w = vb.assert_terms_close(_host(g), r, E, {name: E})
    _report(f"window {window} stamp {kernel} {name} {where}", w)


@pytest.mark.parametrize("nmaps", [1, 2])
def test_window_deterministic(gpu, oracle, monkeypatch, nmaps):
    from asp_amd.device import project2d
    window, kernel = "box", "wendland_c2"
    _knobs(monkeypatch, None, vb.WIDE_TILES)
    s = vb.mixed_set(oracle, kernel, window)
    ref = vb.reference2d(oracle, kernel, window=window)
    u, v, h, a, a0 = _dev(s["u"], s["v"], s["h"], s["a"], s["a0"])
    kw = _mixed_kw(window, kernel, deterministic=True)
    if nmaps == 1:
        g, _ = project2d(u, v, h, a, **kw)
        _mixed_paths_ran()
        w = vb.assert_terms_close(_host(g), ref["r1"], ref["E1"], ref["by_class1"], floor=ref["F1"])
    else:
        g0, g1 = project2d(u, v, h, a0, a, **kw)
        _mixed_paths_ran()
        w = max(vb.assert_terms_close(_host(g0), ref["r0"], ref["E0"], ref["by_class0"],
                                      floor=ref["F0"]),
                vb.assert_terms_close(_host(g1), ref["r1"], ref["E1"], ref["by_class1"],
                                      floor=ref["F1"]))
    _counts_exact(window, s, ref["cnt"], deterministic=True)
    _report(f"window {window} {kernel} fix {nmaps} map(s)", w)


def test_window_props_passes(gpu, oracle, monkeypatch):
    """test_props_passes (k = 4: the EXT passes included) on ``box``."""
    from asp_amd.device import project2d_props
    window, kernel = "box", "wendland_c2"
    _knobs(monkeypatch, None, vb.WIDE_TILES)
    ext = vb.window_ext(window)
    s = vb.mixed_set(oracle, kernel, window)
    ref = vb.reference2d(oracle, kernel, window=window)
    rng = np.random.default_rng(22)
    props = [s["a"], s["a0"], vb.f32(s["a"] * rng.uniform(0.5, 1.5, s["a"].size)),
             vb.f32(s["a"] * (s["T"] - 2.0))]
    u, v, h = _dev(s["u"], s["v"], s["h"])
    outs = project2d_props(u, v, h, _dev(*props), image_size=vb.SIZE2D, extent=ext,
                           chunk_size=vb.CHUNK, kernel=kernel)
    _mixed_paths_ran()
    for k, (p, o) in enumerate(zip(props, outs)):
        if k < 2:
            r, E, by_class = ((ref["r1"], ref["E1"], ref["by_class1"]) if k == 0 else
                              (ref["r0"], ref["E0"], ref["by_class0"]))
        else:
            r, _ = oracle.project_scatter(s["u"], s["v"], s["h"], p, None, vb.SIZE2D, vb.CHUNK,
                                          *ext, kernel=kernel)
            E, by_class = vb.bar2d(oracle, s, p, kernel, ext=ext)
        w = vb.assert_terms_close(_host(o), r, E, by_class)
        _report(f"window {window} props {kernel} map {k}", w)
    ones = _dev(np.ones(s["h"].size))[0]
    cnts = project2d_props(u, v, h, [ones, ones, ones, ones], image_size=vb.SIZE2D, extent=ext,
                           chunk_size=vb.CHUNK, kernel="indicator")
    for c in cnts:
        assert np.array_equal(_host(c), ref["cnt"])


@pytest.mark.parametrize("rows", [(100, 171), (64, 192)], ids=["100-171", "64-192"])
def test_window_rows(gpu, oracle, monkeypatch, rows):
    """Row windows of the ``box`` map: the tiles start at row_lo, so the local frames differ
    from the full map's; the same rows of the oracle map and bar."""
    from asp_amd.device import project2d
    window, kernel = "box", "wendland_c2"
    _knobs(monkeypatch, None, vb.WIDE_TILES)
    s = vb.mixed_set(oracle, kernel, window)
    ref = vb.reference2d(oracle, kernel, window=window)
    u, v, h, a, a0 = _dev(s["u"], s["v"], s["h"], s["a"], s["a0"])
    g0, g1 = project2d(u, v, h, a0, a, rows=rows, **_mixed_kw(window, kernel))
    _mixed_paths_ran()
    _counts_exact(window, s, ref["cnt"][rows[0]:rows[1]], rows=rows)
    cut = lambda m: m[rows[0]:rows[1]]  # noqa: E731
    w0 = vb.assert_terms_close(_host(g0), cut(ref["r0"]), cut(ref["E0"]),
                               {n: cut(m) for n, m in ref["by_class0"].items()})
    w1 = vb.assert_terms_close(_host(g1), cut(ref["r1"]), cut(ref["E1"]),
                               {n: cut(m) for n, m in ref["by_class1"].items()})
    _report(f"window {window} {kernel} rows={rows}", max(w0, w1))


def _raw_positions(s, axis):
    """(N, 3) fp64 positions whose projected columns for ``axis`` are the raw (u, v) -- the
    third column is junk the projection must not read."""
    cu, cv = {0: (1, 2), 1: (0, 2), 2: (0, 1)}[axis]
    pos = np.empty((s["u"].size, 3))
    pos[:, axis] = np.random.default_rng(23).uniform(-1e3, 1e3, s["u"].size)
    pos[:, cu], pos[:, cv] = s["u"], s["v"]
    return pos


@pytest.mark.parametrize("axis", [2, 0])
def test_window_raw_f64(gpu, oracle, monkeypatch, axis):
    """asp_project2d_f64 on raw fp64 arrays off the fp32 lattice: the oracle on those arrays,
    the bar plus the device's own rounding of h and a (value_bar.F64_INPUT_ULPS)."""
    from asp_amd.device import project2d_f64
    window, kernel = "box", "wendland_c2"
    _knobs(monkeypatch, None, vb.WIDE_TILES)
    s = vb.mixed_set(oracle, kernel, window, raw=True)
    ref = vb.reference2d(oracle, kernel, window=window, raw=True)
    pos = _raw_positions(s, axis)
    kw = dict(projection_axis=axis, image_size=vb.SIZE2D, extent=vb.window_ext(window),
              chunk_size=vb.CHUNK)
    h, a, a0 = (np.array(s[k]) for k in ("h", "a", "a0"))  # (the shared set is read-only)
    g0, g1 = project2d_f64(pos, h, a0, a, kernel=kernel, **kw)
    _mixed_paths_ran()
    c, _ = project2d_f64(pos, h, np.ones(h.size), kernel="indicator", **kw)
    assert np.array_equal(np.asarray(c, np.float64), ref["cnt"])
    w0 = vb.assert_terms_close(g0, ref["r0"], ref["E0"], ref["by_class0"])
    w1 = vb.assert_terms_close(g1, ref["r1"], ref["E1"], ref["by_class1"])
    _report(f"window {window} {kernel} raw f64 axis={axis}", max(w0, w1))


def test_window_props_f64(gpu, oracle, monkeypatch):
    from asp_amd.device import project2d_props_f64
    window, kernel = "box", "wendland_c2"
    _knobs(monkeypatch, None, vb.WIDE_TILES)
    ext = vb.window_ext(window)
    s = vb.mixed_set(oracle, kernel, window, raw=True)
    ref = vb.reference2d(oracle, kernel, window=window, raw=True)
    pos = _raw_positions(s, 2)
    props = [np.array(s["a"]), np.array(s["a0"]), s["a"] * (s["T"] - 2.0)]
    kw = dict(projection_axis=2, image_size=vb.SIZE2D, extent=ext, chunk_size=vb.CHUNK)
    h = np.array(s["h"])  # (the shared set is read-only)
    outs = project2d_props_f64(pos, h, props, kernel=kernel, **kw)
    _mixed_paths_ran()
    for k, (p, o) in enumerate(zip(props, outs)):
        if k < 2:
            r, E, by_class = ((ref["r1"], ref["E1"], ref["by_class1"]) if k == 0 else
                              (ref["r0"], ref["E0"], ref["by_class0"]))
        else:
            r, _ = oracle.project_scatter(s["u"], s["v"], s["h"], p, None, vb.SIZE2D, vb.CHUNK,
                                          *ext, kernel=kernel)
            E, by_class = vb.bar2d(oracle, s, p, kernel, ext=ext,
                                   extra_ulps=vb.F64_INPUT_ULPS)
        w = vb.assert_terms_close(_host(o), r, E, by_class)
        _report(f"window {window} props f64 {kernel} map {k}", w)
    ones = np.ones(s["h"].size)
    for c in project2d_props_f64(pos, h, [ones, ones.copy(), ones.copy()], kernel="indicator",
                                 **kw):
        assert np.array_equal(_host(c), ref["cnt"])


def test_window_nonsquare(gpu, oracle, monkeypatch):
    """192 x 256 on ``box``, cubic: the gather forms decide again, with g.mgl."""
    from asp_amd.device import project2d
    window, kernel, size = "box", "cubic", vb.SIZE2D_NONSQUARE
    _knobs(monkeypatch, None, vb.WIDE_TILES)
    s = vb.mixed_set(oracle, kernel, window)
    ref = vb.reference2d(oracle, kernel, size, window=window)
    u, v, h, a, a0 = _dev(s["u"], s["v"], s["h"], s["a"], s["a0"])
    g0, g1 = project2d(u, v, h, a0, a, **_mixed_kw(window, kernel, size))
    _mixed_paths_ran()
    _counts_exact(window, s, ref["cnt"], size=size)
    w0 = vb.assert_terms_close(_host(g0), ref["r0"], ref["E0"], ref["by_class0"])
    w1 = vb.assert_terms_close(_host(g1), ref["r1"], ref["E1"], ref["by_class1"])
    _report(f"window {window} cubic 192x256", max(w0, w1))


# ------------------------------------------------------------------ cube at an offset
def _cube_counts_exact(oracle, s, ext, planes=None):
    from asp_amd.device import project3d
    ones = np.ones(s["h"].size)
    x, y, z, h, a = _dev(s["x"], s["y"], s["z"], s["h"], ones)
    c = project3d(x, y, z, h, a, cube_size=vb.SIZE3D, extent=ext, kernel="indicator",
                  planes=planes)
    want = oracle.project3d(s["x"], s["y"], s["z"], s["h"], ones, vb.SIZE3D, ext,
                            kernel="indicator", planes=planes)
    assert np.array_equal(_host(c), want), "voxel neighbour counts differ from the oracle"


@pytest.mark.parametrize("lane_cols", [None, "0", "100000"],
                         ids=["default", "wave_walk", "lane_per_record"])
@pytest.mark.parametrize("kernel", vb.KERNELS)
def test_window_cube(gpu, oracle, monkeypatch, kernel, lane_cols):
    """test_cube moved by value_bar.CUBE_SHIFT (positions fp32-rounded after the shift),
    held to bar3d unchanged."""
    from asp_amd.device import project3d
    monkeypatch.delenv("ASP_CUBE_LANE_COLS", raising=False)
    if lane_cols is not None:
        monkeypatch.setenv("ASP_CUBE_LANE_COLS", lane_cols)
    ext = vb.cube_ext(vb.CUBE_SHIFT)
    s = vb.cube_set(oracle, kernel, vb.CUBE_SHIFT)
    ref = vb.reference3d(oracle, kernel, vb.CUBE_SHIFT)
    x, y, z, h, a = _dev(s["x"], s["y"], s["z"], s["h"], s["a"])
    g = project3d(x, y, z, h, a, cube_size=vb.SIZE3D, extent=ext, kernel=kernel)
    _cube_counts_exact(oracle, s, ext)
    w = vb.assert_terms_close(_host(g), ref["r"], ref["E"], ref["by_class"])
    _report(f"window cube {kernel} lane_cols={lane_cols}", w)


def test_window_cube_planes_slab(gpu, oracle):
    from asp_amd.device import project3d
    kernel, planes = "wendland_c2", (21, 45)
    ext = vb.cube_ext(vb.CUBE_SHIFT)
    s = vb.cube_set(oracle, kernel, vb.CUBE_SHIFT)
    x, y, z, h, a = _dev(s["x"], s["y"], s["z"], s["h"], s["a"])
    g = project3d(x, y, z, h, a, cube_size=vb.SIZE3D, extent=ext, kernel=kernel, planes=planes)
    r = oracle.project3d(s["x"], s["y"], s["z"], s["h"], s["a"], vb.SIZE3D, ext, kernel=kernel,
                         planes=planes)
    E, by_class = vb.bar3d(oracle, s, kernel, ext=ext, planes=planes)
    full = vb.reference3d(oracle, kernel, vb.CUBE_SHIFT)
    assert np.array_equal(r, full["r"][:, :, planes[0]:planes[1]])
    _cube_counts_exact(oracle, s, ext, planes)
    w = vb.assert_terms_close(_host(g), r, E, by_class)
    _report(f"window cube {kernel} planes={planes}", w)


@pytest.mark.parametrize("lane_cols", ["0", "100000"], ids=["wave_walk", "lane_per_record"])
@pytest.mark.parametrize("kernel", vb.KERNELS)
def test_window_cube_stamp_exact_ties(gpu, oracle, monkeypatch, kernel, lane_cols):
    """test_cube_stamp_exact_ties at the offset: the particle on the voxel corner
    (24, 20, 32) = CUBE_SHIFT, 2h a whole number of z pitches (1/16; 331 + k / 16 is exact
    in fp32 and fp64), so the voxels k +- 2h / pz lie at exactly r = 2h and must be 0."""
    from asp_amd.device import project3d
    monkeypatch.setenv("ASP_CUBE_LANE_COLS", lane_cols)
    ext = vb.cube_ext(vb.CUBE_SHIFT)
    worst = 0.0
    for planes2h in range(3, 10):
        h = planes2h * (4.0 / 64) / 2
        s = dict(x=np.array([vb.CUBE_SHIFT[0]]), y=np.array([vb.CUBE_SHIFT[1]]),
                 z=np.array([vb.CUBE_SHIFT[2]]), h=vb.f32([h]), cls=np.array([0]),
                 names=[f"2h={planes2h}pz"])
        s["a"] = vb.f32(1.25 / vb.w0(oracle, kernel, s["h"]))
        r = oracle.project3d(s["x"], s["y"], s["z"], s["h"], s["a"], vb.SIZE3D, ext, kernel=kernel)
        assert r[24, 20, 32] != 0 and r[24, 20, 32 + planes2h] == 0
        assert r[24, 20, 32 + planes2h - 1] != 0
        E, by_class = vb.bar3d(oracle, s, kernel, ext=ext)
        g = project3d(*_dev(s["x"], s["y"], s["z"], s["h"], s["a"]), cube_size=vb.SIZE3D,
                      extent=ext, kernel=kernel)
        _cube_counts_exact(oracle, s, ext)
        worst = max(worst, vb.assert_terms_close(_host(g), r, E, by_class))
    _report(f"window cube stamp {kernel} lane_cols={lane_cols}", worst)
