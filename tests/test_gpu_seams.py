"""Per-pixel VALUES across the seams of a multi-pass call (DESIGN.md §5 "Bars", §6).

A 2-D map call is a loop of pipeline passes (``project2d_full``): an image of more than 4096
GPU tiles runs as WINDOWS of whole tile rows, footprints clipped to each, and a particle array
beyond one pass as BATCHES whose later passes accumulate into the stored fp32 map.  The
global-peak bar cannot see a large-h particle at all; here the per-pixel bar of
tests/value_bar.py is applied where a wide or gathered footprint is cut by a window seam
(the strip of ``value_bar.STRIPS``: 4104 x 1 tiles, the seam at row 262144, every particle
within a few hundred rows of it) and where batches meet (the 256^2 mixed set and the cube),
for every entry point that goes through the loop.

Every case asserts that its path ran -- the tile count, the streams (``stats()``) and the
number of passes P, read from the library's own launch counts (``_counted``) -- widens the
bar by the pass rule for exactly that P (``value_bar.with_passes``) and prints its worst
err/E (``pytest -s``).  The references are computed once per kernel and strip and shared.
"""
import numpy as np
import pytest

import column_ref as cr
import value_bar as vb
from test_gpu_path_values import THRESHOLDS, _dev, _host, _knobs, _raw_positions

pytestmark = pytest.mark.gpu

NX, NY = vb.STRIP_SIZE
STRIP_TILES = 4104   # 4096 in window 0, 8 in window 1
BATCH = "2000"       # ASP_MAX_BATCH on the 4912-particle mixed set: 3 batches
STRIP_BATCH = "2500"  # on the 4912-particle strip set: 2 batches in each of the 2 windows
CUBE_BATCH = "1000"  # on the 3624-particle cube set: 4 batches
MODES = ("batch", "records")


@pytest.fixture(autouse=True)
def _no_pass_knobs(monkeypatch):
    for name in ("ASP_MAX_BATCH", "ASP_MAX_RECORDS", "ASP_REUSE_LAYOUT"):
        monkeypatch.delenv(name, raising=False)


def _report(label, worst, passes):
    print(f"VALUE_BAR seams {label} P={passes}: worst err/E = {worst:.3f}")


def _counted(call, per_pass=1, stage="deposit", also=()):
    """(call(), P[, launches of the stages ``also``]): the passes of the call, from the
    library's launch counts (asp_profile / asp_profile_read).

    The stage counted is ``deposit`` (``cube_deposit`` for the cube): run_tail launches
    k_deposit exactly once in every pass that completes, a pass on a reused layout included,
    and a pass abandoned for its record count (kRetSplit) returns before it.  The EXT passes
    of asp_project2d_props launch it once more per pair of further properties, which
    ``per_pass`` divides out.  No other stage does: count / colscan / tilescan also run in an
    abandoned pass and not on a reused layout, the scatter may run speculatively and again,
    gather / merge / wide / ratio only where their lists are not empty.  The counts are exact
    up to kMarks = 8 launches of a stage, so every case here stays at P <= 8."""
    from asp_amd import _lib
    _lib.profile(0, True)
    try:
        out = call()
        read = _lib.profile_read(0)
    finally:
        _lib.profile(0, False)
    launches = read[stage][1]
    assert launches > 0 and launches % per_pass == 0, (stage, launches, per_pass)
    passes = launches // per_pass
    assert passes <= 8, passes
    if also:
        return out, passes, tuple(read[k][1] for k in also)
    return out, passes


def _paths_ran(large=True, wide=True, merges=True, tiles=None):
    from asp_amd.device import stats
    st = stats(0)
    if tiles is not None:
        assert st["tiles"] == tiles, st
    assert (st["wide"] > 0) == wide, st
    assert (st["large"] > 0) == large, st
    assert (st["merges"] > 0) == merges, st
    return st


def _bar(ref, k, passes, deterministic=False):
    """(E, by_class, floor) of map ``k`` ('0': a T, '1': a) for a call of ``passes``."""
    return (vb.with_passes(ref["E" + k], ref["S" + k], passes), ref["by_class" + k],
            ref["F" + k] if deterministic else 0.0)


def _check(g, ref, k, passes, deterministic=False, cut=None):
    E, by_class, floor = _bar(ref, k, passes, deterministic)
    r = ref["r" + k]
    if cut is not None:
        r, E, by_class = cut(r), cut(E), {n: cut(m) for n, m in by_class.items()}
    return vb.assert_terms_close(g, r, E, by_class, floor=floor)


def _mixed_props(s):
    """k = 6 properties: a, a T, an independent factor, and three of mixed signs."""
    rng = np.random.default_rng(22)
    n = s["a"].size
    return [np.array(s["a"]), np.array(s["a0"]), vb.f32(s["a"] * rng.uniform(0.5, 1.5, n)),
            vb.f32(s["a"] * (s["T"] - 2.0)), vb.f32(s["a0"] * rng.uniform(-1.0, 1.0, n)),
            vb.f32(-s["a"] * rng.uniform(0.25, 2.0, n))]


def _sph_weights(n):
    """m = U(0.5, 2), rho = exp(U(-6, 3)), both fp32-representable."""
    rng = np.random.default_rng(25)
    return vb.f32(rng.uniform(0.5, 2.0, n)), vb.f32(np.exp(rng.uniform(-6.0, 3.0, n)))


def _sph_product(a, m, rho):
    """fl32(A (m / rho)), formed in fp64 and rounded once, as k_weigh forms it."""
    return vb.f32(np.asarray(a, np.float64) * (m / rho))


# =============================================================== the strip: a window seam
def _strip_kw(name, kernel, **more):
    return dict(image_size=vb.STRIP_SIZE, extent=vb.strip_ext(name), chunk_size=vb.CHUNK,
                kernel=kernel, **more)


def _strip(t, row_lo=0):
    """The rows from STRIP_LO on of a strip map (device tensor or array) whose first row is
    image row ``row_lo``, as float64; the rows before them must be 0."""
    if hasattr(t, "cpu"):
        k = vb.STRIP_LO - row_lo
        assert not bool(t[:k].any()), "pixels below STRIP_LO are not 0"
        return _host(t[k:])
    return vb.strip_crop(t, row_lo)


def _strip_counts_exact(name, s, cnt, passes, **kw):
    from asp_amd.device import project2d
    u, v, h = _dev(s["u"], s["v"], s["h"])
    ones = _dev(np.ones(s["h"].size))[0]
    (c, _), P = _counted(lambda: project2d(u, v, h, ones, **_strip_kw(name, "indicator", **kw)))
    assert P == passes
    assert np.array_equal(_strip(c, kw.get("rows", (0,))[0]), cnt), \
        f"{name}: neighbour counts differ from the oracle"


def _strip_other(oracle, s, p, kernel, name, passes, extra=0.0):
    """(r, E, by_class) of a further property ``p`` on the strip."""
    ext = vb.strip_ext(name)
    r, _ = vb.strip_scatter(oracle, s, p, None, kernel, ext)
    E, by_class = vb.strip_bar(oracle, s, p, kernel, ext, extra + vb.pass_ulps(passes))
    return r, E, by_class


@pytest.mark.parametrize("thresholds", list(THRESHOLDS))
@pytest.mark.parametrize("name", vb.STRIP_NAMES)
@pytest.mark.parametrize("kernel", vb.KERNELS)
def test_strip_two_maps(gpu, oracle, monkeypatch, kernel, name, thresholds):
    """One pass per window: the wide class (k_wide) and the gathered records (k_gather) are
    clipped by the seam, the clump sits on it."""
    from asp_amd.device import project2d
    _knobs(monkeypatch, THRESHOLDS[thresholds], vb.STRIP_WIDE_TILES)
    s = vb.strip_set(oracle, kernel, name)
    ref = vb.strip_reference(oracle, kernel, name)
    u, v, h, a, a0 = _dev(s["u"], s["v"], s["h"], s["a"], s["a0"])
    (g0, g1), P = _counted(lambda: project2d(u, v, h, a0, a, **_strip_kw(name, kernel)))
    assert P == 2
    # (split tiles: the seam halves the clump, so no tile holds the 2048 small records an item
    # takes; the tiles next to the seam are split in the large stream, 256 records an item)
    _paths_ran(large=thresholds != "sweep_all", merges=thresholds != "sweep_all",
               tiles=STRIP_TILES)
    _strip_counts_exact(name, s, ref["cnt"], 2)
    w = max(_check(_strip(g0), ref, "0", P), _check(_strip(g1), ref, "1", P))
    _report(f"strip {name} {kernel} f64 {thresholds} two maps", w, P)


@pytest.mark.parametrize("nmaps,kernel,name", [(1, "cubic", "strip_grid"),
                                               (2, "wendland_c2", "strip_offgrid")])
def test_strip_deterministic(gpu, oracle, monkeypatch, nmaps, kernel, name):
    """The int64 fixed point across the seam, and the call repeated: the second call's first
    pass meets the layout of the first call's LAST pass (another window: another key), so no
    pass may reuse it (``layout_reuse`` 0, as test_gpu_layout_reuse.py's
    test_another_key_is_not_reused), and fixed-point maps are bit-identical."""
    import torch
    from asp_amd.device import project2d
    _knobs(monkeypatch, None, vb.STRIP_WIDE_TILES)
    s = vb.strip_set(oracle, kernel, name)
    ref = vb.strip_reference(oracle, kernel, name)
    u, v, h, a, a0 = _dev(s["u"], s["v"], s["h"], s["a"], s["a0"])
    kw = _strip_kw(name, kernel, deterministic=True)
    call = (lambda: project2d(u, v, h, a, **kw)) if nmaps == 1 else \
        (lambda: project2d(u, v, h, a0, a, **kw))
    first, P = _counted(call)
    assert P == 2
    st = _paths_ran(tiles=STRIP_TILES)
    assert st["layout_reuse"] == 0, st
    again, P2 = _counted(call)
    st = _paths_ran(tiles=STRIP_TILES)
    assert P2 == 2 and st["layout_reuse"] == 0, st
    for x, y in zip(first, again):
        assert (x is None and y is None) or torch.equal(x, y)
    if nmaps == 1:
        w = _check(_strip(again[0]), ref, "1", P, True)
    else:
        w = max(_check(_strip(again[0]), ref, "0", P, True),
                _check(_strip(again[1]), ref, "1", P, True))
    _strip_counts_exact(name, s, ref["cnt"], 2, deterministic=True)
    _report(f"strip {name} {kernel} fix {nmaps} map(s)", w, P)


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
@pytest.mark.parametrize("kernel", vb.KERNELS)
def test_strip_ratio(gpu, oracle, monkeypatch, kernel, fused):
    """ratio=True under the ratio rule.  With the wide class on the wide path each window's
    pass forms the quotient in ratio_stage (one launch per window); with
    ASP_WIDE_TILES=1000000 nothing is wide and the deposit's fused quotient runs."""
    from asp_amd.device import project2d
    name = "strip_offgrid"
    _knobs(monkeypatch, None, "1000000" if fused else vb.STRIP_WIDE_TILES)
    s = vb.strip_set(oracle, kernel, name)
    ref = vb.strip_reference(oracle, kernel, name)
    u, v, h, a, a0 = _dev(s["u"], s["v"], s["h"], s["a"], s["a0"])
    (q, g1), P, (nratio,) = _counted(
        lambda: project2d(u, v, h, a0, a, ratio=True, **_strip_kw(name, kernel)), also=("ratio",))
    assert P == 2 and nratio == (0 if fused else 2)
    _paths_ran(wide=not fused, tiles=STRIP_TILES)
    E0, _, _ = _bar(ref, "0", P)
    E1, _, _ = _bar(ref, "1", P)
    w = vb.assert_ratio_close(_strip(q), ref["r0"], ref["r1"], E0, E1)
    w1 = _check(_strip(g1), ref, "1", P)
    _report(f"strip {name} {kernel} ratio {'fused' if fused else 'ratio_stage'}", max(w, w1), P)


@pytest.mark.parametrize("kernel", vb.KERNELS)
def test_strip_props(gpu, oracle, monkeypatch, kernel):
    """k = 6: the two EXT passes of each window write xo[j] + off."""
    from asp_amd.device import project2d_props
    name = "strip_offgrid" if kernel == "cubic" else "strip_grid"
    _knobs(monkeypatch, None, vb.STRIP_WIDE_TILES)
    s = vb.strip_set(oracle, kernel, name)
    ref = vb.strip_reference(oracle, kernel, name)
    props = _mixed_props(s)
    u, v, h = _dev(s["u"], s["v"], s["h"])
    kw = _strip_kw(name, kernel)
    outs, P = _counted(lambda: project2d_props(u, v, h, _dev(*props), **kw), per_pass=3)
    assert P == 2
    _paths_ran(tiles=STRIP_TILES)
    for k, (p, o) in enumerate(zip(props, outs)):
        if k < 2:
            w = _check(_strip(o), ref, "10"[k], P)
        else:
            w = vb.assert_terms_close(_strip(o), *_strip_other(oracle, s, p, kernel, name, P))
        _report(f"strip {name} props {kernel} map {k}", w, P)
    ones = _dev(np.ones(s["h"].size))[0]
    kw["kernel"] = "indicator"
    cnts, Pc = _counted(lambda: project2d_props(u, v, h, [ones] * 6, **kw), per_pass=3)
    assert Pc == 2
    for c in cnts:
        assert np.array_equal(_strip(c), ref["cnt"])


def test_strip_sph(gpu, oracle, monkeypatch):
    """asp_project2d_sph: the oracle on the coefficients fl32(A m / rho), the bar on them."""
    from asp_amd.device import project2d_props
    kernel, name = "cubic", "strip_grid"
    _knobs(monkeypatch, None, vb.STRIP_WIDE_TILES)
    s = vb.strip_set(oracle, kernel, name)
    m, rho = _sph_weights(s["a"].size)
    u, v, h = _dev(s["u"], s["v"], s["h"])
    outs, P = _counted(lambda: project2d_props(u, v, h, _dev(s["a"], s["a0"]), mass=_dev(m)[0],
                                               density=_dev(rho)[0], **_strip_kw(name, kernel)))
    assert P == 2
    _paths_ran(tiles=STRIP_TILES)
    for k, (A, o) in enumerate(zip((s["a"], s["a0"]), outs)):
        w = vb.assert_terms_close(_strip(o), *_strip_other(oracle, s, _sph_product(A, m, rho),
                                                           kernel, name, P))
        _report(f"strip {name} sph {kernel} map {k}", w, P)


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("axis", [2, 0])
def test_strip_raw_f64(gpu, oracle, monkeypatch, axis, where):
    """asp_project2d_f64 on the raw fp64 set: host arrays (the maps staged in the workspace,
    every window writing d0 + off, copied back once) and device tensors."""
    import torch
    from asp_amd.device import project2d_f64
    kernel, name = "wendland_c2", "strip_offgrid"
    _knobs(monkeypatch, None, vb.STRIP_WIDE_TILES)
    s = vb.strip_set(oracle, kernel, name, raw=True)
    ref = vb.strip_reference(oracle, kernel, name, raw=True)
    arrs = [_raw_positions(s, axis)] + [np.array(s[k]) for k in ("h", "a0", "a")]
    ones = np.ones(s["h"].size)
    if where == "device":
        arrs = [torch.tensor(t, dtype=torch.float64, device="cuda") for t in arrs]
        ones = torch.tensor(ones, dtype=torch.float64, device="cuda")
    kw = dict(projection_axis=axis, image_size=vb.STRIP_SIZE, extent=vb.strip_ext(name),
              chunk_size=vb.CHUNK)
    (g0, g1), P = _counted(lambda: project2d_f64(*arrs, kernel=kernel, **kw))
    assert P == 2
    _paths_ran(tiles=STRIP_TILES)
    (c, _), Pc = _counted(lambda: project2d_f64(arrs[0], arrs[1], ones, kernel="indicator", **kw))
    assert Pc == 2 and np.array_equal(_strip(c), ref["cnt"])
    w = max(_check(_strip(g0), ref, "0", P), _check(_strip(g1), ref, "1", P))
    _report(f"strip {name} {kernel} raw f64 axis={axis} {where}", w, P)


def test_strip_props_f64_sph(gpu, oracle, monkeypatch):
    """asp_project2d_sph_f64, k = 3 (one EXT pass per window): the weights formed in fp64 from
    the raw values; the device still rounds h itself (F64_INPUT_ULPS)."""
    from asp_amd.device import project2d_props_f64
    kernel, name = "cubic", "strip_offgrid"
    _knobs(monkeypatch, None, vb.STRIP_WIDE_TILES)
    s = vb.strip_set(oracle, kernel, name, raw=True)
    m, rho = _sph_weights(s["a"].size)
    props = [np.array(s["a"]), np.array(s["a0"]), s["a"] * (s["T"] - 2.0)]
    outs, P = _counted(lambda: project2d_props_f64(
        _raw_positions(s, 2), np.array(s["h"]), props, mass=m, density=rho, projection_axis=2,
        image_size=vb.STRIP_SIZE, extent=vb.strip_ext(name), chunk_size=vb.CHUNK, kernel=kernel),
        per_pass=2)
    assert P == 2
    _paths_ran(tiles=STRIP_TILES)
    for k, (A, o) in enumerate(zip(props, outs)):
        w = vb.assert_terms_close(_strip(o), *_strip_other(
            oracle, s, _sph_product(A, m, rho), kernel, name, P, vb.F64_INPUT_ULPS))
        _report(f"strip {name} sph f64 {kernel} map {k}", w, P)


def _column_strip_reference(oracle, kernel, name, passes):
    """column_ref's set and bar on the strip (as test_gpu_column.py carries them to ``box``):
    the seam set with the column kernel's equal-peak amplitudes, the fp64 restatement of its
    two maps and their bars for ``passes``."""
    def make():
        s = vb.strip_set(cr.W0, kernel, name)
        ext = vb.strip_ext(name)
        r = cr.scatter_f64(s["u"], s["v"], s["h"], np.stack([s["a0"], s["a"]]), vb.STRIP_SIZE,
                           vb.CHUNK, *ext, kernel=kernel)
        ref = dict(r0=vb.strip_crop(r[0]), r1=vb.strip_crop(r[1]))
        for k, a in (("0", s["a0"]), ("1", s["a"])):
            ref["E" + k] = vb.strip_crop(cr.bar2d(oracle, s["u"], s["v"], s["h"], a, kernel,
                                                  vb.STRIP_SIZE, ext,
                                                  extra_ulps=vb.pass_ulps(passes)))
        return ref
    return vb._cached(("column_strip_ref", kernel, name, passes), make)


def test_strip_column(gpu, oracle, monkeypatch):
    from asp_amd.device import project2d
    kernel, name = "cubic_column", "strip_offgrid"
    _knobs(monkeypatch, None, vb.STRIP_WIDE_TILES)
    s = vb.strip_set(cr.W0, kernel, name)
    u, v, h, a, a0 = _dev(s["u"], s["v"], s["h"], s["a"], s["a0"])
    (g0, g1), P = _counted(lambda: project2d(u, v, h, a0, a, **_strip_kw(name, kernel)))
    assert P == 2
    _paths_ran(tiles=STRIP_TILES)
    ref = _column_strip_reference(oracle, kernel, name, P)
    w = max(vb.assert_terms_close(_strip(g0), ref["r0"], ref["E0"]),
            vb.assert_terms_close(_strip(g1), ref["r1"], ref["E1"]))
    _report(f"strip {name} {kernel}", w, P)


def test_strip_rows(gpu, oracle, monkeypatch):
    """rows = (100, nx): the windows start at row 100, so the seam moves to row 100 + 262144
    and every tile frame with it; the same rows of the reference."""
    from asp_amd.device import project2d
    kernel, name, rows = "wendland_c2", "strip_offgrid", (100, NX)
    _knobs(monkeypatch, None, vb.STRIP_WIDE_TILES)
    s = vb.strip_set(oracle, kernel, name)
    ref = vb.strip_reference(oracle, kernel, name)
    u, v, h, a, a0 = _dev(s["u"], s["v"], s["h"], s["a"], s["a0"])
    (g0, g1), P = _counted(lambda: project2d(u, v, h, a0, a, rows=rows, **_strip_kw(name, kernel)))
    assert P == 2
    _paths_ran(tiles=(NX - 100 + 63) // 64)
    _strip_counts_exact(name, s, ref["cnt"], 2, rows=rows)
    w = max(_check(_strip(g0, rows[0]), ref, "0", P), _check(_strip(g1, rows[0]), ref, "1", P))
    _report(f"strip {name} {kernel} rows={rows}", w, P)


@pytest.mark.parametrize("name", vb.STRIP_NAMES)
@pytest.mark.parametrize("kernel", vb.KERNELS)
def test_strip_stamps(gpu, oracle, monkeypatch, kernel, name):
    """One particle per map against W(r, h) in fp64 NumPy: h = 100 px exactly on (seam, 8)
    -- wide in both windows -- and h = 3 px half a pitch below the seam, one record in each."""
    from asp_amd.device import project2d, stats
    _knobs(monkeypatch, None, vb.STRIP_WIDE_TILES)
    ext = vb.strip_ext(name)
    psx, psy = (ext[1] - ext[0]) / NX, (ext[3] - ext[2]) / NX
    for label, h_px, lu, wide in (("h100 on the seam", 100.0, float(vb.STRIP_SEAM), True),
                                  ("h3 below the seam", 3.0, vb.STRIP_SEAM - 0.5, False)):
        h = float(vb.f32(h_px * max(psx, psy)))
        u, v = float(vb.f32(ext[0] + lu * psx)), float(vb.f32(ext[2] + 8.0 * psy))
        a = float(vb.f32(1.25 / vb.w0(oracle, kernel, h)[0]))
        r, E = vb.stamp_reference(oracle, kernel, u, v, h, a, vb.STRIP_SIZE, ext)
        r, E = vb.strip_crop(r), vb.strip_crop(E)
        k = vb.STRIP_SEAM - vb.STRIP_LO
        assert r[k - 1].any() and r[k].any()
        (g, _), P = _counted(lambda: project2d(*_dev([u], [v], [h], [a]), **_strip_kw(name, kernel)))
        st = stats(0)
        assert P == 2 and st["tiles"] == STRIP_TILES, st
        assert (st["wide"], st["records"]) == ((2, 0) if wide else (0, 2)), st
        c, _ = project2d(*_dev([u], [v], [h], [1.0]), **_strip_kw(name, "indicator"))
        assert np.array_equal(_strip(c), (r != 0).astype(np.float64))
        S = np.where(E > 0, a * vb.w0(oracle, kernel, h)[0], 0.0)  # the one particle's peak
        w = vb.assert_terms_close(_strip(g), r, vb.with_passes(E, S, P), {label: E})
        _report(f"strip {name} stamp {kernel} {label}", w, P)


# ================================================== batches on the 256^2 mixed set
def _mixed_kw(kernel, **more):
    return dict(image_size=vb.SIZE2D, extent=vb.EXT2D, chunk_size=vb.CHUNK, kernel=kernel, **more)


def _batched(monkeypatch, mode, call, n, per_pass=1, stage="deposit", batch=BATCH):
    """``call`` in batches: (call(), P).  ``batch``: ASP_MAX_BATCH = BATCH, P = ceil(n / BATCH).
    ``records``: ASP_MAX_RECORDS at a third of the records of the same call unbatched, so
    for_batches halves the array until every pass fits; not below 5, since one particle makes
    at most 4 records here (one that meets more than ASP_WIDE_TILES = 4 tiles is wide and makes
    none) and a batch of one particle must fit.  The unbatched call's layout is released: a
    pass that reuses a layout does not count, so it never meets the record limit, and the
    limit -- a constant outside the tests -- is no part of the layout's key.  The knob is
    unset again before returning."""
    from asp_amd import _lib
    from asp_amd.device import stats
    if mode == "batch":
        knob, value = "ASP_MAX_BATCH", batch
    else:
        call()
        knob, value = "ASP_MAX_RECORDS", str(max(stats(0)["records"] // 3, 5))
        _lib.check(_lib.lib().asp_release(0))
    monkeypatch.setenv(knob, value)
    try:
        out, P = _counted(call, per_pass, stage)
    finally:
        monkeypatch.delenv(knob)
    if mode == "batch":
        assert P == -(-n // int(batch)), (P, n)
    assert P >= 2
    return out, P


def _mixed_counts_exact(monkeypatch, mode, s, cnt, **kw):
    from asp_amd.device import project2d
    u, v, h = _dev(s["u"], s["v"], s["h"])
    ones = _dev(np.ones(s["h"].size))[0]
    (c, _), _ = _batched(monkeypatch, mode,
                         lambda: project2d(u, v, h, ones, **_mixed_kw("indicator", **kw)),
                         s["h"].size)
    assert np.array_equal(_host(c), cnt), "neighbour counts differ from the oracle"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("deterministic", [False, True], ids=["fp64", "deterministic"])
@pytest.mark.parametrize("kernel", vb.KERNELS)
def test_batched_maps(gpu, oracle, monkeypatch, kernel, deterministic, mode):
    from asp_amd.device import project2d
    _knobs(monkeypatch, None, vb.WIDE_TILES)
    s = vb.mixed_set(oracle, kernel)
    ref = vb.reference2d(oracle, kernel)
    n = s["h"].size
    u, v, h, a, a0 = _dev(s["u"], s["v"], s["h"], s["a"], s["a0"])
    kw = _mixed_kw(kernel, deterministic=deterministic)
    label = f"batched {mode} {kernel} {'fix' if deterministic else 'f64'}"
    (g, _), P = _batched(monkeypatch, mode, lambda: project2d(u, v, h, a, **kw), n)
    _paths_ran()
    _report(label + " one map", _check(_host(g), ref, "1", P, deterministic), P)
    (g0, g1), P = _batched(monkeypatch, mode, lambda: project2d(u, v, h, a0, a, **kw), n)
    _paths_ran()
    w = max(_check(_host(g0), ref, "0", P, deterministic),
            _check(_host(g1), ref, "1", P, deterministic))
    _report(label + " two maps", w, P)
    _mixed_counts_exact(monkeypatch, mode, s, ref["cnt"], deterministic=deterministic)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kernel", vb.KERNELS)
def test_batched_ratio(gpu, oracle, monkeypatch, kernel, mode):
    """The quotient of a batched call is formed once, after the last pass (ratio_stage)."""
    from asp_amd.device import project2d
    _knobs(monkeypatch, None, vb.WIDE_TILES)
    s = vb.mixed_set(oracle, kernel)
    ref = vb.reference2d(oracle, kernel)
    u, v, h, a, a0 = _dev(s["u"], s["v"], s["h"], s["a"], s["a0"])
    (q, g1), P = _batched(monkeypatch, mode,
                          lambda: project2d(u, v, h, a0, a, ratio=True, **_mixed_kw(kernel)),
                          s["h"].size)
    _paths_ran()
    E0, _, _ = _bar(ref, "0", P)
    E1, _, _ = _bar(ref, "1", P)
    w = max(vb.assert_ratio_close(_host(q), ref["r0"], ref["r1"], E0, E1),
            _check(_host(g1), ref, "1", P))
    _report(f"batched {mode} {kernel} ratio", w, P)


@pytest.mark.parametrize("mode", MODES)
def test_batched_accumulate(gpu, oracle, monkeypatch, mode):
    """A caller's accumulate=True: the first pass adds to the caller's map as well, so the
    pass rule counts P + 1.  The pre-fill is fl32(c r), c = U(0, 1/8), where the reference is
    not 0 -- every stored partial sum then stays within 9/8 of the sum the rule multiplies,
    and 3 P / 8 <= 3 ulps at P <= 8 is inside the extra pass -- and 1 where it is 0: E is 0
    there, and those pixels must come back unchanged."""
    import torch
    from asp_amd.device import project2d
    kernel = "wendland_c2"
    _knobs(monkeypatch, None, vb.WIDE_TILES)
    s = vb.mixed_set(oracle, kernel)
    ref = vb.reference2d(oracle, kernel)
    rng = np.random.default_rng(26)
    pre = [np.where(ref["r" + k] != 0, vb.f32(ref["r" + k] * rng.uniform(0.0, 0.125, vb.SIZE2D)),
                    1.0) for k in "01"]
    u, v, h, a, a0 = _dev(s["u"], s["v"], s["h"], s["a"], s["a0"])

    def call():
        o0, o1 = (torch.tensor(p, dtype=torch.float32, device="cuda") for p in pre)
        return project2d(u, v, h, a0, a, accumulate=True, out0=o0, out1=o1, **_mixed_kw(kernel))

    (g0, g1), P = _batched(monkeypatch, mode, call, s["h"].size)
    _paths_ran()
    w = 0.0
    for k, g in (("0", g0), ("1", g1)):
        E, by_class, _ = _bar(ref, k, P + 1)
        w = max(w, vb.assert_terms_close(_host(g), ref["r" + k] + pre[int(k)], E, by_class))
    _report(f"batched {mode} {kernel} accumulate", w, P)


@pytest.mark.parametrize("mode", MODES)
def test_batched_props(gpu, oracle, monkeypatch, mode):
    from asp_amd.device import project2d_props
    kernel = "cubic"
    _knobs(monkeypatch, None, vb.WIDE_TILES)
    s = vb.mixed_set(oracle, kernel)
    ref = vb.reference2d(oracle, kernel)
    n = s["h"].size
    props = _mixed_props(s)
    u, v, h = _dev(s["u"], s["v"], s["h"])
    dprops = _dev(*props)
    outs, P = _batched(monkeypatch, mode,
                       lambda: project2d_props(u, v, h, dprops, **_mixed_kw(kernel)), n, per_pass=3)
    _paths_ran()
    for k, (p, o) in enumerate(zip(props, outs)):
        if k < 2:
            w = _check(_host(o), ref, "10"[k], P)
        else:
            r, _ = oracle.project_scatter(s["u"], s["v"], s["h"], p, None, vb.SIZE2D, vb.CHUNK,
                                          *vb.EXT2D, kernel=kernel)
            E, by_class = vb.bar2d(oracle, s, p, kernel, extra_ulps=vb.pass_ulps(P))
            w = vb.assert_terms_close(_host(o), r, E, by_class)
        _report(f"batched {mode} props {kernel} map {k}", w, P)
    ones = _dev(np.ones(n))[0]
    cnts, _ = _batched(monkeypatch, mode,
                       lambda: project2d_props(u, v, h, [ones] * 6, **_mixed_kw("indicator")), n,
                       per_pass=3)
    for c in cnts:
        assert np.array_equal(_host(c), ref["cnt"])


@pytest.mark.parametrize("mode", MODES)
def test_batched_sph(gpu, oracle, monkeypatch, mode):
    from asp_amd.device import project2d_props
    kernel = "wendland_c2"
    _knobs(monkeypatch, None, vb.WIDE_TILES)
    s = vb.mixed_set(oracle, kernel)
    n = s["h"].size
    m, rho = _sph_weights(n)
    u, v, h = _dev(s["u"], s["v"], s["h"])
    dp, dm, dr = _dev(s["a"], s["a0"]), _dev(m)[0], _dev(rho)[0]
    outs, P = _batched(monkeypatch, mode, lambda: project2d_props(
        u, v, h, dp, mass=dm, density=dr, **_mixed_kw(kernel)), n)
    _paths_ran()
    for k, (A, o) in enumerate(zip((s["a"], s["a0"]), outs)):
        p = _sph_product(A, m, rho)
        r, _ = oracle.project_scatter(s["u"], s["v"], s["h"], p, None, vb.SIZE2D, vb.CHUNK,
                                      *vb.EXT2D, kernel=kernel)
        E, by_class = vb.bar2d(oracle, s, p, kernel, extra_ulps=vb.pass_ulps(P))
        _report(f"batched {mode} sph {kernel} map {k}",
                vb.assert_terms_close(_host(o), r, E, by_class), P)
    ones = _dev(np.ones(n))[0]
    (c,), _ = _batched(monkeypatch, mode, lambda: project2d_props(
        u, v, h, [ones], mass=ones, density=ones, **_mixed_kw("indicator")), n)
    assert np.array_equal(_host(c), vb.reference2d(oracle, kernel)["cnt"])


@pytest.mark.parametrize("mode", MODES)
def test_batched_raw_f64(gpu, oracle, monkeypatch, mode):
    """asp_project2d_f64, axis 0: src_from offsets the stride-3 position columns by the batch
    start; asp_project2d_props_f64 the same with an EXT pass."""
    from asp_amd.device import project2d_f64, project2d_props_f64
    kernel = "cubic"
    _knobs(monkeypatch, None, vb.WIDE_TILES)
    s = vb.mixed_set(oracle, kernel, None, True)
    ref = vb.reference2d(oracle, kernel, raw=True)
    n = s["h"].size
    pos = _raw_positions(s, 0)
    h, a, a0 = (np.array(s[k]) for k in ("h", "a", "a0"))
    kw = dict(projection_axis=0, image_size=vb.SIZE2D, extent=vb.EXT2D, chunk_size=vb.CHUNK)
    (g0, g1), P = _batched(monkeypatch, mode,
                           lambda: project2d_f64(pos, h, a0, a, kernel=kernel, **kw), n)
    _paths_ran()
    w = max(_check(g0, ref, "0", P), _check(g1, ref, "1", P))
    _report(f"batched {mode} {kernel} raw f64 axis=0", w, P)
    (c, _), _ = _batched(monkeypatch, mode,
                         lambda: project2d_f64(pos, h, np.ones(n), kernel="indicator", **kw), n)
    assert np.array_equal(np.asarray(c, np.float64), ref["cnt"])
    props = [a, a0, s["a"] * (s["T"] - 2.0)]
    outs, P = _batched(monkeypatch, mode,
                       lambda: project2d_props_f64(pos, h, props, kernel=kernel, **kw), n,
                       per_pass=2)
    _paths_ran()
    for k, (p, o) in enumerate(zip(props, outs)):
        if k < 2:
            w = _check(_host(o), ref, "10"[k], P)
        else:
            r, _ = oracle.project_scatter(s["u"], s["v"], s["h"], p, None, vb.SIZE2D, vb.CHUNK,
                                          *vb.EXT2D, kernel=kernel)
            E, by_class = vb.bar2d(oracle, s, p, kernel,
                                   extra_ulps=vb.F64_INPUT_ULPS + vb.pass_ulps(P))
            w = vb.assert_terms_close(_host(o), r, E, by_class)
        _report(f"batched {mode} props f64 {kernel} map {k}", w, P)
    cnts, _ = _batched(monkeypatch, mode, lambda: project2d_props_f64(
        pos, h, [np.ones(n), np.ones(n), np.ones(n)], kernel="indicator", **kw), n, per_pass=2)
    for c in cnts:
        assert np.array_equal(_host(c), ref["cnt"])


@pytest.mark.parametrize("mode", MODES)
def test_batched_rows(gpu, oracle, monkeypatch, mode):
    from asp_amd.device import project2d
    kernel, rows = "wendland_c2", (64, 192)
    _knobs(monkeypatch, None, vb.WIDE_TILES)
    s = vb.mixed_set(oracle, kernel)
    ref = vb.reference2d(oracle, kernel)
    u, v, h, a, a0 = _dev(s["u"], s["v"], s["h"], s["a"], s["a0"])
    (g0, g1), P = _batched(monkeypatch, mode,
                           lambda: project2d(u, v, h, a0, a, rows=rows, **_mixed_kw(kernel)),
                           s["h"].size)
    _paths_ran()
    cut = lambda m: m[rows[0]:rows[1]]  # noqa: E731
    w = max(_check(_host(g0), ref, "0", P, cut=cut), _check(_host(g1), ref, "1", P, cut=cut))
    _report(f"batched {mode} {kernel} rows={rows}", w, P)
    _mixed_counts_exact(monkeypatch, mode, s, cut(ref["cnt"]), rows=rows)


@pytest.mark.parametrize("mode", MODES)
def test_batched_column(gpu, oracle, monkeypatch, mode):
    from asp_amd.device import project2d
    kernel = "cubic_column"
    _knobs(monkeypatch, None, vb.WIDE_TILES)
    s = cr.mixed_set(kernel)
    r = vb._cached(("column_mixed_ref", kernel), lambda: cr.scatter_f64(
        s["u"], s["v"], s["h"], np.stack([s["a0"], s["a"]]), vb.SIZE2D, vb.CHUNK, *vb.EXT2D,
        kernel=kernel))
    u, v, h, a, a0 = _dev(s["u"], s["v"], s["h"], s["a"], s["a0"])
    (g0, g1), P = _batched(monkeypatch, mode,
                           lambda: project2d(u, v, h, a0, a, **_mixed_kw(kernel)), s["h"].size)
    _paths_ran()
    w = max(vb.assert_terms_close(_host(g), rk, cr.bar2d(oracle, s["u"], s["v"], s["h"], ak,
                                                        kernel, extra_ulps=vb.pass_ulps(P)))
            for g, rk, ak in ((g0, r[0], s["a0"]), (g1, r[1], s["a"])))
    _report(f"batched {mode} {kernel}", w, P)
    cnt = vb.reference2d(oracle, "cubic")["cnt"]  # (the same positions and h)
    _mixed_counts_exact(monkeypatch, mode, s, cnt)


@pytest.mark.parametrize("kernel", vb.KERNELS)
def test_batched_cube(gpu, oracle, monkeypatch, kernel):
    """asp_project3d's batch loop: bar3d with the pass rule, voxel counts exact."""
    from asp_amd.device import project3d
    s = vb.cube_set(oracle, kernel)
    ref = vb.reference3d(oracle, kernel)
    n = s["h"].size
    x, y, z, h, a = _dev(s["x"], s["y"], s["z"], s["h"], s["a"])
    kw = dict(cube_size=vb.SIZE3D, extent=vb.EXT3D)
    g, P = _batched(monkeypatch, "batch", lambda: project3d(x, y, z, h, a, kernel=kernel, **kw), n,
                    stage="cube_deposit", batch=CUBE_BATCH)
    assert P == 4
    w = vb.assert_terms_close(_host(g), ref["r"], vb.with_passes(ref["E"], ref["S"], P),
                              ref["by_class"])
    _report(f"batched cube {kernel}", w, P)
    ones = _dev(np.ones(n))[0]
    c, _ = _batched(monkeypatch, "batch",
                    lambda: project3d(x, y, z, h, ones, kernel="indicator", **kw), n,
                    stage="cube_deposit", batch=CUBE_BATCH)
    want = oracle.project3d(s["x"], s["y"], s["z"], s["h"], np.ones(n), vb.SIZE3D, vb.EXT3D,
                            kernel="indicator")
    assert np.array_equal(_host(c), want)


# ============================================================== windows x batches
def test_strip_batched_two_maps(gpu, oracle, monkeypatch):
    from asp_amd.device import project2d
    kernel, name = "cubic", "strip_offgrid"
    _knobs(monkeypatch, None, vb.STRIP_WIDE_TILES)
    s = vb.strip_set(oracle, kernel, name)
    ref = vb.strip_reference(oracle, kernel, name)
    u, v, h, a, a0 = _dev(s["u"], s["v"], s["h"], s["a"], s["a0"])
    monkeypatch.setenv("ASP_MAX_BATCH", STRIP_BATCH)
    (g0, g1), P = _counted(lambda: project2d(u, v, h, a0, a, **_strip_kw(name, kernel)))
    assert P == 2 * -(-s["h"].size // int(STRIP_BATCH)) == 4
    _paths_ran(tiles=STRIP_TILES)
    _strip_counts_exact(name, s, ref["cnt"], P)
    w = max(_check(_strip(g0), ref, "0", P), _check(_strip(g1), ref, "1", P))
    _report(f"strip {name} {kernel} f64 batched two maps", w, P)


def test_strip_batched_props(gpu, oracle, monkeypatch):
    from asp_amd.device import project2d_props
    kernel, name = "wendland_c2", "strip_offgrid"
    _knobs(monkeypatch, None, vb.STRIP_WIDE_TILES)
    s = vb.strip_set(oracle, kernel, name)
    ref = vb.strip_reference(oracle, kernel, name)
    props = _mixed_props(s)
    u, v, h = _dev(s["u"], s["v"], s["h"])
    monkeypatch.setenv("ASP_MAX_BATCH", STRIP_BATCH)
    outs, P = _counted(lambda: project2d_props(u, v, h, _dev(*props), **_strip_kw(name, kernel)),
                       per_pass=3)
    assert P == 4
    _paths_ran(tiles=STRIP_TILES)
    for k, (p, o) in enumerate(zip(props, outs)):
        if k < 2:
            w = _check(_strip(o), ref, "10"[k], P)
        else:
            w = vb.assert_terms_close(_strip(o), *_strip_other(oracle, s, p, kernel, name, P))
        _report(f"strip {name} props {kernel} batched map {k}", w, P)


def test_strip_batched_deterministic_repeats(gpu, oracle, monkeypatch):
    """Layout reuse across a multi-pass call: every pass of the repeated call meets another
    pass's layout (another window, another batch), none may take it."""
    import torch
    from asp_amd.device import project2d
    kernel, name = "wendland_c2", "strip_grid"
    _knobs(monkeypatch, None, vb.STRIP_WIDE_TILES)
    s = vb.strip_set(oracle, kernel, name)
    ref = vb.strip_reference(oracle, kernel, name)
    u, v, h, a, a0 = _dev(s["u"], s["v"], s["h"], s["a"], s["a0"])
    monkeypatch.setenv("ASP_MAX_BATCH", STRIP_BATCH)
    call = lambda: project2d(u, v, h, a0, a, **_strip_kw(name, kernel, deterministic=True))  # noqa: E731
    first, P = _counted(call)
    st = _paths_ran(tiles=STRIP_TILES)
    assert P == 4 and st["layout_reuse"] == 0, st
    again, P2 = _counted(call)
    st = _paths_ran(tiles=STRIP_TILES)
    assert P2 == 4 and st["layout_reuse"] == 0, st
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    w = max(_check(_strip(again[0]), ref, "0", P, True), _check(_strip(again[1]), ref, "1", P, True))
    _report(f"strip {name} {kernel} fix batched, repeated", w, P)
