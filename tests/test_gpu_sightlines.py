"""Sightline sampling on the GPU: asp_sample2d, asp_sample2d_f64 and
asp_amd.sightline_columns.

The contract (include/asp.h) is calculate_pixel_value at arbitrary points.  On the pixel
lattice that is the map, so the references there are the oracle's maps and the maps' own
per-pixel bar (tests/value_bar.py, tests/column_ref.py); off the lattice the reference is
the fp64 brute force of tests/sightline_ref.py (tied to the oracle on the lattice by
tests/test_sightline_ref.py) and the SAME bar, e_p summed over each point's exact
neighbour set -- no new constants.  Neighbour counts are exact everywhere.

Every class of the deposit (a lane per particle / the wave per particle) and several grids
are forced with ASP_SAMPLE_WIDE_CELLS and ASP_SAMPLE_CELLS.  Every case prints its worst
err/E (``pytest -s``).
"""
import numpy as np
import pytest

import column_ref as cr
import sightline_ref as sr
import value_bar as vb
from test_sightline_ref import lattice

pytestmark = pytest.mark.gpu

BIG = str(1 << 30)
# ASP_SAMPLE_CELLS, ASP_SAMPLE_WIDE_CELLS (and ASP_SAMPLE_WIDE_POINTS with it): one cell /
# 7 x 7 / the default grid, every particle taken by the wave (0) or by its lane (2^30), or
# split by the default thresholds
SETTINGS = {"default": (None, None), "cells1_wave": ("1", "0"), "cells1_lane": ("1", BIG),
            "cells7_wave": ("7", "0"), "cells7_lane": ("7", BIG), "default_wave": (None, "0"),
            "default_lane": (None, BIG), "default_crowded": (None, BIG, "8")}
ALL_KERNELS = vb.KERNELS + cr.KERNELS


def _knobs(monkeypatch, setting="default"):
    cells, wide, points = (SETTINGS[setting] + (None,))[:3]
    points = points or wide  # the lane settings raise both thresholds
    for name, val in (("ASP_SAMPLE_CELLS", cells), ("ASP_SAMPLE_WIDE_CELLS", wide),
                      ("ASP_SAMPLE_WIDE_POINTS", points),
                      ("ASP_MAX_BATCH", None), ("ASP_SAMPLE_COUNT", None)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)


def _report(label, worst):
    print(f"SIGHTLINE_BAR {label}: worst err/E = {worst:.3f}")


def _f32(x):
    return None if x is None else np.ascontiguousarray(x, np.float32)


def _f64(x):
    return None if x is None else np.ascontiguousarray(x, np.float64)


def _outs(m, second, out0, out1):
    if out0 is None:
        out0 = np.full(m, np.nan, np.float32)
    if second and out1 is None:
        out1 = np.full(m, np.nan, np.float32)
    return out0, out1


def sample(u, v, h, a0, px, py, kernel, a1=None, flags=0, out0=None, out1=None):
    """asp_sample2d on host arrays; returns (out0, out1) as float64."""
    from asp_amd import _lib
    u, v, h, a0, a1 = (_f32(x) for x in (u, v, h, a0, a1))
    px, py = _f64(px), _f64(py)
    out0, out1 = _outs(px.size, a1 is not None, out0, out1)
    P, D = _lib.ptr, (lambda x: _lib.ptr(x, _lib._d))
    _lib.check(_lib.lib().asp_sample2d(P(u), P(v), P(h), P(a0), P(a1), u.size, D(px), D(py), px.size,
                                       sr.KERNEL_IDS[kernel], flags, P(out0), P(out1), 0, None))
    return out0.astype(np.float64), None if out1 is None else out1.astype(np.float64)


def sample64(pos, h, a0, px, py, kernel, axis=2, a1=None, flags=0):
    """asp_sample2d_f64 on host arrays."""
    from asp_amd import _lib
    pos, h, a0, a1, px, py = (_f64(x) for x in (pos, h, a0, a1, px, py))
    out0, out1 = _outs(px.size, a1 is not None, None, None)
    P, D = _lib.ptr, (lambda x: _lib.ptr(x, _lib._d))
    _lib.check(_lib.lib().asp_sample2d_f64(D(pos), D(h), D(a0), D(a1), h.size, axis, D(px), D(py),
                                           px.size, sr.KERNEL_IDS[kernel], flags, P(out0), P(out1),
                                           0, None))
    return out0.astype(np.float64), None if out1 is None else out1.astype(np.float64)


def mixed(oracle, kernel, window=None, raw=False):
    return cr.mixed_set(kernel, window, raw) if kernel in cr.KERNELS else \
        vb.mixed_set(oracle, kernel, window, raw)


def w0(oracle, kernel, h):
    return cr.w0(kernel, h) if kernel in cr.KERNELS else vb.w0(oracle, kernel, h)


# ------------------------------------------------------------ 1. parity on the lattice
def lattice_reference(oracle, kernel):
    """r0 / r1 / E0 / E1 of the mixed set at the 65 536 pixel corners (the maps' shared
    references) and the neighbour counts."""
    if kernel in cr.KERNELS:
        from test_gpu_column import _reference
        ref = _reference(oracle, kernel)
        cnt = vb.reference2d(oracle, cr.BASE[kernel])["cnt"]  # the same positions and h
    else:
        ref = vb.reference2d(oracle, kernel)
        cnt = ref["cnt"]
    return ref, cnt


def shuffled_lattice():
    px, py = lattice()
    perm = np.random.default_rng(41).permutation(px.size)
    return px[perm], py[perm], perm


def unshuffle(g, perm):
    out = np.empty_like(g)
    out[perm] = g
    return out.reshape(vb.SIZE2D)


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("kernel", ALL_KERNELS)
def test_lattice_parity(gpu, oracle, monkeypatch, kernel, setting):
    """The grid corners in a shuffled order: the oracle's maps under the maps' bar, and the
    indicator's counts exactly, for every grid and deposit class."""
    _knobs(monkeypatch, setting)
    s = mixed(oracle, kernel)
    ref, cnt = lattice_reference(oracle, kernel)
    px, py, perm = shuffled_lattice()
    g0, g1 = sample(s["u"], s["v"], s["h"], s["a0"], px, py, kernel, a1=s["a"])
    w = max(vb.assert_terms_close(unshuffle(g0, perm), ref["r0"], ref["E0"]),
            vb.assert_terms_close(unshuffle(g1, perm), ref["r1"], ref["E1"]))
    _report(f"lattice {kernel} {setting}", w)
    c, _ = sample(s["u"], s["v"], s["h"], np.ones(s["h"].size), px, py, "indicator")
    assert np.array_equal(unshuffle(c, perm), cnt)


def test_pair_counter_and_stage_timing(gpu, oracle, monkeypatch):
    """ASP_SAMPLE_COUNT: stats[9] = pairs tested, the map counters 0; the two new profile
    stages record launches."""
    from asp_amd import _lib
    _knobs(monkeypatch)
    monkeypatch.setenv("ASP_SAMPLE_COUNT", "1")
    s = mixed(oracle, "cubic")
    _, cnt = lattice_reference(oracle, "cubic")
    px, py, _ = shuffled_lattice()
    _lib.profile(0, True)
    sample(s["u"], s["v"], s["h"], s["a"], px, py, "cubic")
    prof = _lib.profile_read(0)
    _lib.profile(0, False)
    st = _lib.last_stats(0)
    assert cnt.sum() <= st["evals"] < px.size * s["h"].size, st
    assert all(st[k] == 0 for k in st if k != "evals"), st
    assert prof["sample_prep"][1] == 1 and prof["sample_deposit"][1] >= 2, prof
    monkeypatch.setenv("ASP_SAMPLE_CELLS", "1")  # one cell: every admitted particle, every point
    sample(s["u"], s["v"], s["h"], s["a"], px, py, "cubic")
    assert _lib.last_stats(0)["evals"] == px.size * s["h"].size


ODD = dict(  # appended to a small ordinary set; (u, v, h, a)
    h_zero=(0.1, 0.1, 0.0, 1.0), h_nan=(0.2, 0.1, np.nan, 1.0), h_inf=(0.3, 0.1, np.inf, 1.0),
    h_overflows_fp32=(0.3, 0.2, 3.0e38, 1.0), u_nan=(np.nan, 0.1, 0.05, 1.0),
    v_inf=(0.1, np.inf, 0.05, 1.0), h_negative=(0.1, 0.2, -0.05, 1.0),
    a_nan=(-0.5, -0.5, 0.02, np.nan))


@pytest.mark.parametrize("kernel", vb.KERNELS)
def test_odd_values_are_the_maps(gpu, oracle, monkeypatch, kernel):
    """The odd-value pin: particles with h <= 0, non-finite fields or a NaN amplitude get from
    asp_sample2d at a pixel corner what asp_project2d gives that pixel (one chunk, so the
    chunk cull lets the negative-h disc through): the same neighbour counts exactly, NaN at
    the disc's corners, values within the two results' bars of each other."""
    from asp_amd.device import project2d
    from test_gpu_path_values import _dev, _host
    _knobs(monkeypatch)
    rng = np.random.default_rng(43)
    n = 300
    u = np.concatenate([rng.uniform(-1, 1, n), [o[0] for o in ODD.values()]])
    v = np.concatenate([rng.uniform(-1, 1, n), [o[1] for o in ODD.values()]])
    h = np.concatenate([rng.uniform(1.0, 6.0, n) * vb.PITCH2D, [o[2] for o in ODD.values()]])
    a = np.concatenate([rng.uniform(0.5, 1.5, n), [o[3] for o in ODD.values()]])
    u, v, h, a = (vb.f32(t) for t in (u, v, h, a))
    kw = dict(image_size=vb.SIZE2D, extent=vb.EXT2D, chunk_size=vb.SIZE2D[0])
    tu, tv, th, ta, one = _dev(u, v, h, a, np.ones(h.size))
    m_val = _host(project2d(tu, tv, th, ta, kernel=kernel, **kw)[0]).ravel()
    m_cnt = _host(project2d(tu, tv, th, one, kernel="indicator", **kw)[0]).ravel()
    px, py = lattice()
    g_val, _ = sample(u, v, h, a, px, py, kernel)
    g_cnt, _ = sample(u, v, h, np.ones(h.size), px, py, "indicator")
    assert np.array_equal(g_cnt, m_cnt)
    # the negative-h disc is in both (pi 12.8^2 corners), the others in neither
    ordinary = np.isfinite(h) & (h > 0) & (h < 1e30) & np.isfinite(u) & np.isfinite(v)
    (want,), _ = sr.brute(u[ordinary], v[ordinary], h[ordinary], px, py,
                          [(np.ones(ordinary.sum()), None)])
    extra = g_cnt - want
    assert set(np.unique(extra)) == {0.0, 1.0} and 450 < extra.sum() < 560
    # the NaN amplitude: NaN at exactly the corners inside that particle's disc (pi 5.12^2 of
    # them).  The map's NaN set contains it -- its edge-continuous forms multiply the
    # coefficient by f(q) = 0 over the rest of the particle's candidate box, NaN as well.
    k = h.size - 1
    _, in_disc = sr.brute(u[k:], v[k:], h[k:], px, py, [(np.ones(1), None)])
    nan = np.isnan(g_val)
    assert np.array_equal(nan, in_disc == 1) and 60 < nan.sum() < 105
    assert np.all(np.isnan(m_val)[nan])
    nan = np.isnan(m_val)
    # both are within E of the exact sum: within 2 E of each other
    (E,), _ = sr.brute(u, v, np.where(h < 1e30, h, np.nan), px, py,
                       [(sr.term_bound(oracle, kernel, h, a, vb.PITCH2D), None)])
    # ... outside the negative-h disc: there the counts agree (above) but the values are no
    # physical quantity (q = r / h < 0 in the kernel's polynomial) and the map's own deposit
    # paths do not form them alike (the gathered path gave -2e-6 where the scalar form, which
    # asp_sample2d uses, gives +2.8e4), so there is no map value to pin
    ok = ~nan & (extra == 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(ok & (g_val != m_val), np.abs(g_val - m_val) / (2.0 * E), 0.0)
    k = int(np.argmax(ratio))
    print(f"ODD {kernel}: worst |sample - map| / 2E = {ratio[k]:.3g} at corner {k} "
          f"(sample {g_val[k]:.9g}, map {m_val[k]:.9g}, E {E[k]:.3g}, neighbours {g_cnt[k]:.0f}, "
          f"in the negative-h disc: {bool(extra[k])}); {np.count_nonzero(ratio > 1)} over")
    assert np.all(np.abs(g_val[ok] - m_val[ok]) <= 2.0 * E[ok])
    empty = g_cnt == 0  # (a pair at the very edge may give a term of 0 in one form only)
    assert np.all(g_val[empty] == 0) and np.all(m_val[empty & ~nan] == 0) and empty.sum() > 1000


# ------------------------------------------------------------------ 2. off the lattice
def offlattice_case(oracle, kernel):
    """The mixed set plus the strict-inequality particle, and 3 001 random points in +-1.1
    (some outside every footprint), 1 000 copies of one point inside the clump, points
    exactly on particle positions, and the pair x = 0.5 / nextafter(0.5, 0) for the
    particle at u = 0 with h = 0.25 (alone at v = 5)."""
    s = mixed(oracle, kernel)
    u, v, h = (np.append(s[k], x) for k, x in (("u", 0.0), ("v", 5.0), ("h", 0.25)))
    a = np.append(s["a"], vb.f32(1.0 / w0(oracle, kernel, 0.25))[0])
    a0 = np.append(s["a0"], a[-1])
    rng = np.random.default_rng(44)
    px = np.concatenate([rng.uniform(-1.1, 1.1, 3001), np.full(1000, vb.CLUMP_CENTRE[0] + 1e-3),
                         s["u"][::97], [0.5, np.nextafter(0.5, 0.0)]])
    py = np.concatenate([rng.uniform(-1.1, 1.1, 3001), np.full(1000, vb.CLUMP_CENTRE[1] - 2e-3),
                         s["v"][::97], [5.0, 5.0]])
    return dict(u=u, v=v, h=h, a=a, a0=a0, px=px, py=py)


_off = {}


def offlattice_reference(oracle, kernel):
    if kernel not in _off:
        c = offlattice_case(oracle, kernel)
        (r0, r1), (E0, E1), cnt = sr.reference(oracle, kernel, c["u"], c["v"], c["h"],
                                               [c["a0"], c["a"]], c["px"], c["py"])
        c.update(r0=r0, r1=r1, E0=E0, E1=E1, cnt=cnt,
                 F0=sr.fixed_point_term(oracle, kernel, c["h"], c["a0"]),
                 F1=sr.fixed_point_term(oracle, kernel, c["h"], c["a"]))
        for x in c.values():
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
        _off[kernel] = c
    return _off[kernel]


@pytest.mark.parametrize("setting", ["default", "cells7_wave", "cells7_lane", "cells1_wave",
                                     "default_crowded"])
@pytest.mark.parametrize("kernel", ALL_KERNELS)
def test_off_lattice(gpu, oracle, monkeypatch, kernel, setting):
    _knobs(monkeypatch, setting)
    c = offlattice_reference(oracle, kernel)
    assert c["cnt"][-2:].tolist() == [0, 1]                 # r2 == (2h)^2 is excluded
    assert c["cnt"][3001:4001].min() > 300                   # the contended point
    g0, g1 = sample(c["u"], c["v"], c["h"], c["a0"], c["px"], c["py"], kernel, a1=c["a"])
    w = max(vb.assert_terms_close(g0, c["r0"], c["E0"]), vb.assert_terms_close(g1, c["r1"], c["E1"]))
    _report(f"off-lattice {kernel} {setting}", w)
    cnt, _ = sample(c["u"], c["v"], c["h"], np.ones(c["h"].size), c["px"], c["py"], "indicator")
    assert np.array_equal(cnt, c["cnt"])


# ---------------------------------------------------------------- 3. the fp64 entry
@pytest.mark.parametrize("axis,window", list(enumerate(vb.WINDOW_NAMES)))
@pytest.mark.parametrize("kernel", ["wendland_c2", "cubic_column"])
def test_fp64_entry_in_far_windows(gpu, oracle, monkeypatch, kernel, axis, window):
    """Raw fp64 particles 1e5 .. 4e6 pitches from the origin, points off the lattice inside
    the window: decisions on the fp64 values themselves (counts exact), values under the bar
    with the window's pitch and F64_INPUT_ULPS; each axis selection once."""
    from asp_amd._axes import AXIS_COLUMNS
    _knobs(monkeypatch)
    s = mixed(oracle, kernel, window, raw=True)
    ext = vb.window_ext(window)
    pitch = vb.pitch2d(vb.SIZE2D, ext)
    rng = np.random.default_rng(45)
    wx, wy = ext[1] - ext[0], ext[3] - ext[2]
    px = np.concatenate([rng.uniform(ext[0] - 0.05 * wx, ext[1] + 0.05 * wx, 2000), s["u"][::61]])
    py = np.concatenate([rng.uniform(ext[2] - 0.05 * wy, ext[3] + 0.05 * wy, 2000), s["v"][::61]])
    (r0, r1), (E0, E1), cnt = sr.reference(oracle, kernel, s["u"], s["v"], s["h"],
                                           [s["a0"], s["a"]], px, py, pitch=pitch,
                                           extra_ulps=vb.F64_INPUT_ULPS)
    pos = np.full((s["u"].size, 3), 1.0e300)  # the unused column must not matter
    pos[:, AXIS_COLUMNS[axis][0]] = s["u"]
    pos[:, AXIS_COLUMNS[axis][1]] = s["v"]
    g0, g1 = sample64(pos, s["h"], s["a0"], px, py, kernel, axis=axis, a1=s["a"])
    w = max(vb.assert_terms_close(g0, r0, E0), vb.assert_terms_close(g1, r1, E1))
    _report(f"fp64 {kernel} {window} axis {axis}", w)
    c, _ = sample64(pos, s["h"], np.ones(s["h"].size), px, py, "indicator", axis=axis)
    assert np.array_equal(c, cnt) and cnt.max() > 50


# ----------------------------------------------------------------------- 4. flags
@pytest.mark.parametrize("kernel", ["cubic", "wendland_c2_column"])
def test_ratio(gpu, oracle, monkeypatch, kernel):
    """out0 / out1 with the components' bars propagated: for g_i = r_i + d_i, |d_i| <= E_i,
    |g0/g1 - r0/r1| <= (E0 + |r0/r1| E1) / (|r1| - E1), plus the fp32 division and its
    rounding (<= 2.5 ulp = 5 * 2^-24 relative; 2^-21 taken).  0 exactly where no particle
    reaches the point."""
    from asp_amd import _lib
    _knobs(monkeypatch)
    c = offlattice_reference(oracle, kernel)
    g, _ = sample(c["u"], c["v"], c["h"], c["a0"], c["px"], c["py"], kernel, a1=c["a"],
                  flags=_lib.ASP_F_RATIO)
    cov = c["cnt"] > 0
    assert np.all(g[~cov] == 0) and np.all(np.isfinite(g))
    want = c["r0"][cov] / c["r1"][cov]
    den = np.abs(c["r1"][cov]) - c["E1"][cov]
    sure = den > 0
    bound = (c["E0"][cov] + np.abs(want) * c["E1"][cov])[sure] / den[sure] + 2.0 ** -21 * np.abs(want[sure])
    err = np.abs(g[cov] - want)[sure]
    assert sure.sum() > 0.9 * cov.sum()
    _report(f"ratio {kernel}", float(np.max(err / bound)))
    assert np.all(err <= bound)


@pytest.mark.parametrize("kernel", ["wendland_c2", "cubic_column"])
def test_accumulate(gpu, oracle, monkeypatch, kernel):
    """Two calls, each with half of the particles, the second with ASP_F_ACCUMULATE: the sum
    of one call within the two halves' bars (E_A + E_B = E) plus the rounding of the fp32
    addition that joins them (2^-24 of the result)."""
    from asp_amd import _lib
    _knobs(monkeypatch)
    c = offlattice_reference(oracle, kernel)
    A = np.arange(c["h"].size) % 2 == 0
    out0 = np.full(c["px"].size, np.nan, np.float32)
    out1 = np.full(c["px"].size, np.nan, np.float32)
    for half, flags in ((A, 0), (~A, _lib.ASP_F_ACCUMULATE)):
        g0, g1 = sample(c["u"][half], c["v"][half], c["h"][half], c["a0"][half], c["px"], c["py"],
                        kernel, a1=c["a"][half], flags=flags, out0=out0, out1=out1)
    for g, r, E in ((g0, c["r0"], c["E0"]), (g1, c["r1"], c["E1"])):
        assert np.all(g[r == 0] == 0)
        assert np.all(np.abs(g - r) <= E + 2.0 ** -24 * np.abs(r))


@pytest.mark.parametrize("kernel", ["cubic", "wendland_c2_column"])
def test_deterministic(gpu, oracle, monkeypatch, kernel):
    """Bitwise equal under a permutation of the particles, of the points, with other grids
    and classes, in batches, and from device pointers on a non-default stream; within
    E + fixed_point_term."""
    import torch
    from asp_amd import _lib
    _knobs(monkeypatch)
    c = offlattice_reference(oracle, kernel)
    det = _lib.ASP_F_DETERMINISTIC
    args = (c["u"], c["v"], c["h"], c["a0"])
    g0, g1 = sample(*args, c["px"], c["py"], kernel, a1=c["a"], flags=det)
    w = max(vb.assert_terms_close(g0, c["r0"], c["E0"], floor=c["F0"]),
            vb.assert_terms_close(g1, c["r1"], c["E1"], floor=c["F1"]))
    _report(f"deterministic {kernel}", w)
    assert np.all(g0[3001:4001] == g0[3001])  # copies of one point: one value
    rng = np.random.default_rng(46)
    p = rng.permutation(c["h"].size)
    h0, h1 = sample(*(x[p] for x in args), c["px"], c["py"], kernel, a1=c["a"][p], flags=det)
    assert np.array_equal(h0, g0) and np.array_equal(h1, g1)
    q = rng.permutation(c["px"].size)
    h0, h1 = sample(*args, c["px"][q], c["py"][q], kernel, a1=c["a"], flags=det)
    assert np.array_equal(h0, g0[q]) and np.array_equal(h1, g1[q])
    for setting in ("cells7_wave", "cells1_lane"):
        _knobs(monkeypatch, setting)
        h0, _ = sample(*args, c["px"], c["py"], kernel, a1=c["a"], flags=det)
        assert np.array_equal(h0, g0), setting
    _knobs(monkeypatch)
    monkeypatch.setenv("ASP_MAX_BATCH", "1000")  # for_batches' knob: five batches
    h0, h1 = sample(*args, c["px"], c["py"], kernel, a1=c["a"], flags=det)
    assert np.array_equal(h0, g0) and np.array_equal(h1, g1)
    monkeypatch.delenv("ASP_MAX_BATCH")
    # device pointers, a side stream
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        t = [torch.tensor(np.asarray(x), dtype=torch.float32, device="cuda") for x in args + (c["a"],)]
        tp = [torch.tensor(np.asarray(x), dtype=torch.float64, device="cuda") for x in (c["px"], c["py"])]
        o0 = torch.full((c["px"].size,), float("nan"), dtype=torch.float32, device="cuda")
        o1 = torch.full_like(o0, float("nan"))
        P, D = _lib.ptr, (lambda x: _lib.ptr(x, _lib._d))
        _lib.check(_lib.lib().asp_sample2d(
            P(t[0]), P(t[1]), P(t[2]), P(t[3]), P(t[4]), c["h"].size, D(tp[0]), D(tp[1]),
            c["px"].size, sr.KERNEL_IDS[kernel], det | _lib.ASP_F_DEVICE_PTRS, P(o0), P(o1), 0,
            st.cuda_stream))
    st.synchronize()
    assert np.array_equal(o0.cpu().numpy().astype(np.float64), g0)
    assert np.array_equal(o1.cpu().numpy().astype(np.float64), g1)
    with pytest.raises(ValueError, match="ASP_F_RATIO"):
        sample(*args, c["px"], c["py"], kernel, a1=c["a"], flags=det | _lib.ASP_F_RATIO)


# ----------------------------------------------------------------------- 5. edges
def test_batches_in_fp64_mode(gpu, oracle, monkeypatch):
    """ASP_MAX_BATCH (the knob for_batches honours) forces batch boundaries: the same
    neighbour sets, the same bar."""
    _knobs(monkeypatch)
    monkeypatch.setenv("ASP_MAX_BATCH", "777")
    c = offlattice_reference(oracle, "cubic")
    g0, g1 = sample(c["u"], c["v"], c["h"], c["a0"], c["px"], c["py"], "cubic", a1=c["a"])
    vb.assert_terms_close(g0, c["r0"], c["E0"])
    vb.assert_terms_close(g1, c["r1"], c["E1"])
    cnt, _ = sample(c["u"], c["v"], c["h"], np.ones(c["h"].size), c["px"], c["py"], "indicator")
    assert np.array_equal(cnt, c["cnt"])


def test_edges(gpu, oracle, monkeypatch):
    import torch
    from asp_amd import _lib
    _knobs(monkeypatch)
    c = offlattice_reference(oracle, "cubic")
    # n == 0 with device pointers: zeros written on the stream; untouched under accumulate
    px, py = (torch.tensor(np.asarray(c[k]), dtype=torch.float64, device="cuda") for k in ("px", "py"))
    out = torch.full((px.numel(),), 7.0, dtype=torch.float32, device="cuda")
    call = lambda flags: _lib.check(_lib.lib().asp_sample2d(  # noqa: E731
        None, None, None, None, None, 0, _lib.ptr(px, _lib._d), _lib.ptr(py, _lib._d), px.numel(), 0,
        flags | _lib.ASP_F_DEVICE_PTRS, _lib.ptr(out), None, 0,
        torch.cuda.current_stream().cuda_stream))
    call(_lib.ASP_F_ACCUMULATE)
    assert torch.all(out == 7.0)
    call(0)
    assert torch.all(out == 0.0)
    # m == 1: the contended point alone, against the full call's value for it
    k = 3001
    g, _ = sample(c["u"], c["v"], c["h"], c["a"], c["px"][k:k + 1], c["py"][k:k + 1], "cubic")
    vb.assert_terms_close(g, c["r1"][k:k + 1], c["E1"][k:k + 1])
    # one particle whose disc covers every point (and a NaN point: 0)
    px1 = np.append(c["px"][:3001], [np.nan, 0.3, np.inf])
    py1 = np.append(c["py"][:3001], [0.2, np.nan, 0.0])
    u, v, h = np.array([0.1]), np.array([-0.2]), np.array([4.0])
    a = vb.f32(1.0 / vb.w0(oracle, "cubic", h))
    (r,), (E,), cnt = sr.reference(oracle, "cubic", u, v, h, [a], px1, py1)
    assert cnt[:3001].min() == 1 and cnt[3001:].tolist() == [0, 0, 0]
    for setting in ("default", "default_lane"):
        _knobs(monkeypatch, setting)
        g, _ = sample(u, v, h, a, px1, py1, "cubic")
        vb.assert_terms_close(g, r, E)
        assert np.all(g[3001:] == 0)
    # only non-finite points: zeros
    g, _ = sample(u, v, h, a, np.full(5, np.nan), np.zeros(5), "cubic")
    assert np.all(g == 0)


# ------------------------------------------------------------------- 6. periodic box
@pytest.mark.parametrize("kernel", ["cubic", "cubic_column"])
def test_periodic_composition(gpu, oracle, kernel):
    """asp_stage_particles(..., ASP_PB_IMAGES) feeding asp_sample2d = the brute force with
    minimum-image displacements, at points within 2h of a box face.  Positions and points
    lie on a 2^-16 lattice and L = 4, so the shifted images are exact in fp32 and both
    forms of every difference are exact in fp64: the counts must agree exactly."""
    import torch
    from asp_amd import _lib
    from asp_amd.stage import stage_particles
    rng = np.random.default_rng(47)
    L, n, m = 4.0, 1500, 1200
    q = 2.0 ** -16
    pos = np.floor(rng.uniform(0.0, L, (n, 3)) / q) * q
    pos[0] = [q, 2.0, 1.0]           # hugs the x = 0 face
    pos[1] = [L - q, q, 1.0]         # a corner: three images
    h = vb.f32(rng.uniform(0.02, 0.12, n))
    A = vb.f32(rng.uniform(0.5, 2.0, n) / w0(oracle, kernel, h))
    # points within 2 h_max of a face, on both sides of the box, and the two corners
    face = np.floor(rng.uniform(0.0, 0.2, m) / q) * q
    face = np.where(rng.random(m) < 0.5, face, L - q - face)
    other = np.floor(rng.uniform(0.0, L, m) / q) * q
    swap = rng.random(m) < 0.5
    px = np.concatenate([np.where(swap, face, other), [0.0, L - q]])
    py = np.concatenate([np.where(swap, other, face), [0.0, q]])
    u, v, hf, (a,) = stage_particles(pos, h, A, projection_axis=2, box_width=L, images=True)
    assert u.numel() > n
    tpx, tpy = (torch.tensor(x, dtype=torch.float64, device="cuda") for x in (px, py))
    out = torch.full((px.size,), float("nan"), dtype=torch.float32, device="cuda")
    cnt = torch.full_like(out, float("nan"))
    P, D = _lib.ptr, (lambda x: _lib.ptr(x, _lib._d))
    stream = torch.cuda.current_stream().cuda_stream
    one = torch.ones_like(a)
    for amp, kid, o in ((a, sr.KERNEL_IDS[kernel], out), (one, 2, cnt)):
        _lib.check(_lib.lib().asp_sample2d(P(u), P(v), P(hf), P(amp), None, u.numel(), D(tpx), D(tpy),
                                           px.size, kid, _lib.ASP_F_DEVICE_PTRS, P(o), None, 0, stream))
    fold = lambda d: d - L * np.round(d / L)  # noqa: E731  (exact: lattice values, L = 4)
    (r,), (E,), want = sr.reference(oracle, kernel, pos[:, 0], pos[:, 1], h, [A], px, py,
                                    pitch=0.0, displacement=fold)
    assert np.array_equal(cnt.cpu().numpy(), want) and want.min() >= 0 and want.max() > 5
    # pitch = 0: the pair difference is formed in fp64, no local frame enters
    _report(f"periodic {kernel}", vb.assert_terms_close(out.cpu().numpy(), r, E))


# ------------------------------------------------------------------------ 7. Python
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_sightline_columns(gpu, oracle, monkeypatch, axis):
    """(M, 2) and (M, 3) points, host arrays and tensors: the C-ABI call's result bit for
    bit (deterministic sums), the weighted form against a0 = A w, a1 = w."""
    import torch
    from asp_amd import _lib, sightline_columns
    from asp_amd._axes import AXIS_COLUMNS
    from asp_amd.tools.projections import wendland_c2_column_kernel
    _knobs(monkeypatch)
    rng = np.random.default_rng(48 + axis)
    n, m = 3000, 700
    pos = rng.uniform(0.0, 1.0, (n, 3))
    h = rng.uniform(0.01, 0.08, n)
    A = rng.uniform(0.5, 2.0, n)
    wgt = rng.uniform(0.5, 2.0, n)
    pts3 = rng.uniform(-0.05, 1.05, (m, 3))
    cu, cv = AXIS_COLUMNS[axis]
    pts2 = np.ascontiguousarray(pts3[:, [cu, cv]])
    axes = [axis, "xyz"[axis], _lib_axis(axis)]
    det = _lib.ASP_F_DETERMINISTIC
    want, _ = sample64(pos, h, A, pts2[:, 0], pts2[:, 1], "wendland_c2_column", axis=axis, flags=det)
    assert np.count_nonzero(want) > m // 2
    for k, pts in enumerate((pts2, pts3, pts3)):
        got = sightline_columns(pos, h, A, pts, axes[k], kernel="wendland_c2_column",
                                deterministic=True)
        assert isinstance(got, np.ndarray) and got.dtype == np.float32
        assert np.array_equal(got.astype(np.float64), want)
    tens = lambda x: torch.tensor(x, dtype=torch.float64, device="cuda")  # noqa: E731
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        got = sightline_columns(tens(pos), tens(h), tens(A), tens(pts3), axis,
                                kernel=wendland_c2_column_kernel, deterministic=True, stream=st)
    st.synchronize()
    assert got.is_cuda and np.array_equal(got.cpu().numpy().astype(np.float64), want)
    # the ratio form (the default kernel)
    want, _ = sample64(pos, h, A * wgt, pts2[:, 0], pts2[:, 1], "cubic_column", axis=axis, a1=wgt,
                       flags=_lib.ASP_F_RATIO)
    # (fp64 sums depend on the order of the atomic adds in their last bits: each fp32
    # component may move by an ulp between two calls, the quotient by <= 4 * 2^-24)
    got = sightline_columns(pos, h, A, pts3, axis, weights=wgt)
    assert np.all(np.abs(got - want) <= 2.0 ** -22 * np.abs(want))
    got = sightline_columns(tens(pos), tens(h), tens(A), tens(pts2), axis, weights=tens(wgt))
    assert np.all(np.abs(got.cpu().numpy() - want) <= 2.0 ** -22 * np.abs(want))
    assert np.array_equal(got.cpu().numpy() == 0, want == 0)
    # a weighted mean of A in [0.5, 2]
    assert 0.5 * (1 - 1e-6) <= want[want != 0].min() and want.max() <= 2.0 * (1 + 1e-6)


def _lib_axis(axis):
    from asp_amd import CoordinateAxes
    return CoordinateAxes(axis)
