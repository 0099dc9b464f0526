"""Sightline spectra on the GPU: asp_spectra2d, asp_spectra2d_f64 and
asp_amd.sightline_spectra.

The reference is the fp64 brute force of tests/spectra_ref.py (tied to sightline_ref and to
hand cases by tests/test_spectra_ref.py) and its bar E[s, k]: every bin of every sightline is
compared, |g - r| <= E, and g == 0 where r == 0.  Neighbour sets are checked exactly through
the indicator kernel: in ring mode a sightline's bins sum to its neighbour count.

Particles: value_bar's mixed set (4 912 particles, every h class) plus the strict-inequality
particle.  Sightlines: every 13th of test_gpu_sightlines.offlattice_case's 4 054 points and its
last two (314: random points, copies of the clump point, points on particles, the pair on
either side of r = 2h).  Velocities are seeded: vc uniform over 1.5 x the window, b / dv
log-uniform in [0.05, 40].  Every case prints its worst err/E (``pytest -s``).
"""
import numpy as np
import pytest

import sightline_ref as sr
import spectra_ref as spr
import value_bar as vb
from test_gpu_sightlines import _knobs, mixed, offlattice_case, sample, w0
from test_spectra_host import check_errors
from test_spectra_ref import velocity_inputs

pytestmark = pytest.mark.gpu

V0, DV = -40.0, 1.25
KERNELS = ("cubic", "cubic_column", "wendland_c2_column")
WALK_SETTINGS = ("default", "cells1_wave", "cells1_lane", "cells7_wave", "cells7_lane")


def _report(label, worst):
    print(f"SPECTRA_BAR {label}: worst err/E = {worst:.3f}")


def _f(x, t):
    return None if x is None else np.ascontiguousarray(x, t)


def spectra(c, vc, b, K, ring, kernel, a0="a0", a1=None, flags=0, out0=None, out1=None, sel=None,
            px=None, py=None):
    """asp_spectra2d on host arrays of case ``c`` (``sel``: a subset of its particles);
    returns (out0, out1) as float64 (M, K)."""
    from asp_amd import _lib
    sel = slice(None) if sel is None else sel
    f32, f64 = np.float32, np.float64
    u, v, h = (_f(c[k][sel], f32) for k in ("u", "v", "h"))
    A0 = _f((c[a0] if isinstance(a0, str) else a0)[sel], f32)
    A1 = None if a1 is None else _f((c[a1] if isinstance(a1, str) else a1)[sel], f32)
    vc, b = _f(np.asarray(vc)[sel], f64), _f(np.asarray(b)[sel], f32)
    px, py = _f(c["px"] if px is None else px, f64), _f(c["py"] if py is None else py, f64)
    if out0 is None:
        out0 = np.full(px.size * K, np.nan, f32)
    if A1 is not None and out1 is None:
        out1 = np.full(px.size * K, np.nan, f32)
    P, D = _lib.ptr, (lambda x: _lib.ptr(x, _lib._d))
    _lib.check(_lib.lib().asp_spectra2d(P(u), P(v), P(h), P(A0), P(A1), D(vc), P(b), u.size, D(px), D(py),
                                        px.size, V0, DV, K, int(ring), sr.KERNEL_IDS[kernel], flags,
                                        P(out0), P(out1), 0, None))
    shape = (px.size, K)
    return (out0.astype(f64).reshape(shape), None if out1 is None else out1.astype(f64).reshape(shape))


_cases, _refs = {}, {}


def case(oracle, kernel):
    if kernel not in _cases:
        c = offlattice_case(oracle, kernel)
        pick = np.unique(np.r_[np.arange(0, c["px"].size, 13), c["px"].size - 2, c["px"].size - 1])
        c["px"], c["py"] = c["px"][pick], c["py"][pick]
        for x in c.values():
            x.setflags(write=False)
        _cases[kernel] = c
    return _cases[kernel]


def velocities(n, K, seed=62):
    vc, b = velocity_inputs(n, V0, DV, K, seed)
    return vc, vb.f32(b)  # the fp32 entry takes b in fp32


def reference(oracle, kernel, K, ring, tag="seeded", make=None):
    """The shared reference of (kernel, K, ring) for the seeded velocities, or for those of
    ``make(n, K)`` under ``tag``: c, vc, b, r0 / r1, E0 / E1 (sums of a0 and a), cnt, col1."""
    key = (kernel, K, ring, tag)
    if key not in _refs:
        c = case(oracle, kernel)
        vc, b = (make or velocities)(c["h"].size, K)
        (r0, r1), (E0, E1), cnt, (_, col1) = spr.reference(
            oracle, kernel, c["u"], c["v"], c["h"], [c["a0"], c["a"]], vc, b, c["px"], c["py"], V0, DV,
            K, ring)
        ref = dict(c=c, vc=vc, b=b, r0=r0, r1=r1, E0=E0, E1=E1, cnt=cnt, col1=col1)
        for x in ref.values():
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
        _refs[key] = ref
    return _refs[key]


def assert_counts(c, vc, b, K, cnt):
    """The indicator kernel in ring mode: sum_k out dv is the neighbour count.  Every bin is
    the fp32 rounding (2^-24 relative, all bins >= 0) of a sum that lacks at most erfc(T) of
    each pair and carries the fp64 roundings of the reference's bar (2^-48 per pair and bin)."""
    g, _ = spectra(c, vc, b, K, True, "indicator", a0=np.ones(c["h"].size))
    total = g.sum(axis=1) * DV
    ok = spr.admitted(np.asarray(vc), np.asarray(b), DV)
    assert ok.all()  # (callers pass admitted particles only: the count is over all of them)
    tol = cnt * (2.0 ** -24 + 2.0 ** -36 + K * 2.0 ** -48) * (1 + 2.0 ** -20)
    assert np.all(np.abs(total - cnt) <= tol), float(np.max(np.abs(total - cnt) / np.maximum(tol, 1e-300)))
    assert not g[cnt == 0].any()


def check_both(label, g0, g1, ref):
    w = max(vb.assert_terms_close(g0, ref["r0"], ref["E0"]), vb.assert_terms_close(g1, ref["r1"], ref["E1"]))
    _report(label, w)


# ------------------------------------------------- 1. kernel forms, pair classes, walks
@pytest.mark.parametrize("walk", ["1", "0"])
@pytest.mark.parametrize("setting", WALK_SETTINGS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_kernels_classes_and_walks(gpu, oracle, monkeypatch, kernel, setting, walk):
    """Two sums over a ring of 200 bins, for every kernel form, with the pairs found by the
    lanes, by the wave and by both, deposited by the wave (walk 1) and by the lane (0)."""
    _knobs(monkeypatch, setting)
    monkeypatch.setenv("ASP_SPECTRA_WALK", walk)
    ref = reference(oracle, kernel, 200, True)
    c = ref["c"]
    assert ref["cnt"][-2:].tolist() == [0, 1] and ref["cnt"].max() > 300
    g0, g1 = spectra(c, ref["vc"], ref["b"], 200, True, kernel, a1="a")
    check_both(f"{kernel} {setting} walk {walk}", g0, g1, ref)
    assert_counts(c, ref["vc"], ref["b"], 200, ref["cnt"])


# ----------------------------------------------------------------- 2. bin counts
@pytest.mark.parametrize("walk", ["1", "0"])
@pytest.mark.parametrize("ring", [False, True])
@pytest.mark.parametrize("K", [1, 63, 64, 65, 200])
def test_bin_counts(gpu, oracle, monkeypatch, K, ring, walk):
    """The lane-stride edges of the wave's walk, as a window (clipped runs) and as a ring
    (b / dv up to 40: runs of 400 bins wrap K = 1 .. 65 many times)."""
    _knobs(monkeypatch)
    monkeypatch.setenv("ASP_SPECTRA_WALK", walk)
    ref = reference(oracle, "cubic_column", K, ring)
    g0, g1 = spectra(ref["c"], ref["vc"], ref["b"], K, ring, "cubic_column", a1="a")
    check_both(f"K {K} ring {ring} walk {walk}", g0, g1, ref)
    if not ring:  # some particles lie outside the window: their sightlines' bins hold less
        assert np.any(ref["r1"].sum(axis=1) * DV < 0.9 * ref["col1"])


# --------------------------------------------------------- 3. hard velocity inputs
def hard_velocities(n, K):
    """By particle index mod 8: a line far narrower than a bin exactly on an edge, one ulp
    below and one ulp above it; a line so wide that its run exceeds 2 K bins (a ring wraps
    twice); vc below the window and beyond its end by several widths; vc far outside."""
    rng = np.random.default_rng(63)
    width = K * DV
    edge = V0 + DV * rng.integers(0, K + 1, n)
    vc = np.select(
        [np.arange(n) % 8 == k for k in range(8)],
        [edge, np.nextafter(edge, -np.inf), np.nextafter(edge, np.inf),
         rng.uniform(V0, V0 + width, n), V0 - rng.uniform(0.5, 3.7, n) * width,
         V0 + rng.uniform(1.5, 5.3, n) * width, V0 + 1.0e6 * width + rng.uniform(0, width, n),
         rng.uniform(V0, V0 + width, n)])
    b = np.where(np.arange(n) % 8 < 3, DV * 2.0 ** -20, DV * rng.uniform(0.5, 3.0, n))
    b = np.where(np.arange(n) % 8 == 3, 0.3 * width, b)  # 2 T b / dv = 3 K bins
    return vc, vb.f32(b)


@pytest.mark.parametrize("walk", ["1", "0"])
@pytest.mark.parametrize("ring", [False, True])
def test_hard_velocity_inputs(gpu, oracle, monkeypatch, ring, walk):
    _knobs(monkeypatch)
    monkeypatch.setenv("ASP_SPECTRA_WALK", walk)
    K = 64
    ref = reference(oracle, "cubic", K, ring, "hard", hard_velocities)
    g0, g1 = spectra(ref["c"], ref["vc"], ref["b"], K, ring, "cubic", a1="a")
    check_both(f"hard ring {ring} walk {walk}", g0, g1, ref)
    if ring:
        assert_counts(ref["c"], ref["vc"], ref["b"], K, ref["cnt"])
    else:  # vc = 1e300 as well: no bins, no fault
        vc = np.where(np.arange(ref["vc"].size) % 8 == 6, 1.0e300, ref["vc"])
        h0, _ = spectra(ref["c"], vc, ref["b"], K, ring, "cubic")
        vb.assert_terms_close(h0, ref["r0"], ref["E0"])


# ------------------------------------------------------------------ 4. contention
@pytest.mark.parametrize("walk", ["1", "0"])
def test_contention(gpu, oracle, monkeypatch, walk):
    """One sightline under every particle's disc (all adds go to one row of 64 bins), and 64
    copies of it (each row is the single row, within the bar)."""
    _knobs(monkeypatch)
    monkeypatch.setenv("ASP_SPECTRA_WALK", walk)
    s = mixed(oracle, "cubic_column")
    n, K = s["h"].size, 64
    c = dict(u=vb.f32(0.02 * s["u"]), v=vb.f32(0.02 * s["v"]), h=vb.f32(0.05 + 4.0 * s["h"]), a=s["a"],
             px=np.array([0.001]), py=np.array([-0.002]))
    vc, b = velocities(n, K, seed=64)
    (r,), (E,), cnt, _ = spr.reference(oracle, "cubic_column", c["u"], c["v"], c["h"], [c["a"]], vc, b,
                                       c["px"], c["py"], V0, DV, K, True)
    assert cnt.tolist() == [n]
    g, _ = spectra(c, vc, b, K, True, "cubic_column", a0="a")
    w = vb.assert_terms_close(g, r, E)
    c64 = dict(c, px=np.repeat(c["px"], 64), py=np.repeat(c["py"], 64))
    g64, _ = spectra(c64, vc, b, K, True, "cubic_column", a0="a")
    w = max(w, vb.assert_terms_close(g64, np.repeat(r, 64, axis=0), np.repeat(E, 64, axis=0)))
    _report(f"contention walk {walk}", w)


# -------------------------------------------------------- 5. entry points and flags
def test_ratio(gpu, oracle, monkeypatch):
    """out0 / out1 per bin with the components' bars propagated as value_bar.assert_ratio_close
    does: |q - r0 / r1| <= (E0 + |w| E1) / (r1 - E1) + 2^-23 |w| where r1 > 2 E1, 0 exactly
    where r1 == 0, finite elsewhere (the Gaussian tails, where the bar exceeds the sum)."""
    from asp_amd import _lib
    _knobs(monkeypatch)
    ref = reference(oracle, "cubic_column", 64, False)
    q, g1 = spectra(ref["c"], ref["vc"], ref["b"], 64, False, "cubic_column", a1="a",
                    flags=_lib.ASP_F_RATIO)
    r0, r1, E0, E1 = (ref[k] for k in ("r0", "r1", "E0", "E1"))
    assert np.all(np.isfinite(q)) and not q[r1 == 0].any()
    vb.assert_terms_close(g1, r1, E1)
    ok = r1 > 2.0 * E1
    w = r0[ok] / r1[ok]
    bar = (E0[ok] + np.abs(w) * E1[ok]) / (r1[ok] - E1[ok]) + 2.0 ** -23 * np.abs(w)
    err = np.abs(q[ok] - w)
    print(f"SPECTRA_BAR ratio: worst err/bar = {np.max(err / bar):.3f} over {ok.sum()} of "
          f"{np.count_nonzero(r1)} covered bins")
    assert np.all(err <= bar) and ok.sum() > 0.5 * np.count_nonzero(r1)


def test_accumulate(gpu, oracle, monkeypatch):
    """Two calls, each with half of the particles, the second with ASP_F_ACCUMULATE: one
    call's sums within the two halves' bars (E_A + E_B = E + one more truncation floor, which
    is inside E's) plus the rounding of the fp32 addition that joins them (2^-24 of it)."""
    from asp_amd import _lib
    _knobs(monkeypatch)
    ref = reference(oracle, "cubic", 65, True)
    c = ref["c"]
    A = np.arange(c["h"].size) % 2 == 0
    out0 = np.full(c["px"].size * 65, np.nan, np.float32)
    out1 = np.full(c["px"].size * 65, np.nan, np.float32)
    for half, flags in ((A, 0), (~A, _lib.ASP_F_ACCUMULATE)):
        g0, g1 = spectra(c, ref["vc"], ref["b"], 65, True, "cubic", a1="a", flags=flags, out0=out0,
                         out1=out1, sel=half)
    for g, r, E in ((g0, ref["r0"], ref["E0"]), (g1, ref["r1"], ref["E1"])):
        assert not g[r == 0].any()
        assert np.all(np.abs(g - r) <= E + 2.0 ** -24 * np.abs(r))


def test_batches(gpu, oracle, monkeypatch):
    """ASP_MAX_BATCH=1000: five batches into the same accumulators, the bar of one."""
    _knobs(monkeypatch)
    monkeypatch.setenv("ASP_MAX_BATCH", "1000")
    ref = reference(oracle, "cubic_column", 200, True)
    g0, g1 = spectra(ref["c"], ref["vc"], ref["b"], 200, True, "cubic_column", a1="a")
    check_both("batches", g0, g1, ref)
    assert_counts(ref["c"], ref["vc"], ref["b"], 200, ref["cnt"])


def test_device_caller(gpu, oracle, monkeypatch):
    """Device pointers on a side stream: the host caller's result within the bar."""
    import torch
    from asp_amd import _lib
    _knobs(monkeypatch)
    K = 63
    ref = reference(oracle, "cubic_column", K, True)
    c = ref["c"]
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        t = [torch.tensor(np.asarray(c[k]), dtype=torch.float32, device="cuda")
             for k in ("u", "v", "h", "a0", "a")]
        tb = torch.tensor(np.asarray(ref["b"]), dtype=torch.float32, device="cuda")
        tv, tpx, tpy = (torch.tensor(np.asarray(x), dtype=torch.float64, device="cuda")
                        for x in (ref["vc"], c["px"], c["py"]))
        o0 = torch.full((c["px"].size, K), float("nan"), dtype=torch.float32, device="cuda")
        o1 = torch.full_like(o0, float("nan"))
        P, D = _lib.ptr, (lambda x: _lib.ptr(x, _lib._d))
        _lib.check(_lib.lib().asp_spectra2d(
            P(t[0]), P(t[1]), P(t[2]), P(t[3]), P(t[4]), D(tv), P(tb), c["h"].size, D(tpx), D(tpy),
            c["px"].size, V0, DV, K, 1, sr.KERNEL_IDS["cubic_column"], _lib.ASP_F_DEVICE_PTRS, P(o0),
            P(o1), 0, st.cuda_stream))
    st.synchronize()
    check_both("device caller", o0.cpu().numpy(), o1.cpu().numpy(), ref)


def spectra64(pos, h, a0, vc, b, px, py, K, ring, kernel, axis):
    from asp_amd import _lib
    f64 = np.float64
    pos, h, a0, vc, b, px, py = (_f(x, f64) for x in (pos, h, a0, vc, b, px, py))
    out0 = np.full(px.size * K, np.nan, np.float32)
    D = lambda x: _lib.ptr(x, _lib._d)  # noqa: E731
    _lib.check(_lib.lib().asp_spectra2d_f64(D(pos), D(h), D(a0), None, D(vc), D(b), h.size, axis, D(px),
                                            D(py), px.size, V0, DV, K, int(ring), sr.KERNEL_IDS[kernel], 0,
                                            _lib.ptr(out0), None, 0, None))
    return out0.astype(f64).reshape(px.size, K)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_fp64_entry(gpu, oracle, monkeypatch, axis):
    """asp_spectra2d_f64 on each axis selection (the unused column must not matter), b in
    fp64 as drawn: the bar with F64_INPUT_ULPS, as for asp_sample2d_f64."""
    from asp_amd._axes import AXIS_COLUMNS
    _knobs(monkeypatch)
    c = case(oracle, "wendland_c2_column")
    K = 64
    vc, b = velocity_inputs(c["h"].size, V0, DV, K, 65)
    (r,), (E,), cnt, _ = _fp64_reference(oracle, c, vc, b, K)
    pos = np.full((c["h"].size, 3), 1.0e300)
    pos[:, AXIS_COLUMNS[axis][0]] = c["u"]
    pos[:, AXIS_COLUMNS[axis][1]] = c["v"]
    g = spectra64(pos, c["h"], c["a"], vc, b, c["px"], c["py"], K, True, "wendland_c2_column", axis)
    _report(f"fp64 entry axis {axis}", vb.assert_terms_close(g, r, E))
    n = spectra64(pos, c["h"], np.ones(c["h"].size), vc, b, c["px"], c["py"], K, True, "indicator", axis)
    tol = cnt * (2.0 ** -24 + 2.0 ** -36 + K * 2.0 ** -48) * (1 + 2.0 ** -20)
    assert np.all(np.abs(n.sum(axis=1) * DV - cnt) <= tol)


def _fp64_reference(oracle, c, vc, b, K):
    if "fp64" not in _refs:
        _refs["fp64"] = spr.reference(oracle, "wendland_c2_column", c["u"], c["v"], c["h"], [c["a"]], vc,
                                      b, c["px"], c["py"], V0, DV, K, True,
                                      extra_ulps=vb.F64_INPUT_ULPS)
    return _refs["fp64"]


# ------------------------------------------------------- 6. admission, errors, sizes
@pytest.mark.parametrize("ring", [False, True])
def test_admission(gpu, oracle, monkeypatch, ring):
    """Particles with b in {0, -1, NaN, inf}, vc in {NaN, +-inf} or T b / dv >= 2^24 are in no
    bin and the rest is unchanged: the reference leaves exactly those out.  A sightline with a
    non-finite coordinate reads 0 in every bin."""
    _knobs(monkeypatch)
    K = 64
    c = case(oracle, "cubic")
    n = c["h"].size
    vc, b = velocities(n, K, seed=66)
    vc, b = vc.copy(), b.copy()
    odd_b = [0.0, -1.0, np.nan, np.inf, 2.0 ** 24 * DV / spr.T, 2.0e7 * DV]
    for k, x in enumerate(odd_b):
        b[k::17][: n // 40] = x
    for k, x in enumerate([np.nan, np.inf, -np.inf]):
        vc[len(odd_b) + k::17][: n // 40] = x
    left_out = ~spr.admitted(vc, b, DV)
    assert left_out.sum() == 9 * (n // 40)
    px = np.concatenate([c["px"], [np.nan, 0.1, np.inf]])
    py = np.concatenate([c["py"], [0.1, np.nan, -np.inf]])
    (r,), (E,), cnt, _ = spr.reference(oracle, "cubic", c["u"], c["v"], c["h"], [c["a"]], vc, b, px, py,
                                       V0, DV, K, ring)
    assert cnt[-3:].tolist() == [0, 0, 0]
    g, _ = spectra(c, vc, b, K, ring, "cubic", a0="a", px=px, py=py)
    _report(f"admission ring {ring}", vb.assert_terms_close(g, r, E))
    assert not g[-3:].any()
    # ... and the call without them gives the same reference its own way
    g2, _ = spectra(c, vc, b, K, ring, "cubic", a0="a", px=px, py=py, sel=~left_out)
    vb.assert_terms_close(g2, r, E)
    assert np.array_equal(g == 0, g2 == 0)


def test_errors_and_empty_sizes(gpu, oracle, monkeypatch):
    import torch
    from asp_amd import _lib
    _knobs(monkeypatch)
    check_errors()  # every ASP_ERR_* of the header, with its message
    c = case(oracle, "cubic")
    K = 9
    D = lambda x: _lib.ptr(x, _lib._d)  # noqa: E731
    # m == 0
    assert _lib.lib().asp_spectra2d(None, None, None, None, None, None, None, 0, None, None, 0, V0, DV, K,
                                    0, 0, 0, None, None, 0, None) == _lib.ASP_OK
    # n == 0 with device pointers: zeros written on the stream; untouched under accumulate
    px, py = (torch.tensor(np.asarray(c[k]), dtype=torch.float64, device="cuda") for k in ("px", "py"))
    out = torch.full((px.numel(), K), 7.0, dtype=torch.float32, device="cuda")
    call = lambda flags: _lib.check(_lib.lib().asp_spectra2d(  # noqa: E731
        None, None, None, None, None, None, None, 0, D(px), D(py), px.numel(), V0, DV, K, 1, 0,
        flags | _lib.ASP_F_DEVICE_PTRS, _lib.ptr(out), None, 0, torch.cuda.current_stream().cuda_stream))
    call(_lib.ASP_F_ACCUMULATE)
    assert torch.all(out == 7.0)
    call(0)
    assert torch.all(out == 0.0)
    # n == 0 on host arrays, and only non-finite sightlines
    vc, b = velocities(c["h"].size, K)
    g, _ = spectra(c, vc, b, K, True, "cubic", sel=slice(0, 0))
    assert not g.any()
    g, _ = spectra(c, vc, b, K, True, "cubic", px=np.full(5, np.nan), py=np.zeros(5))
    assert g.shape == (5, K) and not g.any()


# ------------------------------------------------------------------ 7. conservation
@pytest.mark.parametrize("kernel", ["cubic", "wendland_c2_column"])
def test_ring_bins_sum_to_the_sampled_column(gpu, oracle, monkeypatch, kernel):
    """sum_k out[s, k] dv in ring mode against asp_sample2d's output for the same inputs,
    within the sum of both bars: sum_k E[s, k] dv here, sightline_ref's E there."""
    _knobs(monkeypatch)
    ref = reference(oracle, kernel, 200, True)
    c = ref["c"]
    g, _ = spectra(c, ref["vc"], ref["b"], 200, True, kernel, a0="a")
    col, _ = sample(c["u"], c["v"], c["h"], c["a"], c["px"], c["py"], kernel)
    (_,), (Es,), cnt = sr.reference(oracle, kernel, c["u"], c["v"], c["h"], [c["a"]], c["px"], c["py"])
    assert np.array_equal(cnt, ref["cnt"])
    bar = ref["E1"].sum(axis=1) * DV + Es
    err = np.abs(g.sum(axis=1) * DV - col)
    assert np.all(err <= bar) and np.count_nonzero(col) > 250
    print(f"SPECTRA_BAR conservation {kernel}: worst err/bar = {np.max(err[bar > 0] / bar[bar > 0]):.3f}")


# ------------------------------------------------------------------------ 8. Python
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_sightline_spectra(gpu, oracle, monkeypatch, axis):
    """(M, 2) and (M, 3) points, host arrays and tensors, against the C-ABI call: fp64 sums of
    positive terms depend on the order of the atomic adds in their last bits only, so each
    fp32 value may move by an ulp between two calls (2^-23); the weighted form against
    a0 = A w, a1 = w (the quotient of two such values: 4 * 2^-24, as for sightline_columns)."""
    import torch
    from asp_amd import _lib, sightline_spectra
    from asp_amd._axes import AXIS_COLUMNS
    _knobs(monkeypatch)
    rng = np.random.default_rng(67 + axis)
    n, m, K = 3000, 150, 40
    pos = rng.uniform(0.0, 1.0, (n, 3))
    h = rng.uniform(0.01, 0.08, n)
    A = rng.uniform(0.5, 2.0, n)
    wgt = rng.uniform(0.5, 2.0, n)
    vc, b = velocity_inputs(n, V0, DV, K, 68)
    pts3 = rng.uniform(-0.05, 1.05, (m, 3))
    cu, cv = AXIS_COLUMNS[axis]
    pts2 = np.ascontiguousarray(pts3[:, [cu, cv]])

    def c_abi(a0, a1, flags):
        out0 = np.full(m * K, np.nan, np.float32)
        out1 = None if a1 is None else np.full(m * K, np.nan, np.float32)
        D = lambda x: _lib.ptr(x, _lib._d)  # noqa: E731
        _lib.check(_lib.lib().asp_spectra2d_f64(
            D(pos), D(h), D(a0), D(a1), D(vc), D(b), n, axis, D(np.ascontiguousarray(pts2[:, 0])),
            D(np.ascontiguousarray(pts2[:, 1])), m, V0, DV, K, 1, sr.KERNEL_IDS["cubic_column"], flags,
            _lib.ptr(out0), _lib.ptr(out1), 0, None))
        return out0.reshape(m, K)

    want = c_abi(A, None, 0)
    assert np.count_nonzero(want) > m * K // 4
    tens = lambda x: torch.tensor(x, dtype=torch.float64, device="cuda")  # noqa: E731
    for pts in (pts2, pts3):
        got = sightline_spectra(pos, h, A, vc, b, pts, "xyz"[axis], V0, DV, K, ring=True)
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (m, K)
        assert np.all(np.abs(got - want) <= 2.0 ** -23 * np.abs(want))
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        got = sightline_spectra(tens(pos), tens(h), tens(A), tens(vc), tens(b), tens(pts3), axis, V0, DV,
                                K, ring=True, stream=st)
    st.synchronize()
    assert got.is_cuda and tuple(got.shape) == (m, K)
    assert np.all(np.abs(got.cpu().numpy() - want) <= 2.0 ** -23 * np.abs(want))
    # a window is the ring without what wraps into it; the default is the window
    win = sightline_spectra(pos, h, A, vc, b, pts3, axis, V0, DV, K)
    assert np.all(win <= want * (1 + 2.0 ** -22)) and win.sum() < 0.95 * want.sum()
    # the ratio form
    want = c_abi(A * wgt, wgt, _lib.ASP_F_RATIO)
    got = sightline_spectra(pos, h, A, vc, b, pts2, axis, V0, DV, K, ring=True, weights=wgt)
    assert np.all(np.abs(got - want) <= 2.0 ** -22 * np.abs(want))
    got = sightline_spectra(tens(pos), tens(h), tens(A), tens(vc), tens(b), tens(pts2), axis, V0, DV, K,
                            ring=True, weights=tens(wgt))
    assert np.all(np.abs(got.cpu().numpy() - want) <= 2.0 ** -22 * np.abs(want))
    assert 0.5 * (1 - 1e-6) <= want[want != 0].min() and want.max() <= 2.0 * (1 + 1e-6)


# ------------------------------------------------------------- 9. stage and counters
def test_stage_and_counters(gpu, oracle, monkeypatch):
    """ASP_SAMPLE_COUNT: stats[9] = pairs tested, stats[10] = (pair, bin) adds -- every
    included pair's bins that meet vc +- T b, at most one more at either end (the run's ends
    are moved outwards by 2^-40) -- and the other counters 0; the prep is stage sample_prep,
    the zeroing, the deposit and the finalising pass are three launches of spectra_deposit."""
    from asp_amd import _lib
    _knobs(monkeypatch)
    monkeypatch.setenv("ASP_SAMPLE_COUNT", "1")
    K = 200
    ref = reference(oracle, "cubic", K, True)
    c, vc, b = ref["c"], ref["vc"], ref["b"]
    _lib.profile(0, True)
    spectra(c, vc, b, K, True, "cubic")
    prof = _lib.profile_read(0)
    _lib.profile(0, False)
    st = _lib.last_stats(0)
    s, p, _ = spr.pairs(c["u"], c["v"], c["h"], c["px"], c["py"])
    run = (np.floor((vc + spr.T * b - V0) / DV) - np.floor((vc - spr.T * b - V0) / DV) + 1.0)[p]
    assert s.size == ref["cnt"].sum()
    assert s.size <= st["evals"] < c["px"].size * c["h"].size, st
    assert run.sum() <= st["evals_small"] <= run.sum() + 2 * s.size, (st, run.sum())
    assert all(st[k] == 0 for k in st if k not in ("evals", "evals_small")), st
    assert prof["sample_prep"][1] == 1 and prof["spectra_deposit"][1] == 3, prof
    assert prof["sample_deposit"][1] == 0
    monkeypatch.setenv("ASP_SAMPLE_CELLS", "1")  # one cell: every admitted particle, every sightline
    spectra(c, vc, b, K, True, "cubic")
    assert _lib.last_stats(0)["evals"] == c["px"].size * c["h"].size
