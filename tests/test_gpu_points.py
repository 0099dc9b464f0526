"""3-D point sampling on the GPU: asp_sample3d, asp_sample3d_f64, asp_amd.sample_points and
asp_amd.sightline_profiles.

The contract (include/asp_points.h) is asp_project3d's voxel test at arbitrary points.  On
the voxel lattice that is the cube, so the references there are the oracle's cube and the
cube's own per-voxel bar (tests/value_bar.py); off the lattice the reference is the fp64
brute force of tests/sample3d_ref.py (tied to the oracle on the lattice by
tests/test_sample3d_ref.py) and the SAME bar, e_p summed over each point's exact neighbour
set, with pitch = 0: the sampler forms the pair difference in fp64, so there is no frame
term, and the one fp32 rounding of r2 is inside the bar's 2^-21 2h.  Neighbour counts are
exact everywhere.

Every class of the deposit (a lane per particle / the wave per particle, in both walk
forms) and several grids are forced with ASP_SAMPLE_WIDE_CELLS, ASP_SAMPLE3D_WALK and
ASP_SAMPLE_CELLS.  Every case prints its worst err/E (``pytest -s``).
"""
import numpy as np
import pytest

import sample3d_ref as s3
import sightline_ref as sr
import value_bar as vb

pytestmark = pytest.mark.gpu

BIG = str(1 << 30)
# (ASP_SAMPLE_CELLS, ASP_SAMPLE_WIDE_CELLS with ASP_SAMPLE_WIDE_POINTS, ASP_SAMPLE3D_WALK): one
# cell / 7^3 / the default grid; every particle taken by the wave (0), walking the concatenated
# rows (flat) or row by row (row), or by its lane (2^30); or split by the default thresholds
SETTINGS = {"default": (None, None, None),
            "cells1_wave_flat": ("1", "0", "1"), "cells1_wave_row": ("1", "0", "0"),
            "cells1_lane": ("1", BIG, None),
            "cells7_wave_flat": ("7", "0", "1"), "cells7_wave_row": ("7", "0", "0"),
            "cells7_lane": ("7", BIG, None),
            "default_wave_flat": (None, "0", "1"), "default_wave_row": (None, "0", "0"),
            "default_lane": (None, BIG, None), "default_row": (None, None, "0"),
            # the flat walk's per-chunk choice (ASP_SAMPLE3D_WALK_MIX): never row by row (0),
            # nearly always (64); the rows above run the default
            "cells7_wave_mix0": ("7", "0", "1", "0"), "cells7_wave_mix64": ("7", "0", "1", "64"),
            "default_wave_mix0": (None, "0", "1", "0"), "default_wave_mix64": (None, "0", "1", "64")}


def _knobs(monkeypatch, setting="default"):
    cells, wide, walk, mix = (SETTINGS[setting] + (None,))[:4]
    for name, val in (("ASP_SAMPLE_CELLS", cells), ("ASP_SAMPLE_WIDE_CELLS", wide),
                      ("ASP_SAMPLE_WIDE_POINTS", wide), ("ASP_SAMPLE3D_WALK", walk),
                      ("ASP_SAMPLE3D_WALK_MIX", mix),
                      ("ASP_MAX_BATCH", None), ("ASP_SAMPLE_COUNT", None)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)


def _report(label, worst):
    print(f"POINTS_BAR {label}: worst err/E = {worst:.3f}")


def _f32(t):
    return None if t is None else np.ascontiguousarray(t, np.float32)


def _f64(t):
    return None if t is None else np.ascontiguousarray(t, np.float64)


def _outs(m, second, out0, out1):
    if out0 is None:
        out0 = np.full(m, np.nan, np.float32)
    if second and out1 is None:
        out1 = np.full(m, np.nan, np.float32)
    return out0, out1


def sample(x, y, z, h, a0, px, py, pz, kernel, a1=None, flags=0, out0=None, out1=None):
    """asp_sample3d on host arrays; returns (out0, out1) as float64."""
    from asp_amd import _lib
    x, y, z, h, a0, a1 = (_f32(t) for t in (x, y, z, h, a0, a1))
    px, py, pz = _f64(px), _f64(py), _f64(pz)
    out0, out1 = _outs(px.size, a1 is not None, out0, out1)
    P, D = _lib.ptr, (lambda t: _lib.ptr(t, _lib._d))
    _lib.check(_lib.lib().asp_sample3d(P(x), P(y), P(z), P(h), P(a0), P(a1), x.size, D(px), D(py),
                                       D(pz), px.size, s3.KERNEL_IDS[kernel], flags, P(out0),
                                       P(out1), 0, None))
    return out0.astype(np.float64), None if out1 is None else out1.astype(np.float64)


def sample64(pos, h, a0, px, py, pz, kernel, a1=None, flags=0):
    """asp_sample3d_f64 on host arrays."""
    from asp_amd import _lib
    pos, h, a0, a1, px, py, pz = (_f64(t) for t in (pos, h, a0, a1, px, py, pz))
    out0, out1 = _outs(px.size, a1 is not None, None, None)
    P, D = _lib.ptr, (lambda t: _lib.ptr(t, _lib._d))
    _lib.check(_lib.lib().asp_sample3d_f64(D(pos), D(h), D(a0), D(a1), h.size, D(px), D(py), D(pz),
                                           px.size, s3.KERNEL_IDS[kernel], flags, P(out0), P(out1),
                                           0, None))
    return out0.astype(np.float64), None if out1 is None else out1.astype(np.float64)


def xyz(s):
    return s["x"], s["y"], s["z"]


_cache = {}


def _cached(key, make):
    if key not in _cache:
        v = make()
        for t in (v.values() if isinstance(v, dict) else [v]):
            if isinstance(t, np.ndarray):
                t.setflags(write=False)
        _cache[key] = v
    return _cache[key]


# ------------------------------------------------------------ 1. parity on the lattice
def shuffled_lattice():
    def make():
        px, py, pz = s3.lattice()
        perm = np.random.default_rng(41).permutation(px.size)
        return dict(px=px[perm], py=py[perm], pz=pz[perm], perm=perm)
    return _cached("lattice", make)


def unshuffle(g, perm):
    out = np.empty_like(g)
    out[perm] = g
    return out.reshape(vb.SIZE3D)


def lattice_counts(oracle):
    def make():
        s = vb.cube_set(oracle, "cubic")  # the positions and h are the same for every kernel
        return oracle.project3d(*xyz(s), s["h"], np.ones(s["h"].size), vb.SIZE3D, vb.EXT3D,
                                kernel="indicator")
    return _cached("lattice_counts", make)


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("kernel", vb.KERNELS)
def test_lattice_parity(gpu, oracle, monkeypatch, kernel, setting):
    """The 122 880 voxel corners in a shuffled order: the oracle's cube under the cube's bar,
    and the indicator's counts exactly, for every grid, deposit class and walk form."""
    _knobs(monkeypatch, setting)
    s = vb.cube_set(oracle, kernel)
    ref = vb.reference3d(oracle, kernel)
    L = shuffled_lattice()
    g, _ = sample(*xyz(s), s["h"], s["a"], L["px"], L["py"], L["pz"], kernel)
    w = vb.assert_terms_close(unshuffle(g, L["perm"]), ref["r"], ref["E"], ref["by_class"])
    _report(f"lattice {kernel} {setting}", w)
    c, _ = sample(*xyz(s), s["h"], np.ones(s["h"].size), L["px"], L["py"], L["pz"], "indicator")
    assert np.array_equal(unshuffle(c, L["perm"]), lattice_counts(oracle))


# ------------------------------------------------------------------ 2. off the lattice
N_UNIFORM, N_FAR, N_SELF, N_CROWD, N_COPIES, N_LINES, N_BINS = 1500, 100, 50, 8, 64, 16, 64
CROWD = slice(N_UNIFORM + N_FAR + N_SELF, N_UNIFORM + N_FAR + N_SELF + N_CROWD * N_COPIES)


def offlattice_points(s):
    """default_rng(33): 1 500 points uniform in +-2.6, 100 in [8, 9]^3 (no neighbour; they
    stretch the bounding box), the first 50 particle positions (r = 0), 8 positions in +-1
    copied 64 times each (crowded cells), 16 sightlines x 64 bins of length 3."""
    from asp_amd.points import sightline_points
    rng = np.random.default_rng(33)
    uni = rng.uniform(-2.6, 2.6, (N_UNIFORM, 3))
    far = rng.uniform(8.0, 9.0, (N_FAR, 3))
    own = np.stack([t[:N_SELF] for t in xyz(s)], axis=1)
    crowd = np.repeat(rng.uniform(-1.0, 1.0, (N_CROWD, 3)), N_COPIES, axis=0)
    lines = sightline_points(rng.uniform(-1.5, 1.5, (N_LINES, 3)), rng.normal(size=(N_LINES, 3)),
                             3.0, N_BINS).reshape(-1, 3)
    pts = np.concatenate([uni, far, own, crowd, lines])
    return tuple(np.ascontiguousarray(pts[:, d]) for d in range(3))


def offlattice_reference(oracle, kernel):
    """The cube set (a1 = a, a0 = fl32(a T)) at the off-lattice points: r0 / r1, E0 / E1, the
    counts, the fixed-point terms and, per class, the number of points it reaches."""
    def make():
        s = vb.cube_set(oracle, kernel)
        T = vb.f32(np.random.default_rng(34).uniform(1.0, 3.0, s["h"].size))
        a0 = vb.f32(s["a"] * T)
        px, py, pz = offlattice_points(s)
        (r0, r1), (E0, E1), cnt = s3.reference(oracle, kernel, *xyz(s), s["h"], [a0, s["a"]],
                                               px, py, pz)
        per_class, _ = s3.brute(*xyz(s), s["h"], px, py, pz,
                                [((s["cls"] == k).astype(np.float64), None)
                                 for k in range(len(vb.CLASSES_3D))])
        return dict(x=s["x"], y=s["y"], z=s["z"], h=s["h"], a=s["a"], a0=a0, px=px, py=py, pz=pz,
                    r0=r0, r1=r1, E0=E0, E1=E1, cnt=cnt,
                    reached=np.array([np.count_nonzero(c) for c in per_class]),
                    F0=sr.fixed_point_term(oracle, kernel, s["h"], a0),
                    F1=sr.fixed_point_term(oracle, kernel, s["h"], s["a"]))
    return _cached(("off", kernel), make)


def pts(c):
    return c["px"], c["py"], c["pz"]


@pytest.mark.parametrize("setting", ["default", "cells7_wave_flat", "cells7_wave_row", "cells7_lane",
                                     "cells1_wave_flat", "default_wave_flat", "default_row",
                                     "cells7_wave_mix0", "default_wave_mix64"])
@pytest.mark.parametrize("kernel", vb.KERNELS)
def test_off_lattice(gpu, oracle, monkeypatch, kernel, setting):
    _knobs(monkeypatch, setting)
    c = offlattice_reference(oracle, kernel)
    assert np.count_nonzero(c["cnt"] == 0) >= 100, "points with no neighbour"
    assert np.all(c["reached"] >= 1000), c["reached"]
    assert np.all(c["cnt"][N_UNIFORM:N_UNIFORM + N_FAR] == 0)
    g0, g1 = sample(*xyz(c), c["h"], c["a0"], *pts(c), kernel, a1=c["a"])
    w = max(vb.assert_terms_close(g0, c["r0"], c["E0"]), vb.assert_terms_close(g1, c["r1"], c["E1"]))
    _report(f"off-lattice {kernel} {setting}", w)
    assert np.all(g0[c["cnt"] == 0] == 0) and np.all(g1[c["cnt"] == 0] == 0)
    cnt, _ = sample(*xyz(c), c["h"], np.ones(c["h"].size), *pts(c), "indicator")
    assert np.array_equal(cnt, c["cnt"])


# ---------------------------------------------------------------- 3. the fp64 entry
@pytest.mark.parametrize("kernel", vb.KERNELS)
def test_fp64_entry_far_from_the_origin(gpu, oracle, monkeypatch, kernel):
    """The cube set moved by CUBE_SHIFT plus a perturbation below the fp32 spacing there (raw
    fp64 positions, h and a), the points moved alike: decisions on the fp64 values themselves
    (counts exact), values under the bar with pitch = 0 and F64_INPUT_ULPS."""
    _knobs(monkeypatch)
    s = vb.cube_set(oracle, kernel, vb.CUBE_SHIFT)
    base = vb.cube_set(oracle, kernel)
    rng = np.random.default_rng(35)
    n = s["h"].size
    pos = np.stack(xyz(s), axis=1) + rng.uniform(-2.0 ** -20, 2.0 ** -20, (n, 3))
    h = s["h"] * (1.0 + rng.uniform(-2.0 ** -26, 2.0 ** -26, n))
    a0 = s["a"] * (1.0 + rng.uniform(-2.0 ** -26, 2.0 ** -26, n))
    T = rng.uniform(1.0, 3.0, n)
    assert np.any(pos != vb.f32(pos)) and np.any(h != vb.f32(h))
    px, py, pz = (p + vb.CUBE_SHIFT[d] + rng.uniform(-2.0 ** -20, 2.0 ** -20, p.size)
                  for d, p in enumerate(offlattice_points(base)))
    (r0, r1), (E0, E1), cnt = s3.reference(oracle, kernel, pos[:, 0], pos[:, 1], pos[:, 2], h,
                                           [a0 * T, a0], px, py, pz,
                                           extra_ulps=vb.F64_INPUT_ULPS)
    g0, g1 = sample64(pos, h, a0 * T, px, py, pz, kernel, a1=a0)
    w = max(vb.assert_terms_close(g0, r0, E0), vb.assert_terms_close(g1, r1, E1))
    _report(f"fp64 {kernel}", w)
    c, _ = sample64(pos, h, np.ones(n), px, py, pz, "indicator")
    assert np.array_equal(c, cnt) and cnt.max() > 10


# ----------------------------------------------------------------------- 4. flags
@pytest.mark.parametrize("kernel", vb.KERNELS)
def test_ratio(gpu, oracle, monkeypatch, kernel):
    """out0 / out1 with the components' bars propagated: for g_i = r_i + d_i, |d_i| <= E_i,
    |g0/g1 - r0/r1| <= (E0 + |r0/r1| E1) / (|r1| - E1), plus the fp32 division and its
    rounding (<= 2.5 ulp = 5 * 2^-24 relative; 2^-21 taken).  0 exactly where no particle
    reaches the point."""
    from asp_amd import _lib
    _knobs(monkeypatch)
    c = offlattice_reference(oracle, kernel)
    g, _ = sample(*xyz(c), c["h"], c["a0"], *pts(c), kernel, a1=c["a"], flags=_lib.ASP_F_RATIO)
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


@pytest.mark.parametrize("kernel", vb.KERNELS)
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
        g0, g1 = sample(*(t[half] for t in xyz(c)), c["h"][half], c["a0"][half], *pts(c), kernel,
                        a1=c["a"][half], flags=flags, out0=out0, out1=out1)
    for g, r, E in ((g0, c["r0"], c["E0"]), (g1, c["r1"], c["E1"])):
        assert np.all(g[r == 0] == 0)
        assert np.all(np.abs(g - r) <= E + 2.0 ** -24 * np.abs(r))


@pytest.mark.parametrize("kernel", vb.KERNELS)
def test_deterministic(gpu, oracle, monkeypatch, kernel):
    """Bitwise equal under a permutation of the particles, of the points, in every settings
    row, in batches, and from device pointers on a side stream; within E + fixed_point_term."""
    import torch
    from asp_amd import _lib
    _knobs(monkeypatch)
    c = offlattice_reference(oracle, kernel)
    det = _lib.ASP_F_DETERMINISTIC
    args = xyz(c) + (c["h"], c["a0"])
    g0, g1 = sample(*args, *pts(c), kernel, a1=c["a"], flags=det)
    w = max(vb.assert_terms_close(g0, c["r0"], c["E0"], floor=c["F0"]),
            vb.assert_terms_close(g1, c["r1"], c["E1"], floor=c["F1"]))
    _report(f"deterministic {kernel}", w)
    crowd = g0[CROWD].reshape(N_CROWD, N_COPIES)
    assert np.all(crowd == crowd[:, :1])  # copies of one point: one value
    rng = np.random.default_rng(36)
    p = rng.permutation(c["h"].size)
    h0, h1 = sample(*(t[p] for t in args), *pts(c), kernel, a1=c["a"][p], flags=det)
    assert np.array_equal(h0, g0) and np.array_equal(h1, g1)
    q = rng.permutation(c["px"].size)
    h0, h1 = sample(*args, *(t[q] for t in pts(c)), kernel, a1=c["a"], flags=det)
    assert np.array_equal(h0, g0[q]) and np.array_equal(h1, g1[q])
    for setting in SETTINGS:
        _knobs(monkeypatch, setting)
        h0, _ = sample(*args, *pts(c), kernel, flags=det)
        assert np.array_equal(h0, g0), setting
    _knobs(monkeypatch)
    monkeypatch.setenv("ASP_MAX_BATCH", "1000")  # for_batches' knob: four batches
    h0, h1 = sample(*args, *pts(c), kernel, a1=c["a"], flags=det)
    assert np.array_equal(h0, g0) and np.array_equal(h1, g1)
    monkeypatch.delenv("ASP_MAX_BATCH")
    # device pointers, a side stream
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        t = [torch.tensor(np.asarray(v), dtype=torch.float32, device="cuda") for v in args + (c["a"],)]
        tp = [torch.tensor(np.asarray(v), dtype=torch.float64, device="cuda") for v in pts(c)]
        o0 = torch.full((c["px"].size,), float("nan"), dtype=torch.float32, device="cuda")
        o1 = torch.full_like(o0, float("nan"))
        P, D = _lib.ptr, (lambda v: _lib.ptr(v, _lib._d))
        _lib.check(_lib.lib().asp_sample3d(
            P(t[0]), P(t[1]), P(t[2]), P(t[3]), P(t[4]), P(t[5]), c["h"].size, D(tp[0]), D(tp[1]),
            D(tp[2]), c["px"].size, s3.KERNEL_IDS[kernel], det | _lib.ASP_F_DEVICE_PTRS, P(o0),
            P(o1), 0, st.cuda_stream))
    st.synchronize()
    assert np.array_equal(o0.cpu().numpy().astype(np.float64), g0)
    assert np.array_equal(o1.cpu().numpy().astype(np.float64), g1)
    with pytest.raises(ValueError, match="ASP_F_RATIO"):
        sample(*args, *pts(c), kernel, a1=c["a"], flags=det | _lib.ASP_F_RATIO)


def test_batches_and_device_edges(gpu, oracle, monkeypatch):
    """ASP_MAX_BATCH forces batch boundaries in fp64 mode: the same neighbour sets, the same
    bar.  n == 0 with device pointers: zeros on the stream, untouched under accumulate."""
    import torch
    from asp_amd import _lib
    _knobs(monkeypatch)
    monkeypatch.setenv("ASP_MAX_BATCH", "777")
    c = offlattice_reference(oracle, "cubic")
    g0, g1 = sample(*xyz(c), c["h"], c["a0"], *pts(c), "cubic", a1=c["a"])
    vb.assert_terms_close(g0, c["r0"], c["E0"])
    vb.assert_terms_close(g1, c["r1"], c["E1"])
    cnt, _ = sample(*xyz(c), c["h"], np.ones(c["h"].size), *pts(c), "indicator")
    assert np.array_equal(cnt, c["cnt"])
    monkeypatch.delenv("ASP_MAX_BATCH")
    tp = [torch.tensor(np.asarray(v), dtype=torch.float64, device="cuda") for v in pts(c)]
    out = torch.full((tp[0].numel(),), 7.0, dtype=torch.float32, device="cuda")
    D = lambda v: _lib.ptr(v, _lib._d)  # noqa: E731
    call = lambda flags: _lib.check(_lib.lib().asp_sample3d(  # noqa: E731
        None, None, None, None, None, None, 0, D(tp[0]), D(tp[1]), D(tp[2]), tp[0].numel(), 0,
        flags | _lib.ASP_F_DEVICE_PTRS, _lib.ptr(out), None, 0,
        torch.cuda.current_stream().cuda_stream))
    call(_lib.ASP_F_ACCUMULATE)
    assert torch.all(out == 7.0)
    call(0)
    assert torch.all(out == 0.0)
    # one point; only non-finite points
    k = CROWD.start
    g, _ = sample(*xyz(c), c["h"], c["a"], *(t[k:k + 1] for t in pts(c)), "cubic")
    vb.assert_terms_close(g, c["r1"][k:k + 1], c["E1"][k:k + 1])
    g, _ = sample(*xyz(c), c["h"], c["a"], np.full(5, np.nan), np.zeros(5), np.zeros(5), "cubic")
    assert np.all(g == 0)


# ------------------------------------------- 4b. what the 2-D and the 3-D sampler share
N_SHARED, M_SHARED_2D, M_SHARED_3D = 4096, 1500, 3000


def shared_reference(oracle):
    """4 096 particles drawn the way the cube set is (default_rng(39): positions uniform in
    +-2.2, h in the cube set's two narrow classes, a = U(0.5, 1.5) / W(0); the cube set itself
    has 3 624 and cannot be asked for more), a0 = fl32(a T); 1 500 points for the 2-D call
    (the x, y columns of particles and points) and 3 000 for the 3-D call, uniform in +-2.6.
    The references are the two files' brute forces, the bars have pitch = 0 (both samplers
    form the pair difference in fp64: no frame term)."""
    def make():
        rng = np.random.default_rng(39)
        h = vb.f32(rng.uniform(0.6, 3.0, N_SHARED) * vb.PITCH3D)
        x, y, z = (vb.f32(rng.uniform(-2.2, 2.2, N_SHARED)) for _ in range(3))
        a = vb.f32(rng.uniform(0.5, 1.5, N_SHARED) / vb.w0(oracle, "cubic", h))
        a0 = vb.f32(a * vb.f32(rng.uniform(1.0, 3.0, N_SHARED)))
        P = rng.uniform(-2.6, 2.6, (M_SHARED_3D, 3))
        px, py, pz = (np.ascontiguousarray(P[:, d]) for d in range(3))
        c = dict(x=x, y=y, z=z, h=h, a=a, a0=a0, px=px, py=py, pz=pz)
        c["r2"], c["E2"], c["cnt2"] = sr.reference(oracle, "cubic", x, y, h, [a0, a], px[:M_SHARED_2D],
                                                   py[:M_SHARED_2D], pitch=0.0)
        c["r3"], c["E3"], c["cnt3"] = s3.reference(oracle, "cubic", x, y, z, h, [a0, a], px, py, pz)
        c["F"] = [sr.fixed_point_term(oracle, "cubic", h, a0), sr.fixed_point_term(oracle, "cubic", h, a)]
        return c
    return _cached("shared", make)


def sample2d(u, v, h, a0, px, py, kernel, a1, flags):
    """asp_sample2d on host arrays, two sums; returns (out0, out1) as float64."""
    from asp_amd import _lib
    u, v, h, a0, a1 = (_f32(t) for t in (u, v, h, a0, a1))
    px, py = _f64(px), _f64(py)
    out0, out1 = _outs(px.size, True, None, None)
    P, D = _lib.ptr, (lambda t: _lib.ptr(t, _lib._d))
    _lib.check(_lib.lib().asp_sample2d(P(u), P(v), P(h), P(a0), P(a1), u.size, D(px), D(py), px.size,
                                       sr.KERNEL_IDS[kernel], flags, P(out0), P(out1), 0, None))
    return out0.astype(np.float64), out1.astype(np.float64)


@pytest.mark.parametrize("batch", [None, "1000"])
def test_2d_and_3d_calls_share_one_workspace(gpu, oracle, monkeypatch, batch):
    """asp_sample2d (1 500 points), asp_sample3d (3 000), and both again, in one process, from
    host fp32 arrays with two sums under ASP_F_DETERMINISTIC: the sorted coordinates of both
    live in one workspace slot, which grows between the calls, and the particle batches of
    both are staged through the same slots (coordinates, h, the two amplitudes sharing the
    last) -- in one batch and in five (ASP_MAX_BATCH=1000).  The repeats are bitwise equal
    (fixed-point sums do not depend on the order of the adds); every result is under the
    value bar (E + fixed_point_term) and every neighbour count is the oracle's."""
    from asp_amd import _lib
    _knobs(monkeypatch)
    if batch:
        monkeypatch.setenv("ASP_MAX_BATCH", batch)
    c = shared_reference(oracle)
    det, ones = _lib.ASP_F_DETERMINISTIC, np.ones(N_SHARED)
    p2 = (c["px"][:M_SHARED_2D], c["py"][:M_SHARED_2D])
    assert np.count_nonzero(c["cnt2"]) > 1000 and np.count_nonzero(c["cnt3"]) > 1000
    assert np.count_nonzero(c["cnt3"] == 0) > 100, "points with no neighbour"
    got = {2: [], 3: []}
    for _ in range(2):
        got[2].append(sample2d(c["x"], c["y"], c["h"], c["a0"], *p2, "cubic", c["a"], det))
        cnt = sample2d(c["x"], c["y"], c["h"], ones, *p2, "indicator", ones, 0)
        assert np.array_equal(cnt[0], c["cnt2"]) and np.array_equal(cnt[1], c["cnt2"])
        got[3].append(sample(*xyz(c), c["h"], c["a0"], *pts(c), "cubic", a1=c["a"], flags=det))
        cnt = sample(*xyz(c), c["h"], ones, *pts(c), "indicator", a1=ones)
        assert np.array_equal(cnt[0], c["cnt3"]) and np.array_equal(cnt[1], c["cnt3"])
    for dim in (2, 3):
        first, again = got[dim]
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]), dim
        for g in got[dim]:
            w = max(vb.assert_terms_close(g[i], c[f"r{dim}"][i], c[f"E{dim}"][i], floor=c["F"][i])
                    for i in range(2))
            _report(f"shared {dim}-D batch={batch}", w)


# ------------------------------------------------------------------- 5. odd values
ODD = dict(  # appended to a small ordinary set; (x, y, z, h, a)
    h_zero=(0.1, 0.1, 0.1, 0.0, 1.0), h_nan=(0.2, 0.1, 0.0, np.nan, 1.0),
    h_inf=(0.3, 0.1, 0.0, np.inf, 1.0), h_overflows_fp32=(0.3, 0.2, 0.0, 3.0e38, 1.0),
    x_nan=(np.nan, 0.1, 0.0, 0.2, 1.0), z_inf=(0.1, 0.0, np.inf, 0.2, 1.0),
    h_negative=(0.1, 0.2, 0.3, -0.2, 1.0), a_nan=(-0.5, -0.5, -0.5, 0.15, np.nan))


@pytest.mark.parametrize("kernel", vb.KERNELS)
def test_odd_values(gpu, oracle, monkeypatch, kernel):
    """h == 0, non-finite h or coordinates, an h whose 2h overflows fp32: in no neighbour set.
    h < 0: admitted, as in the oracle.  a = NaN: NaN at exactly the points inside its ball.
    Non-finite points read 0."""
    _knobs(monkeypatch)
    rng = np.random.default_rng(37)
    n = 300
    cols = [np.concatenate([rng.uniform(-1, 1, n), [o[d] for o in ODD.values()]]) for d in range(3)]
    h = np.concatenate([rng.uniform(0.05, 0.3, n), [o[3] for o in ODD.values()]])
    a = np.concatenate([rng.uniform(0.5, 1.5, n), [o[4] for o in ODD.values()]])
    x, y, z, h, a = (vb.f32(t) for t in (*cols, h, a))
    P = rng.uniform(-1.2, 1.2, (2000, 3))
    bad = np.array([[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.1, 0.2, -np.inf], [-0.5, -0.5, np.nan]])
    px, py, pz = (np.concatenate([P[:, d], bad[:, d]]) for d in range(3))
    adm = (np.isfinite(h) & (h != 0) & (np.abs(h) < 1e30) & np.isfinite(x) & np.isfinite(y)
           & np.isfinite(z))
    assert adm.sum() == n + 2  # the ordinary ones, h < 0 and a = NaN
    (want,), _ = s3.brute(x[adm], y[adm], z[adm], h[adm], px, py, pz, [(np.ones(adm.sum()), None)])
    g_cnt, _ = sample(x, y, z, h, np.ones(h.size), px, py, pz, "indicator")
    assert np.array_equal(g_cnt, want)
    neg = list(ODD).index("h_negative") + n
    (in_neg,), _ = s3.brute(x[neg:neg + 1], y[neg:neg + 1], z[neg:neg + 1], h[neg:neg + 1], px, py,
                            pz, [(np.ones(1), None)])
    assert 20 < in_neg.sum() < 120  # (4/3 pi 0.4^3 of 2.4^3: 39 of 2000 expected)
    g_val, _ = sample(x, y, z, h, a, px, py, pz, kernel)
    k = h.size - 1
    (in_ball,), _ = s3.brute(x[k:], y[k:], z[k:], h[k:], px, py, pz, [(np.ones(1), None)])
    nan = np.isnan(g_val)
    assert np.array_equal(nan, in_ball == 1) and 5 < nan.sum() < 50  # (16 expected)
    assert np.all(g_val[2000:] == 0) and np.all(g_cnt[2000:] == 0)
    # the rest, outside the negative-h ball (its term is no physical value): under the bar
    ok = adm & (h > 0) & np.isfinite(a)
    (r,), (E,), _ = s3.reference(oracle, kernel, x[ok], y[ok], z[ok], h[ok], [a[ok]], px, py, pz)
    rest = ~nan & (in_neg == 0)
    _report(f"odd {kernel}", vb.assert_terms_close(g_val[rest], r[rest], E[rest]))


# ----------------------------------------------------------- 6. counter and timing
def test_pair_counter_and_stage_timing(gpu, oracle, monkeypatch):
    """ASP_SAMPLE_COUNT: stats[9] = pairs tested -- with one cell, (admitted particles whose
    widened box meets the points' bounding box) x (finite points); never fewer than the pairs
    included.  asp_profile: launches under stages 21 and 22 only."""
    from asp_amd import _lib
    c = offlattice_reference(oracle, "cubic")
    evals = {}
    for setting in SETTINGS:
        _knobs(monkeypatch, setting)
        monkeypatch.setenv("ASP_SAMPLE_COUNT", "1")
        sample(*xyz(c), c["h"], c["a"], *pts(c), "cubic")
        st = _lib.last_stats(0)
        assert c["cnt"].sum() <= st["evals"] <= c["px"].size * c["h"].size, (setting, st)
        assert all(st[k] == 0 for k in st if k != "evals"), st
        evals[setting] = st["evals"]
    # the pairs tested depend on the grid alone, not on the class or the walk that tests them
    for grid in ("cells1", "cells7", "default"):
        same = {v for k, v in evals.items() if k.startswith(grid)}
        assert len(same) == 1, (grid, evals)
    # one cell, the crowded points (inside +-1) and two non-finite ones
    _knobs(monkeypatch, "cells1_lane")
    monkeypatch.setenv("ASP_SAMPLE_COUNT", "1")
    px, py, pz = (np.append(t[CROWD], odd) for t, odd in zip(pts(c), ([np.nan, 0.0], [0.0, np.inf],
                                                                     [0.0, 0.0])))
    nfinite = px.size - 2
    meets = np.ones(c["h"].size, bool)
    for q, p in zip(xyz(c), (px, py, pz)):
        r = 2.0 * np.abs(c["h"])
        rd = r * (1.0 + 2.0 ** -40) + np.abs(q) * 2.0 ** -40  # the kernel's widening
        meets &= (q + rd >= p[:nfinite].min()) & (q - rd <= p[:nfinite].max())
    assert 100 < meets.sum() < c["h"].size
    _lib.profile(0, True)
    sample(*xyz(c), c["h"], c["a"], px, py, pz, "cubic")
    prof = _lib.profile_read(0)
    _lib.profile(0, False)
    assert _lib.last_stats(0)["evals"] == meets.sum() * nfinite
    assert prof["sample_prep"][1] == 1 and prof["sample_deposit"][1] >= 2, prof
    assert all(v[1] == 0 for k, v in prof.items() if k not in ("sample_prep", "sample_deposit")), prof


# ------------------------------------------------------------------------ 7. Python
def test_python_wrappers(gpu, oracle, monkeypatch):
    """sample_points on host arrays and device tensors = the C call bit for bit (deterministic
    sums); the weighted form = the ratio; sightline_profiles = sample_points on its points."""
    import torch
    from asp_amd import _lib, sample_points, sightline_profiles
    from asp_amd.tools.projections import wendland_c2_kernel
    _knobs(monkeypatch)
    rng = np.random.default_rng(38)
    n, m = 3000, 700
    pos = rng.uniform(0.0, 1.0, (n, 3))
    h = rng.uniform(0.02, 0.1, n)
    A = rng.uniform(0.5, 2.0, n)
    wgt = rng.uniform(0.5, 2.0, n)
    P = rng.uniform(-0.05, 1.05, (m, 3))
    det = _lib.ASP_F_DETERMINISTIC
    want, _ = sample64(pos, h, A, P[:, 0], P[:, 1], P[:, 2], "wendland_c2", flags=det)
    assert np.count_nonzero(want) > m // 2
    got = sample_points(pos, h, A, P, kernel="wendland_c2", deterministic=True)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (m,)
    assert np.array_equal(got.astype(np.float64), want)
    tens = lambda t: torch.tensor(t, dtype=torch.float64, device="cuda")  # noqa: E731
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        got = sample_points(tens(pos), tens(h), tens(A), tens(P), kernel=wendland_c2_kernel,
                            deterministic=True, stream=st)
    st.synchronize()
    assert got.is_cuda and np.array_equal(got.cpu().numpy().astype(np.float64), want)
    # the ratio form (fp64 sums depend on the order of the atomic adds in their last bits:
    # each fp32 component may move by an ulp between two calls, the quotient by <= 4 * 2^-24)
    want, _ = sample64(pos, h, A * wgt, P[:, 0], P[:, 1], P[:, 2], "cubic", a1=wgt,
                       flags=_lib.ASP_F_RATIO)
    got = sample_points(pos, h, A, P, weights=wgt)
    assert np.all(np.abs(got - want) <= 2.0 ** -22 * np.abs(want))
    got = sample_points(tens(pos), tens(h), tens(A), tens(P), weights=tens(wgt)).cpu().numpy()
    assert np.all(np.abs(got - want) <= 2.0 ** -22 * np.abs(want))
    assert np.array_equal(got == 0, want == 0)
    assert 0.5 * (1 - 1e-6) <= want[want != 0].min() and want.max() <= 2.0 * (1 + 1e-6)
    # sightline profiles: the points within 2 ulp of the NumPy formula (exactly it on the
    # host), the profiles bitwise those of sample_points on the points
    S, nb = 40, 25
    starts, dirs = rng.uniform(0.0, 1.0, (S, 3)), rng.normal(size=(S, 3))
    lengths = rng.uniform(0.2, 1.0, S)
    unit = dirs / np.sqrt(dirs[:, 0] * dirs[:, 0] + dirs[:, 1] * dirs[:, 1] + dirs[:, 2] * dirs[:, 2])[:, None]
    X = starts[:, None, :] + ((np.arange(nb) + 0.5)[None, :] * (lengths / nb)[:, None])[:, :, None] * unit[:, None, :]
    prof, pts_h = sightline_profiles(pos, h, A, starts, dirs, lengths, nb, deterministic=True,
                                     return_points=True)
    assert prof.shape == (S, nb) and prof.dtype == np.float32 and pts_h.shape == (S, nb, 3)
    assert np.all(np.abs(pts_h - X) <= 2.0 * np.spacing(np.abs(X)))
    flat = sample_points(pos, h, A, pts_h.reshape(-1, 3), deterministic=True)
    assert np.array_equal(prof, flat.reshape(S, nb)) and np.count_nonzero(prof) > S * nb // 2
    prof_d, pts_d = sightline_profiles(tens(pos), tens(h), tens(A), tens(starts), tens(dirs),
                                       tens(lengths), nb, deterministic=True, return_points=True)
    pts_d = pts_d.cpu().numpy()
    assert np.all(np.abs(pts_d - X) <= 2.0 * np.spacing(np.abs(X)))
    flat = sample_points(pos, h, A, pts_d.reshape(-1, 3), deterministic=True)
    assert np.array_equal(prof_d.cpu().numpy(), flat.reshape(S, nb))
    # device tensors are not read back: a zero direction gives non-finite points, which read 0
    dirs0 = dirs.copy()
    dirs0[3] = 0.0
    prof_d = sightline_profiles(tens(pos), tens(h), tens(A), tens(starts), tens(dirs0), 0.5, nb)
    assert torch.all(prof_d[3] == 0) and torch.count_nonzero(prof_d) > 0
    # the weighted profile is the ratio
    got = sightline_profiles(pos, h, A, starts, dirs, lengths, nb, weights=wgt)
    want = sample_points(pos, h, A, pts_h.reshape(-1, 3), weights=wgt).reshape(S, nb)
    assert np.all(np.abs(got - want) <= 2.0 ** -22 * np.abs(want))


@pytest.mark.parametrize("kernel", vb.KERNELS)
def test_sightline_along_z_is_the_cubes_column(gpu, oracle, monkeypatch, kernel):
    """Sightlines along z through lattice columns (i, j), one bin per voxel, starting half a
    pitch below the cube: the z pitch 2^-4 and z_min = -2 make every bin centre the voxel
    corner bit for bit, so the profile is the cube's column under the lattice bar."""
    from asp_amd import sightline_profiles
    _knobs(monkeypatch)
    s = vb.cube_set(oracle, kernel)
    ref = vb.reference3d(oracle, kernel)
    nx, ny, nz = vb.SIZE3D
    ext = vb.EXT3D
    cols = [(0, 0), (5, 7), (24, 20), (47, 39), (13, 31)]
    pz = (ext[5] - ext[4]) / nz
    starts = np.array([[ext[0] + i * ((ext[1] - ext[0]) / nx), ext[2] + j * ((ext[3] - ext[2]) / ny),
                        ext[4] - 0.5 * pz] for i, j in cols])
    dirs = np.tile([0.0, 0.0, 2.5], (len(cols), 1))
    pos = np.stack(xyz(s), axis=1)
    prof, P = sightline_profiles(pos, s["h"], s["a"], starts, dirs, nz * pz, nz, kernel=kernel,
                                 return_points=True)
    assert np.array_equal(P[:, :, 2], np.tile(ext[4] + np.arange(nz) * pz, (len(cols), 1)))
    want = np.stack([ref["r"][i, j] for i, j in cols])
    E = np.stack([ref["E"][i, j] for i, j in cols])
    _report(f"z sightline {kernel}", vb.assert_terms_close(prof, want, E))
