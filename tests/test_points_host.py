"""3-D point sampling (asp_sample3d, asp_sample3d_f64, asp_amd.sample_points,
asp_amd.sightline_profiles): what holds without a GPU -- every argument error is returned
before any device work, m == 0 and (for host arrays) n == 0 need no device, the two symbols
are exported with the prototypes of include/asp_points.h, and the Python wrappers refuse bad
arguments with ValueError before any native call.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args32(**kw):
    from asp_amd import _lib
    f = np.zeros(4, np.float32)
    d = np.zeros(4)
    a = dict(x=f, y=f, z=f, h=f, a0=f, a1=None, n=4, px=d, py=d, pz=d, m=4, kid=0, flags=0,
             out0=np.zeros(4, np.float32), out1=None)
    a.update(kw)
    if a.pop("pair", False):  # a second sum: a1 and out1 together
        a["a1"], a["out1"] = f, np.zeros(4, np.float32)
    P, D = _lib.ptr, (lambda t: _lib.ptr(t, _lib._d))
    return (P(a["x"]), P(a["y"]), P(a["z"]), P(a["h"]), P(a["a0"]), P(a["a1"]), a["n"], D(a["px"]),
            D(a["py"]), D(a["pz"]), a["m"], a["kid"], a["flags"], P(a["out0"]), P(a["out1"]), 0, None)


def _args64(**kw):
    from asp_amd import _lib
    d = np.zeros(4)
    a = dict(pos=np.zeros((4, 3)), h=d, a0=d, a1=None, n=4, px=d, py=d, pz=d, m=4, kid=0,
             flags=0, out0=np.zeros(4, np.float32), out1=None)
    a.update(kw)
    if a.pop("pair", False):
        a["a1"], a["out1"] = d, np.zeros(4, np.float32)
    P, D = _lib.ptr, (lambda t: _lib.ptr(t, _lib._d))
    return (D(a["pos"]), D(a["h"]), D(a["a0"]), D(a["a1"]), a["n"], D(a["px"]), D(a["py"]),
            D(a["pz"]), a["m"], a["kid"], a["flags"], P(a["out0"]), P(a["out1"]), 0, None)


F32 = np.zeros(4, np.float32)
BOTH = [dict(n=-1), dict(m=-1), dict(kid=-1), dict(kid=3), dict(kid=4), dict(kid=5),
        dict(px=None), dict(py=None), dict(pz=None), dict(out0=None), dict(a0=None), dict(h=None),
        dict(out1=F32), dict(flags=0x10), dict(flags=0x2), dict(flags=0x2 | 0x8, pair=True),
        dict(flags=0x2 | 0x4, pair=True), dict(flags=0x10, pair=True)]
ONLY32 = [dict(x=None), dict(y=None), dict(z=None), dict(a1=F32)]
ONLY64 = [dict(pos=None), dict(a1=np.zeros(4))]


def _id(kw):
    return "-".join(f"{k}={'arr' if isinstance(v, np.ndarray) else v}" for k, v in kw.items())


@pytest.mark.parametrize("kw", BOTH + ONLY32, ids=_id)
def test_sample3d_argument_errors_before_any_device_work(asp, kw):
    from asp_amd import _lib
    L = _lib.lib()
    rc = L.asp_sample3d(*_args32(**kw))
    assert rc == _lib.ASP_ERR_INVALID and L.asp_last_error().decode(), kw


@pytest.mark.parametrize("kw", BOTH + ONLY64, ids=_id)
def test_sample3d_f64_argument_errors_before_any_device_work(asp, kw):
    from asp_amd import _lib
    L = _lib.lib()
    rc = L.asp_sample3d_f64(*_args64(**kw))
    assert rc == _lib.ASP_ERR_INVALID and L.asp_last_error().decode(), kw


def test_sizes_that_need_no_device(asp):
    from asp_amd import _lib
    L = _lib.lib()
    # m >= 2^31: unsupported (never dereferenced)
    assert L.asp_sample3d(*_args32(m=1 << 31)) == _lib.ASP_ERR_UNSUPPORTED
    assert L.asp_sample3d_f64(*_args64(m=1 << 31)) == _lib.ASP_ERR_UNSUPPORTED
    assert "2^31" in L.asp_last_error().decode()
    # m == 0 is valid with NULL point arrays and outputs
    none = dict(m=0, px=None, py=None, pz=None, out0=None)
    assert L.asp_sample3d(*_args32(**none)) == _lib.ASP_OK
    assert L.asp_sample3d_f64(*_args64(**none)) == _lib.ASP_OK
    # n == 0 on host arrays: zeros, or untouched under ASP_F_ACCUMULATE
    out0, out1 = np.full(4, 7.0, np.float32), np.full(4, 7.0, np.float32)
    rc = L.asp_sample3d(*_args32(n=0, x=None, y=None, z=None, h=None, a0=None, out0=out0))
    assert rc == _lib.ASP_OK and np.all(out0 == 0)
    out0[:] = 7.0
    rc = L.asp_sample3d_f64(*_args64(n=0, pos=None, h=None, a0=None, a1=np.zeros(4), out0=out0,
                                     out1=out1, flags=_lib.ASP_F_ACCUMULATE))
    assert rc == _lib.ASP_OK and np.all(out0 == 7.0) and np.all(out1 == 7.0)
    rc = L.asp_sample3d_f64(*_args64(n=0, pos=None, h=None, a0=None, a1=np.zeros(4), out0=out0,
                                     out1=out1))
    assert rc == _lib.ASP_OK and np.all(out0 == 0) and np.all(out1 == 0)


def _declared():
    """{name: parameter count} of every function include/asp_points.h declares."""
    hdr = open(os.path.join(REPO, "include", "asp_points.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(asp_\w+)\s*\(([^)]*)\)\s*;", hdr):
        out[m.group(1)] = len([p for p in m.group(2).split(",") if p.strip()])
    return out


def test_symbols_and_prototypes(asp):
    from asp_amd import _lib
    L = _lib.lib()
    declared = _declared()
    assert set(declared) == {"asp_sample3d", "asp_sample3d_f64"} == set(_lib.POINT_PROTOTYPES)
    for name, nparams in declared.items():
        fn = getattr(L, name)  # exported
        assert len(_lib.POINT_PROTOTYPES[name]) == nparams == len(fn.argtypes), name
        assert fn.restype is C.c_int
    assert L.asp_sample3d.argtypes[7] == C.POINTER(C.c_double)
    assert L.asp_sample3d_f64.argtypes[0] == C.POINTER(C.c_double)
    # the table of asp.h and the stage names are as they were
    assert len(_lib.PROTOTYPES) == 34 and not set(_lib.PROTOTYPES) & set(declared)
    assert _lib.ALL_STAGES[21:] == ("sample_prep", "sample_deposit")


def test_sample_points_refuses_bad_arguments():
    """ValueError before any native call (there is no GPU here)."""
    from asp_amd import sample_points
    pos, h, a, pts = np.zeros((4, 3)), np.ones(4), np.ones(4), np.zeros((5, 3))
    with pytest.raises(ValueError, match="shape"):
        sample_points(np.zeros((4, 2)), h, a, pts)
    with pytest.raises(ValueError, match="float64"):
        sample_points(pos.astype(np.float32), h, a, pts)
    with pytest.raises(ValueError, match="smoothing_lengths"):
        sample_points(pos, np.ones(3), a, pts)
    with pytest.raises(ValueError, match="particle_properties"):
        sample_points(pos, h, a.astype(np.float32), pts)
    with pytest.raises(ValueError, match="weights"):
        sample_points(pos, h, a, pts, weights=np.ones(5))
    with pytest.raises(ValueError, match="points"):
        sample_points(pos, h, a, np.zeros((5, 2)))
    with pytest.raises(ValueError, match="points"):
        sample_points(pos, h, a, np.zeros(5))
    with pytest.raises(ValueError, match="points"):
        sample_points(pos, h, a, pts.astype(np.float32))
    with pytest.raises(ValueError, match="kernel"):
        sample_points(pos, h, a, pts, kernel="gaussian")
    for column in ("cubic_column", "wendland_c2_column"):
        with pytest.raises(ValueError, match="column"):
            sample_points(pos, h, a, pts, kernel=column)
    with pytest.raises(ValueError, match="deterministic"):
        sample_points(pos, h, a, pts, weights=h, deterministic=True)
    out = sample_points(pos, h, a, np.zeros((0, 3)))
    assert out.shape == (0,) and out.dtype == np.float32


def test_sightline_profiles_refuses_bad_arguments():
    from asp_amd import sightline_profiles
    pos, h, a = np.zeros((4, 3)), np.ones(4), np.ones(4)
    st, d = np.zeros((2, 3)), np.array([[0.0, 0.0, 1.0], [1.0, 1.0, 0.0]])
    with pytest.raises(ValueError, match="directions"):
        sightline_profiles(pos, h, a, st, np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 0.0]]), 1.0, 4)
    with pytest.raises(ValueError, match="directions"):
        sightline_profiles(pos, h, a, st, np.array([[0.0, np.nan, 1.0], [0.0, 1.0, 0.0]]), 1.0, 4)
    with pytest.raises(ValueError, match="directions"):
        sightline_profiles(pos, h, a, st, d[:1], 1.0, 4)
    with pytest.raises(ValueError, match="n_bins"):
        sightline_profiles(pos, h, a, st, d, 1.0, 0)
    with pytest.raises(ValueError, match="lengths"):
        sightline_profiles(pos, h, a, st, d, -1.0, 4)
    with pytest.raises(ValueError, match="lengths"):
        sightline_profiles(pos, h, a, st, d, np.ones(3), 4)
    with pytest.raises(ValueError, match="starts"):
        sightline_profiles(pos, h, a, np.zeros((2, 2)), d, 1.0, 4)
    with pytest.raises(ValueError, match="float64"):
        sightline_profiles(pos, h, a, st.astype(np.float32), d, 1.0, 4)
    with pytest.raises(ValueError, match="column"):
        sightline_profiles(pos, h, a, st, d, 1.0, 4, kernel="cubic_column")
    with pytest.raises(ValueError, match="deterministic"):
        sightline_profiles(pos, h, a, st, d, 1.0, 4, weights=h, deterministic=True)
    with pytest.raises(ValueError, match="shape"):
        sightline_profiles(np.zeros((4, 2)), h, a, np.zeros((0, 3)), np.zeros((0, 3)), 1.0, 4)
    # no sightlines: empty results, no device needed
    out, pts = sightline_profiles(pos, h, a, np.zeros((0, 3)), np.zeros((0, 3)), 1.0, 4,
                                  return_points=True)
    assert out.shape == (0, 4) and out.dtype == np.float32 and pts.shape == (0, 4, 3)


def test_sightline_points_formula():
    """X[s, b] = start + ((b + 0.5) (length / n_bins)) d / |d|, in this order, on the host."""
    from asp_amd.points import sightline_points
    rng = np.random.default_rng(7)
    st, d, L = rng.uniform(-1, 1, (5, 3)), rng.normal(size=(5, 3)), rng.uniform(0.5, 3.0, 5)
    pts = sightline_points(st, d, L, 6)
    assert pts.shape == (5, 6, 3) and pts.dtype == np.float64
    for s in range(5):
        unit = d[s] / np.sqrt(d[s, 0] * d[s, 0] + d[s, 1] * d[s, 1] + d[s, 2] * d[s, 2])
        for b in range(6):
            assert np.array_equal(pts[s, b], st[s] + ((b + 0.5) * (L[s] / 6)) * unit)
    assert np.array_equal(sightline_points(st, d, 2.0, 3), sightline_points(st, d, np.full(5, 2.0), 3))
