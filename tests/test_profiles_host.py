"""Halo profiles (asp_halo_profiles, asp_amd.haloes.halo_profiles / aperture_sums): what holds
without a GPU -- every argument error is returned before any device work, m == 0 and (for host
arrays) n == 0 need no device, the symbol is exported with the prototype of
include/asp_profiles.h, and the Python wrappers refuse bad arguments with ValueError before any
native call.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(**kw):
    from asp_amd import _lib
    a = dict(pos=np.zeros((4, 3)), props=None, nprops=0, n=4, centres=np.zeros((4, 3)),
             radius=np.ones(4), m=4, edges=np.array([0.0, 1.0, 2.0]), nbins=2, box=1.0,
             count=np.zeros((4, 2), np.int64), sum=None, flags=0)
    a.update(kw)
    D = lambda t: _lib.ptr(t, _lib._d)  # noqa: E731
    return (D(a["pos"]), D(a["props"]), a["nprops"], a["n"], D(a["centres"]), D(a["radius"]),
            a["m"], D(a["edges"]), a["nbins"], a["box"], _lib.ptr(a["count"], _lib._i64),
            D(a["sum"]), a["flags"], 0, None)


P2, S2 = np.zeros((2, 4)), np.zeros((2, 4, 2))
ERRORS = [
    dict(n=-1), dict(m=-1), dict(nprops=-1), dict(nprops=5, props=np.zeros((5, 4))),
    dict(nbins=0), dict(nbins=65, edges=np.arange(66.0)), dict(nbins=-3),
    dict(pos=None), dict(centres=None), dict(count=None), dict(edges=None),
    dict(nprops=2, props=None, sum=S2), dict(nprops=2, props=P2, sum=None),
    dict(box=0.0), dict(box=-1.0), dict(box=np.inf), dict(box=np.nan),
    dict(edges=np.array([0.0, np.nan, 2.0])), dict(edges=np.array([0.0, 1.0, np.inf])),
    dict(edges=np.array([-0.5, 1.0, 2.0])), dict(edges=np.array([0.0, 1.0, 1.0])),
    dict(edges=np.array([0.0, 2.0, 1.0])),
    dict(flags=0x2), dict(flags=0x8), dict(flags=0x10), dict(flags=0x4 | 0x20),
]


def _id(kw):
    return "-".join(f"{k}={'arr' if isinstance(v, np.ndarray) else v}" for k, v in kw.items())


@pytest.mark.parametrize("kw", ERRORS, ids=_id)
def test_argument_errors_before_any_device_work(asp, kw):
    from asp_amd import _lib
    L = _lib.lib()
    rc = L.asp_halo_profiles(*_args(**kw))
    assert rc == _lib.ASP_ERR_INVALID and L.asp_last_error().decode(), kw


def test_sizes_that_need_no_device(asp):
    from asp_amd import _lib
    L = _lib.lib()
    # m * nbins >= 2^31: unsupported (never dereferenced)
    assert L.asp_halo_profiles(*_args(m=1 << 30)) == _lib.ASP_ERR_UNSUPPORTED
    assert "2^31" in L.asp_last_error().decode()
    assert L.asp_halo_profiles(*_args(m=1 << 40)) == _lib.ASP_ERR_UNSUPPORTED
    assert L.asp_halo_profiles(*_args(m=1 << 25, nbins=64, edges=np.arange(65.0))) == \
        _lib.ASP_ERR_UNSUPPORTED
    # m == 0 is valid with NULL centres, radii and outputs
    none = dict(m=0, centres=None, radius=None, count=None)
    assert L.asp_halo_profiles(*_args(**none)) == _lib.ASP_OK
    assert L.asp_halo_profiles(*_args(nprops=2, props=P2, **none)) == _lib.ASP_OK
    # n == 0 on host arrays: zeros, or untouched under ASP_F_ACCUMULATE
    count, sums = np.full((4, 2), 7, np.int64), np.full((2, 4, 2), 7.0)
    kw = dict(n=0, pos=None, props=None, nprops=2, count=count, sum=sums)
    assert L.asp_halo_profiles(*_args(flags=_lib.ASP_F_ACCUMULATE, **kw)) == _lib.ASP_OK
    assert np.all(count == 7) and np.all(sums == 7.0)
    assert L.asp_halo_profiles(*_args(**kw)) == _lib.ASP_OK
    assert np.all(count == 0) and np.all(sums == 0.0)
    count[:] = 7
    assert L.asp_halo_profiles(*_args(n=0, pos=None, radius=None, count=count)) == _lib.ASP_OK
    assert np.all(count == 0)


def _declared():
    """{name: parameter count} of every function include/asp_profiles.h declares."""
    hdr = open(os.path.join(REPO, "include", "asp_profiles.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(asp_\w+)\s*\(([^)]*)\)\s*;", hdr):
        out[m.group(1)] = len([p for p in m.group(2).split(",") if p.strip()])
    return out


def test_symbols_and_prototypes(asp):
    from asp_amd import _lib
    L = _lib.lib()
    declared = _declared()
    assert set(declared) == {"asp_halo_profiles"} == set(_lib.PROFILE_PROTOTYPES)
    for name, nparams in declared.items():
        fn = getattr(L, name)  # exported
        assert len(_lib.PROFILE_PROTOTYPES[name]) == nparams == len(fn.argtypes) == 15, name
        assert fn.restype is C.c_int
    assert L.asp_halo_profiles.argtypes[10] == C.POINTER(C.c_int64)
    assert L.asp_halo_profiles.argtypes[9] is C.c_double
    # the other tables and the stage names are as they were
    assert len(_lib.PROTOTYPES) == 34 and len(_lib.POINT_PROTOTYPES) == 2
    assert not set(declared) & (set(_lib.PROTOTYPES) | set(_lib.POINT_PROTOTYPES))
    assert len(_lib.ALL_STAGES) == 23


def test_halo_profiles_refuses_bad_arguments():
    """ValueError before any native call (there is no GPU here)."""
    from asp_amd.haloes import aperture_sums, halo_profiles
    pos, cen, rad, e, a = np.zeros((4, 3)), np.zeros((5, 3)), np.ones(5), [0.0, 1.0, 2.0], np.ones(4)
    for bad in ([0.0, 2.0, 1.0], [0.0, 1.0, 1.0], [-1.0, 1.0], [0.0, np.nan], [1.0],
                np.arange(66.0), np.zeros((2, 2))):
        with pytest.raises(ValueError, match="edges"):
            halo_profiles(pos, cen, rad, bad, 1.0)
    with pytest.raises(ValueError, match="shape"):
        halo_profiles(np.zeros((4, 2)), cen, rad, e, 1.0)
    with pytest.raises(ValueError, match="centres"):
        halo_profiles(pos, np.zeros((5, 2)), rad, e, 1.0)
    with pytest.raises(ValueError, match="radii"):
        halo_profiles(pos, cen, np.ones(4), e, 1.0)
    with pytest.raises(ValueError, match="radii"):
        halo_profiles(pos, cen, rad.astype(np.float32), e, 1.0)
    with pytest.raises(ValueError, match="props"):
        halo_profiles(pos, cen, rad, e, 1.0, props=[a] * 5)
    with pytest.raises(ValueError, match="props"):
        halo_profiles(pos, cen, rad, e, 1.0, props=np.ones(3))
    with pytest.raises(ValueError, match="props"):
        halo_profiles(pos, cen, rad, e, 1.0, props=[a, a.astype(np.float32)])
    with pytest.raises(ValueError, match="float64"):
        halo_profiles(pos.astype(np.float32), cen, rad, e, 1.0)
    with pytest.raises(ValueError, match="float64"):
        aperture_sums(pos.astype(np.float32), cen, rad, 1.0)
    with pytest.raises(ValueError, match="edges"):
        aperture_sums(pos, cen, rad, 1.0, factor=0.0)
    # no haloes, or no particles: empty or zero results, no device needed
    count, sums = halo_profiles(pos, np.zeros((0, 3)), np.zeros(0), e, 1.0, props=[a, a])
    assert count.shape == (0, 2) and count.dtype == np.int64 and sums.shape == (2, 0, 2)
    count, sums = halo_profiles(np.zeros((0, 3)), cen, None, e, 1.0, props=np.zeros(0))
    assert count.shape == (5, 2) and not count.any() and sums.shape == (1, 5, 2) and not sums.any()
    count, sums = aperture_sums(np.zeros((0, 3)), cen, rad, 1.0)
    assert count.shape == (5,) and sums.shape == (0, 5)
