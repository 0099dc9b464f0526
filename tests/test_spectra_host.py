"""Sightline spectra (asp_spectra2d, asp_spectra2d_f64, asp_amd.sightline_spectra): what holds
without a GPU -- every argument error is returned before any device work with a message that
names it, m == 0 and (for host arrays) n == 0 need no device, the Python wrapper refuses bad
arguments before any native call, and los_coordinate is its NumPy one-liner.
"""
import ctypes as C

import numpy as np
import pytest


def args32(**kw):
    from asp_amd import _lib
    f = np.zeros(4, np.float32)
    d = np.zeros(4)
    a = dict(u=f, v=f, h=f, a0=f, a1=None, vc=d, b=np.ones(4, np.float32), n=4, px=d, py=d, m=4,
             v0=0.0, dv=1.0, nbins=8, ring=0, kid=0, flags=0, out0=np.zeros(32, np.float32), out1=None)
    a.update(kw)
    if a.pop("pair", False):  # a second sum: a1 and out1 together
        a["a1"], a["out1"] = f, np.zeros(32, np.float32)
    P, D = _lib.ptr, (lambda x: _lib.ptr(x, _lib._d))
    return (P(a["u"]), P(a["v"]), P(a["h"]), P(a["a0"]), P(a["a1"]), D(a["vc"]), P(a["b"]), a["n"],
            D(a["px"]), D(a["py"]), a["m"], a["v0"], a["dv"], a["nbins"], a["ring"], a["kid"],
            a["flags"], P(a["out0"]), P(a["out1"]), 0, None)


def args64(**kw):
    from asp_amd import _lib
    d = np.zeros(4)
    a = dict(pos=np.zeros((4, 3)), h=d, a0=d, a1=None, vc=d, b=np.ones(4), n=4, axis=2, px=d, py=d,
             m=4, v0=0.0, dv=1.0, nbins=8, ring=0, kid=0, flags=0, out0=np.zeros(32, np.float32),
             out1=None)
    a.update(kw)
    if a.pop("pair", False):
        a["a1"], a["out1"] = d, np.zeros(32, np.float32)
    P, D = _lib.ptr, (lambda x: _lib.ptr(x, _lib._d))
    return (D(a["pos"]), D(a["h"]), D(a["a0"]), D(a["a1"]), D(a["vc"]), D(a["b"]), a["n"], a["axis"],
            D(a["px"]), D(a["py"]), a["m"], a["v0"], a["dv"], a["nbins"], a["ring"], a["kid"],
            a["flags"], P(a["out0"]), P(a["out1"]), 0, None)


F32 = np.zeros(32, np.float32)
# (arguments, a word of the message)
INVALID = [(dict(dv=0.0), "dv"), (dict(dv=-1.0), "dv"), (dict(dv=np.nan), "dv"), (dict(dv=np.inf), "dv"),
           (dict(v0=np.nan), "v0"), (dict(v0=-np.inf), "v0"), (dict(nbins=0), "nbins"),
           (dict(nbins=-3), "nbins"), (dict(ring=2), "ring"), (dict(ring=-1), "ring"),
           (dict(n=-1), "n < 0"), (dict(m=-1), "m < 0"), (dict(kid=-1), "kernel"), (dict(kid=5), "kernel"),
           (dict(px=None), "point"), (dict(py=None), "point"), (dict(out0=None), "out0"),
           (dict(a0=None), "particle"), (dict(h=None), "particle"), (dict(vc=None), "particle"),
           (dict(b=None), "particle"), (dict(out1=F32), "a1 and out1"),
           (dict(flags=0x10), "ASP_F_DEVICE_OUTPUTS"), (dict(flags=0x2), "ASP_F_RATIO"),
           (dict(flags=0x2 | 0x4, pair=True), "ASP_F_ACCUMULATE")]
ONLY32 = [(dict(u=None), "particle"), (dict(v=None), "particle")]
ONLY64 = [(dict(pos=None), "particle"), (dict(axis=3), "axis"), (dict(axis=-1), "axis"),
          (dict(axis=2 | (1 << 4)), "ASP_AXIS_CULL"), (dict(axis=0 | (3 << 4)), "ASP_AXIS_CULL")]


def check_errors():
    """Every ASP_ERR_* of include/asp_spectra.h, with its message (no device is touched; the
    GPU suite runs this as well)."""
    from asp_amd import _lib
    L = _lib.lib()
    for entry, make, cases in ((L.asp_spectra2d, args32, INVALID + ONLY32),
                               (L.asp_spectra2d_f64, args64, INVALID + ONLY64)):
        for kw, word in cases:
            rc = entry(*make(**kw))
            assert rc == _lib.ASP_ERR_INVALID and word in L.asp_last_error().decode(), (kw, rc)
        assert entry(*make(flags=0x8)) == _lib.ASP_ERR_UNSUPPORTED
        assert "ASP_F_DETERMINISTIC" in L.asp_last_error().decode()
        # m nbins >= 2^31 (never dereferenced), and m itself
        assert entry(*make(m=1 << 20, nbins=1 << 11)) == _lib.ASP_ERR_UNSUPPORTED
        assert "m * nbins" in L.asp_last_error().decode()
        assert entry(*make(m=1 << 31)) == _lib.ASP_ERR_UNSUPPORTED


def test_argument_errors_before_any_device_work(asp):
    check_errors()


def test_sizes_that_need_no_device(asp):
    from asp_amd import _lib
    L = _lib.lib()
    # m == 0 is valid with NULL point arrays and outputs
    assert L.asp_spectra2d(*args32(m=0, px=None, py=None, out0=None)) == _lib.ASP_OK
    assert L.asp_spectra2d_f64(*args64(m=0, px=None, py=None, out0=None)) == _lib.ASP_OK
    # n == 0 on host arrays: zeros in all m nbins values, or untouched under ASP_F_ACCUMULATE
    out0, out1 = np.full(32, 7.0, np.float32), np.full(32, 7.0, np.float32)
    rc = L.asp_spectra2d(*args32(n=0, u=None, v=None, h=None, a0=None, vc=None, b=None, out0=out0))
    assert rc == _lib.ASP_OK and np.all(out0 == 0)
    out0[:] = 7.0
    rc = L.asp_spectra2d_f64(*args64(n=0, pos=None, h=None, a0=None, vc=None, b=None, a1=np.zeros(4),
                                     out0=out0, out1=out1, flags=_lib.ASP_F_ACCUMULATE))
    assert rc == _lib.ASP_OK and np.all(out0 == 7.0) and np.all(out1 == 7.0)


def test_prototypes_and_stage_names(asp):
    from asp_amd import _lib
    L = _lib.lib()
    assert L.asp_spectra2d.argtypes[5] == C.POINTER(C.c_double)   # vc
    assert L.asp_spectra2d.argtypes[6] == C.POINTER(C.c_float)    # b
    assert L.asp_spectra2d_f64.argtypes[5] == C.POINTER(C.c_double)
    assert len(L.asp_spectra2d.argtypes) == len(L.asp_spectra2d_f64.argtypes) == 21
    assert _lib.PROFILE_STAGES[23] == "spectra_deposit" and len(_lib.PROFILE_STAGES) == 24
    assert _lib.PROFILE_STAGES[:23] == _lib.ALL_STAGES  # the existing numbers are unchanged


def test_sightline_spectra_refuses_bad_arguments():
    """ValueError before any native call (there is no GPU here)."""
    from asp_amd import sightline_spectra
    pos, h, a, pts = np.zeros((4, 3)), np.ones(4), np.ones(4), np.zeros((5, 2))
    vc, b = np.zeros(4), np.ones(4)
    tail = (2, 0.0, 1.0, 16)
    with pytest.raises(ValueError, match="shape"):
        sightline_spectra(np.zeros((4, 2)), h, a, vc, b, pts, *tail)
    with pytest.raises(ValueError, match="los_coordinate"):
        sightline_spectra(pos, h, a, np.zeros(3), b, pts, *tail)
    with pytest.raises(ValueError, match="doppler_b"):
        sightline_spectra(pos, h, a, vc, b.astype(np.float32), pts, *tail)
    with pytest.raises(ValueError, match="weights"):
        sightline_spectra(pos, h, a, vc, b, pts, *tail, weights=np.ones(5))
    with pytest.raises(ValueError, match="points"):
        sightline_spectra(pos, h, a, vc, b, np.zeros((5, 4)), *tail)
    with pytest.raises(ValueError, match="kernel"):
        sightline_spectra(pos, h, a, vc, b, pts, *tail, kernel="gaussian")
    with pytest.raises(ValueError, match="n_bins"):
        sightline_spectra(pos, h, a, vc, b, pts, 2, 0.0, 1.0, 0)
    # no sightlines: an empty result, no device needed
    out = sightline_spectra(pos, h, a, vc, b, np.zeros((0, 3)), 0, 0.0, 1.0, 16, ring=True)
    assert out.shape == (0, 16) and out.dtype == np.float32


@pytest.mark.parametrize("axis", [0, 1, 2, "z"])
def test_los_coordinate_is_its_one_liner(axis):
    import torch
    from asp_amd import los_coordinate
    rng = np.random.default_rng(70)
    pos, vel = rng.uniform(0.0, 25.0, (500, 3)), rng.normal(0.0, 300.0, (500, 3))
    H, k = 67.74, 2 if axis == "z" else axis
    want = H * pos[:, k] + vel[:, k]
    got = los_coordinate(pos, vel, axis, H)
    assert got.dtype == np.float64 and np.array_equal(got, want)
    wrapped = los_coordinate(pos, vel, axis, H, box_velocity=H * 25.0)
    assert np.array_equal(wrapped, np.mod(want, H * 25.0))
    assert wrapped.min() >= 0.0 and wrapped.max() < H * 25.0 and np.any(wrapped != want)
    t = los_coordinate(torch.from_numpy(pos), torch.from_numpy(vel), axis, H, box_velocity=H * 25.0)
    assert t.dtype == torch.float64 and np.array_equal(t.numpy(), wrapped)
