"""Sightline sampling (asp_sample2d, asp_sample2d_f64, asp_amd.sightline_columns): what
holds without a GPU -- every argument error is returned before any device work, m == 0 and
(for host arrays) n == 0 need no device, and the Python wrapper refuses bad shapes and
dtypes with ValueError before any native call.
"""
import ctypes as C

import numpy as np
import pytest


def _args32(**kw):
    from asp_amd import _lib
    f = np.zeros(4, np.float32)
    d = np.zeros(4)
    a = dict(u=f, v=f, h=f, a0=f, a1=None, n=4, px=d, py=d, m=4, kid=0, flags=0,
             out0=np.zeros(4, np.float32), out1=None)
    a.update(kw)
    if a.pop("pair", False):  # a second sum: a1 and out1 together
        a["a1"], a["out1"] = f, np.zeros(4, np.float32)
    P, D = _lib.ptr, (lambda x: _lib.ptr(x, _lib._d))
    return (P(a["u"]), P(a["v"]), P(a["h"]), P(a["a0"]), P(a["a1"]), a["n"], D(a["px"]), D(a["py"]),
            a["m"], a["kid"], a["flags"], P(a["out0"]), P(a["out1"]), 0, None)


def _args64(**kw):
    from asp_amd import _lib
    d = np.zeros(4)
    a = dict(pos=np.zeros((4, 3)), h=d, a0=d, a1=None, n=4, axis=2, px=d, py=d, m=4, kid=0,
             flags=0, out0=np.zeros(4, np.float32), out1=None)
    a.update(kw)
    if a.pop("pair", False):
        a["a1"], a["out1"] = d, np.zeros(4, np.float32)
    P, D = _lib.ptr, (lambda x: _lib.ptr(x, _lib._d))
    return (D(a["pos"]), D(a["h"]), D(a["a0"]), D(a["a1"]), a["n"], a["axis"], D(a["px"]),
            D(a["py"]), a["m"], a["kid"], a["flags"], P(a["out0"]), P(a["out1"]), 0, None)


F32 = np.zeros(4, np.float32)
BOTH = [dict(n=-1), dict(m=-1), dict(kid=-1), dict(kid=5), dict(px=None), dict(py=None),
        dict(out0=None), dict(a0=None), dict(h=None), dict(out1=F32), dict(flags=0x10),
        dict(flags=0x2), dict(flags=0x2 | 0x8, pair=True), dict(flags=0x2 | 0x4, pair=True),
        dict(flags=0x10, pair=True)]
ONLY32 = [dict(u=None), dict(v=None), dict(a1=F32)]
ONLY64 = [dict(pos=None), dict(a1=np.zeros(4)), dict(axis=3), dict(axis=-1),
          dict(axis=2 | (1 << 4)), dict(axis=0 | (3 << 4))]


def _id(kw):
    return "-".join(f"{k}={'arr' if isinstance(v, np.ndarray) else v}" for k, v in kw.items())


@pytest.mark.parametrize("kw", BOTH + ONLY32, ids=_id)
def test_sample2d_argument_errors_before_any_device_work(asp, kw):
    from asp_amd import _lib
    L = _lib.lib()
    rc = L.asp_sample2d(*_args32(**kw))
    assert rc == _lib.ASP_ERR_INVALID and L.asp_last_error().decode(), kw


@pytest.mark.parametrize("kw", BOTH + ONLY64, ids=_id)
def test_sample2d_f64_argument_errors_before_any_device_work(asp, kw):
    from asp_amd import _lib
    L = _lib.lib()
    rc = L.asp_sample2d_f64(*_args64(**kw))
    assert rc == _lib.ASP_ERR_INVALID and L.asp_last_error().decode(), kw


def test_sizes_that_need_no_device(asp):
    from asp_amd import _lib
    L = _lib.lib()
    # m >= 2^31: unsupported (never dereferenced)
    assert L.asp_sample2d(*_args32(m=1 << 31)) == _lib.ASP_ERR_UNSUPPORTED
    assert L.asp_sample2d_f64(*_args64(m=1 << 31)) == _lib.ASP_ERR_UNSUPPORTED
    assert "2^31" in L.asp_last_error().decode()
    # m == 0 is valid with NULL point arrays and outputs
    assert L.asp_sample2d(*_args32(m=0, px=None, py=None, out0=None)) == _lib.ASP_OK
    assert L.asp_sample2d_f64(*_args64(m=0, px=None, py=None, out0=None)) == _lib.ASP_OK
    # n == 0 on host arrays: zeros, or untouched under ASP_F_ACCUMULATE
    out0, out1 = np.full(4, 7.0, np.float32), np.full(4, 7.0, np.float32)
    rc = L.asp_sample2d(*_args32(n=0, u=None, v=None, h=None, a0=None, out0=out0))
    assert rc == _lib.ASP_OK and np.all(out0 == 0)
    out0[:] = 7.0
    rc = L.asp_sample2d_f64(*_args64(n=0, pos=None, h=None, a0=None, a1=np.zeros(4), out0=out0,
                                     out1=out1, flags=_lib.ASP_F_ACCUMULATE))
    assert rc == _lib.ASP_OK and np.all(out0 == 7.0) and np.all(out1 == 7.0)


def test_prototypes_and_stage_names(asp):
    from asp_amd import _lib
    L = _lib.lib()
    assert L.asp_sample2d.argtypes[6] == C.POINTER(C.c_double)
    assert L.asp_sample2d_f64.argtypes[0] == C.POINTER(C.c_double)
    assert _lib.ALL_STAGES[21:] == ("sample_prep", "sample_deposit")
    assert _lib.ALL_STAGES[:21] == _lib.STAGES  # the existing numbers are unchanged


def test_sightline_columns_refuses_bad_arguments():
    """ValueError before any native call (there is no GPU here)."""
    from asp_amd import sightline_columns
    pos, h, a, pts = np.zeros((4, 3)), np.ones(4), np.ones(4), np.zeros((5, 2))
    with pytest.raises(ValueError, match="shape"):
        sightline_columns(np.zeros((4, 2)), h, a, pts, 2)
    with pytest.raises(ValueError, match="float64"):
        sightline_columns(pos.astype(np.float32), h, a, pts, 2)
    with pytest.raises(ValueError, match="smoothing_lengths"):
        sightline_columns(pos, np.ones(3), a, pts, 2)
    with pytest.raises(ValueError, match="particle_properties"):
        sightline_columns(pos, h, a.astype(np.float32), pts, 2)
    with pytest.raises(ValueError, match="weights"):
        sightline_columns(pos, h, a, pts, 2, weights=np.ones(5))
    with pytest.raises(ValueError, match="points"):
        sightline_columns(pos, h, a, np.zeros((5, 4)), 2)
    with pytest.raises(ValueError, match="points"):
        sightline_columns(pos, h, a, np.zeros(5), 2)
    with pytest.raises(ValueError, match="points"):
        sightline_columns(pos, h, a, pts.astype(np.float32), 2)
    with pytest.raises(ValueError, match="kernel"):
        sightline_columns(pos, h, a, pts, 2, kernel="gaussian")
    with pytest.raises(ValueError, match="deterministic"):
        sightline_columns(pos, h, a, pts, 2, weights=h, deterministic=True)
    # no points: an empty result, no device needed
    out = sightline_columns(pos, h, a, np.zeros((0, 3)), 0)
    assert out.shape == (0,) and out.dtype == np.float32


def test_kernel_names():
    from asp_amd import sightlines
    from asp_amd.tools.projections import wendland_c2_column_kernel
    ids = sightlines.KERNEL_IDS
    assert ids["cubic_column"] == ids["cubic_spline_column_kernel"] == 3
    assert ids["wendland_c2_column"] == 4 and ids["quartic_spline_kernel"] == ids["cubic"] == 0
    assert ids["wendland_c2"] == 1 and ids["indicator"] == 2
    assert sightlines._kernel_id(wendland_c2_column_kernel) == 4
