"""The Python call layer (asp_amd/_call.py, _axes.axis_code, the kernel-id table, the
prototype table of _lib.py): what holds without a GPU."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from conftest import REPO


def test_host_f64_strict_and_cast():
    from asp_amd._call import host_f64
    good = np.arange(6.0)
    assert host_f64(good, "a", (6,), cast=False) is good  # nothing to do: no copy
    with pytest.raises(ValueError, match=r"a must be float64, got float32"):
        host_f64(good.astype(np.float32), "a", (6,), cast=False)
    for cast in (False, True):
        with pytest.raises(ValueError, match=r"a must have shape \(5,\), got \(6,\)"):
            host_f64(good, "a", (5,), cast=cast)
    for src in (good.astype(np.float32), np.arange(6, dtype=np.int64), [0, 1, 2, 3, 4, 5]):
        x = host_f64(src, "a", (6,), cast=True)
        assert x.dtype == np.float64 and x.flags.c_contiguous and np.array_equal(x, good)
    view = np.arange(24.0).reshape(6, 4)[:, 1]  # a strided float64 view
    assert not view.flags.c_contiguous
    for cast in (False, True):
        x = host_f64(view, "a", (6,), cast=cast)
        assert x.flags.c_contiguous and x.dtype == np.float64 and np.array_equal(x, view)
    col = np.arange(6.0).reshape(6, 1)  # the (N, 1) columns readers hand out
    assert host_f64(col, "a", (6,), cast=False, flat=True).shape == (6,)
    with pytest.raises(ValueError, match="shape"):
        host_f64(col, "a", (6,), cast=False)


def test_positions_f64():
    from asp_amd._call import is_device, positions_f64
    pos = np.arange(12.0).reshape(4, 3)
    got, n, on_device = positions_f64(pos, cast=False)
    assert got is pos and n == 4 and on_device is False and not is_device(pos)
    for bad in (np.zeros((4, 2)), np.zeros(12), np.zeros((2, 2, 3))):
        for cast in (False, True):
            with pytest.raises(ValueError, match=r"positions must have shape \(N, 3\)"):
                positions_f64(bad, cast=cast)
    with pytest.raises(ValueError, match="centres must be float64, got float32"):
        positions_f64(pos.astype(np.float32), "centres", cast=False)
    got, n, _ = positions_f64(pos.astype(np.float32).T.copy().T, cast=True)  # cast, made contiguous
    assert got.dtype == np.float64 and got.flags.c_contiguous and np.array_equal(got, pos)
    assert positions_f64(np.zeros((0, 3)), cast=False)[1] == 0


def test_axis_code():
    from asp_amd import CoordinateAxes
    from asp_amd._axes import axis_code, axis_index

    class RefAxes:  # the reference's enum: only .name matters
        name = "Y"
    for a in (0, 1, 2, 7, "x", "Y", "z", b"x", RefAxes(), *CoordinateAxes):
        assert axis_code(a) == axis_index(a), a
    want = {(0, 0): 0, (0, 1): 0x20, (0, 2): 0x30,
            (1, 0): 0x11, (1, 1): 1, (1, 2): 0x31,
            (2, 0): 0x12, (2, 1): 0x22, (2, 2): 2}
    for (p, c), code in want.items():
        assert axis_code((p, c)) == code, (p, c)
        assert code == (p if c == p else p | (c + 1) << 4)


def test_call_flags():
    from asp_amd import _lib
    from asp_amd._call import call_flags
    names = ("device_ptrs", "ratio", "accumulate", "deterministic", "device_outputs")
    bits = (_lib.ASP_F_DEVICE_PTRS, _lib.ASP_F_RATIO, _lib.ASP_F_ACCUMULATE,
            _lib.ASP_F_DETERMINISTIC, _lib.ASP_F_DEVICE_OUTPUTS)
    assert bits == (0x1, 0x2, 0x4, 0x8, 0x10)
    for on in itertools.product((False, True), repeat=5):
        want = 0
        for b, o in zip(bits, on):
            want |= b if o else 0
        assert call_flags(**dict(zip(names, on))) == want, on
        assert call_flags(*on) == want, on  # the positional order is the same


def test_kernel_tables_and_their_failures():
    from asp_amd import device, sightlines
    from asp_amd.tools.projections import _kernels, wendland_c2_column_kernel
    # the two tables as they stood before they were merged
    assert sightlines.KERNEL_IDS == {
        'cubic': 0, 'cubic_spline': 0, 'cubic_column': 3, 'quartic_spline_kernel': 0,
        'quartic_spline': 0, 'wendland_c2_kernel': 1, 'wendland_c2': 1, 'indicator_kernel': 2,
        'indicator': 2, 'cubic_spline_column_kernel': 3, 'cubic_spline_column': 3,
        'wendland_c2_column_kernel': 4, 'wendland_c2_column': 4}
    assert sightlines.KERNEL_IDS is _kernels.KERNEL_IDS
    device_names = {'cubic': 0, 'quartic_spline_kernel': 0, 'cubic_spline': 0, 'wendland_c2': 1,
                    'indicator': 2, 'cubic_column': 3, 'wendland_c2_column': 4}
    for name, kid in device_names.items():
        assert device.kernel_id(name) == kid, name
    assert set(_kernels.DEVICE_KERNEL_NAMES) == set(device_names)
    # device.kernel_id: ints pass, an unknown or sightline-only name is a KeyError
    assert device.kernel_id(3) == 3 and device.kernel_id(wendland_c2_column_kernel) == 4
    for name in ("gaussian", "quartic_spline", "indicator_kernel"):
        with pytest.raises(KeyError):
            device.kernel_id(name)
    with pytest.raises(TypeError):
        device.kernel_id(lambda r, h: r)
    # sightlines._kernel_id: ValueError for everything it does not know, ints included
    assert sightlines._kernel_id("quartic_spline") == 0
    assert sightlines._kernel_id(wendland_c2_column_kernel) == 4
    for bad in ("gaussian", 3, None, lambda r, h: r):
        with pytest.raises(ValueError, match="kernel"):
            sightlines._kernel_id(bad)
    # the kernel_func= mirrors: TypeError
    assert _kernels.kernel_id_of(lambda r, h: r) is None
    for bad in ("cubic", 3):
        with pytest.raises(TypeError):
            _kernels.kernel_id_of(bad)
    with pytest.raises(TypeError):
        _kernels.native_kernel_id(lambda r, h: r)


def _declared():
    """{name: (return type, parameter count)} of every function include/asp.h declares."""
    hdr = open(os.path.join(REPO, "include", "asp.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", "", hdr)
    out = {}
    for ret, name, params in re.findall(
            r"^\s*((?:const\s+)?\w+\s*\*?)\s*(asp_\w+)\s*\(([^)]*)\)", hdr, re.M):
        params = [p.strip() for p in params.split(",")]
        out[name] = (" ".join(ret.split()), 0 if params in (["void"], [""]) else len(params))
    return out


def test_prototypes_match_the_header(asp):
    from asp_amd import _lib
    declared = _declared()
    assert len(declared) == 34
    assert set(_lib.EXPORTS) == set(declared) == set(_lib.PROTOTYPES)
    assert len(set(_lib.EXPORTS)) == len(_lib.EXPORTS)
    L = _lib.lib()
    for name, (ret, nparams) in declared.items():
        fn = getattr(L, name)
        assert len(fn.argtypes or ()) == nparams, name
        if name == "asp_last_error":
            assert ret == "const char *" and fn.restype is C.c_char_p
        else:
            assert ret == "int" and fn.restype is C.c_int, name


def test_raw_stream_without_a_device():
    from asp_amd._call import raw_stream

    class Stream:  # what a torch.cuda.Stream offers
        cuda_stream = 5678
    assert raw_stream(1234, None) == 1234
    assert raw_stream(Stream(), None) == 5678
    assert raw_stream(0, None) == 0  # the null stream's handle is a handle, not "no stream"


def test_stream_scope_keeps_and_records(monkeypatch):
    """stream_scope with torch's stream classes replaced by recorders: the block runs inside
    torch.cuda.stream(ExternalStream(raw)), and exactly the kept non-None tensors are
    record_stream-ed, after the block."""
    import torch
    from asp_amd._call import stream_scope
    log = []

    class Ext:
        def __init__(self, raw, device=None):
            self.raw, self.device = raw, device

    class Ctx:
        def __init__(self, s):
            self.s = s

        def __enter__(self):
            log.append(("enter", self.s.raw))

        def __exit__(self, *exc):
            log.append(("exit", self.s.raw))

    class T:
        def __init__(self, tag):
            self.tag = tag

        def record_stream(self, s):
            log.append(("record", self.tag, s.raw))

    monkeypatch.setattr(torch.cuda, "ExternalStream", Ext)
    monkeypatch.setattr(torch.cuda, "stream", Ctx)
    with stream_scope("dev", 77) as scope:
        assert scope.raw == 77
        scope.keep(T("a"), None, T("b"))
        scope.keep(None)
        log.append("body")
    assert log == [("enter", 77), "body", ("exit", 77), ("record", "a", 77), ("record", "b", 77)]


def test_alloc_out_host():
    from asp_amd._call import alloc_out
    z = alloc_out((3, 4), np.float32, None, zeros=True)
    assert z.shape == (3, 4) and z.dtype == np.float32 and not z.any()
    assert alloc_out((3, 4), np.float32, None).shape == (3, 4)
    assert alloc_out((3, 4), np.float32, None, z) is z
    assert alloc_out((12,), np.float32, None, z) is z  # the element count is what matters
    for bad in (z.astype(np.float64), np.zeros((3, 5), np.float32), z.T, [0.0] * 12):
        with pytest.raises(ValueError, match="outputs must be contiguous"):
            alloc_out((3, 4), np.float32, None, bad)
