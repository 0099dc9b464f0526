"""Device-resident entry point: project float32 SoA torch tensors already in HBM.

This is the path ``bench.py`` and the multi-GPU driver use (no host round trip).  torch
only provides the device memory and the stream; all compute is libasp_hip.so.
"""
from __future__ import annotations

from . import _lib
from ._axes import axis_code
from ._call import (alloc_out, call_flags, dev_f64, dptr, host_f64, is_device, positions_f64,
                    raw_stream, stream_scope, upload_f64)
from .tools.projections._kernels import device_kernel_id as kernel_id  # noqa: F401


def _check(t, name, n=None, device=None):
    import torch
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch tensor")
    if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.dim() != 1:
        raise ValueError(f"{name} must be a contiguous 1-D float32 device tensor")
    if n is not None and t.shape[0] != n:
        raise ValueError(f"{name} has {t.shape[0]} elements, expected {n}")
    if device is not None and t.device != device:
        raise ValueError(f"{name} is on {t.device}, expected {device}")


def project2d(u, v, h, a0, a1=None, *, image_size, extent, chunk_size: int = 64,
              kernel="cubic", ratio: bool = False, accumulate: bool = False, out0=None,
              out1=None, stream=None, deterministic: bool = False, rows=None):
    """Project device-resident particles; returns ``(out0, out1)`` (out1 None for one map).

    ``extent = (u_min, u_max, v_min, v_max)``; images are (nx, ny) float32 tensors on the
    particles' device.  ``ratio`` turns (sum a0 W, sum a1 W) into their ratio in out0.
    ``rows = (row_lo, row_hi)``: only those image rows (asp_project2d_rows, the row-slab
    decomposition): outputs are (row_hi - row_lo, ny), each pixel the whole image's.
    """
    import torch
    dev = u.device
    n = u.shape[0]
    for t, name in ((u, "u"), (v, "v"), (h, "h"), (a0, "a0")):
        _check(t, name, n, dev)
    if a1 is not None:
        _check(a1, "a1", n, dev)
    nx, ny = int(image_size[0]), int(image_size[1])
    r0, r1 = (0, nx) if rows is None else (int(rows[0]), int(rows[1]))
    if not 0 <= r0 < r1 <= nx:
        raise ValueError(f"rows must satisfy 0 <= row_lo < row_hi <= nx, got {(r0, r1)}")
    shape = (r1 - r0, ny)  # the rows written
    out0 = alloc_out(shape, torch.float32, dev, out0)
    if a1 is not None or out1 is not None:
        out1 = alloc_out(shape, torch.float32, dev, out1)
    flags = call_flags(True, ratio, accumulate, deterministic)
    stream = raw_stream(stream, dev)
    P = _lib.ptr
    x_min, x_max, y_min, y_max = (float(e) for e in extent)
    if rows is None:
        _lib.check(_lib.lib().asp_project2d(
            P(u), P(v), P(h), P(a0), P(a1), n, x_min, x_max, y_min, y_max, nx, ny,
            int(chunk_size), kernel_id(kernel), flags, P(out0), P(out1), dev.index or 0, stream))
    else:
        _lib.check(_lib.lib().asp_project2d_rows(
            P(u), P(v), P(h), P(a0), P(a1), n, x_min, x_max, y_min, y_max, nx, ny,
            int(chunk_size), r0, r1, kernel_id(kernel), flags, P(out0), P(out1), dev.index or 0,
            stream))
    return out0, (out1 if a1 is not None else None)


def _check_props(k, mass, density, ratio):
    if not 1 <= k <= 6:
        raise ValueError("props: 1 .. 6 arrays")
    if density is not None and mass is None:
        raise ValueError("density needs mass (the weights are m / rho)")
    if ratio and k != 2:
        raise ValueError("ratio needs exactly two properties")


def project2d_props(u, v, h, props, *, image_size, extent, chunk_size: int = 64,
                    kernel="cubic", accumulate: bool = False, outs=None, stream=None,
                    mass=None, density=None, ratio: bool = False):
    """asp_project2d_props: one map per property of ``props`` (1..6 device float32 arrays)
    from ONE binning of the particles -- the same neighbour sets, the counting and
    scattering done once.  Returns the list of (nx, ny) float32 maps.

    ``mass`` (and ``density``): the SPH-weighted maps of asp_project2d_sph,
    sum_j (m_j / rho_j) A_j W (``density`` None: sum_j m_j A_j W); ``ratio`` (two
    properties): out0 = the weighted mean of props[0] over props[1]'s weights."""
    import torch
    dev = u.device
    n = u.shape[0]
    k = len(props)
    _check_props(k, mass, density, ratio)
    for t, name in ((u, "u"), (v, "v"), (h, "h"), *((a, f"props[{j}]") for j, a in enumerate(props))):
        _check(t, name, n, dev)
    for t, name in ((mass, "mass"), (density, "density")):
        if t is not None:
            _check(t, name, n, dev)
    nx, ny = int(image_size[0]), int(image_size[1])
    if outs is None:
        outs = [None] * k
    if len(outs) != k:
        raise ValueError("one output per property")
    outs = [alloc_out((nx, ny), torch.float32, dev, o) for o in outs]
    P = _lib.ptr
    pa = (_lib._f * k)(*[P(a) for a in props])
    po = (_lib._f * k)(*[P(o) for o in outs])
    x_min, x_max, y_min, y_max = (float(e) for e in extent)
    tail = (n, x_min, x_max, y_min, y_max, nx, ny, int(chunk_size), kernel_id(kernel),
            call_flags(True, ratio, accumulate), po, dev.index or 0, raw_stream(stream, dev))
    if mass is not None:
        _lib.check(_lib.lib().asp_project2d_sph(P(u), P(v), P(h), P(mass), P(density), pa, k, *tail))
    else:
        _lib.check(_lib.lib().asp_project2d_props(P(u), P(v), P(h), pa, k, *tail))
    return outs


def project2d_props_f64(positions, h, props, *, projection_axis=2, image_size, extent,
                        chunk_size: int = 64, kernel="cubic", device: int = 0, mass=None,
                        density=None, ratio: bool = False):
    """asp_project2d_props_f64 on the reader's float64 arrays (host NumPy arrays or float64
    device tensors; host arrays are copied to the device): the maps of every property from
    one binning, every decision the reference's fp64 test.  Returns float32 device maps.
    ``mass`` / ``density`` / ``ratio``: as :func:`project2d_props` (asp_project2d_sph_f64;
    the weights m / rho are formed in fp64 from the reader's values)."""
    import torch
    axis = axis_code(projection_axis)
    k = len(props)
    _check_props(k, mass, density, ratio)
    dev = positions.device if is_device(positions) else torch.device("cuda", device)
    n = int(positions.shape[0])
    with stream_scope(dev, None) as scope:  # the uploads and casts ordered on the call's stream
        pos = upload_f64(positions, "positions", (n, 3), dev, cast=True)[0]
        hh, wm, wr, *pr = (None if a is None else upload_f64(a, name, (n,), dev, cast=True, flat=True)[0]
                           for a, name in ((h, "h"), (mass, "mass"), (density, "density"),
                                           *((a, f"props[{j}]") for j, a in enumerate(props))))
        scope.keep(pos, hh, wm, wr, *pr)
        nx, ny = int(image_size[0]), int(image_size[1])
        outs = [alloc_out((nx, ny), torch.float32, dev) for _ in range(k)]
        pa = (_lib._d * k)(*[dptr(a) for a in pr])
        po = (_lib._f * k)(*[_lib.ptr(o) for o in outs])
        x_min, x_max, y_min, y_max = (float(e) for e in extent)
        tail = (n, axis, x_min, x_max, y_min, y_max, nx, ny, int(chunk_size), kernel_id(kernel),
                call_flags(True, ratio), po, dev.index or 0, scope.raw)
        if wm is not None:
            _lib.check(_lib.lib().asp_project2d_sph_f64(dptr(pos), dptr(hh), dptr(wm), dptr(wr), pa,
                                                        k, *tail))
        else:
            _lib.check(_lib.lib().asp_project2d_props_f64(dptr(pos), dptr(hh), pa, k, *tail))
    return outs


def project2d_f64(positions, h, a0, a1=None, *, projection_axis=2, image_size, extent,
                  chunk_size: int = 64, kernel="cubic", ratio: bool = False,
                  accumulate: bool = False, out0=None, out1=None, device: int = 0,
                  stream=None, deterministic: bool = False, device_out: bool = False):
    """asp_project2d_f64: the reader's float64 arrays (positions (N, 3), h, a0[, a1]) --
    host NumPy arrays or float64 device tensors -- projected with the reference's fp64
    decisions on those values.  ``projection_axis``: an axis (int 0/1/2, enum, "x") or a
    (pixel axis, cull axis) pair (asp_amd._axes.reference_axes).  Returns float32 maps:
    device tensors for device inputs or ``device_out`` (host inputs staged through pinned
    buffers, maps left on ``device`` -- e.g. for an RCCL sum), else NumPy arrays."""
    import numpy as np
    import torch
    axis = axis_code(projection_axis)
    on_dev = is_device(positions)
    fields = ((h, "smoothing_lengths"), (a0, "a0"), (a1, "a1"))
    if any(a is not None and is_device(a) != on_dev for a, _ in fields):
        raise ValueError("positions and fields must all be host arrays or all device tensors")
    if on_dev:
        dev = positions.device
        device = dev.index or 0
        with stream_scope(dev, stream) as scope:  # any .contiguous() copy on the call's stream
            pos, n, _ = positions_f64(positions, cast=True)
            hh, b0, b1 = (None if a is None else dev_f64(a, name, (n,), dev) for a, name in fields)
            scope.keep(pos, hh, b0, b1)
        stream = scope.raw
    else:
        pos, n, _ = positions_f64(positions, cast=True)
        hh, b0, b1 = (None if a is None else host_f64(a, name, (n,), cast=True, flat=True)
                      for a, name in fields)
        _lib.require_gpu(device)
        dev = torch.device("cuda", device) if device_out else None
        if dev is not None or stream is not None:
            stream = raw_stream(stream, dev)
    nx, ny = int(image_size[0]), int(image_size[1])
    dtype = np.float32 if dev is None else torch.float32
    zeros = dev is None or (accumulate and not on_dev)  # (a fresh device_out map is summed into)
    out0 = alloc_out((nx, ny), dtype, dev, out0, zeros=zeros)
    if a1 is not None or out1 is not None:
        out1 = alloc_out((nx, ny), dtype, dev, out1, zeros=zeros)
    x_min, x_max, y_min, y_max = (float(np.asarray(e)) for e in extent)
    _lib.check(_lib.lib().asp_project2d_f64(
        dptr(pos), dptr(hh), dptr(b0), dptr(b1), n, axis, x_min, x_max, y_min, y_max, nx, ny,
        int(chunk_size), kernel_id(kernel),
        call_flags(on_dev, ratio, accumulate, deterministic, device_out and not on_dev),
        _lib.ptr(out0), _lib.ptr(out1), int(device), stream))
    return out0, (out1 if a1 is not None else None)


def project3d(x, y, z, h, a, *, cube_size, extent, kernel="cubic", planes=None,
              accumulate: bool = False, out=None, stream=None):
    """Deposit device-resident particles into a voxel cube (asp_project3d).

    ``extent = (x_min, x_max, y_min, y_max, z_min, z_max)``; ``planes = (k_lo, k_hi)``
    restricts the output to those z planes (default: all).  Returns the
    (nx, ny, k_hi - k_lo) float32 tensor on the particles' device.
    """
    import torch
    dev = x.device
    n = x.shape[0]
    for t, name in ((x, "x"), (y, "y"), (z, "z"), (h, "h"), (a, "a")):
        _check(t, name, n, dev)
    nx, ny, nz = (int(c) for c in cube_size)
    k_lo, k_hi = (0, nz) if planes is None else (int(planes[0]), int(planes[1]))
    out = alloc_out((nx, ny, max(0, k_hi - k_lo)), torch.float32, dev, out, name="out")
    P = _lib.ptr
    e = [float(v) for v in extent]
    _lib.check(_lib.lib().asp_project3d(P(x), P(y), P(z), P(h), P(a), n, *e, nx, ny, nz, k_lo,
                                        k_hi, kernel_id(kernel), call_flags(True, accumulate=accumulate),
                                        P(out), dev.index or 0, raw_stream(stream, dev)))
    return out


def stats(device: int = 0):
    """Counters of the last projection on ``device`` (records, work items, wide, ...)."""
    return _lib.last_stats(device)
