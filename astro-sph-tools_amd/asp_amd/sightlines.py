"""SPH sums at sightline positions, on the GPU.

The reference's unit of work, ``calculate_pixel_value`` (_pixel_calculations.pyx:9-36), takes
an arbitrary corner (x, y); only ``create_image`` restricts it to a pixel lattice.
:func:`sightline_columns` evaluates it at M arbitrary points -- the start positions of
``LineOfSightFileBase`` (_LineOfSightBase.py:16-73), quasar sightlines at given impact
parameters -- through asp_sample2d_f64 (csrc/asp_sample.hip): the neighbour test
``r2 < (2h)**2`` in fp64 on the reader's own arrays, bit-exact neighbour sets, fp32 terms.
With a column kernel (the default) and ion masses from ``asp_amd.ionisation`` the result is
the ion's column density at each sightline.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._axes import AXIS_COLUMNS, axis_index
from .tools.projections import _kernels

# the names _kernels.py knows: each kernel object's __name__, with and without "_kernel", and
# the short spellings used for the same ids elsewhere
KERNEL_IDS = {"cubic": _lib.ASP_KERNEL_CUBIC_SPLINE, "cubic_spline": _lib.ASP_KERNEL_CUBIC_SPLINE,
              "cubic_column": _lib.ASP_KERNEL_CUBIC_SPLINE_COLUMN}
for _k in _kernels.KERNELS.values():
    KERNEL_IDS[_k.__name__] = _k.kernel_id
    KERNEL_IDS[_k.__name__[:-len("_kernel")]] = _k.kernel_id


def _kernel_id(kernel) -> int:
    if isinstance(kernel, _kernels.SPHKernel):
        return kernel.kernel_id
    if isinstance(kernel, str) and kernel in KERNEL_IDS:
        return KERNEL_IDS[kernel]
    raise ValueError(f"kernel {kernel!r} is not one of {sorted(KERNEL_IDS)} or an SPHKernel")


def _host_field(a, name, n):
    x = np.asarray(a)
    if x.dtype != np.float64:
        raise ValueError(f"{name} must be float64, got {x.dtype}")
    if x.shape != (n,):
        raise ValueError(f"{name} must have shape ({n},), got {x.shape}")
    return np.ascontiguousarray(x)


def _dev_field(t, name, n, dev):
    import torch
    if not hasattr(t, "is_cuda") or t.dtype != torch.float64 or t.device != dev:
        raise ValueError(f"{name} must be a float64 tensor on {dev}")
    if tuple(t.shape) != (n,):
        raise ValueError(f"{name} must have shape ({n},), got {tuple(t.shape)}")
    return t.contiguous()


def sightline_columns(positions, smoothing_lengths, particle_properties, points, projection_axis,
                      kernel="cubic_column", weights=None, deterministic: bool = False, *,
                      device: int = 0, stream=None):
    """``sum_p A_p W(r, h_p)`` at every point, over the particles with ``r2 < (2 h_p)**2``,
    r the distance between particle and point in the plane normal to ``projection_axis``.

    ``positions`` (N, 3), ``smoothing_lengths`` (N,), ``particle_properties`` (N,) and the
    optional ``weights`` (N,): float64 NumPy (or unyt) host arrays, returning a NumPy
    float32 array of length M, or float64 torch tensors on the GPU, returning a tensor
    there, the work ordered on ``stream`` (default: the current stream).

    ``points``: (M, 2) in projected (u, v) order -- X -> (y, z), Y -> (x, z), Z -> (x, y) --
    or (M, 3) box positions such as ``get_sightline_start_position``, reduced with the same
    axis selection as the particles.  The sightline runs ALONG ``projection_axis``; a
    direction vector that is not along it is out of scope (rotate the particles first).

    ``kernel``: an ``SPHKernel`` or its name ("cubic_column", "wendland_c2_column",
    "quartic_spline", "wendland_c2", "indicator", ...).  With a column kernel the result is a
    column density, [A] / L^2.  ``weights``: the weighted mean
    ``sum w A W / sum w W`` (0 where no particle reaches the point).  ``deterministic``:
    int64 fixed-point sums, bitwise reproducible whatever the order of particles and
    points (not with ``weights``).

    Periodic boxes need no flag: stage the particles with their periodic images and sample
    the staged float32 arrays (asp_sample2d, the fp32 entry point)::

        u, v, h, (a,) = stage_particles(pos, h, A, projection_axis=2, box_width=L, images=True)
        # px, py, out: device tensors (float64, float64, float32)
        _lib.lib().asp_sample2d(ptr(u), ptr(v), ptr(h), ptr(a), None, len(u), ptr(px, _d),
                                ptr(py, _d), M, kernel_id, ASP_F_DEVICE_PTRS, ptr(out), None,
                                0, stream)
    """
    import torch
    kid = _kernel_id(kernel)
    axis = axis_index(projection_axis)
    if deterministic and weights is not None:
        raise ValueError("deterministic sums cannot be combined with weights (a ratio)")
    on_device = hasattr(positions, "is_cuda") and positions.is_cuda
    cu, cv = AXIS_COLUMNS[axis]
    flags = _lib.ASP_F_DETERMINISTIC if deterministic else 0
    if weights is not None:
        flags |= _lib.ASP_F_RATIO
    D = _lib._d
    if on_device:
        pos = positions
        if pos.dtype != torch.float64 or pos.dim() != 2 or pos.shape[1] != 3:
            raise ValueError("positions must be an (N, 3) float64 tensor")
        dev = pos.device
        pos = pos.contiguous()
        n = pos.shape[0]
        h = _dev_field(smoothing_lengths, "smoothing_lengths", n, dev)
        a0 = _dev_field(particle_properties, "particle_properties", n, dev)
        a1 = None if weights is None else _dev_field(weights, "weights", n, dev)
        pts = points
        if (not hasattr(pts, "is_cuda") or pts.dtype != torch.float64 or pts.device != dev
                or pts.dim() != 2 or pts.shape[1] not in (2, 3)):
            raise ValueError(f"points must be an (M, 2) or (M, 3) float64 tensor on {dev}")
        m = pts.shape[0]
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        stream = getattr(stream, "cuda_stream", stream)  # a torch stream or a raw handle
        ext = torch.cuda.ExternalStream(stream, device=dev)
        with torch.cuda.stream(ext):  # the temporaries are ordered on the call's stream
            c = (0, 1) if pts.shape[1] == 2 else (cu, cv)
            px, py = pts[:, c[0]].contiguous(), pts[:, c[1]].contiguous()
            if a1 is not None:
                a0 = a0 * a1
            out0 = torch.empty(m, dtype=torch.float32, device=dev)
            out1 = None if a1 is None else torch.empty(m, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().asp_sample2d_f64(
            _lib.ptr(pos, D), _lib.ptr(h, D), _lib.ptr(a0, D), _lib.ptr(a1, D), n, axis,
            _lib.ptr(px, D), _lib.ptr(py, D), m, kid, flags | _lib.ASP_F_DEVICE_PTRS,
            _lib.ptr(out0), _lib.ptr(out1), dev.index or 0, stream))
        for t in (px, py, a0, out1):  # freed by the caching allocator only after the stream's work
            if t is not None:
                t.record_stream(ext)
        return out0
    pos = np.asarray(positions)
    if pos.ndim != 2 or pos.shape[1] != 3:
        raise ValueError(f"positions must have shape (N, 3), got {pos.shape}")
    if pos.dtype != np.float64:
        raise ValueError(f"positions must be float64, got {pos.dtype}")
    pos = np.ascontiguousarray(pos)
    n = pos.shape[0]
    h = _host_field(smoothing_lengths, "smoothing_lengths", n)
    a0 = _host_field(particle_properties, "particle_properties", n)
    a1 = None if weights is None else _host_field(weights, "weights", n)
    pts = np.asarray(points)
    if pts.ndim != 2 or pts.shape[1] not in (2, 3):
        raise ValueError(f"points must have shape (M, 2) or (M, 3), got {pts.shape}")
    if pts.dtype != np.float64:
        raise ValueError(f"points must be float64, got {pts.dtype}")
    c = (0, 1) if pts.shape[1] == 2 else (cu, cv)
    px, py = np.ascontiguousarray(pts[:, c[0]]), np.ascontiguousarray(pts[:, c[1]])
    m = pts.shape[0]
    if a1 is not None:
        a0 = a0 * a1
    out0 = np.zeros(m, dtype=np.float32)
    out1 = None if a1 is None else np.zeros(m, dtype=np.float32)
    if m == 0:
        return out0
    _lib.require_gpu(device)
    _lib.check(_lib.lib().asp_sample2d_f64(
        _lib.ptr(pos, D), _lib.ptr(h, D), _lib.ptr(a0, D), _lib.ptr(a1, D), n, axis,
        _lib.ptr(px, D), _lib.ptr(py, D), m, kid, flags, _lib.ptr(out0), _lib.ptr(out1), device,
        None))
    return out0
