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
from ._call import (alloc_out, call_flags, dev_f64, dptr, host_f64, is_device, positions_f64,
                    stream_scope)
from .tools.projections._kernels import KERNEL_IDS, named_kernel_id as _kernel_id  # noqa: F401


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
    axis selection as the particles.  The sightline runs ALONG ``projection_axis`` and the
    result is its total column; for a direction vector that is not along an axis, or for the
    run of a field along the sightline, use ``asp_amd.sightline_profiles`` (3-D sums at the
    centres of the sightline's bins).

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
    kid = _kernel_id(kernel)
    axis = axis_index(projection_axis)
    if deterministic and weights is not None:
        raise ValueError("deterministic sums cannot be combined with weights (a ratio)")
    cols = AXIS_COLUMNS[axis]
    fields = ((smoothing_lengths, "smoothing_lengths"), (particle_properties, "particle_properties"),
              (weights, "weights"))
    if is_device(positions):
        import torch
        dev = positions.device
        pts = points
        if (not is_device(pts) or pts.dtype != torch.float64 or pts.device != dev
                or pts.dim() != 2 or pts.shape[1] not in (2, 3)):
            raise ValueError(f"points must be an (M, 2) or (M, 3) float64 tensor on {dev}")
        m = pts.shape[0]
        with stream_scope(dev, stream) as scope:  # the temporaries are ordered on the call's stream
            pos, n, _ = positions_f64(positions, cast=False)
            h, a0, a1 = (None if a is None else dev_f64(a, name, (n,), dev) for a, name in fields)
            c = (0, 1) if pts.shape[1] == 2 else cols
            px, py = pts[:, c[0]].contiguous(), pts[:, c[1]].contiguous()
            if a1 is not None:
                a0 = a0 * a1
            out0 = alloc_out((m,), torch.float32, dev)
            out1 = None if a1 is None else alloc_out((m,), torch.float32, dev)
            scope.keep(pos, h, a0, a1, px, py, out1)
            _lib.check(_lib.lib().asp_sample2d_f64(
                dptr(pos), dptr(h), dptr(a0), dptr(a1), n, axis, dptr(px), dptr(py), m, kid,
                call_flags(True, weights is not None, deterministic=deterministic),
                _lib.ptr(out0), _lib.ptr(out1), dev.index or 0, scope.raw))
        return out0
    pos, n, _ = positions_f64(positions, cast=False)
    h, a0, a1 = (None if a is None else host_f64(a, name, (n,), cast=False) for a, name in fields)
    pts = np.asarray(points)
    if pts.ndim != 2 or pts.shape[1] not in (2, 3):
        raise ValueError(f"points must have shape (M, 2) or (M, 3), got {pts.shape}")
    pts = host_f64(pts, "points", cast=False)
    c = (0, 1) if pts.shape[1] == 2 else cols
    px, py = np.ascontiguousarray(pts[:, c[0]]), np.ascontiguousarray(pts[:, c[1]])
    m = pts.shape[0]
    if a1 is not None:
        a0 = a0 * a1
    out0 = alloc_out((m,), np.float32, None, zeros=True)
    out1 = None if a1 is None else alloc_out((m,), np.float32, None, zeros=True)
    if m == 0:
        return out0
    _lib.require_gpu(device)
    _lib.check(_lib.lib().asp_sample2d_f64(
        dptr(pos), dptr(h), dptr(a0), dptr(a1), n, axis, dptr(px), dptr(py), m, kid,
        call_flags(False, weights is not None, deterministic=deterministic),
        _lib.ptr(out0), _lib.ptr(out1), device, None))
    return out0
