"""SPH sums at sightline positions, on the GPU.

The reference's unit of work, ``calculate_pixel_value`` (_pixel_calculations.pyx:9-36), takes
an arbitrary corner (x, y); only ``create_image`` restricts it to a pixel lattice.
:func:`sightline_columns` evaluates it at M arbitrary points -- the start positions of
``LineOfSightFileBase`` (_LineOfSightBase.py:16-73), quasar sightlines at given impact
parameters -- through asp_sample2d_f64 (csrc/asp_sample.hip, csrc/asp_sample.hpp): the neighbour test
``r2 < (2h)**2`` in fp64 on the reader's own arrays, bit-exact neighbour sets, fp32 terms.
With a column kernel (the default) and ion masses from ``asp_amd.ionisation`` the result is
the ion's column density at each sightline.
"""
from __future__ import annotations

from ._axes import AXIS_COLUMNS, axis_index
from ._call import sample_sums
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
    return sample_sums("asp_sample2d_f64", (axis,), positions, smoothing_lengths, particle_properties,
                       weights, points, (2, 3), lambda w: (0, 1) if w == 2 else AXIS_COLUMNS[axis], kid,
                       deterministic, device, stream)
