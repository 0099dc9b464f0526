"""SPH sums at arbitrary 3-D positions, on the GPU.

:func:`sample_points` evaluates ``sum_p A_p W(r, h_p)`` -- the sum ``asp_project3d`` forms at
the corners of a voxel lattice -- at M arbitrary positions: halo centres, star or black-hole
particles, the particles of another snapshot.  :func:`sightline_profiles` places the points
along sightlines of any direction (the start position and direction vector of
``LineOfSightFileBase``, _LineOfSightBase.py:16-73) and returns the run of the field along
each one.  Both go through asp_sample3d_f64 (include/asp_points.h; csrc/asp_sample3d.hip and the
point grid it shares with the 2-D sampler, csrc/asp_sample.hpp):
the neighbour test ``r2 < (2h)**2`` in fp64 on the reader's own arrays, bit-exact neighbour
sets, fp32 terms.
"""
from __future__ import annotations

import numpy as np

from ._call import dev_f64, host_f64, is_device, sample_sums, stream_scope
from .tools.projections._kernels import COLUMN_KERNEL_IDS, named_kernel_id

__all__ = ["sample_points", "sightline_profiles", "sightline_points"]


def _volume_kernel_id(kernel) -> int:
    kid = named_kernel_id(kernel)
    if kid in COLUMN_KERNEL_IDS:
        raise ValueError(f"kernel {kernel!r} is a column kernel: it has no 3-D form (use "
                         "sightline_columns for columns along the projection axis)")
    return kid


def sample_points(positions, smoothing_lengths, particle_properties, points, kernel="cubic",
                  weights=None, deterministic: bool = False, *, device: int = 0, stream=None):
    """``sum_p A_p W(r, h_p)`` at every point, over the particles with ``r2 < (2 h_p)**2``,
    r the 3-D distance between particle and point.

    ``positions`` (N, 3), ``smoothing_lengths`` (N,), ``particle_properties`` (N,), the
    optional ``weights`` (N,) and ``points`` (M, 3): float64 NumPy (or unyt) host arrays,
    returning a NumPy float32 array of length M, or float64 torch tensors on the GPU,
    returning a tensor there, the work ordered on ``stream`` (default: the current stream).

    ``kernel``: an ``SPHKernel`` or its name ("cubic", "quartic_spline", "wendland_c2",
    "indicator"); a column kernel raises ``ValueError``.  ``weights``: the weighted mean
    ``sum w A W / sum w W`` (0 where no particle reaches the point).  ``deterministic``:
    int64 fixed-point sums, bitwise reproducible whatever the order of particles and points
    (not with ``weights``).  A point with a non-finite coordinate reads 0.
    """
    kid = _volume_kernel_id(kernel)
    if deterministic and weights is not None:
        raise ValueError("deterministic sums cannot be combined with weights (a ratio)")
    return sample_sums("asp_sample3d_f64", (), positions, smoothing_lengths, particle_properties,
                       weights, points, (3,), lambda w: (0, 1, 2), kid, deterministic, device, stream)


def sightline_points(starts, directions, lengths, n_bins):
    """The (S, n_bins, 3) float64 bin centres of S sightlines,

        ``X[s, b] = start_s + ((b + 0.5) * (length_s / n_bins)) * d_s / |d_s|``,
        ``|d| = sqrt(dx*dx + dy*dy + dz*dz)``,

    formed with plain elementwise operators in exactly this order: NumPy for host arrays,
    torch (on the tensors' device and current stream) for device tensors.  ``starts`` and
    ``directions`` are (S, 3); ``lengths`` a scalar or (S,).

    Host arrays are checked: a zero or non-finite direction, ``n_bins < 1`` or a negative
    length raises ``ValueError``.  Device tensors are not read back: such rows become
    non-finite points, which read 0 in :func:`sample_points`.
    """
    if int(n_bins) != n_bins or n_bins < 1:
        raise ValueError(f"n_bins must be an integer >= 1, got {n_bins!r}")
    n_bins = int(n_bins)
    if is_device(starts):
        import torch
        dev = starts.device
        if starts.dtype != torch.float64 or starts.dim() != 2 or starts.shape[1] != 3:
            raise ValueError("starts must be an (S, 3) float64 tensor")
        s = starts.shape[0]
        d = dev_f64(directions, "directions", (s, 3), dev)
        if is_device(lengths):
            length = dev_f64(lengths, "lengths", (s,), dev)
        else:
            length = torch.as_tensor(np.broadcast_to(host_f64(lengths, "lengths", cast=True), (s,)).copy(),
                                     device=dev)
        b = torch.arange(n_bins, dtype=torch.float64, device=dev)
        sqrt = torch.sqrt
        # a tensor, not a Python scalar: torch divides by a scalar as a multiplication by its
        # reciprocal, which is not the formula's correctly rounded length / n_bins
        n_bins = torch.tensor(float(n_bins), dtype=torch.float64, device=dev)
    else:
        st = np.asarray(starts)
        if st.ndim != 2 or st.shape[1] != 3:
            raise ValueError(f"starts must have shape (S, 3), got {st.shape}")
        starts = host_f64(st, "starts", cast=False)
        s = starts.shape[0]
        d = host_f64(directions, "directions", (s, 3), cast=False)
        length = np.asarray(lengths, np.float64)
        if length.ndim not in (0, 1) or (length.ndim == 1 and length.shape != (s,)):
            raise ValueError(f"lengths must be a scalar or have shape ({s},), got {length.shape}")
        length = np.ascontiguousarray(np.broadcast_to(length, (s,)))
        if not np.all(np.isfinite(d)) or np.any(np.all(d == 0.0, axis=1)):
            raise ValueError("directions must be finite and non-zero")
        if not np.all(length >= 0.0):
            raise ValueError("lengths must be >= 0")
        b = np.arange(n_bins, dtype=np.float64)
        sqrt = np.sqrt
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    norm = sqrt(dx * dx + dy * dy + dz * dz)
    unit = d / norm[:, None]
    step = (b[None, :] + 0.5) * (length / n_bins)[:, None]
    return starts[:, None, :] + step[:, :, None] * unit[:, None, :]


def sightline_profiles(positions, smoothing_lengths, particle_properties, starts, directions,
                       lengths, n_bins, kernel="cubic", weights=None, deterministic: bool = False,
                       return_points: bool = False, *, device: int = 0, stream=None):
    """The run of ``sum_p A_p W(r, h_p)`` along S sightlines of any direction: the field at
    the centres of ``n_bins`` equal bins of each sightline (:func:`sightline_points`),
    through :func:`sample_points`.  Returns (S, n_bins) float32 -- and the (S, n_bins, 3)
    float64 points with ``return_points`` -- as NumPy arrays for host inputs, tensors for
    device tensors (particle arrays and sightline arrays on the same side).

    Host arrays: a zero or non-finite direction, ``n_bins < 1`` or a negative length raises
    ``ValueError``.  Device tensors are not read back: those rows become non-finite points
    and read 0.  ``kernel``, ``weights``, ``deterministic``, ``device``, ``stream``: as
    :func:`sample_points`.
    """
    _volume_kernel_id(kernel)
    if deterministic and weights is not None:
        raise ValueError("deterministic sums cannot be combined with weights (a ratio)")
    if is_device(positions) != is_device(starts):
        raise ValueError("positions and starts must both be host arrays or both device tensors")
    if is_device(starts):
        with stream_scope(starts.device, stream):
            pts = sightline_points(starts, directions, lengths, n_bins)
    else:
        pts = sightline_points(starts, directions, lengths, n_bins)
    s = pts.shape[0]
    out = sample_points(positions, smoothing_lengths, particle_properties, pts.reshape(-1, 3),
                        kernel, weights, deterministic, device=device, stream=stream)
    out = out.reshape(s, int(n_bins))
    return (out, pts) if return_points else out
