"""Sightline spectra on the GPU: SPH columns deposited in velocity bins.

The reference's sightline objects (``LineOfSightBase``, _LineOfSightBase.py:130-189) carry
positions, velocities, masses, temperatures, densities and smoothing lengths -- the inputs of
an absorption spectrum.  :func:`sightline_spectra` spreads every particle's column at a
sightline (the pair term of :func:`asp_amd.sightline_columns`) over velocity bins with the
bin-averaged Gaussian of its Doppler width, through asp_spectra2d_f64
(csrc/asp_spectra.hip; include/asp_spectra.h has the definition).  With ion masses from
``asp_amd.ionisation`` the result is the ion's column density per unit velocity; optical
depths, fluxes and other line profiles are per-bin arithmetic on it.
"""
from __future__ import annotations

import numpy as np

from ._axes import AXIS_COLUMNS, axis_index
from ._call import sample_sums
from .tools.projections._kernels import named_kernel_id as _kernel_id


def los_coordinate(positions, velocities, axis, hubble_rate, box_velocity=None):
    """The velocity-space coordinate along ``axis``, ``hubble_rate * x + v`` in float64, from
    (N, 3) ``positions`` and ``velocities`` (NumPy arrays, or torch tensors, which stay where
    they are); wrapped into ``[0, box_velocity)`` when that is given (a periodic box of
    velocity width ``hubble_rate * L``)."""
    k = axis_index(axis)
    if hasattr(positions, "is_cuda"):
        import torch
        vc = hubble_rate * positions[:, k].to(torch.float64) + velocities[:, k].to(torch.float64)
        return vc if box_velocity is None else torch.remainder(vc, box_velocity)
    vc = hubble_rate * np.asarray(positions, np.float64)[:, k] + np.asarray(velocities, np.float64)[:, k]
    return vc if box_velocity is None else np.mod(vc, box_velocity)


def sightline_spectra(positions, smoothing_lengths, particle_properties, los_coordinate, doppler_b,
                      points, projection_axis, v_min, dv, n_bins, ring: bool = False,
                      kernel="cubic_column", weights=None, *, device: int = 0, stream=None):
    """``sum_p A_p W(r, h_p) G_p(k)`` for every sightline and velocity bin k: the column of
    :func:`asp_amd.sightline_columns` (same neighbour sets, same term) times the fraction
    per unit velocity of a Gaussian centred on ``los_coordinate[p]`` with Doppler parameter
    ``doppler_b[p]`` (``exp(-(v / b)**2)``) that falls into bin
    ``[v_min + k dv, v_min + (k + 1) dv)``.  Returns (M, n_bins) float32.

    Arguments, host / device handling, ``points`` as (M, 2) or (M, 3), ``kernel`` and
    ``weights`` (the weighted mean per bin, ``sum w A W G / sum w W G``, 0 where nothing
    reaches the bin) are those of ``sightline_columns``; ``los_coordinate`` and ``doppler_b``
    are (N,) float64 like the other particle fields (see :func:`los_coordinate`).

    ``ring=False``: the bins are a window; what falls outside is dropped.  ``ring=True``: the
    ``n_bins`` bins are a periodic ring of width ``n_bins * dv`` (a periodic box), and
    ``out.sum(axis=1) * dv`` is the sightline's total column.  A particle is deposited over
    ``los_coordinate +- 5 doppler_b`` (what lies beyond is below 2e-12 of its column); one with
    a non-finite ``los_coordinate``, or a ``doppler_b`` that is not finite and positive, is in
    no bin.
    """
    kid = _kernel_id(kernel)
    axis = axis_index(projection_axis)
    n_bins = int(n_bins)
    bins = (float(v_min), float(dv), n_bins, 1 if ring else 0)
    if n_bins < 1:
        raise ValueError("n_bins must be >= 1")
    return sample_sums("asp_spectra2d_f64", (axis,), positions, smoothing_lengths, particle_properties,
                       weights, points, (2, 3), lambda w: (0, 1) if w == 2 else AXIS_COLUMNS[axis], kid,
                       False, device, stream,
                       extra=((los_coordinate, "los_coordinate"), (doppler_b, "doppler_b")),
                       bins=bins, width=n_bins)
