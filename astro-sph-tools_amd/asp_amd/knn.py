"""Smoothing lengths from the k-th nearest neighbour, on the GPU.

Replaces the scipy KDTree query of the reference's SWIFT reader
(/root/reference/src/astro_sph_tools/io/SWIFT/_SnapshotSWIFT.py:62-83), which gives dark
matter particles ``h = tree.query(positions, k=32)[0][:, 31]``: the distance to the 32nd
nearest particle, the particle itself counted.  Same distance arithmetic (fp64
Euclidean), so the values are bit-identical (asp_knn_smoothing_lengths, csrc/asp_knn.hip).
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._call import alloc_out, call_flags, dptr, is_device, positions_f64, stream_scope


def knn_smoothing_lengths(positions, k: int = 32, *, device: int = 0, stream=None):
    """Distance from every particle to its k-th nearest neighbour (itself included).

    ``positions``: (N, 3) float64 -- a NumPy (or unyt) host array, returning a NumPy
    array, or a float64 torch tensor on the GPU, returning a tensor there.  ``inf`` where
    fewer than k particles exist (as scipy reports a missing neighbour).

    Non-finite values (scipy raises; here they are defined): a row with a NaN or infinite
    coordinate is nobody's neighbour and gets ``inf``; every other row gets its k-th smallest
    finite squared distance among the rows with a position, or ``inf`` if fewer than k are
    finite (too few such rows, or squares that overflow) -- what scipy returns for the finite
    rows alone.
    """
    k = int(k)
    if is_device(positions):
        dev = positions.device
        with stream_scope(dev, stream) as scope:  # a .contiguous() copy is ordered on the stream
            pos, n, _ = positions_f64(positions, cast=True)
            scope.keep(pos)
            h = alloc_out((n,), pos.dtype, dev)
            _lib.check(_lib.lib().asp_knn_smoothing_lengths(
                dptr(pos), n, k, dptr(h), call_flags(device_ptrs=True), dev.index or 0, scope.raw))
        return h
    pos, n, _ = positions_f64(positions, cast=True)
    _lib.require_gpu(device)
    h = alloc_out((n,), np.float64, None)
    _lib.check(_lib.lib().asp_knn_smoothing_lengths(dptr(pos), n, k, dptr(h), 0, device, None))
    return h
