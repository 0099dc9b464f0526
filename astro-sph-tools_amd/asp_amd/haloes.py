"""Nearest halo centre of every particle in a periodic box, on the GPU.

Replaces the numerical core of the reference's second command-line tool
(_scripts/find_nearest_haloes.py:196-221): per minimum-halo-mass cut,
``KDTree(halo_centres[mask], boxsize=box_width).query(particle_positions)``.  Here all the
cuts go to the device in one call (asp_nearest, csrc/asp_nearest.hip): same arithmetic as
scipy's periodic distance, so the distances are bit-identical; the indices refer to the
full ``centres`` array (``np.take(halo_ids, index)`` needs no masked copy) and exact ties
go to the lowest index.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._call import alloc_out, call_flags, dptr, is_device, positions_f64, stream_scope

MAX_SETS = 8


def halo_mass_masks(halo_masses, minimum_log10_halo_masses):
    """The script's ``halo_masks`` (lines 166-176): every halo with a mass, then one mask per
    minimum log10 mass, in the given order."""
    m = np.asarray(halo_masses)
    return [m > 0] + [m > 10 ** t for t in minimum_log10_halo_masses]


def _member_words(masks, m):
    """Boolean masks -> one uint32 per centre, bit s = membership of set s."""
    if len(masks) < 1 or len(masks) > MAX_SETS:
        raise ValueError(f"between 1 and {MAX_SETS} masks per call, got {len(masks)}")
    words = np.zeros(max(m, 1), dtype=np.uint32)  # (never an empty buffer: NULL means no masks)
    for s, mask in enumerate(masks):
        if hasattr(mask, "is_cuda"):
            mask = mask.cpu().numpy()
        mask = np.asarray(mask)
        if mask.dtype != np.bool_ or mask.shape != (m,):
            raise ValueError(f"mask {s} must be a boolean array of length {m}, got "
                             f"{mask.dtype} {mask.shape}")
        words[:m] |= mask.astype(np.uint32) << np.uint32(s)
    return words


def nearest_haloes(positions, centres, box_width, masks=None, *, device: int = 0, stream=None):
    """(index, distance) of the nearest centre of every position in the periodic box of
    width ``box_width``, per mask.

    ``positions``: (N, 3) float64 -- a NumPy (or unyt) host array, returning NumPy arrays,
    or a float64 torch tensor on the GPU, returning tensors there.  ``centres``: (M, 3)
    float64 with every coordinate in [0, box_width).  ``masks``: None (every centre), or up
    to 8 boolean arrays of length M (any masks, not only nested ones).  Returns
    ``(len(masks) or 1, N)`` arrays: int32 positions in ``centres`` (-1 for an empty mask,
    distance inf; -1 and NaN for a position with a non-finite coordinate) and float64
    distances.
    """
    on_device = is_device(positions)
    if not on_device:
        pos, n, _ = positions_f64(positions, cast=False)
    cen = positions_f64(centres.cpu() if hasattr(centres, "is_cuda") else centres, "centres",
                        cast=False)[0]
    m = cen.shape[0]
    words = None if masks is None else _member_words(list(masks), m)
    nsets = 1 if masks is None else len(masks)
    box_width = float(box_width)
    u32 = _lib.C.POINTER(_lib.C.c_uint32)
    if on_device:
        import torch
        dev = positions.device
        with stream_scope(dev, stream) as scope:  # the centres' upload ordered on the call's stream
            pos, n, _ = positions_f64(positions, cast=False)
            dcen = torch.from_numpy(cen).to(dev)
            dwords = None if words is None else torch.from_numpy(words.view(np.int32)).to(dev)
            scope.keep(pos, dcen, dwords)
            index = alloc_out((nsets, n), torch.int32, dev)
            distance = alloc_out((nsets, n), torch.float64, dev)
            _lib.check(_lib.lib().asp_nearest(
                dptr(pos), n, dptr(dcen), m, _lib.ptr(dwords, u32), nsets, box_width,
                _lib.ptr(index, _lib._i32), dptr(distance), call_flags(device_ptrs=True),
                dev.index or 0, scope.raw))
        return index, distance
    _lib.require_gpu(device)
    index = alloc_out((nsets, n), np.int32, None)
    distance = alloc_out((nsets, n), np.float64, None)
    _lib.check(_lib.lib().asp_nearest(
        dptr(pos), n, dptr(cen), m, _lib.ptr(words, u32), nsets, box_width,
        _lib.ptr(index, _lib._i32), dptr(distance), 0, device, None))
    return index, distance
