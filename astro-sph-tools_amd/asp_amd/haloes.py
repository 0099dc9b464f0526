"""Nearest halo centre of every particle in a periodic box, and halo-centred radial profiles
and aperture sums, on the GPU.

Replaces the numerical core of the reference's second command-line tool
(_scripts/find_nearest_haloes.py:196-221): per minimum-halo-mass cut,
``KDTree(halo_centres[mask], boxsize=box_width).query(particle_positions)``.  Here all the
cuts go to the device in one call (asp_nearest, csrc/asp_nearest.hip): same arithmetic as
scipy's periodic distance, so the distances are bit-identical; the indices refer to the
full ``centres`` array (``np.take(halo_ids, index)`` needs no masked copy) and exact ties
go to the lowest index.

The only use of a distance stored beside an R200 is ``r / R200``: ``halo_profiles`` and
``aperture_sums`` (asp_halo_profiles, csrc/asp_profiles.hip) give the number of particles and
the sum of up to four particle properties in every radial bin around every halo, with the same
periodic arithmetic; haloes may overlap, so a particle counts for every halo it lies in.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._call import (alloc_out, call_flags, dev_f64, dptr, host_f64, is_device, positions_f64,
                    stream_scope)

MAX_SETS = 8
MAX_PROPS = 4
MAX_BINS = 64


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


def _host_centres(centres):
    """The (M, 3) float64 centres as a host array, given on the host or as a tensor."""
    return positions_f64(centres.cpu() if hasattr(centres, "is_cuda") else centres, "centres",
                         cast=False)[0]


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
    cen = _host_centres(centres)
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


def _profile_edges(edges):
    e = np.ascontiguousarray(np.asarray(edges.cpu() if hasattr(edges, "is_cuda") else edges),
                             dtype=np.float64)
    if e.ndim != 1 or not 2 <= e.size <= MAX_BINS + 1:
        raise ValueError(f"edges must be a 1-D array of 2 .. {MAX_BINS + 1} values, got shape "
                         f"{e.shape}")
    if not np.all(np.isfinite(e)) or e[0] < 0 or not np.all(np.diff(e) > 0):
        raise ValueError("edges must be finite, >= 0 and strictly ascending")
    return e


def _prop_list(props):
    """None, one array or a sequence of arrays -> a list (a 2-D array or tensor is its rows)."""
    if props is None:
        return []
    if hasattr(props, "is_cuda") or isinstance(props, np.ndarray) or hasattr(props, "units"):
        return [props] if props.ndim == 1 else list(props)
    props = list(props)
    if props and np.ndim(props[0]) == 0:  # one property given as a plain sequence of numbers
        return [np.asarray(props, dtype=np.float64)]
    return props


def halo_profiles(positions, centres, radii, edges, box_width, props=None, *, device: int = 0,
                  stream=None, accumulate=None):
    """``(count, sums)``: the number of particles and the sums of their properties in every
    radial bin around every halo, in the periodic box of width ``box_width``.

    ``positions``: (N, 3) float64, any values -- a NumPy (or unyt) host array, returning NumPy
    arrays, or a float64 torch tensor on the GPU, returning tensors there (``props`` are then
    tensors on that device too).  ``centres``: (M, 3) float64 with every coordinate in
    [0, box_width).  ``radii``: (M,) float64, finite and >= 0; bin b of halo j holds the
    particles with ``(edges[b] radii[j])**2 <= d2 < (edges[b + 1] radii[j])**2``, d2 the squared
    periodic distance to the centre (each particle's nearest image, once).  ``radii=None``:
    the edges are lengths.  ``edges``: B + 1 finite, strictly ascending values >= 0,
    1 <= B <= 64.  ``props``: None, one (N,) float64 array or a sequence of up to 4.
    ``accumulate``: a ``(count, sums)`` pair of an earlier call to add into (the pieces of a
    particle set split over readers).  Returns ``count`` (M, B) int64 and ``sums``
    (len(props), M, B) float64.
    """
    on_device = is_device(positions)
    if not on_device:
        pos, n, _ = positions_f64(positions, cast=False)
    plist = _prop_list(props)
    if len(plist) > MAX_PROPS:
        raise ValueError(f"at most {MAX_PROPS} props per call, got {len(plist)}")
    cen = _host_centres(centres)
    m = cen.shape[0]
    rad = None
    if radii is not None:
        rad = host_f64(radii.cpu() if hasattr(radii, "is_cuda") else radii, "radii", (m,),
                       cast=False)
    e = _profile_edges(edges)
    nbins, nprops = e.size - 1, len(plist)
    box_width = float(box_width)
    if on_device:
        import torch
        dev = positions.device
        with stream_scope(dev, stream) as scope:  # the uploads ordered on the call's stream
            pos, n, _ = positions_f64(positions, cast=False)
            dprops = None
            if nprops:
                dprops = torch.stack([dev_f64(p, f"props[{k}]", (n,), dev)
                                      for k, p in enumerate(plist)])
            dcen = torch.from_numpy(cen).to(dev)
            drad = None if rad is None else torch.from_numpy(rad).to(dev)
            dedges = torch.from_numpy(e).to(dev)
            scope.keep(pos, dprops, dcen, drad, dedges)
            given = accumulate or (None, None)
            count = alloc_out((m, nbins), torch.int64, dev, given[0], name="accumulate[0]")
            sums = alloc_out((nprops, m, nbins), torch.float64, dev, given[1], name="accumulate[1]")
            _lib.check(_lib.lib().asp_halo_profiles(
                dptr(pos), dptr(dprops), nprops, n, dptr(dcen), dptr(drad), m, dptr(dedges), nbins,
                box_width, _lib.ptr(count, _lib._i64), dptr(sums),
                call_flags(device_ptrs=True, accumulate=accumulate is not None),
                dev.index or 0, scope.raw))
        return count, sums
    hprops = None
    if nprops:
        hprops = np.stack([host_f64(p, f"props[{k}]", (n,), cast=False)
                           for k, p in enumerate(plist)])
    given = accumulate or (None, None)
    count = alloc_out((m, nbins), np.int64, None, given[0], zeros=True, name="accumulate[0]")
    sums = alloc_out((nprops, m, nbins), np.float64, None, given[1], zeros=True,
                     name="accumulate[1]")
    if m > 0 and n > 0:
        _lib.require_gpu(device)
    _lib.check(_lib.lib().asp_halo_profiles(
        dptr(pos), dptr(hprops), nprops, n, dptr(cen), dptr(rad), m, dptr(e), nbins, box_width,
        _lib.ptr(count, _lib._i64), dptr(sums) if nprops else None,
        call_flags(accumulate=accumulate is not None), device, None))
    return count, sums


def aperture_sums(positions, centres, radii, box_width, props=None, factor=1.0, **kw):
    """``(count (M,), sums (nprops, M))`` inside ``factor * radii`` of every halo: the one bin
    ``[0, factor]`` of :func:`halo_profiles` (``radii=None``: inside the length ``factor``)."""
    count, sums = halo_profiles(positions, centres, radii, [0.0, float(factor)], box_width, props,
                                **kw)
    return count[:, 0], sums[:, :, 0]
