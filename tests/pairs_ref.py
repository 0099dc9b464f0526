"""The pair lists of the kernel_func plug-in (asp_pairs_begin / _emit / _end, include/asp.h),
pair by pair: a plain helper module -- NumPy only, no GPU, no project code, no fixtures.

``reference_pairs`` restates the reference's two decisions in fp64 and in its own operation
order (_projector.py:38-48 the chunk cull, _pixel_calculations.pyx:11-14 the pixel corner,
:20-31 the distance test; oracle/asp_oracle.c states the same as cull_pass / pixel_pass):

    psx    = (x_max - x_min) / nx           the u pitch of the corners and of the cull
    psy_c  = (y_max - y_min) / ny           the cull's v pitch
    psy    = (y_max - y_min) / nx           the pixel's v pitch (quirk S2: nx)
    corner   X = x_min + xi * psx,  Y = y_min + yi * psy
    cull     (w_min + c0 * pitch) - 2h <= w < (w_min + c_end * pitch) + 2h   on (cu, cv),
             [c0, c_end) the chunk of the pixel on that axis (c_end clipped to the image)
    pair     r2 = dx*dx + dy*dy < (2h)*(2h),  dx = u - X, dy = v - Y         on (u, v)

Every comparison made with it is exact: pixel ids, particle indices and the BITS of r2.

``decode_emit`` turns one emit's CSR (pixels tile by tile, lx * 64 + ly inside a tile)
back into image pixels; ``assert_pairs_equal`` holds it to the reference.
"""
from collections import namedtuple

import numpy as np

TILE = 64
TILE_PIX = TILE * TILE

Pairs = namedtuple("Pairs", "pixel particle r2")
# offsets: as emitted.  pixel / particle / r2: sorted by (pixel, particle), or None when
# the offsets cannot be decoded.  outside: the slots of the range outside the image.
Emit = namedtuple("Emit", "pixel particle r2 offsets outside t0 t1 nty size tile_pairs")


def _span(w, reach, w_min, pitch, npx):
    """A pixel range [i0, i1) that holds every pixel whose corner lies within ``reach`` of
    w, with two pixels to spare (the masks decide); the whole axis for non-finite input."""
    with np.errstate(all="ignore"):
        lo, hi = (w - reach - w_min) / pitch, (w + reach - w_min) / pitch
    if not (np.isfinite(lo) and np.isfinite(hi)):
        return 0, npx
    i0 = int(min(max(np.floor(lo) - 2, 0), npx))
    i1 = int(min(max(np.ceil(hi) + 3, 0), npx))
    return i0, i1


def reference_pairs(u, v, cu, cv, h, size, chunk, ext, cull=True):
    """Every (pixel, particle) pair create_image includes, as Pairs(pixel_id, particle, r2)
    sorted by (pixel_id, particle); pixel_id = xi * ny + yi.  (cu, cv): the cull's columns
    (None: the pixel's own u, v).  ``cull=False``: the pixel test alone (what a cull removes
    is measured against this)."""
    u, v, h = (np.ascontiguousarray(a, dtype=np.float64) for a in (u, v, h))
    cu = u if cu is None else np.ascontiguousarray(cu, dtype=np.float64)
    cv = v if cv is None else np.ascontiguousarray(cv, dtype=np.float64)
    nx, ny = int(size[0]), int(size[1])
    cs = int(chunk)
    x_min, x_max, y_min, y_max = (float(e) for e in ext)
    psx = (x_max - x_min) / nx
    psy_c = (y_max - y_min) / ny
    psy = (y_max - y_min) / nx
    ix, iy = np.arange(nx), np.arange(ny)
    X = x_min + ix.astype(np.float64) * psx
    Y = y_min + iy.astype(np.float64) * psy
    c0x, c0y = (ix // cs) * cs, (iy // cs) * cs
    xlo = x_min + c0x * psx
    xhi = x_min + np.minimum(c0x + cs, nx) * psx
    ylo = y_min + c0y * psy_c
    yhi = y_min + np.minimum(c0y + cs, ny) * psy_c
    pix, part, r2s = [], [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for p in range(h.size):
            up, vp, hp = u[p], v[p], h[p]
            if np.isnan(up) or np.isnan(vp) or np.isnan(hp):
                continue  # every comparison with a NaN is false: no pairs
            h2 = 2 * hp
            t = 2.0 * hp
            i0, i1 = _span(up, abs(t), x_min, psx, nx)
            j0, j1 = _span(vp, abs(t), y_min, psy, ny)
            if i0 >= i1 or j0 >= j1:
                continue
            rows = (cu[p] >= xlo[i0:i1] - h2) & (cu[p] < xhi[i0:i1] + h2)
            cols = (cv[p] >= ylo[j0:j1] - h2) & (cv[p] < yhi[j0:j1] + h2)
            dx, dy = up - X[i0:i1], vp - Y[j0:j1]
            r2 = (dx * dx)[:, None] + (dy * dy)[None, :]
            inc = r2 < t * t
            if cull:
                inc &= rows[:, None] & cols[None, :]
            a, b = np.nonzero(inc)
            if a.size:
                pix.append((a + i0).astype(np.int64) * ny + (b + j0))
                part.append(np.full(a.size, p, np.int32))
                r2s.append(r2[a, b])
    if not pix:
        return Pairs(np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0))
    pix, part, r2s = np.concatenate(pix), np.concatenate(part), np.concatenate(r2s)
    order = np.lexsort((part, pix))
    return Pairs(pix[order], part[order], r2s[order])


def pixel_counts(pairs, size):
    """Pairs per pixel, int64 (nx, ny)."""
    nx, ny = int(size[0]), int(size[1])
    return np.bincount(pairs.pixel, minlength=nx * ny).reshape(nx, ny)


def tile_of(pixel, size):
    """The GPU tile t = tx * ceil(ny / 64) + ty of pixel ids."""
    ny = int(size[1])
    nty = -(-ny // TILE)
    return (pixel // ny) // TILE * nty + (pixel % ny) // TILE


def tile_counts(pairs, size):
    """Pairs per GPU tile of the whole image (the session's tile_pairs)."""
    ntx, nty = -(-int(size[0]) // TILE), -(-int(size[1]) // TILE)
    return np.bincount(tile_of(pairs.pixel, size), minlength=ntx * nty).astype(np.int64)


def slot_pixels(t0, t1, nty, size):
    """(xi, yi, inside) of every slot q of the tile range [t0, t1)."""
    nx, ny = int(size[0]), int(size[1])
    q = np.arange((t1 - t0) * TILE_PIX, dtype=np.int64)
    t, k = t0 + q // TILE_PIX, q % TILE_PIX
    xi = (t // nty) * TILE + k // TILE
    yi = (t % nty) * TILE + k % TILE
    return xi, yi, (xi < nx) & (yi < ny)


def decode_emit(offsets, particle, r2, t0, t1, nty, size, tile_pairs=None):
    """One emit of the tiles [t0, t1) as an Emit: slot q -> (tile, lx, ly) -> (xi, yi), the
    pairs sorted by (pixel_id, particle), and the slots that lie outside the image.
    ``tile_pairs``: the session's per-tile totals (whole image), kept for the assertions."""
    offsets = np.asarray(offsets, np.int64)
    particle = np.asarray(particle, np.int32)
    r2 = np.asarray(r2, np.float64)
    nslots = (t1 - t0) * TILE_PIX
    xi, yi, inside = slot_pixels(t0, t1, nty, size)
    outside = np.nonzero(~inside)[0]
    counts = np.diff(offsets)
    ok = (offsets.size == nslots + 1 and (counts >= 0).all() and offsets[0] == 0
          and offsets[-1] == particle.size == r2.size)
    if not ok:
        return Emit(None, None, None, offsets, outside, t0, t1, nty, tuple(size), tile_pairs)
    pix = np.repeat(xi * int(size[1]) + yi, counts)
    order = np.lexsort((r2, particle, pix))
    return Emit(pix[order], particle[order], r2[order], offsets, outside, t0, t1, nty,
                tuple(size), tile_pairs)


def _describe(pixel, particle, r2, k, ny):
    if k >= pixel.size:
        return "(none)"
    return (f"(xi={int(pixel[k] // ny)}, yi={int(pixel[k] % ny)}, particle={int(particle[k])}, "
            f"r2={r2[k]!r} [{r2[k].hex()}])")


def assert_pairs_equal(got, want):
    """``got``: an Emit; ``want``: the reference Pairs of the WHOLE image.  In this order:
    the offsets (non-decreasing, from 0, ending at the tile totals' sum), the slots outside
    the image (empty), each tile's total, the (pixel, particle) lists, the bits of r2."""
    nx, ny = got.size
    off = got.offsets
    nslots = (got.t1 - got.t0) * TILE_PIX
    assert off.size == nslots + 1, f"{off.size} offsets for {nslots} slots"
    assert off[0] == 0, f"offsets[0] = {off[0]}"
    d = np.diff(off)
    assert (d >= 0).all(), f"offsets decrease at slot {int(np.argmax(d < 0))}"
    if got.tile_pairs is not None:
        total = int(np.asarray(got.tile_pairs)[got.t0:got.t1].sum())
        assert off[-1] == total, f"offsets end at {off[-1]}, tile_pairs sum to {total}"
    assert got.pixel is not None, "offsets[-1] and the pair arrays' sizes disagree"
    bad = got.outside[d[got.outside] != 0]
    assert bad.size == 0, f"{bad.size} slots outside the image hold pairs (first: slot {bad[:1]})"
    sel = (tile_of(want.pixel, got.size) >= got.t0) & (tile_of(want.pixel, got.size) < got.t1)
    wpix, wpart, wr2 = want.pixel[sel], want.particle[sel], want.r2[sel]
    ntiles = -(-nx // TILE) * got.nty
    wt = np.bincount(tile_of(wpix, got.size), minlength=ntiles)[got.t0:got.t1]
    if got.tile_pairs is not None:
        gt = np.asarray(got.tile_pairs)[got.t0:got.t1]
        diff = np.nonzero(gt != wt)[0]
        assert diff.size == 0, (f"tile_pairs differ in {diff.size} tiles; first: tile "
                                f"{got.t0 + int(diff[0])}: {int(gt[diff[0]])} (device) vs "
                                f"{int(wt[diff[0]])} (reference)")
    same = (got.pixel.size == wpix.size and np.array_equal(got.pixel, wpix)
            and np.array_equal(got.particle, wpart))
    if not same:
        m = min(got.pixel.size, wpix.size)
        ne = np.nonzero((got.pixel[:m] != wpix[:m]) | (got.particle[:m] != wpart[:m]))[0]
        k = int(ne[0]) if ne.size else m
        raise AssertionError(
            f"pair lists differ ({got.pixel.size} device pairs, {wpix.size} reference pairs); "
            f"first difference at sorted pair {k}: device "
            f"{_describe(got.pixel, got.particle, got.r2, k, ny)}, reference "
            f"{_describe(wpix, wpart, wr2, k, ny)}")
    gb, wb = got.r2.view(np.uint64), np.ascontiguousarray(wr2).view(np.uint64)
    if not np.array_equal(gb, wb):
        ne = np.nonzero(gb != wb)[0]
        k = int(ne[0])
        raise AssertionError(
            f"r2 differs in its bits for {ne.size} of {gb.size} pairs; first: device "
            f"{_describe(got.pixel, got.particle, got.r2, k, ny)}, reference "
            f"{_describe(wpix, wpart, wr2, k, ny)}")
