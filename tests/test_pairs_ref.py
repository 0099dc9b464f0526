"""tests/pairs_ref.py against the oracle, on the CPU: the NumPy reference that
tests/test_gpu_pairs.py holds the device's pair lists to is itself held to
oracle/asp_oracle.c (cull_pass / pixel_pass, pinned to the reference's own output by
tests/test_oracle_golden.py), on the very input sets of the GPU cases a to d:

* per-pixel COUNTS equal ``oracle.project_scatter(kernel="indicator")`` bit for bit;
* per-pixel particle LISTS equal ``oracle.pixel_neighbours`` on 200 sampled pixels.  That
  oracle call has no cull columns of its own, so for the mixed axis spellings the lists
  are pinned through three exact integer checksums per pixel instead (the sums of p, of
  p^2 and of (p * 2654435761) mod 2^20 over the pixel's particles p, all below 2^53),
  which ``project_scatter(cu=, cv=)`` forms over every pixel.

The decoder and the assertions are checked on a hand-made CSR of a 70 x 130 image.
"""
import numpy as np
import pytest

import pairs_cases as pc
import pairs_ref as pr


def _counts_match(oracle, c, ref):
    n = c["h"].size
    want, _ = oracle.project_scatter(c["u"], c["v"], c["h"], np.ones(n), None, c["size"],
                                     c["chunk"], *c["ext"], kernel="indicator", cu=c["cu"],
                                     cv=c["cv"])
    got = pr.pixel_counts(ref, c["size"])
    assert want.sum() > 0
    assert np.array_equal(got, want)
    return got


def _lists_match(oracle, c, ref, counts, seed):
    nx, ny = c["size"]
    rng = np.random.default_rng(seed)
    busy = np.nonzero(counts.reshape(-1))[0]
    pix = np.unique(np.concatenate([rng.choice(busy, min(150, busy.size), replace=False),
                                    rng.integers(0, nx * ny, 50),
                                    [0, ny - 1, (nx - 1) * ny, nx * ny - 1]]))
    offs, idx = oracle.pixel_neighbours(c["pos"], c["h"], c["size"], c["chunk"], c["axes"][0],
                                        *c["ext"], pix)
    lo = np.searchsorted(ref.pixel, pix, side="left")
    hi = np.searchsorted(ref.pixel, pix, side="right")
    assert np.array_equal(hi - lo, np.diff(offs))
    for k in range(pix.size):
        assert np.array_equal(ref.particle[lo[k]:hi[k]], idx[offs[k]:offs[k + 1]]), pix[k]


def _checksums_match(oracle, c, ref):
    n = c["h"].size
    p = np.arange(n, dtype=np.int64)
    for w in (p, p * p, (p * 2654435761) % (1 << 20)):
        want, _ = oracle.project_scatter(c["u"], c["v"], c["h"], w.astype(np.float64), None,
                                         c["size"], c["chunk"], *c["ext"], kernel="indicator",
                                         cu=c["cu"], cv=c["cv"])
        got = np.bincount(ref.pixel, weights=w[ref.particle].astype(np.float64),
                          minlength=want.size).reshape(want.shape)
        assert np.array_equal(got, want)


def _sorted_and_unique(ref, size):
    key = ref.pixel * (1 << 31) + ref.particle
    assert (np.diff(key) > 0).all()
    assert ref.pixel.size == 0 or (0 <= ref.pixel.min() and ref.pixel.max() < size[0] * size[1])


@pytest.mark.parametrize("window", [None, "box"])
def test_reference_square(oracle, window):
    c = pc.mixed_case(oracle, window)
    ref = pc.reference(("mixed", window, c["size"], c["chunk"]), c)
    _sorted_and_unique(ref, c["size"])
    counts = _counts_match(oracle, c, ref)
    _lists_match(oracle, c, ref, counts, 1)
    # r2 is the pixel's own expression (spot check in scalar Python floats)
    nx, ny = c["size"]
    ext = c["ext"]
    psx, psy = (ext[1] - ext[0]) / nx, (ext[3] - ext[2]) / nx
    for k in np.linspace(0, ref.pixel.size - 1, 50).astype(int):
        xi, yi, p = int(ref.pixel[k] // ny), int(ref.pixel[k] % ny), int(ref.particle[k])
        dx = float(c["u"][p]) - (ext[0] + xi * psx)
        dy = float(c["v"][p]) - (ext[2] + yi * psy)
        assert ref.r2[k] == dx * dx + dy * dy


@pytest.mark.parametrize("window", [None, "box"])
@pytest.mark.parametrize("size,chunk", pc.NONSQUARE, ids=lambda s: str(s).replace(" ", ""))
def test_reference_nonsquare(oracle, window, size, chunk):
    if size == (200, 150):
        c, key = pc.edge_case(oracle, window, chunk), ("edge", window, chunk)
    else:
        c, key = pc.mixed_case(oracle, window, size, chunk), ("mixed", window, size, chunk)
    ref = pc.reference(key, c)
    _sorted_and_unique(ref, c["size"])
    counts = _counts_match(oracle, c, ref)
    _lists_match(oracle, c, ref, counts, 2)


@pytest.mark.parametrize("name", pc.SPELLINGS)
def test_reference_mixed_spellings(oracle, name):
    c = pc.spelling_case(oracle, name)
    ref = pc.reference(("spelling", name), c)
    _sorted_and_unique(ref, c["size"])
    _counts_match(oracle, c, ref)
    _checksums_match(oracle, c, ref)
    # the cull bites, and leaves most of the pairs: the same conditions the GPU case asserts
    free = pc.unculled_reference(name, c)
    assert 0.5 * free.pixel.size <= ref.pixel.size <= 0.95 * free.pixel.size, \
        (ref.pixel.size, free.pixel.size)


@pytest.mark.parametrize("window", [None, "box"])
def test_reference_edge_particles(oracle, window):
    c = pc.edge_case(oracle, window, 32)
    ref = pc.reference(("edge", window, 32), c)
    sp = c["special"]
    has = np.zeros(c["h"].size, bool)
    has[ref.particle] = True
    neg = sp["negated"]
    assert (c["h"][neg] < 0).all()
    # negative h: the disc stays, the cull narrows; some of them keep pairs (on 200 x 150 the
    # v cull's other pitch, quirk S2, removes most particles of either sign)
    assert has[neg].sum() >= 10
    for k in ("zero_h", "nan_u", "nan_h", "outside"):
        assert not has[sp[k]], k
    nx, ny = c["size"]
    last = ref.particle[ref.pixel == nx * ny - 1]
    assert sp["last_corner"] in last
    assert ref.r2[(ref.pixel == nx * ny - 1) & (ref.particle == sp["last_corner"])][0] == 0.0


def test_reference_boundary_set(oracle):
    c = pc.boundary_case()
    ref = pc.reference(("boundary",), c)
    counts = _counts_match(oracle, c, ref)
    _lists_match(oracle, c, ref, counts, 3)
    _checksums_match(oracle, c, ref)


# ------------------------------------------------------------------------ the decoder
def _hand_made():
    """A 70 x 130 image: 2 x 3 tiles, partial on both axes.  Pairs of tiles [1, 6)."""
    size, nty = (70, 130), 3
    want = [  # (xi, yi, particle, r2)
        (0, 64, 5, 0.25), (0, 64, 2, 0.5), (3, 127, 9, 1.0),      # tile 1
        (63, 129, 1, 2.0), (10, 128, 1, 3.0),                      # tile 2 (2 columns wide)
        (64, 0, 4, 4.0), (69, 63, 4, 5.0), (69, 63, 0, 6.0),       # tile 3 (6 rows high)
        (69, 129, 7, 7.0),                                         # tile 5: the last pixel
    ]
    t0, t1 = 1, 6
    counts = np.zeros((t1 - t0) * pr.TILE_PIX, np.int64)
    slot = {}
    for xi, yi, p, r2 in want:
        t = (xi // 64) * nty + yi // 64
        q = (t - t0) * pr.TILE_PIX + (xi % 64) * 64 + yi % 64
        counts[q] += 1
        slot.setdefault(q, []).append((p, r2))
    offsets = np.concatenate([[0], np.cumsum(counts)])
    particle = np.array([p for q in sorted(slot) for p, _ in slot[q]], np.int32)
    r2 = np.array([r for q in sorted(slot) for _, r in slot[q]])
    tile_pairs = np.array([99, 3, 2, 3, 0, 1], np.int64)  # tile 0 is not in the range
    rows = sorted((xi * size[1] + yi, p, r) for xi, yi, p, r in want)
    ref = pr.Pairs(np.array([r[0] for r in rows], np.int64), np.array([r[1] for r in rows], np.int32),
                   np.array([r[2] for r in rows]))
    return size, nty, t0, t1, offsets, particle, r2, tile_pairs, ref


def test_decoder_on_a_hand_made_csr():
    size, nty, t0, t1, offsets, particle, r2, tile_pairs, ref = _hand_made()
    got = pr.decode_emit(offsets, particle, r2, t0, t1, nty, size, tile_pairs)
    assert np.array_equal(got.pixel, ref.pixel) and np.array_equal(got.particle, ref.particle)
    # tile 2 keeps 2 of its 64 columns, tile 3 keeps 6 of its 64 rows, tile 5 keeps 6 x 2
    assert got.outside.size == 64 * 62 + 58 * 64 + 58 * 64 + (4096 - 12)
    pr.assert_pairs_equal(got, ref)
    # the reference may hold pairs of tiles outside the range: they are not compared
    more = pr.Pairs(np.concatenate([[5], ref.pixel]), np.concatenate([[3], ref.particle]).astype(np.int32),
                    np.concatenate([[0.1], ref.r2]))
    pr.assert_pairs_equal(got, more)


def _fails(match, *args):
    with pytest.raises(AssertionError, match=match):
        pr.assert_pairs_equal(*args)


def test_assertions_reject_every_kind_of_error():
    size, nty, t0, t1, offsets, particle, r2, tile_pairs, ref = _hand_made()
    dec = lambda o=offsets, p=particle, r=r2, tp=tile_pairs: pr.decode_emit(  # noqa: E731
        o, p, r, t0, t1, nty, size, tp)
    # a pair moved into a slot outside the image (tile 2, column 2 = image column 130)
    q_out = (2 - t0) * pr.TILE_PIX + 10 * 64 + 2
    q_in = (2 - t0) * pr.TILE_PIX + 10 * 64 + 0
    o = offsets.copy()
    o[q_in + 1:q_out + 1] -= 1
    _fails("outside the image", dec(o=o), ref)
    # a pair in the neighbouring pixel of the same tile
    o = offsets.copy()
    q = (1 - t0) * pr.TILE_PIX + 3 * 64 + 63
    o[q] += 1  # (3, 127) -> (3, 126)
    _fails("pair lists differ.*xi=3, yi=126", dec(o=o), ref)
    # a wrong particle with the right r2; a duplicate that cancels a dropped pair
    p = particle.copy()
    p[2] ^= 1
    _fails("pair lists differ", dec(p=p), ref)
    p = particle.copy()
    p[1] = p[0]
    _fails("pair lists differ", dec(p=p), ref)
    # one bit of r2
    r = r2.copy()
    r[4] = np.nextafter(r[4], 9.0)
    _fails("r2 differs in its bits for 1 of 9", dec(r=r), ref)
    # tile totals, offsets
    tp = tile_pairs.copy()
    tp[2], tp[3] = 3, 2
    _fails("tile_pairs differ", dec(tp=tp), ref)
    tp = tile_pairs.copy()
    tp[5] = 2
    _fails("offsets end at 9", dec(tp=tp), ref)
    o = offsets.copy()
    o[100] = o[-1] + 1
    _fails("offsets decrease", dec(o=o), ref)
    o = offsets + 1
    _fails(r"offsets\[0\]", dec(o=o), ref)
    # a pair the device lost
    _fails("pair lists differ", dec(tp=None), pr.Pairs(np.concatenate([ref.pixel, [70 * 130 - 1]]),
                                                 np.concatenate([ref.particle, [8]]).astype(np.int32),
                                                 np.concatenate([ref.r2, [1.5]])))
