"""The 2-D map's bin layout, restated in NumPy ("Layout reuse").

A pass that reuses the previous map's layout is accepted exactly when every
(scatter workgroup, histogram column) count and the wide count are what a count pass over
the arrays' present contents would find.  This module states those counts for a SQUARE
image at the origin of its window with fp32 inputs (``CULL = false``: no chunk clipping),
so that the tests can PREDICT the verdict of a rewrite before the GPU gives it:

* ``boxes``          ``footprint()`` of ``csrc/asp_device.hpp``, one axis at a time, in
                     ``np.float32`` arithmetic in the order the device code is written;
* ``columns``        the insertions of ``k_count`` / ``k_scatter`` (``csrc/asp_map_bin.hip``:
                     ``column``, ``maybe_large``; ``csrc/asp_map_device.hpp``: ``tile_box``,
                     ``box_large``) and the wide test;
* ``scatter_group``  which scatter workgroup bins particle p;
* ``layout_counts``  the dense table [scatter workgroup, column] and the wide count;
* ``verdict``        1 (accepted) iff two such layouts are equal, else 2 (rejected).

The device compiler may contract a product and a sum of ``footprint`` into one fma, so a
bound can differ from this restatement by an ulp of a pixel coordinate (3e-5 px at 256).
The particle set below keeps every box edge at least 0.05 px from the pixel lattice, and
the footprint's own margin is below 7e-4 px there, so the boxes are the same either way:
``slack_set`` puts every particle on a SLACK LATTICE,

    u = x_min + (i + f) pitch,  f in [0.40, 0.60]        (v likewise)
    2h = (k + g) pitch,         g in [0.15, 0.25]

so (w -+ 2h) / pitch has a fractional part in [0.15, 0.45] or [0.55, 0.85].

``MUTATIONS`` is the catalogue of in-place rewrites the suite pins, each with the verdict
this module predicts for it; ``tests/test_layout_ref.py`` checks the predictions against
``layout_counts`` and ``tests/test_gpu_layout_reuse.py`` against the GPU.
"""
import numpy as np

F = np.float32

K_TILE = 64          # csrc/asp_device.hpp: kTile
K_BATCH = 1024       # csrc/asp_map.hpp: kBatch = kCountBlock (256) * kCountUnroll (4)
K_PER_BLOCK = 8192   # csrc/asp_project2d.hip: nblk = min(bin_blocks, max(1, ceil(n / 8192)))

G = 256
EXT = (-4.0, 4.0, -4.0, 4.0)
N = 50_000

# The knobs the layout depends on, all read per call and held in the layout key.  The
# gather thresholds are chosen so that the three box classes below land on both sides of
# them: 8 x 8 boxes (mid) are not large, 24 x 24 boxes are, their slivers at tile edges
# are not.
KNOBS = dict(wide_tiles=4, gather_min=10, gather_area=100, bin_blocks=7, group=4)
ENV = {"ASP_WIDE_TILES": "4", "ASP_GATHER_MIN": "10", "ASP_GATHER_AREA": "100",
       "ASP_BIN_BLOCKS": "7", "ASP_SCATTER_GROUP": "4"}

STAT_KEYS = ("records", "items", "wide", "merges", "slabs", "large", "records_per_item")


# ----------------------------------------------------------------------------------
# the layout's definition
# ----------------------------------------------------------------------------------
def _axis(w, hd, w_min, pitch, lo, hi):
    """One axis of ``footprint``: the clipped float bounds (fx0, fx1), fp32 throughout."""
    wminf = F(w_min)
    ips = F(1.0 / pitch)
    c = (w - wminf) * ips
    r = hd * ips
    d = (np.abs(w) + np.abs(wminf) + hd) * ips * F(2.0 ** -20) + F(2.0 ** -12)
    f0 = np.maximum(np.ceil(c - r - d), F(lo))
    f1 = np.minimum(np.floor(c + r + d), F(hi))
    return f0, f1


def boxes(u, v, h, size=G, ext=EXT, rows=None):
    """Candidate boxes: ``(ok, x0, x1, y0, y1)``, inclusive pixel ranges, x relative to the
    window's first row (``rows = (row_lo, row_hi)``, default the whole image); ``ok`` False
    where ``footprint`` returns false (the bounds are 0 there)."""
    u, v, h = (np.asarray(a, dtype=F) for a in (u, v, h))
    x_min, x_max, y_min, y_max = ext
    psx = (x_max - x_min) / size
    psy = (y_max - y_min) / size  # the reference's pitch of y is over nx as well (square: the same)
    ox, r1 = (0, size) if rows is None else rows
    with np.errstate(invalid="ignore", over="ignore"):
        hd = np.abs(F(2.0) * h)
        ok = (hd > 0) & np.isfinite(hd) & np.isfinite(u) & np.isfinite(v)
        fx0, fx1 = _axis(u, hd, x_min, psx, ox, r1 - 1)
        fy0, fy1 = _axis(v, hd, y_min, psy, 0, size - 1)
        ok &= (fx0 <= fx1) & (fy0 <= fy1)
        x0, x1, y0, y1 = (np.where(ok, f, 0).astype(np.int64) for f in (fx0, fx1, fy0, fy1))
    return ok, np.where(ok, x0 - ox, 0), np.where(ok, x1 - ox, 0), y0, y1


def _large(bw, bh, gather_min, gather_area):
    return ((bw >= gather_min) & (bh >= gather_min)) | (bw * bh >= gather_area)


def columns(box, nty, ntiles, wide_tiles, gather_min, gather_area):
    """The insertions of the count pass: ``(wide, pidx, col)`` -- ``wide[p]`` True for a
    particle over more than ``wide_tiles`` tiles (no insertion), else one insertion
    ``(pidx[k], col[k])`` per tile (tx, ty) its box meets, ``col = tx nty + ty``, plus
    ``ntiles`` when the unclipped box (``maybe_large``) and the box clipped to the tile
    (``box_large``) are both large."""
    ok, x0, x1, y0, y1 = box
    tx0, tx1, ty0, ty1 = x0 // K_TILE, x1 // K_TILE, y0 // K_TILE, y1 // K_TILE
    wide = ok & ((tx1 - tx0 + 1) * (ty1 - ty0 + 1) > wide_tiles)
    reg = ok & ~wide
    maybe = _large(x1 - x0 + 1, y1 - y0 + 1, gather_min, gather_area)
    pidx, col = [], []
    if reg.any():
        for dx in range(int((tx1 - tx0)[reg].max()) + 1):
            for dy in range(int((ty1 - ty0)[reg].max()) + 1):
                tx, ty = tx0 + dx, ty0 + dy
                m = reg & (tx <= tx1) & (ty <= ty1)
                X0, Y0 = tx * K_TILE, ty * K_TILE
                bw = np.minimum(x1, X0 + K_TILE - 1) - np.maximum(x0, X0) + 1
                bh = np.minimum(y1, Y0 + K_TILE - 1) - np.maximum(y0, Y0) + 1
                lg = maybe & _large(bw, bh, gather_min, gather_area)
                c = tx * nty + ty + np.where(lg, ntiles, 0)
                pidx.append(np.nonzero(m)[0])
                col.append(c[m])
    cat = lambda a: np.concatenate(a) if a else np.zeros(0, np.int64)  # noqa: E731
    return wide, cat(pidx), cat(col)


def scatter_group(p, n, bin_blocks, group):
    """The scatter workgroup of particle p: batches of ``K_BATCH`` particles are dealt to
    the ``nblk`` count workgroups round-robin, and a scatter workgroup takes over ``group``
    consecutive count workgroups."""
    nblk = min(bin_blocks, max(1, -(-n // K_PER_BLOCK)))
    return ((np.asarray(p) // K_BATCH) % nblk) // group


def layout_counts(u, v, h, size=G, ext=EXT, rows=None, knobs=KNOBS):
    """``(table, n_wide)``: ``table[scatter workgroup, column]`` insertions (2 ntiles
    columns: small / mid-size stream, then the large one) and the number of wide particles."""
    n = len(u)
    ox, r1 = (0, size) if rows is None else rows
    nty = -(-size // K_TILE)
    ntiles = -(-(r1 - ox) // K_TILE) * nty
    wide, pidx, col = columns(boxes(u, v, h, size, ext, rows), nty, ntiles, knobs["wide_tiles"],
                              knobs["gather_min"], knobs["gather_area"])
    grp = scatter_group(np.arange(n), n, knobs["bin_blocks"], knobs["group"])
    table = np.zeros((int(grp.max()) + 1, 2 * ntiles), np.int64)
    np.add.at(table, (grp[pidx], col), 1)
    return table, int(wide.sum())


def verdict(before, after):
    """1 (the cached layout is the present contents' layout) or 2."""
    return 1 if np.array_equal(before[0], after[0]) and before[1] == after[1] else 2


def slack(u, v, h, size=G, ext=EXT):
    """The smallest distance, in pixels, of any box edge (w -+ 2|h|) / pitch from the pixel
    lattice, over the particles with finite values (fp64 from the fp32 values)."""
    u, v, h = (np.asarray(a, dtype=np.float64) for a in (u, v, h))
    best = np.inf
    for w, w_min, w_max in ((u, ext[0], ext[1]), (v, ext[2], ext[3])):
        pitch = (w_max - w_min) / size
        for e in ((w - w_min - 2.0 * np.abs(h)) / pitch, (w - w_min + 2.0 * np.abs(h)) / pitch):
            e = e[np.isfinite(e)]
            best = min(best, float(np.min(np.abs(e - np.round(e)))))
    return best


# ----------------------------------------------------------------------------------
# the particle set
# ----------------------------------------------------------------------------------
SMALL, MID, LARGE, WIDE, CLUMP, OUTSIDE = range(6)
CLASS_K = {SMALL: 1, MID: 4, LARGE: 12, WIDE: 150, CLUMP: 1, OUTSIDE: 1}
N_WIDE, N_OUTSIDE, N_CLUMP, N_LARGE, N_MID = 40, 20, 6000, 3000, 8000
CLUMP_TILE = (2, 1)      # (tx, ty); the clump keeps 2 px from the tile's edges
HEAD = 2000              # the first HEAD particles are neither wide nor outside (many_wide)
OUT_PIXEL = 11 * G       # first pixel index of x_max + 10 (x_max - x_min)


class Set:
    """fp32 arrays u, v, h, a0, a1 and the class code of every particle."""

    def __init__(self, u, v, h, a0, a1, cls):
        self.u, self.v, self.h, self.a0, self.a1, self.cls = u, v, h, a0, a1, cls

    def uvh(self):
        return self.u.copy(), self.v.copy(), self.h.copy()


def _pitch(ext=EXT, size=G):
    return (ext[1] - ext[0]) / size


def on_lattice(i, f):
    """fp32 coordinate of lattice position i + f (pixels from the image's corner)."""
    return (EXT[0] + (np.asarray(i) + f) * _pitch()).astype(F)


def h_of(k, g):
    """fp32 h with 2h = (k + g) pitches."""
    return (0.5 * (np.asarray(k) + g) * _pitch()).astype(F)


def pixel_of(w):
    """(i, f) of an fp32 coordinate."""
    e = (np.asarray(w, dtype=np.float64) - EXT[0]) / _pitch()
    i = np.floor(e)
    return i.astype(np.int64), e - i


_sets = {}


def slack_set(seed=1):
    """N particles on the slack lattice (built once per seed; do not write to the arrays)."""
    if seed in _sets:
        return _sets[seed]
    rng = np.random.default_rng(seed)
    cls = np.full(N, SMALL, np.int8)
    rest = rng.permutation(np.arange(HEAD, N))
    cls[rest[:N_WIDE]] = WIDE
    cls[rest[N_WIDE:N_WIDE + N_OUTSIDE]] = OUTSIDE
    body = rng.permutation(np.concatenate((np.arange(HEAD), rest[N_WIDE + N_OUTSIDE:])))
    cls[body[:N_CLUMP]] = CLUMP
    cls[body[N_CLUMP:N_CLUMP + N_LARGE]] = LARGE
    cls[body[N_CLUMP + N_LARGE:N_CLUMP + N_LARGE + N_MID]] = MID
    i = rng.integers(0, G, N)
    j = rng.integers(0, G, N)
    c = cls == CLUMP
    i[c] = CLUMP_TILE[0] * K_TILE + rng.integers(2, K_TILE - 3, int(c.sum()))
    j[c] = CLUMP_TILE[1] * K_TILE + rng.integers(2, K_TILE - 3, int(c.sum()))
    i[cls == OUTSIDE] += OUT_PIXEL
    k = np.array([CLASS_K[int(q)] for q in cls])
    u = on_lattice(i, rng.uniform(0.40, 0.60, N))
    v = on_lattice(j, rng.uniform(0.40, 0.60, N))
    h = h_of(k, rng.uniform(0.15, 0.25, N))
    p = np.arange(N)
    a0 = (1.0 + p / N).astype(F)      # positive (the ulp bars) and distinct per particle
    a1 = (1.5 - 0.25 * p / N).astype(F)
    s = Set(u, v, h, a0, a1, cls)
    for a in (u, v, h, a0, a1, cls):
        a.setflags(write=False)
    _sets[seed] = s
    return s


def single_tile(s, classes=(SMALL,), margin=0, rows=None):
    """Indices of the particles of ``classes`` whose box lies in ONE tile, at least
    ``margin`` pixels from its edges (and, with ``rows``, inside that window)."""
    ok, x0, x1, y0, y1 = boxes(s.u, s.v, s.h)
    m = ok & np.isin(s.cls, classes)
    m &= (x0 % K_TILE >= margin) & (y0 % K_TILE >= margin)
    m &= (x0 // K_TILE == (x1 + margin) // K_TILE) & (y0 // K_TILE == (y1 + margin) // K_TILE)
    if rows is not None:
        m &= (x0 >= rows[0]) & (x1 < rows[1])
    return np.nonzero(m)[0]


def tile_of(s, p):
    ok, x0, x1, y0, y1 = boxes(s.u[p], s.v[p], s.h[p])
    return (x0 // K_TILE) * (G // K_TILE) + y0 // K_TILE


# ----------------------------------------------------------------------------------
# the mutation catalogue: fn(s, u, v, h, rng) edits the copies u, v, h of s's arrays in
# place and returns {"targets": indices it rewrote, "swapped": (a, b) index arrays or None}
# ----------------------------------------------------------------------------------
def _info(targets, swapped=None):
    return {"targets": np.asarray(targets), "swapped": swapped}


def _jitter(s, u, v, h, rng, who):
    px = _pitch()
    u[who] = (u[who].astype(np.float64) + rng.uniform(-0.05, 0.05, len(who)) * px).astype(F)
    v[who] = (v[who].astype(np.float64) + rng.uniform(-0.05, 0.05, len(who)) * px).astype(F)
    return _info(who)


def jitter(s, u, v, h, rng):
    return _jitter(s, u, v, h, rng, np.nonzero(s.cls != OUTSIDE)[0])


def clump_reshuffle(s, u, v, h, rng):
    return _jitter(s, u, v, h, rng, np.nonzero(s.cls == CLUMP)[0])


def breathe(s, u, v, h, rng):
    who = np.nonzero(s.cls != WIDE)[0]
    h[who] = (h[who].astype(np.float64) + 0.5 * rng.uniform(-0.04, 0.04, len(who)) * _pitch()).astype(F)
    return _info(who)


def _exchange(arrs, a, b):
    for w in arrs:
        w[a], w[b] = w[b].copy(), w[a].copy()


def swap_in_batch(s, u, v, h, rng):
    """500 pairs (2j, 2j + 1) -- always one batch -- exchange (u, v, h); the amplitudes stay."""
    cand = np.arange(0, N, 2)
    cand = cand[(s.cls[cand] != s.cls[cand + 1]) | (s.cls[cand] == LARGE)]
    a = np.sort(rng.choice(cand, 500, replace=False))
    _exchange((u, v, h), a, a + 1)
    return _info(np.concatenate((a, a + 1)), (a, a + 1))


def _pair(s, classes, same_group, margin=0):
    """Two particles of ``classes`` in one tile each, in different tiles, of the same or of
    different scatter workgroups: the first of them, and of its partners at least N / 4
    indices further on the one whose h differs most from its own."""
    c = single_tile(s, classes, margin)
    g = scatter_group(c, N, KNOBS["bin_blocks"], KNOBS["group"])
    t = tile_of(s, c)
    a = c[0]
    m = ((g == g[0]) == same_group) & (t != t[0]) & (c > a + N // 4)
    return a, c[m][np.argmax(np.abs(s.h[c[m]] - s.h[a]))]


def swap_positions_same_h(s, u, v, h, rng):
    """Two LARGE particles (boxes inside their tiles) of one scatter workgroup and different
    tiles exchange (u, v): each keeps its h, so the discs change as well as the owners."""
    a, b = _pair(s, (LARGE,), True, margin=1)
    _exchange((u, v), [a], [b])
    return _info([a, b], (np.array([a]), np.array([b])))


def wide_walks(s, u, v, h, rng):
    who = np.nonzero(s.cls == WIDE)[0]
    i, f = pixel_of(u[who])
    step = rng.integers(30, 61, len(who))
    i = np.where(i + step < G, i + step, i - step)
    u[who] = on_lattice(i, f)
    return _info(who)


def wide_in_wide_out(s, u, v, h, rng):
    w = np.nonzero(s.cls == WIDE)[0][0]
    o = np.nonzero(s.cls == OUTSIDE)[0]
    o = o[np.argmax(np.abs(o - w))]   # far apart: amplitudes 1 + p / N that differ visibly
    _exchange((u, v, h), [w], [o])
    return _info([w, o], (np.array([w]), np.array([o])))


def pick_one_tile_over(s, rows=None):
    """A SMALL particle in one tile that is still inside (the window) 64 px further in u."""
    c = single_tile(s, (SMALL,), rows=rows)
    i, _ = pixel_of(s.u[c])
    return c[i + K_TILE + 2 < (G if rows is None else rows[1])][0]


def move_one_tile(u, p):
    i, f = pixel_of(u[p])
    u[p] = on_lattice(i + K_TILE, f)


def one_tile_over(s, u, v, h, rng):
    p = pick_one_tile_over(s)
    move_one_tile(u, p)
    return _info([p])


def across_groups(s, u, v, h, rng):
    a, b = _pair(s, (SMALL,), False)
    _exchange((u, v, h), [a], [b])
    return _info([a, b], (np.array([a]), np.array([b])))


def small_to_large(s, u, v, h, rng):
    p = single_tile(s, (SMALL,), margin=13)[0]
    h[p] = h_of(CLASS_K[LARGE], 0.2)
    return _info([p])


def outside_to_wide(s, u, v, h, rng):
    p = np.nonzero(s.cls == OUTSIDE)[0][0]
    u[p] = on_lattice(100, 0.5)
    h[p] = h_of(CLASS_K[WIDE], 0.2)
    return _info([p])


def wide_to_outside(s, u, v, h, rng):
    p = np.nonzero(s.cls == WIDE)[0][0]
    i, f = pixel_of(u[p])
    u[p] = on_lattice(i + OUT_PIXEL, f)
    return _info([p])


def drops_out(s, u, v, h, rng):
    p = single_tile(s, (SMALL,))[0]
    u[p] = np.nan
    return _info([p])


def drops_out_h0(s, u, v, h, rng):
    p = single_tile(s, (SMALL,))[0]
    h[p] = 0.0
    return _info([p])


def many_wide(s, u, v, h, rng):
    who = np.arange(HEAD)
    h[who] = h_of(CLASS_K[WIDE], rng.uniform(0.15, 0.25, HEAD))
    return _info(who)


MUTATIONS = (
    ("jitter", jitter, 1),
    ("breathe", breathe, 1),
    ("swap_in_batch", swap_in_batch, 1),
    ("swap_positions_same_h", swap_positions_same_h, 1),
    ("wide_walks", wide_walks, 1),
    ("wide_in_wide_out", wide_in_wide_out, 1),
    ("clump_reshuffle", clump_reshuffle, 1),
    ("one_tile_over", one_tile_over, 2),
    ("across_groups", across_groups, 2),
    ("small_to_large", small_to_large, 2),
    ("outside_to_wide", outside_to_wide, 2),
    ("wide_to_outside", wide_to_outside, 2),
    ("drops_out", drops_out, 2),
    ("drops_out_h0", drops_out_h0, 2),
    ("many_wide", many_wide, 2),
)
ACCEPTED = tuple(name for name, _, want in MUTATIONS if want == 1)
REJECTED = tuple(name for name, _, want in MUTATIONS if want == 2)
# Rewrites under which a map of unit amplitudes (the indicator counts) cannot change: the
# first two leave the multiset of (u, v, h) inside the image as it was; the clump's discs
# (radius 1.15 .. 1.25 px about a point 0.35 .. 0.65 px from its pixel's corners) hold the
# four corners of their 2 x 2 box (at most 0.92 px away) and no other (1.35 px or more)
# wherever the jitter puts them.
UNIT_MAP_UNCHANGED = ("swap_in_batch", "wide_in_wide_out", "clump_reshuffle")

_applied = {}


def mutated(name, seed=1, base=None):
    """``(u, v, h, info)`` of mutation ``name`` applied to copies of ``slack_set(seed)``'s
    arrays (or of ``base = (u, v, h)``, still described by that set's classes).  Results on
    the set itself are cached: do not write to them."""
    s = slack_set(seed)
    fn = {n: f for n, f, _ in MUTATIONS}[name]
    rng = np.random.default_rng([seed, [n for n, _, _ in MUTATIONS].index(name)])
    if base is not None:
        u, v, h = (np.array(a, dtype=F) for a in base)
        return (u, v, h, fn(s, u, v, h, rng))
    if (name, seed) not in _applied:
        u, v, h = s.uvh()
        info = fn(s, u, v, h, rng)
        for a in (u, v, h):
            a.setflags(write=False)
        _applied[name, seed] = (u, v, h, info)
    return _applied[name, seed]


# ----------------------------------------------------------------------------------
# the sweep: single-particle moves with both verdicts
# ----------------------------------------------------------------------------------
SWEEP_SEED = 3
SWEEP_MOVES = 24


def sweep(seed=SWEEP_SEED, moves=SWEEP_MOVES):
    """``moves`` single-particle moves applied one after another to ``slack_set()``: a list
    of ``(p, u, v, h, verdict)`` -- particle p takes the fp32 values (u, v, h); ``verdict``
    is ``layout_counts`` before against after that move.  The new position is on the slack
    lattice, 13 px or more inside a tile drawn at random -- half of the time the
    particle's own, so that both verdicts occur -- and the new class is the old one half
    of the time, else drawn from small / mid / large."""
    s = slack_set()
    rng = np.random.default_rng(seed)
    u, v, h = s.uvh()
    k_now = np.array([CLASS_K[int(q)] for q in s.cls])
    pool = np.nonzero(np.isin(s.cls, (SMALL, MID, LARGE)))[0]
    nt = G // K_TILE
    out = []
    before = layout_counts(u, v, h)
    for p in rng.choice(pool, moves, replace=False):
        (i, j), _ = pixel_of(np.array([u[p], v[p]]))
        tx, ty = (int(i) // K_TILE, int(j) // K_TILE) if rng.random() < 0.5 else rng.integers(0, nt, 2)
        k = k_now[p] if rng.random() < 0.5 else rng.choice([1, 4, 12])
        i, j = (int(t) * K_TILE + int(rng.integers(13, K_TILE - 13)) for t in (tx, ty))
        u[p] = on_lattice(i, rng.uniform(0.40, 0.60))
        v[p] = on_lattice(j, rng.uniform(0.40, 0.60))
        h[p] = h_of(k, rng.uniform(0.15, 0.25))
        k_now[p] = k
        after = layout_counts(u, v, h)
        out.append((int(p), u[p], v[p], h[p], verdict(before, after)))
        before = after
    return out
