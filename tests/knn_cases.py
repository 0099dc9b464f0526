"""Seeded inputs for the k-NN search (csrc/asp_knn.hip), each built so that one path of the
search runs at the smallest size at which it can, and the one reference of every k-NN test:
``scipy.spatial.KDTree(pos).query(pos, k)[0][:, k - 1]``, the reference reader's own call.

The bar is bit-exact fp64 everywhere (``same_bits``); no tolerance.  ``want(name, k)`` caches
the reference of a named case, read-only, so the tests that share a case share one tree query.
tests/test_knn_cases.py holds every case to a brute-force restatement of the device's
arithmetic and states each case's defining property on the input alone;
tests/test_gpu_knn_paths.py runs them on the device.
"""
import functools

import numpy as np
from scipy.spatial import KDTree

# Ragged sizes and table edges: a last wave of one lane (65, 129, 257, 321, 513, 577, 4097), a
# last block of one wave (257, 513, 4097), the cell level switch 8^L < n at 64 / 512 / 4096,
# the largest n whose default window is the whole array (320), and the 4097-entry
# suffix-minimum table (n in 513 .. 4096: L = 4), whose second block holds one entry.
RAGGED_N = (63, 64, 65, 127, 128, 129, 255, 256, 257, 320, 321, 511, 512, 513, 576, 577,
            4095, 4096, 4097)
RAGGED_K = (1, 7, 32, 33, 63, 64)
SUB_N, SUB_DENSE, SUB_LEVEL = 3000, 2000, 4       # n = 3000: level-4 cell table, 16 cells an axis
SUB_CELLS = {"first": (0, 0, 0), "middle": (9, 4, 6), "last": (15, 15, 15)}
ISLANDS, ISLAND_PTS, ISLAND_RADIUS = 300, 32, 1e-4  # clump radius over the clumps' spacing
BALL_N, BALL_SCATTER = 66_000, 31
BIG_N = (1 << 21) + 1


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def scipy_h(pos, k):
    """The reference; +inf where fewer than k points exist (scipy's missing neighbour)."""
    d = KDTree(pos).query(pos, k=k)[0]
    return d if k == 1 else d[:, k - 1]


def brute_h(pos, k, rows=512):
    """The device's definition: k-th smallest of ((dx^2 + dy^2) + dz^2), then sqrt."""
    out = np.full(len(pos), np.inf)
    if k > len(pos):
        return out
    with np.errstate(under="ignore", over="ignore"):
        for a in range(0, len(pos), rows):
            d = pos[a:a + rows, None, :] - pos[None, :, :]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            out[a:a + rows] = np.sqrt(np.partition(d2, k - 1, axis=1)[:, k - 1])
    return out


def morton_cell(pos, level, lo=None, span=None):
    """Per-axis cell index at ``level`` of the search's grid: the bounding cube of edge
    span (1 + 2^-20) from the per-axis minima (asp_knn.hip k_bbox_final, quant)."""
    lo = pos.min(axis=0) if lo is None else lo
    span = (pos.max(axis=0) - pos.min(axis=0)).max() if span is None else span
    q = np.floor((pos - lo) * ((1 << 21) / (span * (1.0 + 2.0 ** -20)))).astype(np.int64)
    return np.clip(q, 0, (1 << 21) - 1) >> (21 - level)


def uniform(n):
    return np.random.default_rng(1000 + n).uniform(0.0, 25.0, (n, 3))


def lattice(m):  # spacing 0.5: every distance exact, ties everywhere
    g = np.arange(float(m)) * 0.5
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def clumps100():
    """12 clumps of 100 identical points (a run of equal keys longer than a wave, so it
    straddles a window's first or last entry) among 300 distinct points, shuffled."""
    rng = np.random.default_rng(21)
    pos = np.concatenate([np.repeat(rng.uniform(0.0, 1.0, (12, 3)), 100, axis=0),
                          rng.uniform(0.0, 1.0, (300, 3))])
    rng.shuffle(pos)
    return pos


def identical(n=1000):
    return np.tile(np.array([[0.3, -1.7, 2.5]]), (n, 1))


def on_axis(n=1000):
    pos = np.zeros((n, 3))
    pos[:, 0] = np.random.default_rng(22).uniform(-4.0, 9.0, n)
    return pos


def subtable(where):
    """n = 3000 in the unit cube (its corners included, so the cube is the grid): 2000 points
    in a ball of 1e-3 of the span at the centre of one level-4 cell -- the first, a middle or
    the last cell in key order (last: the cell's end is tab[ncell] = n)."""
    rng = np.random.default_rng(23)
    c = (np.array(SUB_CELLS[where]) + 0.5) / (1 << SUB_LEVEL)
    v = rng.standard_normal((SUB_DENSE, 3))
    ball = c + 1e-3 * rng.uniform(0.0, 1.0, (SUB_DENSE, 1)) ** (1 / 3) * v / np.linalg.norm(v, axis=1)[:, None]
    pos = np.concatenate([ball, rng.uniform(0.0, 1.0, (SUB_N - SUB_DENSE - 2, 3)),
                          np.zeros((1, 3)), np.ones((1, 3))])
    rng.shuffle(pos)
    return pos


def island_centres():
    return np.random.default_rng(24).uniform(0.0, 1.0, (ISLANDS, 3))


def islands():
    """300 clumps of 32 points, each of radius 1e-4 of the clumps' mean spacing.  A wave's 64
    curve neighbours come from two clumps or more, so at the cell level of its radii (about the
    clump radius) its common box is thousands of cells wide: the shared pass gives up."""
    rng = np.random.default_rng(25)
    r = ISLAND_RADIUS * ISLANDS ** (-1 / 3)
    pos = (island_centres()[:, None, :] + rng.uniform(-r, r, (ISLANDS, ISLAND_PTS, 3)) / np.sqrt(3.0))
    return pos.reshape(-1, 3)


def ball_and_scatter():
    """66 000 points in a ball of 1e-4 just above the centre of the unit cube (the first keys
    of the last octant) and 31 scattered points: the 32nd neighbour of a scattered point lies
    in the ball, and the points of the other octants sort before it, so the first wave's
    shared pass meets more entries than it can address."""
    rng = np.random.default_rng(26)
    v = rng.standard_normal((BALL_N, 3))
    ball = 0.5 + 2e-4 + 1e-4 * rng.uniform(0.0, 1.0, (BALL_N, 1)) ** (1 / 3) * v / np.linalg.norm(v, axis=1)[:, None]
    pos = np.concatenate([ball, rng.uniform(0.0, 1.0, (BALL_SCATTER, 3))])
    rng.shuffle(pos)
    return pos


def tiny_clump():
    """2000 points of unit scale and a clump of 40 of scale 1e-160 at the origin (their
    squared distances are subnormal)."""
    rng = np.random.default_rng(27)
    pos = np.concatenate([rng.uniform(-1.0, 1.0, (2000, 3)), rng.standard_normal((40, 3)) * 1e-160])
    rng.shuffle(pos)
    return pos


def clustered_big():
    """2^21 + 1 Plummer particles: the first n with a level-8 cell table, 8^8 + 1 entries =
    4097 suffix-minimum blocks, so k_sfx_top's carry loop runs (five chunks of 1024)."""
    from asp_amd.plummer import plummer
    return plummer(BIG_N, seed=9, h_law="pixel", grid=64)["pos"]


# The uniform set the scale cases multiply.  d2 ~ 1e300 (finite), ~1e-300, 0 or subnormal
# (1e-170: the fp32 prefilter's fp64 branch, T.mx < 2^-100), and -- 1e-22 -- d2 ~ 1e-43: a
# radius whose square is subnormal in fp32, where the prefilter's bound rounds coarsely.
SCALE_N = 4096
SCALES = (1e150, 1e-150, 1e-170, 1e-22)

CASES = {
    **{f"uniform{n}": functools.partial(uniform, n) for n in RAGGED_N},
    "lattice6": functools.partial(lattice, 6),
    "lattice11": functools.partial(lattice, 11),
    "clumps100": clumps100,
    "identical1000": identical,
    "axis1000": on_axis,
    **{f"sub_{w}": functools.partial(subtable, w) for w in SUB_CELLS},
    "islands": islands,
    "ball66000": ball_and_scatter,
    "tiny_clump": tiny_clump,
    **{f"scale{s:g}": (lambda s=s: uniform(SCALE_N) * s) for s in SCALES},
}


@functools.lru_cache(maxsize=None)
def case(name):
    pos = np.ascontiguousarray(CASES[name](), dtype=np.float64)
    pos.setflags(write=False)
    return pos


@functools.lru_cache(maxsize=None)
def want(name, k):
    pos = case(name)
    h = scipy_h(pos, k) if k <= len(pos) else np.full(len(pos), np.inf)
    h.setflags(write=False)
    return h


def _with_rows(n, rows, fill, seed):
    """uniform(n) with ``rows`` seeded rows overwritten by ``fill(rng, rows)`` ((rows, 3))."""
    rng = np.random.default_rng(seed)
    pos = uniform(n).copy()
    at = rng.choice(n, rows, replace=False)
    pos[at] = fill(rng, pos[at])
    return pos


def _one_coordinate(value):
    def fill(rng, rows):
        rows[np.arange(len(rows)), rng.integers(0, 3, len(rows))] = value
        return rows
    return fill


def two_clumps(m):
    """Two clumps of m points 1e160 apart: the squared distance between them overflows."""
    rng = np.random.default_rng(40 + m)
    pos = rng.uniform(0.0, 1.0, (2 * m, 3))
    pos[m:, 0] += 1e160
    rng.shuffle(pos)
    return pos


# Inputs with rows that have no position, or distances that overflow (n <= 600).
NONFINITE = {
    "nan_1": lambda: _with_rows(600, 1, lambda r, x: np.full_like(x, np.nan), 41),
    "nan_10pc": lambda: _with_rows(600, 60, lambda r, x: np.full_like(x, np.nan), 42),
    "nan_50pc": lambda: _with_rows(600, 300, lambda r, x: np.full_like(x, np.nan), 43),
    "nan_one_coordinate": lambda: _with_rows(577, 58, _one_coordinate(np.nan), 44),
    "plus_inf": lambda: _with_rows(577, 30, _one_coordinate(np.inf), 45),
    "minus_inf": lambda: _with_rows(577, 30, _one_coordinate(-np.inf), 46),
    "inf_rows": lambda: _with_rows(321, 40, lambda r, x: r.choice([np.inf, -np.inf], x.shape), 47),
    "few_finite": lambda: _with_rows(100, 80, _one_coordinate(np.nan), 48),  # 20 finite rows
    "overflow_all": lambda: uniform(600) * 1e200,
    "clumps_20": lambda: two_clumps(20),
    "clumps_40": lambda: two_clumps(40),
}


def finite_rows(pos):
    return np.isfinite(pos).all(axis=1)


def want_nonfinite(pos, k):
    """The contract for non-finite rows (include/asp.h): a row with a non-finite coordinate is
    nobody's neighbour and gets +inf; every other row its k-th smallest finite d2 among the
    finite rows, +inf if there are fewer than k.  scipy refuses such arrays, so this is
    scipy_h on the finite subset."""
    f = finite_rows(pos)
    out = np.full(len(pos), np.inf)
    if k <= f.sum():
        with np.errstate(over="ignore"):
            out[f] = scipy_h(np.ascontiguousarray(pos[f]), k)
    return out
