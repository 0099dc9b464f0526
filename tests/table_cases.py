"""Inputs and the one reference of the ionisation-table tests (no GPU needed here).

The reference is scipy's own ``RegularGridInterpolator`` (linear, ``bounds_error=False``,
``fill_value=-inf``) -- the interpolator ``IonisationTableBase`` wraps
(data_structures/_IonisationTable.py:44-58) -- given the table object itself, so that scipy
picks its own 2-D arithmetic order from the dtype, flags and byte order.  Every input is
seeded and generated; the case lists below are imported by the CPU tests
(test_table_cases.py: the restatement equals scipy, every case meets the share condition)
and by the GPU tests (test_gpu_table_forms.py).

The shapes stand on the dispatch edges of csrc/asp_table.hip (kTabLdsAxis = 2048 axis nodes
in LDS, kSlabMax = 16384 slab doubles); test_table_cases.py reads the constants from the
source, so a retuned constant fails there instead of moving the shapes off the edges.
"""
import functools
import zlib

import numpy as np

N_POINTS = 20_000

# the share condition on the reference's output, so that no case hides in fills
MIN_FINITE, MIN_FILL, MIN_NAN = 0.50, 0.01, 0.005


def reference(table, grids, points, zaxis=None, z=None):
    """scipy on ``points`` ((N, ndim)); with ``zaxis`` the constant ``z`` is inserted as
    that column first, as IonisationTableBase.evaluate_at_redshift does (:54-58)."""
    from scipy.interpolate import RegularGridInterpolator
    rgi = RegularGridInterpolator(tuple(grids), table, bounds_error=False, fill_value=-np.inf)
    P = np.asarray(points, dtype=float)
    if zaxis is not None:
        full = np.empty((P.shape[0], P.shape[1] + 1), dtype=float)
        full[:, np.arange(len(grids)) != zaxis] = P
        full[:, zaxis] = z
        P = full
    with np.errstate(all="ignore"):
        return rgi(P)


def axis(kind, n, rng):
    """A strictly ascending axis of n >= 2 nodes."""
    assert n >= 2
    if kind == "uniform":
        g = np.linspace(-3.0, 4.0, n)
    elif kind == "jitter":
        g = np.cumsum(rng.uniform(0.05, 0.2, n)) - 3.0
    elif kind == "log":
        g = np.logspace(-8, 6, n)
    elif kind == "log600":
        g = np.logspace(-300, 300, n)
    elif kind == "neglog600":  # the same, mirrored: ascending negative nodes
        g = -np.logspace(-300, 300, n)[::-1].copy()
    elif kind == "cluster":  # n - 2 nodes inside 1e-6, one far node on each side
        inner = 0.25 + np.sort(rng.uniform(0.0, 1e-6, n - 2))
        g = np.concatenate([[-0.75], inner, [1.25]])
    elif kind == "far":
        g = 1e9 + np.cumsum(rng.uniform(1e-4, 2e-4, n))
    elif kind == "subnormal":
        assert n == 4
        g = np.array([0.0, 5e-324, 1e-323, 1.0])
    else:
        raise ValueError(kind)
    g = np.ascontiguousarray(g, dtype=np.float64)
    assert g.size == n and np.all(np.diff(g) > 0), (kind, n)
    return g


def points(grids, n, rng, margin=0.01):
    """(n, len(grids)) query rows: uniform over each axis span widened by margin * span on
    both sides; per column about every 7th row exactly on a random node, about every 100th
    one ulp above and every 100th one ulp below a random node (first and last included, so
    some are one ulp outside); one column NaN on every 97th row; a handful of +-inf."""
    D = len(grids)
    P = np.empty((n, D))
    for c, g in enumerate(grids):
        span = g[-1] - g[0]
        x = rng.uniform(g[0] - margin * span, g[-1] + margin * span, n)
        u = rng.random(n)
        node = g[rng.integers(0, g.size, n)]
        x = np.where(u < 1 / 7, node, x)
        x = np.where((u >= 0.50) & (u < 0.51), np.nextafter(node, np.inf), x)
        x = np.where((u >= 0.60) & (u < 0.61), np.nextafter(node, -np.inf), x)
        P[:, c] = x
    if D:
        P[::97, int(rng.integers(0, D))] = np.nan
        for k, v in enumerate((np.inf, -np.inf) * 3):
            if n > 50:
                P[int(rng.integers(0, n)), (k // 2) % D] = v
    P.flags.writeable = False
    return P


def shares(want):
    """(finite, fill, NaN) fractions of a reference output."""
    want = np.asarray(want)
    return (float(np.isfinite(want).mean()), float((want == -np.inf).mean()),
            float(np.isnan(want).mean()))


def check_shares(want, what=""):
    fin, fill, nan = shares(want)
    assert fin >= MIN_FINITE and fill >= MIN_FILL and nan >= MIN_NAN, \
        f"{what}: finite {fin:.3f} fill {fill:.3f} NaN {nan:.4f} misses the share condition"


def assert_same(got, want, what=""):
    """NaN masks equal, -inf masks equal, every other element equal as uint64 bits
    (-0.0 != +0.0).  NaN sign and payload are not compared: inf * 0 gives a differently
    signed NaN on x86 and on the GPU."""
    got = np.ascontiguousarray(np.asarray(got, dtype=np.float64))
    want = np.ascontiguousarray(np.asarray(want, dtype=np.float64))
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), \
        f"{what}: NaN masks differ at rows {np.flatnonzero(gn != wn)[:8]}"
    gf, wf = got == -np.inf, want == -np.inf
    assert np.array_equal(gf, wf), \
        f"{what}: -inf masks differ at rows {np.flatnonzero(gf != wf)[:8]}"
    rest = ~(wn | wf)
    bad = got[rest].view(np.uint64) != want[rest].view(np.uint64)
    if bad.any():
        rows = np.flatnonzero(rest)[bad][:8]
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.size} elements differ in bits, "
                             f"first rows {rows}: got {got[rows]} want {want[rows]}")


def redshifts(g):
    """The fixed-axis values every at-redshift form runs: (label, z, inside the axis)."""
    k = g.size // 2 if g.size > 2 else 1  # an interior node (the last of a 2-node axis)
    return [("first", g[0], True), ("node", g[k], True),
            ("node-ulp", np.nextafter(g[k], -np.inf), True),
            ("mid", g[k - 1] + 0.5 * (g[k] - g[k - 1]), True), ("last", g[-1], True),
            ("last+ulp", np.nextafter(g[-1], np.inf), False),
            ("far", g[-1] + 10.0 * (g[-1] - g[0]), False), ("nan", np.nan, False)]


def poison(table, rng):
    """A copy with 5 % of the entries -inf (log10 of a zero fraction) and 1 % NaN.  The -inf
    entries fill four boxes in the table's own proportions at random places, as zero
    fractions fill regions of a real table (single entries make up the exact count):
    independent single entries would leave 0.94^(2^D) of the cells finite, 37 % at four
    axes, and the share condition asks for half of the rows.  NaN entries are single and
    independent."""
    t = np.array(table, dtype=np.float64)
    want = max(1, round(0.05 * t.size))
    left, sides = want / 4.0, [1] * t.ndim
    order = [int(d) for d in np.argsort(t.shape, kind="stable")]  # the short axes first
    for j, d in enumerate(order):
        frac = (left / np.prod([t.shape[e] for e in order[j:]])) ** (1.0 / (t.ndim - j))
        sides[d] = int(np.clip(np.floor(t.shape[d] * frac), 1, t.shape[d]))
        left /= sides[d]
    for _ in range(4):
        t[tuple(slice(a, a + s) for a, s in
                ((int(rng.integers(0, n - s + 1)), s) for n, s in zip(t.shape, sides)))] = -np.inf
    flat = t.reshape(-1)
    left = want - int(np.isinf(flat).sum())
    assert left >= 0, (t.shape, sides)
    if left > 0:
        flat[rng.choice(np.flatnonzero(np.isfinite(flat)), left, replace=False)] = -np.inf
    flat[rng.choice(np.flatnonzero(np.isfinite(flat)), max(1, round(0.01 * flat.size)),
                    replace=False)] = np.nan
    return t


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ---- (a) kernel form x shape: 3-D tables through IonisationTable ---------------------------
# name -> (shape, axis kinds).  The kernel each reaches, from the dispatcher: n0+n1+n2 <= 2048
# puts the axes in LDS (k_table<*,true>), zaxis 2 with n0*n1*2 <= 16384 and n0+n1 <= 2048
# takes k_table_slab.
FORM_CASES = {
    "2x2x2": ((2, 2, 2), ("uniform", "uniform", "uniform")),
    "sum2048": ((2, 3, 2043), ("jitter", "cluster", "log")),
    "sum2049": ((2, 3, 2044), ("jitter", "cluster", "log")),
    "slab16384": ((64, 128, 5), ("cluster", "log", "uniform")),
    "slab16512": ((64, 129, 5), ("cluster", "log", "uniform")),
    "pair2048": ((4, 2044, 3), ("uniform", "cluster", "log")),
    "pair2049": ((4, 2045, 3), ("uniform", "cluster", "log")),
    "large": ((17, 700, 1400), ("log", "cluster", "far")),
    "extreme": ((40, 25, 4), ("log600", "neglog600", "subnormal")),
}
HM01_SHAPE = (41, 141, 49)  # (b): point counts and tails
POISON_CASES = ("slab16384", "sum2049")  # (c): -inf and NaN table entries
# Few cells carry most of the rows on clustered and logarithmic axes, and a fixed z on a node
# with a -inf entry turns a whole call non-finite, so the finite share of a poisoned case
# swings with the placement: these seeds are ones whose every call form and every z
# inside the table meets the share condition (test_table_cases.py holds them to it).
POISON_SEED = {"slab16384": 6, "sum2049": 6, "4d": 3}
TAIL_COUNTS = (1, 255, 1023, 1024, 1025, 4095, 4096, 4097)


@functools.lru_cache(maxsize=None)
def form_case(name):
    """{table, grids, P (N, 3), P2: {zaxis: (N, 2)}}, values in [-10, 0] (log10 fractions)."""
    rng = _rng("form:" + name)
    if name == "hm01":
        shape, kinds = HM01_SHAPE, ("jitter", "jitter", "jitter")
        n = max(TAIL_COUNTS)
    else:
        shape, kinds = FORM_CASES[name]
        n = N_POINTS
    grids = [axis(k, m, rng) for k, m in zip(kinds, shape)]
    table = rng.uniform(-10.0, 0.0, shape)
    return {"table": table, "grids": grids, "P": points(grids, n, rng),
            "P2": {z: points([g for d, g in enumerate(grids) if d != z], n, rng)
                   for z in range(3)}}


@functools.lru_cache(maxsize=None)
def poison_case(name):
    case = dict(form_case(name))
    case["table"] = poison(case["table"], _rng(f"poison:{name}:{POISON_SEED[name]}"))
    return case


def slab_trip_points(cus):
    """(b): 2 * CUs * 4096 + 4097 points on the HM01-sized table, so that k_table_slab's
    persistent loop (min(need, 2 * CUs) blocks of 4096 points) makes a second, ragged trip."""
    grids = form_case("hm01")["grids"]
    return points(grids[:2], 2 * cus * 4096 + 4097, _rng("slab-trip"))


# ---- (d) N-D: asp_table_interp -------------------------------------------------------------
ND_CASES = ("1-two", "1-cluster", "2", "3", "4", "5", "6")


@functools.lru_cache(maxsize=None)
def nd_case(name):
    """2 .. 5 nodes per axis, one 2-node axis and one cluster axis in each table (1-D: one
    table of each); {table, grids, P (N, ndim), P1: {zaxis: (N, ndim - 1)}, zaxes}."""
    rng = _rng("nd:" + name)
    ndim = int(name[0])
    if ndim == 1:
        shape, kinds = ((2,), ["uniform"]) if name == "1-two" else ((5,), ["cluster"])
    else:
        shape = [int(x) for x in rng.integers(2, 6, ndim)]
        kinds = [str(k) for k in rng.choice(["uniform", "jitter", "log", "far"], ndim)]
        two, clu = (int(x) for x in rng.choice(ndim, 2, replace=False))
        shape[two] = 2
        shape[clu] = max(shape[clu], 3)
        kinds[clu] = "cluster"
    grids = [axis(k, m, rng) for k, m in zip(kinds, shape)]
    table = rng.uniform(-10.0, 0.0, tuple(shape))
    zaxes = sorted({0, ndim // 2, ndim - 1}) if ndim >= 2 else []  # first, middle, last
    return {"table": table, "grids": grids, "P": points(grids, N_POINTS, rng), "zaxes": zaxes,
            "P1": {z: points([g for d, g in enumerate(grids) if d != z], N_POINTS, rng)
                   for z in zaxes}}


@functools.lru_cache(maxsize=None)
def poison_nd_case():
    """(c): a 4-D table with -inf and NaN entries."""
    rng = _rng("poison-4d")
    shape, kinds = (12, 10, 12, 10), ("jitter", "uniform", "far", "jitter")
    grids = [axis(k, m, rng) for k, m in zip(kinds, shape)]
    table = poison(rng.uniform(-10.0, 0.0, shape), _rng(f"poison:4d:{POISON_SEED['4d']}"))
    return {"table": table, "grids": grids, "P": points(grids, N_POINTS, rng), "zaxes": [0, 2, 3],
            "P1": {z: points([g for d, g in enumerate(grids) if d != z], N_POINTS, rng)
                   for z in (0, 2, 3)}}


ORDER_KINDS = ("writeable", "readonly", "float32", "big-endian", "int64", "fortran")


def order_variant(table, kind):
    """The 2-D table kinds scipy routes differently (scipy/interpolate/_rgi.py:409-412: its
    Cython fast path for writeable native float64 -- int64 becomes a fresh float array, and
    a Fortran-ordered one qualifies -- and _evaluate_linear for every other)."""
    if kind == "writeable":
        return table.copy()
    if kind == "readonly":
        t = table.copy()
        t.flags.writeable = False
        return t
    if kind == "float32":
        return table.astype(np.float32)
    if kind == "big-endian":
        return table.astype(">f8")
    if kind == "int64":
        return np.round(table * 1000.0).astype(np.int64)
    if kind == "fortran":
        return np.asfortranarray(table.copy())
    raise ValueError(kind)


def weights(n, rng):
    """(e): a0, a1 in (0.5, 1.5) with a few rows of 0, negative, inf and NaN."""
    a0, a1 = rng.uniform(0.5, 1.5, n), rng.uniform(0.5, 1.5, n)
    for k, v in enumerate((0.0, -1.25, np.inf, np.nan, -0.0, -np.inf)):
        rows = rng.integers(0, n, 12)
        (a0 if k % 2 else a1)[rows] = v
    return a0, a1
