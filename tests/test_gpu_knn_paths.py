"""GPU: every path of the k-NN search (csrc/asp_knn.hip) at the smallest size at which it runs.

tests/test_gpu_knn.py holds the search to scipy at n <= 100 (the window is the whole array:
no cell is ever looked up) and at n >= 27 000 (table edges met by chance, a failure names one
index in millions).  Here every case of tests/knn_cases.py runs with the default window and
with ASP_KNN_WINDOW=0 -- the window is then the wave's own 64 particles, so the cell passes
carry the whole search from n = 65 up -- and is held to scipy bit for bit (no tolerance).
With ASP_KNN_COUNT the counters say which pass did the work, so the shared pass's three
fallbacks are known to have run where the input forces them.
"""
import os
import time

import numpy as np
import pytest
from scipy.spatial import KDTree

import knn_cases as kc

pytestmark = pytest.mark.gpu

WINDOWS = ("default", "0")
SMALL_SETS = ("uniform577", "uniform4097", "lattice6", "lattice11", "clumps100", "identical1000",
              "axis1000", "sub_first", "sub_middle", "sub_last", "tiny_clump")


@pytest.fixture
def knn(gpu, monkeypatch):
    """knn(name or array, k, **env): the smoothing lengths with ASP_KNN_<KEY> set for the call
    (every other ASP_KNN_* variable unset; a value of None leaves the default)."""
    from asp_amd.knn import knn_smoothing_lengths
    for v in [v for v in os.environ if v.startswith("ASP_KNN_")]:
        monkeypatch.delenv(v)

    def run(pos, k, **env):
        with monkeypatch.context() as m:
            for key, val in env.items():
                if val is not None and not (key == "WINDOW" and val == "default"):
                    m.setenv(f"ASP_KNN_{key}", str(val))
            return knn_smoothing_lengths(kc.case(pos) if isinstance(pos, str) else pos, k)
    return run


def check(knn, name, ks, **env):
    for k in ks:
        h = knn(name, k, **env)
        w = kc.want(name, k)
        bad = np.flatnonzero(kc.bits(h) != kc.bits(w))
        assert bad.size == 0, (name, k, env, bad[:8], h[bad[:8]], w[bad[:8]])


def counters(knn, name, k, **env):
    from asp_amd.device import stats
    h = knn(name, k, COUNT=1, **env)
    st = stats(0)
    assert kc.same_bits(h, kc.want(name, k)), (name, k, env)
    return st


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("n", kc.RAGGED_N)
def test_ragged_sizes(knn, n, window):
    """Uniform points at the sizes where a wave, a block, the table level or the suffix-minimum
    table ends (knn_cases.RAGGED_N), k at 1, inside TopK<32>, at its end and across TopK<64>
    (33 .. 63 leave -inf filler slots); n = k, n = k + 1 and n < k (+inf) are among them."""
    check(knn, f"uniform{n}", kc.RAGGED_K, WINDOW=window)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("name", ["lattice6", "lattice11", "clumps100", "identical1000", "axis1000"])
def test_key_span_edges(knn, name, window):
    """Exact ties, runs of equal keys longer than a wave across a window's ends (the window's
    key span klo / khi must not count a half-covered key as covered), one key for the whole
    set (span 0 -> 1.0), two axes of zero extent."""
    check(knn, name, kc.RAGGED_K, WINDOW=window)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("submin", [None, 8])
@pytest.mark.parametrize("where", list(kc.SUB_CELLS))
def test_subtables(knn, where, submin, window):
    """A level-L cell with a sub-table first, in the middle and last in key order (the last
    one's end is tab[ncell] = n; its last particle closes the sub-table), and with
    ASP_KNN_SUBMIN=8 sub-tables for most of the occupied cells."""
    check(knn, f"sub_{where}", (7, 32, 64), WINDOW=window, SUBMIN=submin)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("fill", [1, 0])
@pytest.mark.parametrize("name", ["uniform4097", "lattice11", "clumps100", "sub_first", "sub_middle",
                                  "sub_last"])
def test_topk64_through_the_cell_passes(knn, name, fill, window):
    """TopK<64> with filler slots (k = 33, 48, 63) and without (64: the 64-wide bitonic fill,
    or 64 insertions with ASP_KNN_FILL=0) beyond the window."""
    check(knn, name, (33, 48, 63, 64), WINDOW=window, FILL=fill)


SWITCHES = [("MASK", 0), ("NEAR", 0), ("F32", 0), ("UNION", 0), ("UNION", 1), ("UNION", 32),
            ("UNION", 63), ("FINE", 0), ("FINE", 3), ("THREAD", 1)]


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("switch", SWITCHES, ids=[f"{a}{b}" for a, b in SWITCHES])
def test_switches(knn, switch, window):
    """Every switch off its default on the small sets: the 8-slot entry buffer, the window in
    array order, the fp64 window (no shared pass), the shared pass off or over a quantile of
    the lanes (the others keep their own pass), finer and coarser cells, and the one-lane
    form ASP_KNN_THREAD, which reads no table."""
    for name in SMALL_SETS:
        check(knn, name, (7, 32, 64), WINDOW=window, **{switch[0]: switch[1]})


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("name", [f"scale{s:g}" for s in kc.SCALES] + ["tiny_clump"])
def test_scales(knn, name, window):
    """d2 ~ 1e300, ~1e-300, zero or subnormal, subnormal in fp32 only, and a 1e-160 clump
    inside a unit-scale set: the fp32 prefilter's bound must pass every true candidate."""
    check(knn, name, (1, 7, 32, 64), WINDOW=window)
    check(knn, name, (32,), WINDOW=window, MASK=0)


def test_suffix_minimum_beyond_1024_blocks(knn):
    """n = 2^21 + 1 is the smallest n with a level-8 cell table: 8^8 + 1 entries, 4097
    suffix-minimum blocks, so k_sfx_top's carry loop runs more than once -- no smaller input
    reaches it (this is why the case is this large).  The wave form (all tables) against the
    one-lane form (ASP_KNN_THREAD searches the keys directly, reads no table) bit for bit, and
    against scipy on 2000 seeded rows."""
    pos = kc.clustered_big()
    t0 = time.perf_counter()
    h = knn(pos, 32)
    t1 = time.perf_counter()
    ht = knn(pos, 32, THREAD=1)
    t2 = time.perf_counter()
    print(f"n = {len(pos)}: wave form {t1 - t0:.2f} s, one-lane form {t2 - t1:.2f} s")
    assert kc.same_bits(h, ht), np.flatnonzero(kc.bits(h) != kc.bits(ht))[:8]
    rows = np.random.default_rng(31).choice(len(pos), 2000, replace=False)
    want = KDTree(pos).query(pos[rows], k=32, workers=-1)[0][:, 31]
    assert kc.same_bits(h[rows], want)


@pytest.mark.parametrize("window", WINDOWS)
def test_counters_shared_pass_off(knn, window):
    """ASP_KNN_UNION=0: no entry goes through the shared pass."""
    for name in ("uniform577", "uniform4097", "clumps100"):
        st = counters(knn, name, 32, WINDOW=window, UNION=0)
        assert st["evals_gather"] == 0 and st["knn_fallbacks"] == 0, (name, st)


@pytest.mark.parametrize("n", [n for n in kc.RAGGED_N if n <= 320])
def test_counters_window_is_the_whole_array(knn, n):
    """n <= 320 at the default window: every wave's window is the whole array, so no cell pass
    evaluates a distance."""
    for k in (7, 32, 64):
        st = counters(knn, f"uniform{n}", k)
        assert st["evals_small"] == 0 and st["evals_gather"] == 0 and st["knn_fallbacks"] == 0, (k, st)


@pytest.mark.parametrize("n", [n for n in kc.RAGGED_N if n >= 129])
def test_counters_cell_passes_carry_the_search(knn, n):
    """ASP_KNN_WINDOW=0 and three waves or more of uniform points: a wave's window is its own
    64 particles, and the neighbours beyond them come from the cell passes."""
    for k in (7, 32, 64):
        st = counters(knn, f"uniform{n}", k, WINDOW=0)
        assert st["evals_small"] + st["evals_gather"] > 0, (k, st)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("n", [n for n in kc.RAGGED_N if n > 64])
def test_no_fallback_on_uniform_points(knn, n, window):
    """Uniform points: a wave's balls overlap, so its common box is a few cells wide and the
    shared pass never gives up."""
    for k in (7, 32, 64):
        st = counters(knn, f"uniform{n}", k, WINDOW=window)
        assert st["knn_fallbacks"] == 0, (k, st)


@pytest.mark.parametrize("window", WINDOWS)
def test_fallback_box_too_wide(knn, window):
    """Islands (knn_cases.islands): each wave spans two clumps or more, its radii are of the
    clump's size and its box of cells at that level is thousands of cells wide -- more than
    kUScan columns (or kUCells ranges): the wave falls back to the per-lane pass."""
    st = counters(knn, "islands", 7, WINDOW=window)
    assert st["knn_fallbacks"] > 0, st
    check(knn, "islands", (32, 33), WINDOW=window)  # k > a clump's 32: the balls reach other clumps


@pytest.mark.parametrize("window", WINDOWS)
def test_fallback_too_many_entries(knn, window):
    """66 000 points in a ball and 31 scattered ones, k = 32: a scattered point's ball reaches
    the ball, whose entries outside the window are more than kUMaxEnt = 65 535 (the 16-bit
    offsets of the range list): the wave falls back to the per-lane pass."""
    st = counters(knn, "ball66000", 32, WINDOW=window)
    assert st["knn_fallbacks"] > 0, st
    assert st["evals_small"] >= kc.BALL_N - 64 - 2 * 256, st  # a lane scanned the ball itself
