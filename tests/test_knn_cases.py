"""CPU: the k-NN cases of tests/knn_cases.py are what they claim to be.

Every case of n <= 4096 is held to ``brute_h == scipy_h`` bit for bit (the brute-force
restatement of the device's distance arithmetic against the reference, so a device mismatch is
the device's), and each case's defining property -- what makes the search take the path the
case is for -- is asserted on the input alone.
"""
import numpy as np
import pytest
from scipy.spatial import KDTree

import knn_cases as kc

SMALL = [name for name in kc.CASES if name not in ("islands", "ball66000", "uniform4097")]


@pytest.mark.parametrize("name", SMALL)
def test_brute_force_is_scipy(name):
    pos = kc.case(name)
    assert len(pos) <= 4096
    for k in (1, 7, 32, 33, 63, 64):
        if k <= len(pos):
            assert kc.same_bits(kc.brute_h(pos, k), kc.want(name, k)), (name, k)


def test_ragged_sizes_cover_the_edges():
    ns = set(kc.RAGGED_N)
    for edge in (64, 512, 4096):  # 8^L < n switches the table level; 64-lane waves, 256-lane blocks
        assert {edge - 1, edge, edge + 1} <= ns
    assert {320, 321} <= ns  # 64 + 256: the last n whose default window is the whole array
    assert {n for n in ns if n % 64 == 1} >= {65, 129, 257, 321, 513, 577, 4097}  # one-lane wave
    assert {n for n in ns if n % 256 == 1} >= {257, 513, 4097}  # a last block of one wave
    assert {(n, k) for n in ns for k in kc.RAGGED_K if n == k} == {(63, 63), (64, 64)}
    assert {(n, k) for n in ns for k in kc.RAGGED_K if n == k + 1} == {(64, 63), (65, 64)}
    for n in kc.RAGGED_N:
        pos = kc.case(f"uniform{n}")
        assert pos.shape == (n, 3) and len(np.unique(pos, axis=0)) == n


def test_lattices_have_exact_ties():
    for m in (6, 11):
        pos = kc.case(f"lattice{m}")
        assert len(pos) == m ** 3
        d = KDTree(pos).query(np.full(3, (m // 2) * 0.5), k=7)[0]  # an interior point
        assert np.all(d[1:] == 0.5)  # six neighbours at exactly one spacing


def test_clumps_are_longer_than_a_wave():
    pos = kc.case("clumps100")
    _, counts = np.unique(pos, axis=0, return_counts=True)
    assert len(pos) == 1500 and sorted(counts)[-12:] == [100] * 12 and sorted(counts)[:-12] == [1] * 300
    assert len(np.unique(kc.case("identical1000"), axis=0)) == 1 and len(kc.case("identical1000")) == 1000
    ax = kc.case("axis1000")
    assert np.all(ax[:, 1:] == 0.0) and len(np.unique(ax[:, 0])) == 1000


@pytest.mark.parametrize("where", list(kc.SUB_CELLS))
def test_subtable_cluster_fills_one_cell(where):
    pos = kc.case(f"sub_{where}")
    assert len(pos) == kc.SUB_N and np.all(pos.min(axis=0) == 0.0) and np.all(pos.max(axis=0) == 1.0)
    centre = (np.array(kc.SUB_CELLS[where]) + 0.5) / 16
    near = np.linalg.norm(pos - centre, axis=1) <= 1e-3 * (1 + 1e-12)  # 1e-3 of the span (1.0)
    assert near.sum() == kc.SUB_DENSE  # the cluster's share: 2/3 of the points
    cells = kc.morton_cell(pos, kc.SUB_LEVEL)
    assert np.all(cells[near] == np.array(kc.SUB_CELLS[where]))
    # key order at level 4: x is the most significant axis of the Morton code
    code = lambda c: sum(((c[..., a] >> b) & 1) << (3 * b + 2 - a) for a in range(3) for b in range(4))
    codes = code(cells)
    mine = code(np.array(kc.SUB_CELLS[where]))
    assert {"first": mine == codes.min() == 0, "last": mine == codes.max() == 4095,
            "middle": codes.min() < mine < codes.max()}[where]
    assert (codes == mine).sum() > 64  # above kSubMin: the cell gets a sub-table


def test_islands_are_far_apart():
    pos, c = kc.case("islands"), kc.island_centres()
    assert len(pos) == kc.ISLANDS * kc.ISLAND_PTS == 9600
    radius = np.linalg.norm(pos.reshape(kc.ISLANDS, kc.ISLAND_PTS, 3) - c[:, None, :], axis=2).max()
    spacing = kc.ISLANDS ** (-1 / 3)  # the clumps' mean spacing in the unit cube
    assert radius <= kc.ISLAND_RADIUS * spacing
    sep = KDTree(c).query(c, k=2)[0][:, 1].min()
    assert sep / radius > 500  # the closest two clumps: hundreds of clump radii apart
    # k = 7 stays inside a clump of 32: the radii are of the clump's scale
    assert kc.want("islands", 7).max() <= 2 * radius


def test_ball_and_scatter_reach_the_ball():
    pos = kc.case("ball66000")
    c = 0.5 + 2e-4
    inball = np.linalg.norm(pos - c, axis=1) <= 1e-4 * (1 + 1e-9)
    assert inball.sum() == kc.BALL_N and len(pos) == kc.BALL_N + kc.BALL_SCATTER
    assert np.all(pos[inball] > 0.5)  # the last octant
    sc = pos[~inball]
    assert (sc[:, 0] < 0.5).any()  # x is the code's top bit: these sort before the ball
    # 31 scattered points: the 32nd neighbour of each is in the ball
    d_ball = np.linalg.norm(sc - c, axis=1)
    h = kc.want("ball66000", 32)[~inball]
    assert np.all(np.abs(h - d_ball) <= 1e-4 * (1 + 1e-9))


def test_scales_and_tiny_clump():
    base = kc.case(f"uniform{kc.SCALE_N}")
    for s, (lo, hi) in zip(kc.SCALES, [(1e299, 1e304), (1e-301, 1e-296), (0.0, 5e-324 * 2 ** 40),
                                      (2.0 ** -149, 2.0 ** -126)]):
        pos = kc.case(f"scale{s:g}")
        assert np.array_equal(pos, base * s)
        with np.errstate(under="ignore"):
            d2 = kc.want(f"scale{s:g}", 32) ** 2
        assert np.all(np.isfinite(d2)) and lo <= np.median(d2) <= hi, (s, np.median(d2))
    pos = kc.case("tiny_clump")
    tiny = np.abs(pos).max(axis=1) < 1e-158
    assert tiny.sum() == 40 and len(pos) == 2040
    h = kc.want("tiny_clump", 32)[tiny]
    assert np.all(h > 0) and np.all(h * h < 2.0 ** -1022)  # subnormal squared distances


def test_nonfinite_cases():
    """Each non-finite case holds what it names, at least half of its rows (few_finite aside)
    finite, and on the overflow cases scipy itself gives what the contract asks: +inf where
    fewer than k squared distances are finite (bit-identical to the brute force)."""
    finite = {name: kc.finite_rows(f()).sum() for name, f in kc.NONFINITE.items()}
    sizes = {name: len(f()) for name, f in kc.NONFINITE.items()}
    assert max(sizes.values()) <= 600
    assert finite == {"nan_1": 599, "nan_10pc": 540, "nan_50pc": 300, "nan_one_coordinate": 519,
                      "plus_inf": 547, "minus_inf": 547, "inf_rows": 281, "few_finite": 20,
                      "overflow_all": 600, "clumps_20": 40, "clumps_40": 80}
    for name, value in (("nan_one_coordinate", np.nan), ("plus_inf", np.inf), ("minus_inf", -np.inf)):
        pos = kc.NONFINITE[name]()
        bad = pos[~kc.finite_rows(pos)]
        hit = np.isnan(bad) if np.isnan(value) else bad == value
        assert np.all(hit.sum(axis=1) == 1) and np.all(np.isfinite(bad).sum(axis=1) == 2)
    assert sizes["few_finite"] >= 64 > finite["few_finite"] >= 7  # n >= k, finite rows < k (32, 64)
    for name in ("overflow_all", "clumps_20", "clumps_40"):
        pos = kc.NONFINITE[name]()
        for k in (7, 32, 64):
            h = kc.want_nonfinite(pos, k)
            assert kc.same_bits(h, kc.brute_h(pos, k)), (name, k)
            enough = {"overflow_all": 1, "clumps_20": 20, "clumps_40": 40}[name] >= k
            assert np.all(np.isfinite(h)) if enough else np.all(np.isinf(h)), (name, k)


def test_nonfinite_contract_reference():
    """want_nonfinite: the finite subset through scipy; non-finite rows and rows with fewer
    than k finite rows about them +inf."""
    pos = kc.uniform(200).copy()
    pos[[3, 50], 1] = np.nan
    pos[7, 0] = np.inf
    h = kc.want_nonfinite(pos, 7)
    f = kc.finite_rows(pos)
    assert f.sum() == 197 and np.all(np.isinf(h[~f])) and np.all(np.isfinite(h[f]))
    assert kc.same_bits(h[f], kc.brute_h(pos[f], 7))
    assert np.all(np.isinf(kc.want_nonfinite(pos, 198)))
