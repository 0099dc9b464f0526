"""Periodic nearest-halo search on the GPU (asp_nearest, asp_amd.haloes.nearest_haloes)
against the reference's own call: scipy.spatial.KDTree(centres[mask], boxsize=L).query(
positions, workers=16), one tree per mask as _scripts/find_nearest_haloes.py:196-221 does,
subset indices mapped back through np.flatnonzero(mask).

The bar of every case:
  1. distances bit-identical to scipy's;
  2. d2(query, centres[index]) equals the minimum d2 bit for bit;
  3. index is the lowest-index minimiser of the brute-force NumPy restatement
     (tests/test_nearest_host.py pins that restatement to scipy on the CPU); on inputs
     without exact ties it is scipy's index too.
The lowest-index minimiser of every row comes from ``lowest_minimiser``: rows whose two
nearest scipy distances differ have one minimiser (scipy's); every other row (ties, or one
centre) is brute-forced over all centres.  The lattice case is brute-forced throughout, and
the random cases brute-force a seeded sample of rows besides.
"""
import numpy as np
import pytest
from scipy.spatial import KDTree

from periodic_ref import bits, brute_nearest, restated_d2, wrap


def scipy_nearest(q, c, L, mask=None):
    """(index into c, distance) as the script computes them; -1 / inf for an empty mask."""
    if mask is None:
        mask = np.ones(len(c), bool)
    if not mask.any():
        return np.full(len(q), -1, np.int64), np.full(len(q), np.inf)
    d, i = KDTree(c[mask], boxsize=L).query(q, workers=16)
    return np.flatnonzero(mask)[i], d


def d2_at(q, c, idx, L):
    """The restated d2 between each query and centre idx of its row."""
    d = wrap(q, L) - c[idx]
    d = np.where(d < -0.5 * L, L + d, np.where(d > 0.5 * L, d - L, d))
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def lowest_minimiser(q, c, L, mask=None):
    """(lowest-index minimiser in c, min d2) of every row, exactly."""
    if mask is None:
        mask = np.ones(len(c), bool)
    sub = np.flatnonzero(mask)
    cs = c[sub]
    if len(cs) >= 2:
        d, i = KDTree(cs, boxsize=L).query(q, k=2, workers=16)
        unique = d[:, 0] < d[:, 1]
        idx = i[:, 0].copy()
    else:
        unique = np.zeros(len(q), bool)
        idx = np.zeros(len(q), np.int64)
    rows = np.flatnonzero(~unique)
    if len(rows):
        idx[rows] = brute_nearest(q[rows], cs, L)[0]
    return sub[idx], d2_at(q, cs, idx, L)


def assert_bar(q, c, L, index, distance, mask=None, tie_free=False, sample=0, seed=0):
    """The three-part bar for one set's outputs."""
    q = np.asarray(q)
    want_i, want_d = scipy_nearest(q, c, L, mask)
    assert index.dtype == np.int32 and distance.dtype == np.float64
    assert np.array_equal(bits(distance), bits(want_d)), "1: distances differ from scipy's"
    low_i, min_d2 = lowest_minimiser(q, c, L, mask)
    assert np.array_equal(bits(np.sqrt(min_d2)), bits(want_d))  # (the oracle agrees with itself)
    assert index.min() >= 0 and index.max() < len(c)
    assert np.array_equal(bits(d2_at(q, c, index, L)), bits(min_d2)), "2: d2 at index is not the minimum"
    assert np.array_equal(index, low_i), "3: not the lowest-index minimiser"
    if tie_free:
        assert np.array_equal(index, want_i), "scipy's index"
    if sample:
        rows = np.random.default_rng(seed).choice(len(q), min(sample, len(q)), replace=False)
        sub = np.flatnonzero(mask) if mask is not None else np.arange(len(c))
        bi, bd2 = brute_nearest(q[rows], c[sub], L)
        assert np.array_equal(sub[bi], index[rows]) and np.array_equal(bits(bd2), bits(min_d2[rows]))


def run(q, c, L, masks=None):
    from asp_amd.haloes import nearest_haloes
    index, distance = nearest_haloes(q, c, L, masks)
    nsets = 1 if masks is None else len(masks)
    assert index.shape == (nsets, len(q)) and distance.shape == (nsets, len(q))
    return index, distance


def uniform_case(scale=1.0, n=200_000, m=5000, seed=21):
    rng = np.random.default_rng(seed)
    L = 25.0 * scale
    c = rng.uniform(0.0, 25.0, (m, 3)) * scale
    c = np.where(c >= L, 0.0, c)
    q = rng.uniform(-12.5, 50.0, (n, 3)) * scale  # inside the box and around it
    return q, c, L


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1.0, 1e-3 / 25.0, 1e6 / 25.0], ids=["L25", "L1e-3", "L1e6"])
def test_uniform(gpu, scale):
    q, c, L = uniform_case(scale)
    index, distance = run(q, c, L)
    assert_bar(q, c, L, index[0], distance[0], tie_free=True, sample=4_000)


def _plummer_box(n, seed, L):
    from asp_amd.plummer import plummer
    p = plummer(n, seed=seed, h_law="pixel", grid=64)["pos"]
    w = wrap(p * (L / 8.0) + 0.5 * L, L)
    return np.where(w >= L, 0.0, w)


@pytest.mark.gpu
def test_clustered(gpu):
    """A Plummer sphere wrapped into the box plus tight clumps: cells with hundreds of
    members beside long empty stretches (many shells before the first centre)."""
    rng = np.random.default_rng(22)
    L = 40.0
    clumps = [wrap(rng.standard_normal((400, 3)) * 1e-4 * L + rng.uniform(0, L, 3), L) for _ in range(5)]
    c = np.concatenate([_plummer_box(18_000, 3, L)] + clumps)
    c = np.where(c >= L, 0.0, c)
    assert len(c) == 20_000
    q = np.concatenate([rng.uniform(0.0, L, (60_000, 3)), _plummer_box(18_000, 3, L)])
    index, distance = run(q, c, L)
    assert_bar(q, c, L, index[0], distance[0], sample=1_000)
    assert np.all(distance[0][60_000:] == 0.0)  # the Plummer's own points are centres


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["corner", "plane"])
def test_degenerate_grids(gpu, kind):
    rng = np.random.default_rng(23)
    L = 10.0
    if kind == "corner":  # the nearest lies across periodic faces; shells are empty until the wrap
        c = rng.uniform(0.0, 1e-6 * L, (3000, 3))
    else:
        c = np.concatenate([rng.uniform(0.0, L, (3000, 2)), np.full((3000, 1), 0.3 * L)], axis=1)
    q = rng.uniform(0.0, L, (50_000, 3))
    index, distance = run(q, c, L)
    assert_bar(q, c, L, index[0], distance[0], sample=5_000)


@pytest.mark.gpu
def test_boundaries_and_ties(gpu):
    """Integer lattice in L = 64: queries on half-integer points have up to 8 exactly tied
    centres (lowest index wins), on integer points distance 0 or exact ties at 1; brute
    force throughout."""
    rng = np.random.default_rng(24)
    L = 64.0
    g = np.arange(64.0)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    c = lattice[rng.choice(len(lattice), 30_000, replace=False)]  # in random order
    special = np.array([0.0, L, 0.5 * L, -L, 2.5 * L])
    q = np.concatenate([rng.integers(0, 64, (1000, 3)) + 0.5, rng.integers(-64, 128, (1000, 3)) * 1.0,
                        np.stack(np.meshgrid(special, special, special, indexing="ij"), -1).reshape(-1, 3),
                        c[:500]])
    index, distance = run(q, c, L)
    bi, bd2 = brute_nearest(q, c, L)
    want_d = scipy_nearest(q, c, L)[1]
    assert np.array_equal(bits(distance[0]), bits(want_d))
    assert np.array_equal(bits(np.sqrt(bd2)), bits(want_d))
    assert np.array_equal(bits(d2_at(q, c, index[0], L)), bits(bd2))
    assert np.array_equal(index[0], bi)
    assert np.all(distance[0][-500:] == 0.0)
    ties = (restated_d2(q[:300], c, L) == bd2[:300, None]).sum(axis=1)
    assert (ties > 1).sum() > 50  # the case does have many exact ties


@pytest.mark.gpu
def test_tiny(gpu):
    rng = np.random.default_rng(25)
    L = 3.0
    q = rng.uniform(-L, 2 * L, (1000, 3))
    for m in (1, 2, 3):
        c = rng.uniform(0.0, L, (m, 3))
        index, distance = run(q, c, L)
        assert_bar(q, c, L, index[0], distance[0])
    index, distance = run(np.zeros((0, 3)), rng.uniform(0.0, L, (5, 3)), L)
    assert index.shape == (1, 0) and distance.shape == (1, 0)
    index, distance = run(q, np.zeros((0, 3)), L)  # no centres at all
    assert np.all(index == -1) and np.all(np.isposinf(distance))
    index, distance = run(q, rng.uniform(0.0, L, (5, 3)), L, [np.zeros(5, bool)])
    assert np.all(index == -1) and np.all(np.isposinf(distance))


def eight_masks(rng, m):
    mass = 10 ** rng.uniform(9, 14, m)
    few = np.zeros(m, bool)
    few[[7, m // 2, m - 1]] = True
    return [np.ones(m, bool), mass > 1e10, mass > 1e11, mass > 1e13, rng.random(m) < 0.5,
            rng.random(m) < 0.02, few, np.zeros(m, bool)]


@pytest.mark.gpu
def test_sets(gpu):
    """Eight masks in one call equal eight scipy trees: all, nested mass cuts, two
    non-nested random masks, three members, none."""
    rng = np.random.default_rng(26)
    q, c, L = uniform_case(n=50_000, seed=27)
    masks = eight_masks(rng, len(c))
    index, distance = run(q, c, L, masks)
    for s, mask in enumerate(masks[:7]):
        assert_bar(q, c, L, index[s], distance[s], mask=mask, tie_free=True, sample=1_000, seed=s)
        assert mask[index[s]].all()
    assert np.all(index[7] == -1) and np.all(np.isposinf(distance[7]))


@pytest.mark.gpu
def test_non_finite_queries(gpu):
    q, c, L = uniform_case(n=5000, seed=28)
    clean_i, clean_d = run(q, c, L)
    bad = q.copy()
    rows = np.array([0, 63, 64, 1000, 4999])
    bad[rows, [0, 1, 2, 0, 1]] = [np.nan, np.inf, -np.inf, np.nan, np.inf]
    index, distance = run(bad, c, L, [np.ones(len(c), bool), np.zeros(len(c), bool)])
    assert np.all(index[:, rows] == -1) and np.all(np.isnan(distance[:, rows]))
    keep = np.setdiff1d(np.arange(len(q)), rows)
    assert np.array_equal(index[0, keep], clean_i[0, keep])
    assert np.array_equal(bits(distance[0, keep]), bits(clean_d[0, keep]))
    assert np.all(index[1, keep] == -1) and np.all(np.isposinf(distance[1, keep]))


@pytest.mark.gpu
@pytest.mark.parametrize("value", ["L", "negative", "nan"])
def test_invalid_centres(gpu, value):
    q, c, L = uniform_case(n=100, m=500, seed=29)
    c[321, 1] = {"L": L, "negative": -1e-9, "nan": np.nan}[value]
    with pytest.raises(ValueError, match="box"):
        run(q, c, L)


@pytest.fixture(scope="module")
def device_case():
    """N = 10^6, M = 10^5, four sets, with scipy's answer -- computed once."""
    rng = np.random.default_rng(30)
    L = 100.0
    c = rng.uniform(0.0, L, (100_000, 3))
    q = rng.uniform(-L, 2 * L, (1_000_000, 3))
    mass = 10 ** rng.uniform(9, 14, len(c))
    masks = [np.ones(len(c), bool), mass > 1e11, mass > 1e13, rng.random(len(c)) < 0.3]
    want = [scipy_nearest(q, c, L, mk) for mk in masks]
    return dict(q=q, c=c, L=L, masks=np.stack(masks), index=np.stack([w[0] for w in want]),
                distance=np.stack([w[1] for w in want]))


@pytest.mark.gpu
def test_device_tensors_on_a_stream(gpu, device_case):
    import torch
    from asp_amd.haloes import nearest_haloes
    d = device_case
    pos = torch.from_numpy(d["q"]).cuda()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    index, distance = nearest_haloes(pos, d["c"], d["L"], list(d["masks"]), stream=stream)
    assert index.is_cuda and distance.is_cuda
    assert index.dtype == torch.int32 and distance.dtype == torch.float64
    stream.synchronize()
    assert np.array_equal(index.cpu().numpy(), d["index"])
    assert np.array_equal(bits(distance.cpu().numpy()), bits(d["distance"]))


@pytest.mark.gpu
@pytest.mark.parametrize("sort", ["0", "1"])
def test_query_order_switch(gpu, device_case, monkeypatch, sort):
    """ASP_NEAREST_SORT (read per call): queries searched in the caller's order (0) or in the
    order of their cell key (1), over several batches -- same results, device tensors on a
    stream and host arrays."""
    import torch
    from asp_amd.haloes import nearest_haloes
    monkeypatch.setenv("ASP_NEAREST_SORT", sort)
    monkeypatch.setenv("ASP_NEAREST_BATCH", "400000")
    d = device_case
    pos = torch.from_numpy(d["q"]).cuda()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    index, distance = nearest_haloes(pos, d["c"], d["L"], list(d["masks"]), stream=stream)
    stream.synchronize()
    assert np.array_equal(index.cpu().numpy(), d["index"])
    assert np.array_equal(bits(distance.cpu().numpy()), bits(d["distance"]))
    hi, hd = nearest_haloes(d["q"][:70_001], d["c"], d["L"], list(d["masks"]))
    assert np.array_equal(hi, d["index"][:, :70_001])
    assert np.array_equal(bits(hd), bits(d["distance"][:, :70_001]))


@pytest.mark.gpu
def test_order_independence(gpu):
    q, c, L = uniform_case(n=50_000, seed=31)  # tie-free
    rng = np.random.default_rng(32)
    index, distance = run(q, c, L)
    pq = rng.permutation(len(q))
    i2, d2 = run(q[pq], c, L)
    assert np.array_equal(i2[0], index[0][pq]) and np.array_equal(bits(d2[0]), bits(distance[0][pq]))
    pc = rng.permutation(len(c))
    i3, d3 = run(q, c[pc], L)
    assert np.array_equal(pc[i3[0]], index[0]) and np.array_equal(bits(d3[0]), bits(distance[0]))


@pytest.mark.gpu
def test_lds_path_batches_and_counter(gpu, monkeypatch):
    """The switches read per call: ASP_NEAREST_SMALL raises the size up to which a set is
    staged through LDS (here every set, so the chunk loop runs 20 times per workgroup),
    ASP_NEAREST_BATCH splits the queries over launches, ASP_NEAREST_PRUNE=0 scans every cell
    of every shell, ASP_NEAREST_COUNT reports the distances evaluated -- exactly N M_s summed
    over the sets on the LDS path."""
    from asp_amd.device import stats
    rng = np.random.default_rng(33)
    q, c, L = uniform_case(n=30_000, seed=34)
    masks = [np.ones(len(c), bool), rng.random(len(c)) < 0.1, np.zeros(len(c), bool)]
    grid_i, grid_d = run(q, c, L, masks)
    assert_bar(q, c, L, grid_i[1], grid_d[1], mask=masks[1], tie_free=True)
    monkeypatch.setenv("ASP_NEAREST_BATCH", "7001")
    monkeypatch.setenv("ASP_NEAREST_COUNT", "1")
    bat_i, bat_d = run(q, c, L, masks)
    evals_grid = stats(0)["evals"]
    monkeypatch.setenv("ASP_NEAREST_SMALL", "100000")
    lds_i, lds_d = run(q, c, L, masks)
    assert stats(0)["evals"] == len(q) * (masks[0].sum() + masks[1].sum())
    assert 0 < evals_grid < stats(0)["evals"] // 10
    monkeypatch.delenv("ASP_NEAREST_SMALL")
    monkeypatch.setenv("ASP_NEAREST_PRUNE", "0")  # every cell of every shell
    all_i, all_d = run(q, c, L, masks)
    assert stats(0)["evals"] > 2 * evals_grid
    for i, d in ((bat_i, bat_d), (lds_i, lds_d), (all_i, all_d)):
        assert np.array_equal(i, grid_i) and np.array_equal(bits(d), bits(grid_d))
