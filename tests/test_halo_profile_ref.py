"""The brute force the GPU profiles are held to (tests/halo_profile_ref.py) against scipy's
periodic KDTree, and the half-open bin convention on exact ties -- on the CPU.
"""
import numpy as np
from scipy.spatial import KDTree

from halo_profile_ref import brute_profiles, lattice_case, lattice_shells, mixed_case
from periodic_ref import wrap


def test_cumulative_counts_are_scipys_ball_counts():
    """Per upper edge, the brute force's cumulative count equals
    KDTree(wrap(pos), boxsize=L).query_ball_point(centres, edges[b] * radii, return_length=True).
    scipy's test is inclusive and its arithmetic is its own, so the comparison means something
    only where no pair sits on a threshold: the case's threshold gap is asserted first."""
    c = mixed_case()
    ref = brute_profiles(c["pos"], c["centres"], c["radii"], c["edges"], c["L"])
    assert ref.gap > 2.0 ** -40, ref.gap
    L = c["L"]
    w = wrap(c["pos"], L)
    tree = KDTree(np.where(w >= L, 0.0, w), boxsize=L)
    cum = np.cumsum(ref.count, axis=1)
    pairs = 0
    for b in range(1, len(c["edges"])):
        want = tree.query_ball_point(c["centres"], c["edges"][b] * c["radii"], return_length=True)
        assert np.array_equal(cum[:, b - 1], want), f"edge {b}"
        pairs += int(want.sum())
    assert pairs > 500_000                                  # (the comparison is not empty)
    assert (3.0 * c["radii"] > 0.5 * L).sum() >= 20        # reaches beyond L / 2
    assert cum[6, -1] == len(c["pos"]) and cum[5, -1] == 0  # the all-particle halo; radius 0


def test_lattice_ties_are_half_open():
    c = lattice_case()
    shells = lattice_shells()
    assert shells == [1, 26, 66]  # d2 = 0; 1, 2, 3 (6 + 12 + 8); 4, 5, 6, 8 (6 + 24 + 24 + 12)
    ref = brute_profiles(c["pos"], c["centres"], c["radii"], c["edges"], c["L"], c["props"])
    assert ref.gap == 0.0  # pairs do sit exactly on thresholds
    for j in range(len(c["centres"])):
        assert ref.count[j].tolist() == shells, j
    assert np.array_equal(ref.sums[0], ref.count.astype(np.float64))
    # edges[0] > 0: the particle on the centre is left out
    ref = brute_profiles(c["pos"], c["centres"], c["radii"], [0.5, 1.0, 2.0, 3.0], c["L"])
    assert ref.count[0].tolist() == [0, 26, 66]


def test_odd_values_in_the_brute_force():
    c = mixed_case()
    pos, props = c["pos"][:2000].copy(), [c["props"][0][:2000].copy()]
    clean = brute_profiles(pos, c["centres"], c["radii"], c["edges"], c["L"], props)
    pos[[3, 700], [0, 2]] = [np.nan, np.inf]
    odd = brute_profiles(pos, c["centres"], c["radii"], c["edges"], c["L"], props)
    assert np.all(odd.count <= clean.count) and odd.count.sum() < clean.count.sum()
    assert np.all(np.isfinite(odd.sums))
