"""A float64 NumPy brute force of asp_halo_profiles' definition (include/asp_profiles.h), the
seeded cases the CPU and GPU tests share, and the bar the GPU results are held to.

Per halo j: w = wrap(x), d = w - c folded per axis (d < -L/2 -> L + d, else d > L/2 -> d - L),
d2 = (dx dx + dy dy) + dz dz, T_b = (edges[b] * radius[j])**2; the particle is in bin
``np.searchsorted(T, d2, side="right") - 1`` when that is in [0, nbins).
"""
import numpy as np

from periodic_ref import wrap


class Ref:
    """count (M, B) int64; sums, sabs (P, M, B): the sums of prop and of |prop| per bin;
    gap: the smallest |d2 - T_b| / T_b over all pairs and all thresholds with T_b > 0."""

    def __init__(self, count, sums, sabs, gap):
        self.count, self.sums, self.sabs, self.gap = count, sums, sabs, gap


def brute_profiles(pos, centres, radii, edges, L, props=()):
    pos, centres = np.asarray(pos, np.float64), np.asarray(centres, np.float64)
    edges = np.asarray(edges, np.float64)
    props = [np.asarray(p, np.float64) for p in props]
    m, nbins = len(centres), len(edges) - 1
    count = np.zeros((m, nbins), np.int64)
    sums = np.zeros((len(props), m, nbins))
    sabs = np.zeros((len(props), m, nbins))
    gap = np.inf
    with np.errstate(invalid="ignore", over="ignore"):
        w = wrap(pos, L)
        for j in range(m):
            d = w - centres[j]
            d = np.where(d < -0.5 * L, L + d, np.where(d > 0.5 * L, d - L, d))
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            t = edges * (1.0 if radii is None else radii[j])
            T = t * t
            b = np.searchsorted(T, d2, side="right") - 1
            inside = (b >= 0) & (b < nbins) & np.isfinite(d2)
            bi = b[inside]
            count[j] = np.bincount(bi, minlength=nbins)
            for k, p in enumerate(props):
                sums[k, j] = np.bincount(bi, weights=p[inside], minlength=nbins)
                sabs[k, j] = np.bincount(bi, weights=np.abs(p[inside]), minlength=nbins)
            fin = d2[np.isfinite(d2)]
            for Tb in T[(T > 0) & np.isfinite(T)]:
                if len(fin):
                    gap = min(gap, float(np.min(np.abs(fin - Tb)) / Tb))
    return Ref(count, sums, sabs, gap)


MIXED_EDGES = np.array([0.0, 0.25, 0.5, 1.0, 2.0, 3.0])


def mixed_case():
    """Seed 7, L = 10, 20 000 particles uniform in [-L, 2L) (so the wrap is exercised), the
    first 40 % redrawn as Gaussians (sigma 0.15) on the first 8 of 300 centres; centres 0 .. 3
    on box faces, at the middle and at the origin; radii log-uniform in [1e-3 L, 0.3 L] with
    one 0 and one 0.3 L (3 x 0.3 L = 9 exceeds the box's largest separation: that halo holds
    every particle).  Four properties: three signed, one of ones."""
    rng = np.random.default_rng(7)
    L, n, m = 10.0, 20_000, 300
    centres = rng.uniform(0.0, L, (m, 3))
    centres = np.where(centres >= L, 0.0, centres)
    centres[:4] = [(0.01, 0.02, 9.99), (9.995, 5.0, 5.0), (5.0, 5.0, 5.0), (0.0, 0.0, 0.0)]
    pos = rng.uniform(-L, 2 * L, (n, 3))
    k = (4 * n) // 10
    pos[:k] = centres[np.arange(k) % 8] + rng.normal(0.0, 0.15, (k, 3))
    radii = 10 ** rng.uniform(np.log10(1e-3 * L), np.log10(0.3 * L), m)
    radii[5], radii[6] = 0.0, 0.3 * L
    props = [rng.normal(size=n), rng.normal(size=n) * 10 ** rng.uniform(-3, 3, n),
             rng.normal(size=n) - 0.5, np.ones(n)]
    return dict(pos=pos, centres=centres, radii=radii, edges=MIXED_EDGES.copy(), L=L, props=props)


def lattice_case():
    """Ties on every threshold: particles on the integer lattice of a box L = 8, centres on
    lattice points ((0, 0, 0) among them), radius 1, edges [0, 1, 2, 3]: d2 is an integer and
    T = [0, 1, 4, 9], so d2 = 1, 4 and 9 sit exactly on thresholds."""
    g = np.arange(8.0)
    pos = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    centres = np.array([(0.0, 0.0, 0.0), (4.0, 4.0, 4.0), (7.0, 0.0, 3.0), (1.0, 7.0, 7.0)])
    return dict(pos=pos, centres=centres, radii=np.ones(len(centres)),
                edges=np.array([0.0, 1.0, 2.0, 3.0]), L=8.0, props=[np.ones(len(pos))])


def lattice_shells():
    """Integer points with d2 in [0, 1), [1, 4), [4, 9), by enumeration (|d| <= 3 on every axis
    holds them all; in L = 8 no two of them are images of each other)."""
    r = np.arange(-3, 4)
    d2 = (r[:, None, None] ** 2 + r[None, :, None] ** 2 + r[None, None, :] ** 2).ravel()
    return [int(((d2 >= lo) & (d2 < hi)).sum()) for lo, hi in ((0, 1), (1, 4), (4, 9))]


def assert_bar(count, sums, ref):
    """The bar of every GPU case: counts exact; a sum is exactly 0 where count == 0, bit-equal
    to the member's property where count == 1, and elsewhere within count * 2^-52 * S_abs of the
    brute force -- two fp64 summation orders of k terms are each within (k - 1) 2^-53 S_abs of
    the exact sum.  A bin the brute force finds non-finite (a NaN property of a member) must be
    non-finite, and no other."""
    count, sums = np.asarray(count), np.asarray(sums)
    assert count.dtype == np.int64 and count.shape == ref.count.shape
    assert np.array_equal(count, ref.count), (
        f"{(count != ref.count).sum()} of {count.size} counts differ")
    assert sums.dtype == np.float64 and sums.shape == ref.sums.shape
    for k in range(sums.shape[0]):
        s, want, sabs = sums[k], ref.sums[k], ref.sabs[k]
        bad = ~np.isfinite(want)
        assert np.array_equal(~np.isfinite(s), bad), "non-finite bins differ"
        assert np.all(s[count == 0] == 0.0)
        one = (count == 1) & ~bad
        assert np.array_equal(s[one].view(np.uint64), want[one].view(np.uint64))
        ok = ~bad
        err = np.abs(s[ok] - want[ok])
        assert np.all(err <= count[ok] * 2.0 ** -52 * sabs[ok]), (
            f"prop {k}: max excess {np.max(err - count[ok] * 2.0 ** -52 * sabs[ok]):.3e}")
