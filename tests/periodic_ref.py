"""The periodic-box definition the device implements (csrc/asp_periodic.hpp), restated in NumPy.

tests/test_nearest_host.py pins ``restated_d2`` bit for bit to the reference's own call,
``scipy.spatial.KDTree(centres, boxsize=L).query(positions)``; tests/test_gpu_nearest.py and
tests/halo_profile_ref.py use it as their brute-force reference.
"""
import numpy as np


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def wrap(x, L):
    """scipy's wrap of query coordinates into the box, with its two corrections."""
    w = x - np.floor(x / L) * L
    w = np.where(w >= L, w - L, w)
    return np.where(w < 0, w + L, w)


def restated_d2(q, c, L):
    """(len(q), len(c)) squared periodic distances by asp.h's definition of asp_nearest:
    per axis d = w - c, d < -L/2 -> L + d, else d > L/2 -> d - L; ((dx dx + dy dy) + dz dz)."""
    w = wrap(q, L)
    ct = np.ascontiguousarray(c.T)
    out = None
    for a in range(3):
        d = w[:, a, None] - ct[a][None, :]
        lo, hi = d < -0.5 * L, d > 0.5 * L
        np.add(L, d, out=d, where=lo)
        np.subtract(d, L, out=d, where=hi)
        np.multiply(d, d, out=d)
        out = d if out is None else np.add(out, d, out=out)
    return out


def brute_nearest(q, c, L, chunk=None):
    """(lowest-index minimiser, min d2) per query, in chunks of queries."""
    chunk = chunk or max(1, 50_000 // max(1, len(c)))
    idx = np.empty(len(q), np.int64)
    d2 = np.empty(len(q))
    for a in range(0, len(q), chunk):
        D = restated_d2(q[a:a + chunk], c, L)
        idx[a:a + chunk] = D.argmin(axis=1)  # argmin returns the first (lowest) minimiser
        d2[a:a + chunk] = D[np.arange(D.shape[0]), idx[a:a + chunk]]
    return idx, d2
