"""tests/sightline_ref.py, the brute force the sightline GPU tests use off the pixel lattice,
tied to the oracle ON the lattice: at the 256^2 pixel corners of value_bar's grid it must
give the oracle's maps of the mixed set (to fp64 summation noise) and its neighbour counts
(exactly).  On a square image the chunk cull removes nothing from a disc
(value_bar.stamp_reference), so create_image's map at a corner IS calculate_pixel_value
there.
"""
import numpy as np
import pytest

import sightline_ref as sr
import value_bar as vb


def lattice(size=vb.SIZE2D, ext=vb.EXT2D):
    """(px, py) of every pixel corner, row-major: x_min + i ((x_max - x_min) / nx), and the
    reference's y pitch, which also divides by nx."""
    nx, ny = size
    X = ext[0] + np.arange(nx, dtype=np.float64) * ((ext[1] - ext[0]) / nx)
    Y = ext[2] + np.arange(ny, dtype=np.float64) * ((ext[3] - ext[2]) / nx)
    return np.repeat(X, ny), np.tile(Y, nx)


@pytest.mark.parametrize("kernel", vb.KERNELS)
def test_brute_force_is_the_oracle_on_the_lattice(oracle, kernel):
    s = vb.mixed_set(oracle, kernel)
    ref = vb.reference2d(oracle, kernel)
    px, py = lattice()
    (r0, r1, ones), cnt = sr.brute(s["u"], s["v"], s["h"], px, py,
                                   [(s["a0"], kernel), (s["a"], kernel), (np.ones(s["h"].size), None)])
    want = ref["cnt"].ravel()
    assert np.array_equal(cnt, want.astype(np.int64))
    assert np.array_equal(ones, want)  # W = 1: the indicator map itself
    # fp64 noise: the oracle's W and this module's differ by a few roundings per term (<= 16
    # ulp allowed), and a sum of cnt positive terms in another order by <= cnt ulp of the sum
    for g, r in ((r0, ref["r0"].ravel()), (r1, ref["r1"].ravel())):
        assert np.array_equal(g == 0, r == 0)
        assert np.all(np.abs(g - r) <= 2.0 ** -52 * (want + 16.0) * np.abs(r))
    assert cnt.max() > 100 and cnt.min() < 10  # the clump, and corners only the wide discs reach


def test_strict_inequality_and_odd_values():
    """r2 == (2h)^2 is excluded; NaN and h == 0 fall out of the comparison; a negative h
    passes it."""
    u = np.array([0.0, 3.0, 3.0, np.nan, 5.0])
    v = np.array([0.0, 0.0, 0.0, 0.0, 0.0])
    h = np.array([0.25, 0.0, np.nan, 1.0, -0.25])
    px = np.array([0.5, np.nextafter(0.5, 0.0), 3.0, np.nan, 5.1])
    py = np.zeros(5)
    (ones,), cnt = sr.brute(u, v, h, px, py, [(np.ones(5), None)])
    assert cnt.tolist() == [0, 1, 0, 0, 1] and ones.tolist() == [0.0, 1.0, 0.0, 0.0, 1.0]
