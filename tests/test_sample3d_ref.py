"""tests/sample3d_ref.py, the brute force the 3-D point-sampling GPU tests use off the voxel
lattice, tied to the oracle ON the lattice: at the 122 880 voxel corners of value_bar's cube
it must give the oracle's cube of the cube set (to fp64 summation noise, 1e-6 of the
per-voxel bar E) and its neighbour counts (exactly).
"""
import numpy as np
import pytest

import sample3d_ref as s3
import value_bar as vb


def test_counts_are_the_oracles_on_the_lattice(oracle):
    s = vb.cube_set(oracle, "cubic")
    want = oracle.project3d(s["x"], s["y"], s["z"], s["h"], np.ones(s["h"].size), vb.SIZE3D,
                            vb.EXT3D, kernel="indicator")
    px, py, pz = s3.lattice()
    assert px.size == 122880
    (ones,), cnt = s3.brute(s["x"], s["y"], s["z"], s["h"], px, py, pz,
                            [(np.ones(s["h"].size), None)])
    assert np.array_equal(cnt, want.ravel().astype(np.int64))
    assert np.array_equal(ones, want.ravel())
    print(f"SAMPLE3D_REF pairs = {cnt.sum()}")
    assert cnt.sum() > 1_000_000  # (every corner has a neighbour: the h6-14 class spans the cube)


@pytest.mark.parametrize("kernel", vb.KERNELS)
def test_values_are_the_oracles_on_the_lattice(oracle, kernel):
    s = vb.cube_set(oracle, kernel)
    ref = vb.reference3d(oracle, kernel)
    px, py, pz = s3.lattice()
    (g,), _ = s3.brute(s["x"], s["y"], s["z"], s["h"], px, py, pz, [(s["a"], kernel)])
    r, E = ref["r"].ravel(), ref["E"].ravel()
    assert np.array_equal(g == 0, r == 0)
    nz = r != 0
    worst = float(np.max(np.abs(g - r)[nz] / E[nz]))
    print(f"SAMPLE3D_REF {kernel}: worst |brute - oracle| / E = {worst:.3g}")
    assert worst <= 1e-6


def test_strict_inequality_and_odd_values():
    """r2 == (2h)^2 is excluded; NaN and h == 0 fall out of the comparison; a negative h
    passes it; the third axis counts."""
    x = np.array([0.0, 3.0, 3.0, np.nan, 5.0, 7.0])
    y = np.zeros(6)
    z = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
    h = np.array([0.25, 0.0, np.nan, 1.0, -0.25, 0.25])
    px = np.array([0.0, 0.0, 3.0, np.nan, 5.1, 7.0])
    py = np.zeros(6)
    pz = np.array([0.5, np.nextafter(0.5, 0.0), 0.0, 0.0, 0.0, 0.4])
    (ones,), cnt = s3.brute(x, y, z, h, px, py, pz, [(np.ones(6), None)])
    assert cnt.tolist() == [0, 1, 0, 0, 1, 0] and ones.tolist() == [0.0, 1.0, 0.0, 0.0, 1.0, 0.0]
