"""Periodic nearest-halo search (asp_nearest, asp_amd.haloes): what holds without a GPU.

The definition the device implements is restated in NumPy (``restated_d2``,
tests/periodic_ref.py) and pinned here bit for bit to the reference's own call,
``scipy.spatial.KDTree(centres, boxsize=L).query(positions)``
(_scripts/find_nearest_haloes.py:196-221, scipy 1.15.3 here).  tests/test_gpu_nearest.py
imports the restatement as its brute-force reference.
"""
import ctypes as C

import numpy as np
import pytest
from scipy.spatial import KDTree

from periodic_ref import bits, brute_nearest


@pytest.mark.parametrize("L", [25.0, 100.0, 67.77, 1.0])
@pytest.mark.parametrize("M", [1, 2, 50, 3000])
def test_restatement_is_scipys(L, M):
    rng = np.random.default_rng(int(L * 100) + M)
    c = rng.uniform(0.0, L, (M, 3))
    c = np.where(c >= L, 0.0, c)
    special = np.array([0.0, 0.5 * L, L, -0.0])
    q = np.concatenate([rng.uniform(0.0, L, (700, 3)), rng.uniform(-2.5 * L, 3.5 * L, (700, 3)),
                        c[:200], np.stack(np.meshgrid(special, special, special, indexing="ij"),
                                          -1).reshape(-1, 3)])
    want = KDTree(c, boxsize=L).query(q)[0]
    _, d2 = brute_nearest(q, c, L)
    assert np.array_equal(bits(np.sqrt(d2)), bits(want))


def _call(L, n=4, m=4, member=None, nsets=1, box=1.0):
    from asp_amd import _lib
    d = np.zeros((4, 3))
    idx = np.zeros(8, np.int32)
    dist = np.zeros(8)
    rc = L.asp_nearest(_lib.ptr(d, _lib._d), n, _lib.ptr(d, _lib._d), m, member, nsets, box,
                       _lib.ptr(idx, _lib._i32), _lib.ptr(dist, _lib._d), 0, 0, None)
    return rc, L.asp_last_error().decode()


@pytest.mark.parametrize("kw", [dict(box=0.0), dict(box=-1.0), dict(box=float("nan")),
                                dict(box=float("inf")), dict(nsets=0), dict(nsets=9),
                                dict(nsets=2), dict(n=-1), dict(m=-1)],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_argument_errors_before_any_device_work(asp, kw):
    """Each is ASP_ERR_INVALID with a message, with or without a device."""
    from asp_amd import _lib
    rc, msg = _call(_lib.lib(), **kw)
    assert rc == _lib.ASP_ERR_INVALID and msg, (rc, msg)


def test_null_arrays_and_too_many_centres(asp):
    from asp_amd import _lib
    L = _lib.lib()
    d = np.zeros((4, 3))
    rc = L.asp_nearest(None, 4, _lib.ptr(d, _lib._d), 4, None, 1, 1.0, None, None, 0, 0, None)
    assert rc == _lib.ASP_ERR_INVALID
    out_i, out_d = np.zeros(4, np.int32), np.zeros(4)
    rc = L.asp_nearest(_lib.ptr(d, _lib._d), 4, None, 4, None, 1, 1.0, _lib.ptr(out_i, _lib._i32),
                       _lib.ptr(out_d, _lib._d), 0, 0, None)
    assert rc == _lib.ASP_ERR_INVALID
    rc = L.asp_nearest(_lib.ptr(d, _lib._d), 4, _lib.ptr(d, _lib._d), 1 << 31, None, 1, 1.0,
                       _lib.ptr(out_i, _lib._i32), _lib.ptr(out_d, _lib._d), 0, 0, None)
    assert rc == _lib.ASP_ERR_UNSUPPORTED
    # n == 0 is valid and needs no device
    rc = L.asp_nearest(None, 0, _lib.ptr(d, _lib._d), 4, None, 1, 1.0, None, None, 0, 0, None)
    assert rc == _lib.ASP_OK


def test_stage_names_appended(asp):
    from asp_amd import _lib
    assert _lib.STAGES[17:] == ("knn_prep", "knn_search", "nearest_prep", "nearest_search")
    assert _lib.lib().asp_nearest.argtypes[4] == C.POINTER(C.c_uint32)


def test_halo_mass_masks_are_the_scripts():
    from asp_amd.haloes import halo_mass_masks
    rng = np.random.default_rng(5)
    masses = np.concatenate([10 ** rng.uniform(8, 15, 500), np.zeros(20)])
    rng.shuffle(masses)
    thresholds = [12.0, 10.5, 14.0, 11.0]  # unsorted: the given order is kept
    got = halo_mass_masks(masses, thresholds)
    want = [masses > 0] + [masses > 10 ** t for t in thresholds]
    assert len(got) == 5
    for g, w in zip(got, want):
        assert g.dtype == np.bool_ and np.array_equal(g, w)
    assert got[0].sum() == 500
    assert len(halo_mass_masks(masses, [])) == 1


def test_member_words_pack_the_masks():
    from asp_amd.haloes import _member_words
    a = np.array([True, False, True, False])
    b = np.array([False, False, True, True])
    assert _member_words([a, b], 4).tolist() == [1, 0, 3, 2]
    assert _member_words([a] * 8, 4).tolist() == [255, 0, 255, 0]


def test_nearest_haloes_refuses_bad_arguments():
    """Shape, dtype and length errors are ValueErrors before any native call (no GPU here)."""
    from asp_amd.haloes import nearest_haloes
    d = np.zeros((4, 3))
    ok = np.ones(4, bool)
    with pytest.raises(ValueError, match="shape"):
        nearest_haloes(np.zeros((3, 2)), d, 1.0)
    with pytest.raises(ValueError, match="float64"):
        nearest_haloes(d, d.astype(np.float32), 1.0)
    with pytest.raises(ValueError, match="length 4"):
        nearest_haloes(d, d, 1.0, [ok, np.ones(3, bool)])
    with pytest.raises(ValueError, match="masks"):
        nearest_haloes(d, d, 1.0, [ok] * 9)
    with pytest.raises(ValueError, match="boolean"):
        nearest_haloes(d, d, 1.0, [np.ones(4, np.int32)])
    with pytest.raises(ValueError, match="shape"):
        nearest_haloes(d, np.zeros((4, 2)), 1.0)
