"""tests/spectra_ref.py, the brute force the spectra GPU tests are held to, tied to
tests/sightline_ref.py (itself tied to the oracle) and to two cases worked by hand.
"""
import numpy as np
import pytest

import sightline_ref as sr
import spectra_ref as spr
import value_bar as vb


def velocity_inputs(n, v0, dv, K, seed):
    """vc uniform over 1.5 x the window (centred on it, so some fall outside on both sides),
    b / dv log-uniform in [0.05, 40]."""
    rng = np.random.default_rng(seed)
    width = K * dv
    vc = rng.uniform(v0 - 0.25 * width, v0 + 1.25 * width, n)
    b = dv * np.exp(rng.uniform(np.log(0.05), np.log(40.0), n))
    return vc, b


@pytest.mark.parametrize("kernel", vb.KERNELS)
def test_ring_bins_sum_to_the_column(oracle, kernel):
    """G is the bin-averaged Gaussian: in ring mode sum_k r[s, k] dv is sightline_ref.brute's
    column, to 1e-12 relative, on the mixed set."""
    s = vb.mixed_set(oracle, kernel)
    rng = np.random.default_rng(60)
    px = np.append(rng.uniform(-1.0, 1.0, 150), vb.CLUMP_CENTRE[0])  # the last: inside the clump
    py = np.append(rng.uniform(-1.0, 1.0, 150), vb.CLUMP_CENTRE[1])
    v0, dv, K = -30.0, 2.5, 64
    vc, b = velocity_inputs(s["h"].size, v0, dv, K, 61)
    (r,), (E,), cnt, (col,) = spr.reference(oracle, kernel, s["u"], s["v"], s["h"], [s["a"]], vc, b,
                                            px, py, v0, dv, K, True)
    (want,), want_cnt = sr.brute(s["u"], s["v"], s["h"], px, py, [(s["a"], kernel)])
    assert np.array_equal(cnt, want_cnt) and cnt.max() > 50
    total = r.sum(axis=1) * dv
    assert np.all(np.abs(total - want) <= 1e-12 * np.abs(want)) and np.count_nonzero(want) > 100
    assert np.all(np.abs(col - want) <= 1e-12 * np.abs(want))
    assert np.all(E[cnt > 0] > 0) and not E[cnt == 0].any()
    # ... and a window takes a part of it
    (rw,), _, _, _ = spr.reference(oracle, kernel, s["u"], s["v"], s["h"], [s["a"]], vc, b, px, py,
                                   v0, dv, K, False)
    assert np.all(rw.sum(axis=1) * dv <= want * (1 + 1e-12)) and rw.sum() < 0.9 * r.sum()


def _one_particle(oracle, vc, b, K=8, v0=10.0, dv=2.0, ring=False):
    """One particle on the sightline: (the bins, N = a W(0, h))."""
    one = np.ones(1)
    (r,), _, cnt, (col,) = spr.reference(oracle, "cubic", 0.5 * one, 0.25 * one, 0.1 * one, [3.0 * one],
                                         vc * one, b * one, 0.5 * one, 0.25 * one, v0, dv, K, ring)
    assert cnt.tolist() == [1] and col[0] == 3.0 * sr.kernel_f64("cubic", 0.0 * one, 0.1 * one)[0]
    return r[0], col[0]


def test_narrow_line_mid_bin_lands_in_one_bin(oracle):
    r, N = _one_particle(oracle, vc=10.0 + 2.0 * 3.5, b=1e-3)  # the middle of bin 3
    want = np.zeros(8)
    want[3] = N / 2.0  # N / dv
    assert np.array_equal(r, want) and N > 0


def test_narrow_line_on_an_edge_is_halved(oracle):
    r, N = _one_particle(oracle, vc=10.0 + 2.0 * 3.0, b=1e-3)  # the edge between bins 2 and 3
    want = np.zeros(8)
    want[2] = want[3] = 0.5 * N / 2.0
    assert np.array_equal(r, want)
    # on the window's first edge half of it is outside; the ring keeps that half in its last bin
    r, _ = _one_particle(oracle, vc=10.0, b=1e-3)
    assert r[0] == 0.25 * N and not r[1:].any()
    r, _ = _one_particle(oracle, vc=10.0, b=1e-3, ring=True)
    assert r[0] == 0.25 * N and r[7] == 0.25 * N and not r[1:7].any()


def test_admission():
    ok = spr.admitted(np.array([0.0, np.nan, np.inf, 0.0, 0.0, 0.0, 0.0, 0.0]),
                      np.array([1.0, 1.0, 1.0, 0.0, -1.0, np.nan, np.inf, 2.0 ** 24 / 5.0]), 1.0)
    assert ok.tolist() == [True] + [False] * 7
