"""GPU: the k-NN search on rows without a position and on distances that overflow.

The contract (include/asp.h): a row with a non-finite coordinate is nobody's neighbour and
gets +inf; every other row gets its k-th smallest finite d2 among the finite rows, +inf if
there are fewer than k.  scipy refuses such arrays, so the reference is scipy on the finite
subset (knn_cases.want_nonfinite); where only the distances overflow it is scipy itself.
Every lane's work is bounded by n for any input bits ("k-NN: every path ..."): a
lane without a radius (fewer than k finite distances in its window) scans the array once.
All cases have n <= 600, at the default window and with the window the wave's own 64.
"""
import numpy as np
import pytest

import knn_cases as kc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("window", ["default", "0"])
@pytest.mark.parametrize("name", list(kc.NONFINITE))
def test_nonfinite_rows_and_overflow(gpu, monkeypatch, name, window):
    from asp_amd.knn import knn_smoothing_lengths
    if window != "default":
        monkeypatch.setenv("ASP_KNN_WINDOW", window)
    pos = kc.NONFINITE[name]()
    for k in (7, 32, 64):
        want = kc.want_nonfinite(pos, k)
        for thread in (False, True):  # the wave form and the one-lane form (ASP_KNN_THREAD)
            with monkeypatch.context() as m:
                if thread:
                    m.setenv("ASP_KNN_THREAD", "1")
                h = knn_smoothing_lengths(pos, k)
            bad = np.flatnonzero(kc.bits(h) != kc.bits(want))
            assert bad.size == 0, (name, k, thread, bad[:8], h[bad[:8]], want[bad[:8]])
