"""Float64 NumPy brute force of asp_spectra2d's contract (include/asp_spectra.h): a plain
helper module, no fixtures.

    N_ps   = a[p] W(r, h_p)                 over the pairs of sightline_ref.brute's mask
    edge_j = v0 + j dv
    G_p(j) = [erf((edge_{j+1} - vc_p) / b_p) - erf((edge_j - vc_p) / b_p)] / (2 dv)
    window: out[s, k] = sum_p N_ps G_p(k);   ring: out[s, k] = sum_p N_ps sum_{j = k mod K} G_p(j)

A dense (sightline x particle) pass like ``sightline_ref.brute`` finds the pairs; every
included pair then gets the exact, untruncated G with ``scipy.special.erf`` -- over all K bins
of a window; in ring mode over the bins that meet vc +- SATURATED b, beyond which both erf
values of a bin are +-1.0 exactly in float64 and G is exactly 0 -- added with ``np.add.at``.

The bar of a (sightline, bin) is

    E[s, k] = sum over the sightline's pairs of  e_p |G_p(k)| + |N_ps| (erfc(T) / 2 + 2^-48) / dv

e_p: ``sightline_ref.term_bound`` (the device's error in the pair term, pitch = 0: the pair
difference is formed in fp64); erfc(T) / (2 dv): what the truncation at T b drops per (pair,
bin); 2^-48 / dv: two fp64 erf roundings and the fp64 product.  Both are derived, not tuned.
"""
import numpy as np
from scipy.special import erf, erfc

import sightline_ref as sr

T = 5.0           # ASP_SPECTRA_T
SATURATED = 7.0   # erfc(7) = 4e-23 < 2^-54: erf(+-x) == +-1.0 in float64 for x >= 7
MAX_RUN = float(2 ** 24)


def admitted(vc, b, dv):
    """The velocity part of the admission: vc finite, b finite and > 0, T b / dv < 2^24."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.isfinite(vc) & np.isfinite(b) & (b > 0) & (T * b / dv < MAX_RUN)


def pairs(u, v, h, px, py, block=512):
    """(s, p, r): sightline, particle and distance of every included pair -- the mask of
    ``sightline_ref.brute`` (r2 = dx dx + dy dy < (2h)(2h), a NaN anywhere excludes)."""
    u, v, h, px, py = (np.ascontiguousarray(a, np.float64) for a in (u, v, h, px, py))
    t = 2.0 * h
    thr = t * t
    S, P, R = [], [], []
    for a in range(0, px.size, block):
        dx = u[None, :] - px[a:a + block, None]
        dy = v[None, :] - py[a:a + block, None]
        r2 = dx * dx + dy * dy
        with np.errstate(invalid="ignore"):
            k, p = np.nonzero(r2 < thr[None, :])
        S.append(k + a)
        P.append(p)
        R.append(np.sqrt(r2[k, p]))
    return np.concatenate(S), np.concatenate(P), np.concatenate(R)


def bin_fractions(vc, b, v0, dv, j):
    """G_p(j) for index arrays j (pairs x bins), vc and b per pair."""
    lo = (v0 + j * dv - vc[:, None]) / b[:, None]
    hi = (v0 + (j + 1.0) * dv - vc[:, None]) / b[:, None]
    return (erf(hi) - erf(lo)) / (2.0 * dv)


def reference(oracle, kernel, u, v, h, amps, vc, b, px, py, v0, dv, K, ring, extra_ulps=0.0,
              chunk=2048):
    """(r, E, cnt, col): r[i] / E[i] the (M, K) sums and bars of amps[i]; cnt the (M,)
    neighbour counts over ALL particles the sampler admits; col[i] the (M,) float64 columns
    sum_p N_ps over the pairs whose particle the velocity part admits (what ring-mode bins
    sum to, times dv)."""
    vc, b = np.asarray(vc, np.float64), np.asarray(b, np.float64)
    s, p, r = pairs(u, v, h, px, py)
    m = np.asarray(px).size
    cnt = np.bincount(s, minlength=m)
    ok = admitted(vc, b, dv)[p]
    s, p, r = s[ok], p[ok], r[ok]
    w = sr.kernel_f64(kernel, r, np.asarray(h, np.float64)[p])
    N = [np.asarray(a, np.float64)[p] * w for a in amps]
    e = [sr.term_bound(oracle, kernel, h, a, 0.0, extra_ulps)[p] for a in amps]
    out = [np.zeros((m, K)) for _ in amps]
    E = [np.zeros((m, K)) for _ in amps]
    floor = (0.5 * erfc(T) + 2.0 ** -48) / dv
    pvc, pb = vc[p], b[p]
    if ring:  # the longest runs together, so that a chunk's common length stays tight
        jlo = np.floor((pvc - SATURATED * pb - v0) / dv)
        run = np.floor((pvc + SATURATED * pb - v0) / dv) - jlo + 1.0
        order = np.argsort(run, kind="stable")
    else:
        order = np.arange(s.size)
    for a in range(0, s.size, chunk):
        q = order[a:a + chunk]
        if ring:
            j = jlo[q, None] + np.arange(int(run[q].max()))[None, :]
            k = np.mod(j, K).astype(np.int64)
        else:
            j = np.broadcast_to(np.arange(K, dtype=np.float64), (q.size, K))
            k = np.broadcast_to(np.arange(K), (q.size, K))
        G = bin_fractions(pvc[q], pb[q], v0, dv, j)
        for i in range(len(amps)):
            np.add.at(out[i], (s[q, None], k), N[i][q, None] * G)
            np.add.at(E[i], (s[q, None], k), e[i][q, None] * np.abs(G))
    col = [np.bincount(s, weights=n, minlength=m) for n in N]
    for i in range(len(amps)):
        E[i] += floor * np.bincount(s, weights=np.abs(N[i]), minlength=m)[:, None]
    return out, E, cnt, col
