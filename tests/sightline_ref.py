"""Float64 NumPy brute force of asp_sample2d's contract (include/asp.h): a plain helper
module, no fixtures.

    out[k] = sum_p a[p] W(r, h_p)  over p with  r2 = dx*dx + dy*dy < (2 h_p)*(2 h_p),
    dx = u_p - px[k],  dy = v_p - py[k]

-- calculate_pixel_value (_pixel_calculations.pyx:20-34) at arbitrary points, every (point,
particle) pair formed, M x N dense in blocks of points.  There is no chunk cull.  NaN and
h == 0 fall out of the comparison as they do in the reference (every comparison false).

``brute`` returns the sums of any number of amplitude rows over the SAME neighbour sets and
the exact neighbour counts; ``kernel=None`` is W = 1, which is how the value bar
E(point) = sum over the point's neighbours of e_p (tests/value_bar.py) is formed for points
that are not on a pixel lattice.
"""
import numpy as np

import column_ref as cr
import value_bar as vb

KERNEL_IDS = {"cubic": 0, "wendland_c2": 1, "indicator": 2, "cubic_column": 3,
              "wendland_c2_column": 4}


def kernel_f64(kernel, r, h):
    """W(r, h) in float64 for the pairs the test included."""
    if kernel is None or kernel == "indicator":
        return np.ones_like(r)
    if kernel in cr.KERNELS:
        return cr.column_kernel(kernel, r, h)
    return vb.kernel_f64(kernel, r, h)


def brute(u, v, h, px, py, fields, block=512, displacement=None):
    """``fields``: a list of (amplitudes, kernel name or None).  Returns (sums, counts):
    sums[i] the float64 sum of fields[i] at every point, counts the int64 neighbour counts.
    ``displacement(d)`` maps the per-axis differences before they are squared (the
    minimum-image fold of a periodic box); None: the differences as they are."""
    u, v, h, px, py = (np.ascontiguousarray(a, np.float64) for a in (u, v, h, px, py))
    amps = [np.ascontiguousarray(a, np.float64) for a, _ in fields]
    m = px.size
    sums = [np.zeros(m) for _ in fields]
    counts = np.zeros(m, np.int64)
    t = 2.0 * h
    thr = t * t
    reach = 2.0 * np.abs(h) * (1.0 + 1e-9)
    for a in range(0, m, block):
        b = min(m, a + block)
        sel = np.arange(u.size)
        if displacement is None:
            # particles that cannot reach the block's bounding box are left out of the dense
            # pass (decisively too far on one axis, with a 1e-9 margin over the fp64 roundings;
            # a NaN anywhere keeps the particle in)
            with np.errstate(invalid="ignore"):
                bx, by = px[a:b][np.isfinite(px[a:b])], py[a:b][np.isfinite(py[a:b])]
                far = np.zeros(u.size, bool)
                if bx.size and by.size:
                    far = ((u < bx.min() - reach) | (u > bx.max() + reach)
                           | (v < by.min() - reach) | (v > by.max() + reach))
            sel = np.flatnonzero(~far)
        dx = u[None, sel] - px[a:b, None]
        dy = v[None, sel] - py[a:b, None]
        if displacement is not None:
            dx, dy = displacement(dx), displacement(dy)
        r2 = dx * dx + dy * dy
        with np.errstate(invalid="ignore"):
            k, p = np.nonzero(r2 < thr[None, sel])
        counts[a:b] = np.bincount(k, minlength=b - a)
        r = np.sqrt(r2[k, p])
        p = sel[p]
        for i, (_, kernel) in enumerate(fields):
            w = kernel_f64(kernel, r, h[p])
            sums[i][a:b] = np.bincount(k, weights=amps[i][p] * w, minlength=b - a)
    return sums, counts


def term_bound(oracle, kernel, h, a, pitch, extra_ulps=0.0):
    """e_p of value_bar (ids 0, 1) or column_ref (ids 3, 4), on |h| (a negative h enters the
    kernels' normalisations with its sign)."""
    h = np.abs(np.asarray(h, np.float64))
    a = np.asarray(a, np.float64)
    ok = np.isfinite(h) & (h > 0.0) & np.isfinite(a)  # the others are in no neighbour set,
    h, a = np.where(ok, h, 1.0), np.where(ok, a, 0.0)  # or make their points NaN
    if kernel in cr.KERNELS:
        return cr.term_bound(kernel, h, a, pitch, extra_ulps)
    return vb.term_bound(oracle, kernel, h, a, pitch, extra_ulps)


def fixed_point_term(oracle, kernel, h, a):
    if kernel in cr.KERNELS:
        return cr.fixed_point_term(kernel, h, a)
    return vb.fixed_point_term(oracle, kernel, h, a)


def reference(oracle, kernel, u, v, h, amps, px, py, pitch=vb.PITCH2D, extra_ulps=0.0,
              displacement=None):
    """(r, E, cnt): r[i] / E[i] the sums and bars of amps[i] at every point, cnt the
    neighbour counts -- one brute-force pass."""
    fields = [(a, kernel) for a in amps]
    fields += [(term_bound(oracle, kernel, h, a, pitch, extra_ulps), None) for a in amps]
    sums, cnt = brute(u, v, h, px, py, fields, displacement=displacement)
    k = len(amps)
    return sums[:k], sums[k:], cnt
