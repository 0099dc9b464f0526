"""Float64 NumPy brute force of asp_sample3d's contract (include/asp_points.h): a plain helper
module, no fixtures.

    out[k] = sum_p a[p] W(r, h_p)  over p with  r2 < (2 h_p)*(2 h_p),
    r2 = (dx*dx + dy*dy) + dz*dz,  dx = x_p - px[k],  dy = y_p - py[k],  dz = z_p - pz[k]

-- voxel_pass of the oracle at arbitrary points, every (point, particle) pair formed, M x N
dense in blocks of points, the parenthesisation kept.  NaN and h == 0 fall out of the
comparison (every comparison false); a negative h passes it.

``brute`` returns the sums of any number of amplitude rows over the SAME neighbour sets and
the exact neighbour counts; ``kernel=None`` is W = 1, which is how the value bar
E(point) = sum over the point's neighbours of e_p (tests/value_bar.py) is formed.
"""
import numpy as np

import sightline_ref as sr
import value_bar as vb

KERNEL_IDS = {"cubic": 0, "wendland_c2": 1, "indicator": 2}


def kernel_f64(kernel, r, h):
    if kernel is None or kernel == "indicator":
        return np.ones_like(r)
    return vb.kernel_f64(kernel, r, h)


def brute(x, y, z, h, px, py, pz, fields, block=512):
    """``fields``: a list of (amplitudes, kernel name or None).  Returns (sums, counts):
    sums[i] the float64 sum of fields[i] at every point, counts the int64 neighbour counts."""
    x, y, z, h, px, py, pz = (np.ascontiguousarray(a, np.float64) for a in (x, y, z, h, px, py, pz))
    amps = [np.ascontiguousarray(a, np.float64) for a, _ in fields]
    m = px.size
    sums = [np.zeros(m) for _ in fields]
    counts = np.zeros(m, np.int64)
    t = 2.0 * h
    thr = t * t
    reach = 2.0 * np.abs(h) * (1.0 + 1e-9)
    for a in range(0, m, block):
        b = min(m, a + block)
        # particles that cannot reach the block's bounding box are left out of the dense pass
        # (decisively too far on one axis, with a 1e-9 margin over the fp64 roundings; a NaN
        # anywhere keeps the particle in)
        far = np.zeros(x.size, bool)
        fin = np.isfinite(px[a:b]) & np.isfinite(py[a:b]) & np.isfinite(pz[a:b])
        if fin.any():
            with np.errstate(invalid="ignore"):
                for c, pc in ((x, px[a:b][fin]), (y, py[a:b][fin]), (z, pz[a:b][fin])):
                    far |= (c < pc.min() - reach) | (c > pc.max() + reach)
        sel = np.flatnonzero(~far)
        dx = x[None, sel] - px[a:b, None]
        dy = y[None, sel] - py[a:b, None]
        dz = z[None, sel] - pz[a:b, None]
        r2 = (dx * dx + dy * dy) + dz * dz
        with np.errstate(invalid="ignore"):
            k, p = np.nonzero(r2 < thr[None, sel])
        counts[a:b] = np.bincount(k, minlength=b - a)
        r = np.sqrt(r2[k, p])
        p = sel[p]
        for i, (_, kernel) in enumerate(fields):
            w = kernel_f64(kernel, r, h[p])
            sums[i][a:b] = np.bincount(k, weights=amps[i][p] * w, minlength=b - a)
    return sums, counts


def reference(oracle, kernel, x, y, z, h, amps, px, py, pz, pitch=0.0, extra_ulps=0.0):
    """(r, E, cnt): r[i] / E[i] the sums and bars of amps[i] at every point, cnt the neighbour
    counts -- one brute-force pass.  ``pitch`` = 0: the sampler has no frame term (the pair
    difference is formed in fp64; the term's coordinate error is one fp32 rounding of r2,
    which the bar's 2^-21 2h covers)."""
    fields = [(a, kernel) for a in amps]
    fields += [(sr.term_bound(oracle, kernel, h, a, pitch, extra_ulps), None) for a in amps]
    sums, cnt = brute(x, y, z, h, px, py, pz, fields)
    k = len(amps)
    return sums[:k], sums[k:], cnt


def lattice(size=vb.SIZE3D, ext=vb.EXT3D):
    """(px, py, pz) of every voxel corner, row-major (z fastest): x_min + i ((x_max - x_min) / nx)
    per axis, each axis with its own pitch (asp_project3d's lattice)."""
    axes = [ext[2 * d] + np.arange(size[d], dtype=np.float64) * ((ext[2 * d + 1] - ext[2 * d]) / size[d])
            for d in range(3)]
    X, Y, Z = np.meshgrid(*axes, indexing="ij")
    return X.ravel(), Y.ravel(), Z.ravel()
