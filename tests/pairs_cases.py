"""The input sets of the pair-list tests (tests/test_pairs_ref.py on the CPU,
tests/test_gpu_pairs.py on the device) and their shared, cached references: a plain helper
module, no fixtures.  Every set is raw fp64 (off the fp32 lattice), so an r2 formed from
the device's fp32 working copies differs from the reference's in its low bits.

A case is a dict: pos (n, 3), h, axis (the C-ABI's axis code), axes (pixel axis, cull axis),
u, v, cu, cv (cull columns, None where they are the pixel's), size, chunk, ext.
"""
import numpy as np

import pairs_ref as pr
import value_bar as vb

_cache = {}


def _cached(key, make):
    if key not in _cache:
        v = make()
        vb._freeze(v)
        if isinstance(v, pr.Pairs):
            for a in v:
                a.setflags(write=False)
        _cache[key] = v
    return _cache[key]


def axis_cull(c):
    """ASP_AXIS_CULL(c) of include/asp.h."""
    return (c + 1) << 4


COLS = {0: (1, 2), 1: (0, 2), 2: (0, 1)}  # (u, v) columns per axis (_projector.py:38-46)


def make_case(pos, h, axes, size, chunk, ext):
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    h = np.ascontiguousarray(h, dtype=np.float64)
    pa, ca = axes
    u, v = (np.ascontiguousarray(pos[:, c]) for c in COLS[pa])
    cu = cv = None
    if ca != pa:
        cu, cv = (np.ascontiguousarray(pos[:, c]) for c in COLS[ca])
    return dict(pos=pos, h=h, axes=(pa, ca), axis=pa | (axis_cull(ca) if ca != pa else 0),
                u=u, v=v, cu=cu, cv=cv, size=tuple(size), chunk=int(chunk),
                ext=tuple(float(e) for e in ext))


def reference(case_key, case):
    """The case's reference pairs, computed once per process."""
    return _cached(("ref",) + case_key, lambda: pr.reference_pairs(
        case["u"], case["v"], case["cu"], case["cv"], case["h"], case["size"], case["chunk"],
        case["ext"]))


# ------------------------------------------------------------- a, b, e: the mixed set
def mixed_case(oracle, window, size=vb.SIZE2D, chunk=vb.CHUNK):
    """value_bar's raw mixed set at ``window`` (None: the origin), axis Z."""
    def make():
        s = vb.mixed_set(oracle, "cubic", window, raw=True)
        pos = np.stack([s["u"], s["v"], np.zeros(s["h"].size)], 1)
        return make_case(pos, s["h"], (2, 2), size, chunk, vb.window_ext(window))
    return _cached(("mixed", window, tuple(size), chunk), make)


NONSQUARE = ((vb.SIZE2D_NONSQUARE, 64), ((200, 150), 32), ((200, 150), 7))


# ----------------------------------------------------------- d: edge particles, 200 x 150
def edge_case(oracle, window, chunk):
    """The mixed set on 200 x 150 with every 50th h negated, one h == 0, one NaN coordinate,
    one NaN h, a particle wholly outside the image, one exactly on the last pixel's corner
    and one on the image's far corner (x_max, y_max)."""
    def make():
        s = vb.mixed_set(oracle, "cubic", window, raw=True)
        size, ext = (200, 150), vb.window_ext(window)
        u, v, h = s["u"].copy(), s["v"].copy(), s["h"].copy()
        h[::50] = -h[::50]
        h[7] = 0.0
        u[11] = np.nan
        h[13] = np.nan
        u[17] = ext[1] + 10.0 * (ext[1] - ext[0])
        psx, psy = (ext[1] - ext[0]) / size[0], (ext[3] - ext[2]) / size[0]
        u[19], v[19] = ext[0] + (size[0] - 1) * psx, ext[2] + (size[1] - 1) * psy
        h[19] = 12.0 * psx  # wide enough to pass the v cull of the last chunk (quirk S2)
        u[23], v[23] = ext[1], ext[3]
        pos = np.stack([u, v, np.zeros(h.size)], 1)
        c = make_case(pos, h, (2, 2), size, chunk, ext)
        c["special"] = dict(negated=np.arange(0, h.size, 50), zero_h=7, nan_u=11, nan_h=13,
                            outside=17, last_corner=19, far_corner=23)
        return c
    return _cached(("edge", window, chunk), make)


def boundary_case():
    """The set of test_gpu_parity.test_boundary_pairs_exact: 20 000 particles at 2h +- 0-4
    ulp (fp32) from pixel corners, 64 x 64, chunk 8."""
    def make():
        rng = np.random.default_rng(3)
        G = 64
        ps = 2.0 / G
        n = 20000
        xi = rng.integers(4, G - 4, n)
        yi = rng.integers(4, G - 4, n)
        h = np.float32(ps) * rng.choice([0.5, 0.75, 1.0, 1.25, 1.5], n).astype(np.float32)
        ang = rng.uniform(0, 2 * np.pi, n)
        X = -1.0 + xi * ps
        Y = -1.0 + yi * ps
        u = (X + 2.0 * h * np.cos(ang)).astype(np.float32)
        v = (Y + 2.0 * h * np.sin(ang)).astype(np.float32)
        k = rng.integers(-4, 5, n).astype(np.float32)
        u = (u + k * np.spacing(u)).astype(np.float32)
        axis_aligned = rng.random(n) < 0.3  # exact 2h offsets along one axis
        u[axis_aligned] = (X[axis_aligned] + 2.0 * h[axis_aligned]).astype(np.float32)
        v[axis_aligned] = Y[axis_aligned].astype(np.float32)
        pos = np.stack([u, v, np.zeros(n, np.float32)], 1).astype(np.float64)
        return make_case(pos, h.astype(np.float64), (2, 2), (G, G), 8, (-1.0, 1.0, -1.0, 1.0))
    return _cached(("boundary",), make)


# ------------------------------------------------------------- c: mixed axis spellings
SQUARE_RANGE_BOX = (67.25, 67.25 + 2.0 ** -6, 67.25, 67.25 + 2.0 ** -6)
SPELLINGS = ("z_cull_y", "y_cull_z", "z_cull_x")


def spelling_case(oracle, name):
    """192 x 256, chunk 64, off the origin; the cull reads other columns than the pixel test.

    z_cull_y  axis 2 | CULL(1), positions [u, v, cv]: the cull reads (u, cv)
    y_cull_z  axis 1 | CULL(2), positions [u, cv, v]: the cull reads (u, cv)
              both on the "box" window, cv = v + uniform(+-1 chunk of the v extent)
    z_cull_x  axis 2 | CULL(0), positions [u, v, w]: the cull reads (v, w), neither column
              in its pixel role.  v must then lie in the u range as well, so the extent is
              the box's u range on both axes, v = u + uniform(+-1 chunk of the u extent)
              (the particles along the diagonal) and w = v + uniform(+-1 chunk).
    """
    def make():
        size, chunk = vb.SIZE2D_NONSQUARE, 64
        s = vb.mixed_set(oracle, "cubic", "box", raw=True)
        rng = np.random.default_rng(31)
        n = s["h"].size
        if name == "z_cull_x":
            ext = SQUARE_RANGE_BOX
            u = s["u"]
            v = u + rng.uniform(-1.0, 1.0, n) * chunk * ((ext[1] - ext[0]) / size[0])
            w = v + rng.uniform(-1.0, 1.0, n) * chunk * ((ext[3] - ext[2]) / size[1])
            return make_case(np.stack([u, v, w], 1), s["h"], (2, 0), size, chunk, ext)
        ext = vb.window_ext("box")
        cv = s["v"] + rng.uniform(-1.0, 1.0, n) * chunk * ((ext[3] - ext[2]) / size[1])
        if name == "z_cull_y":
            return make_case(np.stack([s["u"], s["v"], cv], 1), s["h"], (2, 1), size, chunk, ext)
        return make_case(np.stack([s["u"], cv, s["v"]], 1), s["h"], (1, 2), size, chunk, ext)
    return _cached(("spelling", name), make)


def unculled_reference(name, case):
    """The same pixel test with no cull at all."""
    return _cached(("unculled", name), lambda: pr.reference_pairs(
        case["u"], case["v"], None, None, case["h"], case["size"], case["chunk"], case["ext"],
        cull=False))


# ----------------------------------------------------------------- g: the window seam
SEAM_SIZE = (4160, 4160)  # 65 x 65 tiles: windows of floor(4096 / 65) = 63 tile rows
SEAM_ROW = 63 * 64        # image row 4032: the first row of the second window
SEAM_WIDE_TILES = "4"


def seam_case():
    """About 300 particles within +-3 tile rows of the seam, h from 0.6 to 30 pixel pitches
    (log-uniform); the first 24 have h = 30 pitches, sit 20 rows before or after the seam and
    in the middle of a tile column, so each has pairs in 2 x 3 tiles of one window (wide at
    ASP_WIDE_TILES = 4) and 1 x 3 in the other (binned)."""
    def make():
        nx, ny = SEAM_SIZE
        ext = (-1.0, 1.0, -1.0, 1.0)
        ps = 2.0 / nx
        rng = np.random.default_rng(41)
        n, nbig = 300, 24
        row = SEAM_ROW + rng.uniform(-3 * 64, 3 * 64, n)
        col = rng.uniform(0, ny, n)
        hp = np.exp(rng.uniform(np.log(0.6), np.log(30.0), n))
        k = np.arange(nbig)
        row[:nbig] = SEAM_ROW + np.where(k % 2 == 0, -20.0, 20.0) + rng.uniform(-0.5, 0.5, nbig)
        col[:nbig] = (2 + 2 * k) * 64 + 32 + rng.uniform(-0.5, 0.5, nbig)
        hp[:nbig] = 30.0
        pos = np.stack([-1.0 + row * ps, -1.0 + col * ps, np.zeros(n)], 1)
        return make_case(pos, hp * ps, (2, 2), SEAM_SIZE, 64, ext)
    return _cached(("seam",), make)


# ----------------------------------------------------- 4: the host wrapper, 96 x 80
WRAPPER_SIZE, WRAPPER_CHUNK, WRAPPER_EXT = (96, 80), 32, (-1.0, 1.0, -1.0, 1.0)


def wrapper_set():
    """(pos, h, ids): 1500 particles along the diagonal of all three coordinates, so that
    every spelling (the str "x" culls on (x, y) and measures on (y, z)) keeps pairs; ids are
    integers below 4096."""
    def make():
        rng = np.random.default_rng(53)
        n = 1500
        t = rng.uniform(-1.1, 1.1, n)
        pos = np.stack([t + rng.uniform(-0.3, 0.3, n), t, t + rng.uniform(-0.3, 0.3, n)], 1)
        h = rng.uniform(0.6, 4.0, n) * (2.0 / 80)
        ids = ((np.arange(n) * 37) % 4096).astype(np.float64)
        return dict(pos=pos, h=h, ids=ids)
    return _cached(("wrapper",), make)
