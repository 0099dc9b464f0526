"""Per-pixel value bar (DESIGN.md §5 "Bars"): a plain helper module, no fixtures.

The global-peak bar of ``test_gpu_parity.assert_map_close`` cannot see an error in a
particle whose own peak W(0, h) ~ 1/h^3 is small next to the map's maximum: exactly the
large-h particles of the gathered deposit, the wide path and the cube's wave walk.  This
bar is per pixel.  For inputs that are exactly fp32-representable the only error of the
device is its fp32 evaluation of each term; it is bounded per (particle, pixel) pair and
summed over the pixel's EXACT neighbour set, which is one oracle call with the indicator
kernel and the per-particle factor e_p as the property:

    E(pixel) = sum_{p included in pixel} e_p
    e_p      = |a_p| W(0, h_p) (BETA eps_p / h_p + ALPHA 2^-24)
    eps_p    = 2^-21 (M + 2 h_p),   M = 128 pixel pitches (the larger pitch)

Where the constants come from (none of them from the device's output):

* eps_p is DESIGN §3's documented bound on the coordinate roundings of a pair (staging,
  frame shift, corner table, subtraction, squares and sum), stated there with a >= 2x
  margin and with ``g.mgl`` = 128 pitches for record frames.  The cube's frames are
  smaller (2^-24 (|lx| + 16 pitches) in its comments), so M = 128 is conservative there.
* BETA = 1.1 bounds max |dW/dq| / W(0): exactly 1 for the cubic spline (q = 2/3), 1.055
  for Wendland C2 (q = 1/2).  A position error eps changes the term by at most
  W(0) BETA eps / h; both kernels are continuous at q = 2, so this also covers the
  edge-continuous forms that evaluate instead of deciding.
* ALPHA = 16 covers the remaining roundings of one term in units of u = 2^-24 of
  |a| W(0).  Counted from ``accumulate`` / ``kernel_shape`` / ``kernel_shape2`` /
  ``edge_shape2`` (2-D) and ``column_e`` / ``plane_walk`` (cube):
    - coefficient fl32(a sigma / h^3) (formed in fp64, rounded once)            1 u
    - q: 1/h by the hardware reciprocal (1 ulp = 2 u), the hardware sqrt (2 u), their
      product (1 u) -- 5 u relative in 2-D; the cube forms q in units of h from
      hinv^2, s hinv^2, z hinv, two fmas and the sqrt, <= 7 u relative.  A relative
      error d of q moves f by q |f'(q)| d, and max q |f'(q)| = 0.79 (cubic, q = 0.89),
      0.69 (Wendland, q = 0.8)                                          <= 0.79 * 7 < 6 u
    - the polynomial, worst at q -> 0 where f = 1 and the q term above vanishes:
      cubic as t^3 - s^3/2 (f/2 = 0.5): (2.5 + 1.25 + 0.25) u absolute = 8 u of f(0);
      Wendland t^4 (1 + 2q): 2 + 1 + 0.5 + 1 + 0.5 = 5 u                         <= 8 u
      (at the q that maximise the q term the polynomial's own roundings are < 2 u, so
      the two together stay <= 8 u; their plain sum is 14 u)
    - the product coefficient * f                                                  1 u
    - the fp32 store of the pixel, |r| <= sum |a| W(0)                             1 u
  11 u taken jointly, 17 u as a plain sum of every item's own maximum: 16 is the count
  rounded up to a power of two.  (The dead zone of the edge forms, DESIGN §3, moves a
  term by tau^2 <= 1e-8 of the peak, < 0.2 u.)
* ``deterministic=True`` (int64 fixed point) adds the header's documented term, bounded
  from above by F = 2^-37 n max_p(|a_p| W(0, h_p)), n the call's particle count.

``assert_terms_close(g, r, E)`` asserts g == 0 exactly where r == 0 and |g - r| <= E at
every pixel; a failure reports the worst err/E, its pixel and the class of particle
that dominates E there.

The module also builds the input sets the value tests share (equal-peak amplitudes
a_p = fl32(U(0.5, 1.5) / W(0, h_p)), so every particle's own peak is O(1) whatever its h)
and a straightforward float32 NumPy evaluation that the CPU tests hold to the same bar.
"""
import numpy as np

ALPHA = 16.0
BETA = 1.1
M_PITCHES = 128.0
U24 = 2.0 ** -24

KERNELS = ("cubic", "wendland_c2")

# ---------------------------------------------------------------------------- inputs
SIZE2D = (256, 256)
SIZE2D_NONSQUARE = (192, 256)
EXT2D = (-1.0, 1.0, -1.0, 1.0)
CHUNK = 64
PITCH2D = 2.0 / 256

# (name, h range in pixel pitches, particles)
CLASSES_2D = (("h0.55-0.75", 0.55, 0.75, 1500), ("h0.8-1.2", 0.8, 1.2, 800),
              ("h2-4", 2.0, 4.0, 400), ("h6-12", 6.0, 12.0, 200), ("h40-120", 40.0, 120.0, 12))
CLUMP = ("clump", 0.55, 1.2, 2000)  # sigma = 2 px about the centre of tile (2, 1)
CLUMP_CENTRE = (0.25, -0.25)
WIDE_TILES = "4"  # ASP_WIDE_TILES for the 2-D sets: the h40-120 class takes the wide path

SIZE3D = (48, 40, 64)
EXT3D = (-2.0, 2.0, -2.0, 2.0, -2.0, 2.0)
PITCH3D = 4.0 / 40  # the larger voxel pitch
CLASSES_3D = (("h0.6-1.0", 0.6, 1.0, 3000), ("h1.5-3", 1.5, 3.0, 600), ("h6-14", 6.0, 14.0, 24))


def f32(a):
    """Round through float32 (what every entry point is handed), kept as float64."""
    return np.asarray(a, np.float32).astype(np.float64)


def w0(oracle, kernel, h):
    h = np.atleast_1d(np.asarray(h, np.float64))
    return oracle.kernel_eval(kernel, np.zeros_like(h), h)


_cache = {}


def _freeze(v):
    """Shared references stay unchanged: their arrays are made read-only."""
    if isinstance(v, np.ndarray):
        v.setflags(write=False)
    elif isinstance(v, dict):
        for a in v.values():
            _freeze(a)


def _cached(key, make):
    if key not in _cache:
        v = make()
        _freeze(v)
        _cache[key] = v
    return _cache[key]


def mixed_set(oracle, kernel):
    """The 2-D mixed set: every class of CLASSES_2D uniform in the extent plus the clump.
    Keys u, v, h, a, T, a0 (= fl32(a T)), cls (class index), names."""
    def make():
        rng = np.random.default_rng(20)
        u, v, h, cls = [], [], [], []
        for k, (_, lo, hi, n) in enumerate(CLASSES_2D + (CLUMP,)):
            if k < len(CLASSES_2D):
                u.append(rng.uniform(-1.0, 1.0, n))
                v.append(rng.uniform(-1.0, 1.0, n))
            else:
                u.append(rng.normal(CLUMP_CENTRE[0], 2 * PITCH2D, n))
                v.append(rng.normal(CLUMP_CENTRE[1], 2 * PITCH2D, n))
            h.append(rng.uniform(lo, hi, n) * PITCH2D)
            cls.append(np.full(n, k))
        u, v, h = (f32(np.concatenate(t)) for t in (u, v, h))
        a = f32(rng.uniform(0.5, 1.5, h.size) / w0(oracle, kernel, h))
        T = f32(rng.uniform(1.0, 3.0, h.size))
        return dict(u=u, v=v, h=h, a=a, T=T, a0=f32(a * T), cls=np.concatenate(cls),
                    names=[c[0] for c in CLASSES_2D + (CLUMP,)])
    return _cached(("mixed", kernel), make)


def cube_set(oracle, kernel):
    """The cube set: positions uniform in +-2.2 (footprints clipped at the faces, some
    missing the cube).  Keys x, y, z, h, a, cls, names."""
    def make():
        rng = np.random.default_rng(21)
        h, cls = [], []
        for k, (_, lo, hi, n) in enumerate(CLASSES_3D):
            h.append(rng.uniform(lo, hi, n) * PITCH3D)
            cls.append(np.full(n, k))
        h = f32(np.concatenate(h))
        x, y, z = (f32(rng.uniform(-2.2, 2.2, h.size)) for _ in range(3))
        a = f32(rng.uniform(0.5, 1.5, h.size) / w0(oracle, kernel, h))
        return dict(x=x, y=y, z=z, h=h, a=a, cls=np.concatenate(cls),
                    names=[c[0] for c in CLASSES_3D])
    return _cached(("cube", kernel), make)


# Stamps: one particle per map.  (path name, h in pixel pitches, ASP_GATHER_MIN,
# ASP_GATHER_AREA, ASP_WIDE_TILES, what stats() must show).  The sweep-all thresholds keep
# the 4-wide and mid-size boxes out of the large stream; 5 / 6 gathers every box of at
# least 6 pixels, clipped slivers included; a wide tile limit of 2 makes the h = 80 disc
# wide at every position (outside the image it still meets 4 tiles).
STAMP_PATHS = (("small3", 0.65, "65", str(1 << 30), "256", "small"),
               ("deferred4", 1.0, "65", str(1 << 30), "256", "small"),
               ("swept", 3.0, "65", str(1 << 30), "256", "small"),
               ("gather_mid", 3.0, "5", "6", "256", "large"),
               ("gather", 9.0, "5", "6", "256", "large"),
               ("wide", 80.0, "5", "20", "2", "wide"))
STAMP_POSITIONS = ("inside", "corner", "edge", "outside")


def stamp_particle(oracle, kernel, h_px, where):
    """(u, v, h, a) of one stamp, all fp32-representable."""
    h = float(f32(h_px * PITCH2D))
    if where == "inside":      # inside tile (1, 0), off the pixel corners
        u, v = -1.0 + 100.3 * PITCH2D, -1.0 + 37.6 * PITCH2D
    elif where == "corner":    # exactly on the four-tile corner at pixel (128, 128)
        u, v = 0.0, 0.0
    elif where == "edge":      # half a pitch inside the image's low-x edge
        u, v = -1.0 + 0.5 * PITCH2D, -1.0 + 150.25 * PITCH2D
    else:                      # outside, the disc (radius 2h) reaching in by h / 2
        u, v = -1.0 - 1.5 * h, -1.0 + 90.4 * PITCH2D
    u, v = float(f32(u)), float(f32(v))
    a = float(f32(1.25 / w0(oracle, kernel, h)[0]))
    return u, v, h, a


# ------------------------------------------------------------------------- the bar
def pitch2d(size, ext):
    """The larger of the two pixel pitches (the reference's v pitch divides by nx)."""
    return max((ext[1] - ext[0]) / size[0], (ext[3] - ext[2]) / size[0])


def pitch3d(size, ext):
    return max((ext[1] - ext[0]) / size[0], (ext[3] - ext[2]) / size[1],
               (ext[5] - ext[4]) / size[2])


def term_bound(oracle, kernel, h, a, pitch):
    """e_p: the bound on the device's error in ONE term of particle p."""
    h = np.atleast_1d(np.asarray(h, np.float64))
    a = np.atleast_1d(np.asarray(a, np.float64))
    eps = 2.0 ** -21 * (M_PITCHES * pitch + 2.0 * h)
    return np.abs(a) * w0(oracle, kernel, h) * (BETA * eps / h + ALPHA * U24)


def fixed_point_term(oracle, kernel, h, a):
    """F: the upper bound of the int64 fixed-point accumulation's own error."""
    h = np.atleast_1d(np.asarray(h, np.float64))
    return 2.0 ** -37 * h.size * np.max(np.abs(a) * w0(oracle, kernel, h))


def bar2d(oracle, s, a, kernel, size=SIZE2D, ext=EXT2D, chunk=CHUNK, deterministic=False):
    """(E, by_class): E over the exact neighbour sets, and each class's share of it."""
    e = term_bound(oracle, kernel, s["h"], a, pitch2d(size, ext))
    by_class = {}
    for k, name in enumerate(s["names"]):
        m = s["cls"] == k
        by_class[name], _ = oracle.project_scatter(s["u"][m], s["v"][m], s["h"][m], e[m], None,
                                                   size, chunk, *ext, kernel="indicator")
    E = sum(by_class.values())
    if deterministic:
        E = E + fixed_point_term(oracle, kernel, s["h"], a)
    return E, by_class


def bar3d(oracle, s, kernel, size=SIZE3D, ext=EXT3D, planes=None):
    e = term_bound(oracle, kernel, s["h"], s["a"], pitch3d(size, ext))
    by_class = {}
    for k, name in enumerate(s["names"]):
        m = s["cls"] == k
        by_class[name] = oracle.project3d(s["x"][m], s["y"][m], s["z"][m], s["h"][m], e[m], size,
                                          ext, kernel="indicator", planes=planes)
    return sum(by_class.values()), by_class


def assert_terms_close(g, r, E, by_class=None, floor=0.0):
    """g == 0 exactly where r == 0, and |g - r| <= E (+ floor, the fixed-point term where
    it is kept apart) at every pixel.  Returns the worst err / E."""
    g = np.asarray(g, np.float64)
    r = np.asarray(r, np.float64)
    E = np.asarray(E, np.float64) + floor
    assert g.shape == r.shape == E.shape, (g.shape, r.shape, E.shape)
    assert np.all(np.isfinite(g)), "non-finite pixels"
    nz = np.count_nonzero(g[r == 0])
    assert nz == 0, f"{nz} pixels that are 0 in the reference are not 0"
    err = np.abs(g - r)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / E)  # err > 0 on E == 0: inf
    if ratio.size == 0:
        return 0.0
    worst = np.unravel_index(np.argmax(ratio), ratio.shape)
    if ratio[worst] > 1.0:
        msg = (f"worst err/E = {ratio[worst]:.3g} at pixel {tuple(int(i) for i in worst)} "
               f"(g = {g[worst]:.9g}, r = {r[worst]:.9g}, E = {E[worst]:.3g}); "
               f"{np.count_nonzero(ratio > 1.0)} pixels over the bar")
        if by_class:
            share = {n: float(m[worst]) for n, m in by_class.items()}
            top = max(share, key=share.get)
            msg += (f"; E there is dominated by class {top} "
                    f"({share[top] / max(E[worst], 1e-300):.0%} of E)")
        raise AssertionError(msg)
    return float(ratio[worst])


# ---------------------------------------------------- fp64 / fp32 NumPy evaluations
def kernel_f64(kernel, r, h):
    """W(r, h) in float64 NumPy (the oracle's expressions)."""
    q = r / h
    if kernel == "cubic":
        t = 2.0 - q
        f = np.where(q < 1.0, 1.0 - 1.5 * (q * q) + 0.75 * (q * q * q),
                     np.where(q < 2.0, 0.25 * (t * t * t), 0.0))
        return f / (np.pi * h ** 3)
    t = 1.0 - 0.5 * q
    return np.where(q < 2.0, 21.0 / (16.0 * np.pi * h ** 3) * t ** 4 * (1.0 + 2.0 * q), 0.0)


def _shape_f32(kernel, q):
    """f(q) with every operation rounded to float32 (q a float32 array)."""
    one, two = np.float32(1.0), np.float32(2.0)
    if kernel == "cubic":
        q2 = q * q
        a = one - np.float32(1.5) * q2 + np.float32(0.75) * (q2 * q)
        t = two - q
        b = np.float32(0.25) * (t * t * t)
        return np.where(q < one, a, b)
    t = one - np.float32(0.5) * q
    t2 = t * t
    return (t2 * t2) * (one + two * q)


def _coef_f32(kernel, a, h):
    K = np.float32(1.0 / np.pi if kernel == "cubic" else 21.0 / (16.0 * np.pi))
    h = np.float32(h)
    return np.float32(a) * (K / (h * h * h))


def stamp_reference(oracle, kernel, u, v, h, a, size=SIZE2D, ext=EXT2D):
    """One particle on a square grid: (r, E) with r = a W(r, h) in float64 NumPy at every
    pixel the reference includes (r2 < (2h)^2 on the reference's fp64 expressions; on a
    square grid the chunk cull removes nothing from the disc) and E that particle's own
    term over the same pixels."""
    nx, ny = size
    X = ext[0] + np.arange(nx, dtype=np.float64) * ((ext[1] - ext[0]) / nx)
    Y = ext[2] + np.arange(ny, dtype=np.float64) * ((ext[3] - ext[2]) / nx)
    dx, dy = u - X[:, None], v - Y[None, :]
    r2 = dx * dx + dy * dy
    t = 2.0 * h
    inc = r2 < t * t
    r = np.where(inc, a * kernel_f64(kernel, np.sqrt(r2), h), 0.0)
    E = np.where(inc, term_bound(oracle, kernel, h, a, pitch2d(size, ext))[0], 0.0)
    return r, E


def eval_f32_2d(s, a, kernel, size=SIZE2D, ext=EXT2D, chunk=CHUNK):
    """A straightforward float32 evaluation of the map: absolute-frame dx, dy, every
    operation of a term rounded to float32, terms accumulated in float64.  The neighbour
    sets are the reference's (fp64 test and chunk cull).  Returns (map, neighbour counts)."""
    nx, ny = size
    x_min, x_max, y_min, y_max = ext
    psx, psy, psyc = (x_max - x_min) / nx, (y_max - y_min) / nx, (y_max - y_min) / ny
    X = x_min + np.arange(nx, dtype=np.float64) * psx
    Y = y_min + np.arange(ny, dtype=np.float64) * psy
    X32, Y32 = X.astype(np.float32), Y.astype(np.float32)
    i0c, j0c = (np.arange(nx) // chunk) * chunk, (np.arange(ny) // chunk) * chunk
    xlo, xhi = x_min + i0c * psx, x_min + np.minimum(i0c + chunk, nx) * psx
    ylo, yhi = y_min + j0c * psyc, y_min + np.minimum(j0c + chunk, ny) * psyc
    out = np.zeros((nx, ny))
    cnt = np.zeros((nx, ny))
    for u, v, h, ap in zip(s["u"], s["v"], s["h"], a):
        h2 = 2.0 * h
        i0 = max(0, int(np.floor((u - h2 - x_min) / psx)) - 2)
        i1 = min(nx - 1, int(np.ceil((u + h2 - x_min) / psx)) + 2)
        j0 = max(0, int(np.floor((v - h2 - y_min) / psy)) - 2)
        j1 = min(ny - 1, int(np.ceil((v + h2 - y_min) / psy)) + 2)
        if i0 > i1 or j0 > j1:
            continue
        si, sj = slice(i0, i1 + 1), slice(j0, j1 + 1)
        dx, dy = u - X[si, None], v - Y[None, sj]
        inc = (dx * dx + dy * dy) < h2 * h2
        inc &= ((u >= xlo[si] - h2) & (u < xhi[si] + h2))[:, None]
        inc &= ((v >= ylo[sj] - h2) & (v < yhi[sj] + h2))[None, :]
        dx32 = np.float32(u) - X32[si, None]
        dy32 = np.float32(v) - Y32[None, sj]
        q = np.sqrt(dx32 * dx32 + dy32 * dy32) / np.float32(h)
        term = _coef_f32(kernel, ap, h) * _shape_f32(kernel, q)
        out[si, sj] += np.where(inc, term.astype(np.float64), 0.0)
        cnt[si, sj] += inc
    return out, cnt


def eval_f32_3d(s, kernel, size=SIZE3D, ext=EXT3D):
    """The cube's counterpart of eval_f32_2d (each axis its own pitch, no cull)."""
    n = size
    lo = (ext[0], ext[2], ext[4])
    ps = [(ext[2 * d + 1] - ext[2 * d]) / n[d] for d in range(3)]
    C = [lo[d] + np.arange(n[d], dtype=np.float64) * ps[d] for d in range(3)]
    C32 = [c.astype(np.float32) for c in C]
    out = np.zeros(n)
    cnt = np.zeros(n)
    for x, y, z, h, ap in zip(s["x"], s["y"], s["z"], s["h"], s["a"]):
        h2 = 2.0 * h
        sl = []
        for d, w in enumerate((x, y, z)):
            a0 = max(0, int(np.floor((w - h2 - lo[d]) / ps[d])) - 1)
            a1 = min(n[d] - 1, int(np.ceil((w + h2 - lo[d]) / ps[d])) + 1)
            sl.append(slice(a0, a1 + 1))
        if any(q.start >= q.stop for q in sl):
            continue
        dx = x - C[0][sl[0], None, None]
        dy = y - C[1][None, sl[1], None]
        dz = z - C[2][None, None, sl[2]]
        inc = (dx * dx + dy * dy + dz * dz) < h2 * h2
        dx32 = np.float32(x) - C32[0][sl[0], None, None]
        dy32 = np.float32(y) - C32[1][None, sl[1], None]
        dz32 = np.float32(z) - C32[2][None, None, sl[2]]
        q = np.sqrt(dx32 * dx32 + dy32 * dy32 + dz32 * dz32) / np.float32(h)
        term = _coef_f32(kernel, ap, h) * _shape_f32(kernel, q)
        out[tuple(sl)] += np.where(inc, term.astype(np.float64), 0.0)
        cnt[tuple(sl)] += inc
    return out, cnt


# ------------------------------------------------------- shared references (cached)
def reference2d(oracle, kernel, size=SIZE2D):
    """The mixed set's oracle maps and bars on ``size``: r0 / r1 (a0 = a T, a1 = a),
    E0 / E1, by_class0 / by_class1, and the fixed-point terms F0 / F1."""
    def make():
        s = mixed_set(oracle, kernel)
        r0, r1 = oracle.project_scatter(s["u"], s["v"], s["h"], s["a0"], s["a"], size, CHUNK,
                                        *EXT2D, kernel=kernel)
        E0, c0 = bar2d(oracle, s, s["a0"], kernel, size)
        E1, c1 = bar2d(oracle, s, s["a"], kernel, size)
        return dict(r0=r0, r1=r1, E0=E0, E1=E1, by_class0=c0, by_class1=c1,
                    F0=fixed_point_term(oracle, kernel, s["h"], s["a0"]),
                    F1=fixed_point_term(oracle, kernel, s["h"], s["a"]))
    return _cached(("ref2d", kernel, size), make)


def reference3d(oracle, kernel):
    def make():
        s = cube_set(oracle, kernel)
        r = oracle.project3d(s["x"], s["y"], s["z"], s["h"], s["a"], SIZE3D, EXT3D, kernel=kernel)
        E, c = bar3d(oracle, s, kernel)
        return dict(r=r, E=E, by_class=c)
    return _cached(("ref3d", kernel), make)


def class_map2d(oracle, s, a, kernel, k, size=SIZE2D):
    m = s["cls"] == k
    return oracle.project_scatter(s["u"][m], s["v"][m], s["h"][m], np.asarray(a)[m], None, size,
                                  CHUNK, *EXT2D, kernel=kernel)[0]


def class_map3d(oracle, s, kernel, k):
    m = s["cls"] == k
    return oracle.project3d(s["x"][m], s["y"][m], s["z"][m], s["h"][m], s["a"][m], SIZE3D, EXT3D,
                            kernel=kernel)
