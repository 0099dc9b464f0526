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

* The bar has no term in |u| or |corner|: DESIGN §3 claims the pair error is 2^-24 of the
  pair distance.  WINDOWS puts the same sets at zoom windows 1e5 .. 1e7 pitches from the
  origin to test exactly that; for the raw-fp64 entry points F64_INPUT_ULPS (derived where
  it is defined) covers the device's own rounding of h and a.

* A call of several pipeline passes (windows, batches) widens the bar by the pass rule
  (PASS_STORES, ``with_passes``); a ratio map is held to the ratio rule
  (RATIO_TAIL_SHARE, ``assert_ratio_close``).  Both are derived where they are defined.

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

# Offset windows: zoom maps far from the origin, (name, ext) on SIZE2D with
# chunk CHUNK.  The sets keep their LOCAL positions -- the same rng draws, class table,
# clump and stamp positions, in pixel pitches from the window's corner -- mapped as
# x_min + local_pitches * pitch, then rounded to fp32 for the fp32 entry points and kept
# raw for the fp64 ones.  The bar is the same: it has no |corner| term.
#   box          corners and pitch (2^-14) exact in fp32, |corner| / pitch = 1.1e6; fp32
#                positions near 67 lie on a 2^-17 lattice, 1/8 pitch (1/64 pitch in v)
#   box_offgrid  neither the corners nor the pitch are fp32-representable
#   far_negative pitch 2^-12; fp32 positions near -1000 lie on a 2^-14 lattice, 1/4 pitch
#                in u, while v in [0, 2^-4) is fine-grained (2^-28 or finer, <= 2^-16
#                pitch): |u| is large and negative, v near 0, so mg is asymmetric
WINDOWS = (("box", (67.25, 67.25 + 2.0 ** -6, 12.5, 12.5 + 2.0 ** -6)),
           ("box_offgrid", (67.3, 67.3157, 12.1, 12.1157)),
           ("far_negative", (-1000.5, -1000.5 + 2.0 ** -4, 0.0, 2.0 ** -4)))
WINDOW_NAMES = tuple(w[0] for w in WINDOWS)
CUBE_SHIFT = (67.25, 12.5, 331.0)  # the cube's offset: EXT3D moved by it (corners exact)

# The raw-fp64 entry points (asp_project2d_f64 / _props_f64): r is the oracle on the raw
# fp64 arrays, and the device additionally rounds h and a to fp32 once each (k_to_f32,
# round to nearest: relative error <= 2^-24 = 1 u each) before term_coef / kernel_norm64
# and the shapes read them.  In units of u = 2^-24 of |a| W(0):
#   - a -> fl32(a): the coefficient is linear in a                              1 u
#   - h -> fl32(h) through the coefficient a K / h^3 (kernel_norm64 cubes it)   3 u
#   - h -> fl32(h) through q = r / h: a relative error u of q moves f by
#     q |f'(q)| u, max q |f'(q)| = 0.79 (see ALPHA)                          0.79 u
# 4.79 u, taken as 5.  No coordinate term: the local coordinates are formed from the
# resident fp64 positions (src_u / src_v) and rounded once, which eps_p already holds.
F64_INPUT_ULPS = 5.0

# Pass seams: a 2-D map call is a loop of pipeline passes -- WINDOWS of whole
# tile rows where the image has more than 4096 GPU tiles, particle BATCHES where the array
# exceeds one pass.  The strip makes the window seam cheap: nty = 1 and ntx = 4104, so
# window 0 is rows [0, 262144) with exactly 4096 tiles, window 1 the last 512 rows, the seam
# at row STRIP_SEAM, and every particle lies within a few hundred rows of it.  The pixels
# are square (equal u and v extents: the v pitch divides by nx); the image is not, so the
# chunk cull is active as on SIZE2D_NONSQUARE.
#   strip_grid     corners k 2^-10 <= 256.5, all exact in fp32 (the seam at u = 256.0)
#   strip_offgrid  neither the corners nor the pitch are fp32-representable
STRIP_SEAM = 262144
STRIP_SIZE = (STRIP_SEAM + 512, 16)
STRIP_WIDE_TILES = "2"  # ASP_WIDE_TILES: the strip's wide class alone meets > 2 tiles
STRIPS = (("strip_grid", (0.0, STRIP_SIZE[0] * 2.0 ** -10, 0.0, STRIP_SIZE[0] * 2.0 ** -10)),
          ("strip_offgrid", (-3.3, 253.9157, 0.7, 257.9157)))
STRIP_NAMES = tuple(w[0] for w in STRIPS)
# The strip's classes: CLASSES_2D with u within +-384 pitches of the seam and v in [-4, 20)
# pitches, but the wide class at h = 90 .. 120 pitches within +-40 pitches of the seam:
# 2h - 40 >= 140 pitches, so each of them reaches three tiles on either side; the clump as
# CLUMP, sigma = 2 pitches about (STRIP_SEAM, 8).
STRIP_WIDE = ("h90-120", 90.0, 120.0, 12)
STRIP_CLASSES = CLASSES_2D[:-1] + (STRIP_WIDE,)
STRIP_REACH, STRIP_WIDE_REACH = 384.0, 40.0
# No footprint reaches below row STRIP_SEAM - 384 - 24 (wide: - 40 - 240), so the strip's
# references keep rows [STRIP_LO, nx) only; strip_crop asserts that the rest is 0.
STRIP_LO = STRIP_SEAM - 512

# Pass rule.  A call of P passes gets extra_ulps = 3 (P - 1) in term_bound: within a pass a
# pixel is stored at most three times (by the deposit, by the merge of a split tile, by the
# wide path; gather_emit and the merges always accumulate), passes after the first add to
# the fp32 map, and each store rounds a partial sum bounded by sum |a_p| W(0, h_p) over the
# pixel's included particles -- the sum extra_ulps multiplies.  Nothing of it is measured.
PASS_STORES = 3.0

# Ratio rule (ratio=True: q = g0 / g1 formed in fp32 from the stored components).  With
# g = r + d, |d| <= E and w = r0 / r1:
#   |g0 / g1 - w| = |d0 r1 - r0 d1| / (r1 (r1 + d1)) <= (E0 + |w| E1) / (r1 - E1),
# plus the division's rounding 2^-24 |q| <= 2^-23 |w|, wherever r1 > 2 E1 (so r1 - E1 >
# r1 / 2); q == 0 exactly where r1 == 0.  Pixels with 0 < r1 <= 2 E1 see kernel tails only:
# their quotient has no relative precision and is required to be finite; at most
# RATIO_TAIL_SHARE of the covered pixels may be of that kind, which is asserted of the
# reference alone (ratio_tail_share).
RATIO_TAIL_SHARE = 0.02

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


def window_ext(window):
    """The extent of a window of WINDOWS by name (None: EXT2D)."""
    return EXT2D if window is None else dict(WINDOWS)[window]


def _placer(window):
    """(place_u, place_v, pitch): maps of the sets' EXT2D coordinates into the window --
    the identity for None, else x_min + local_pitches * pitch with local_pitches =
    (w + 1) / PITCH2D -- and the pitch the h classes are scaled with."""
    if window is None:
        return (lambda w: w), (lambda w: w), PITCH2D
    ext = window_ext(window)
    psx, psy = (ext[1] - ext[0]) / SIZE2D[0], (ext[3] - ext[2]) / SIZE2D[0]
    return ((lambda w: ext[0] + ((np.asarray(w) + 1.0) / PITCH2D) * psx),
            (lambda w: ext[2] + ((np.asarray(w) + 1.0) / PITCH2D) * psy), max(psx, psy))


def mixed_set(oracle, kernel, window=None, raw=False):
    """The 2-D mixed set: every class of CLASSES_2D uniform in the extent plus the clump.
    Keys u, v, h, a, T, a0 (= fl32(a T)), cls (class index), names.  ``window``: the same
    local positions and h (in pixel pitches) at that window of WINDOWS.  ``raw``: nothing is
    rounded to fp32 (the inputs of the fp64 entry points; a = U(0.5, 1.5) / W(0, h) on the
    raw h, a0 = a T)."""
    def make():
        pu, pv, pitch = _placer(window)
        rnd = (lambda t: np.asarray(t, np.float64)) if raw else f32
        rng = np.random.default_rng(20)
        u, v, h, cls = [], [], [], []
        for k, (_, lo, hi, n) in enumerate(CLASSES_2D + (CLUMP,)):
            if k < len(CLASSES_2D):
                u.append(pu(rng.uniform(-1.0, 1.0, n)))
                v.append(pv(rng.uniform(-1.0, 1.0, n)))
            else:
                u.append(pu(rng.normal(CLUMP_CENTRE[0], 2 * PITCH2D, n)))
                v.append(pv(rng.normal(CLUMP_CENTRE[1], 2 * PITCH2D, n)))
            h.append(rng.uniform(lo, hi, n) * pitch)
            cls.append(np.full(n, k))
        u, v, h = (rnd(np.concatenate(t)) for t in (u, v, h))
        a = rnd(rng.uniform(0.5, 1.5, h.size) / w0(oracle, kernel, h))
        T = rnd(rng.uniform(1.0, 3.0, h.size))
        return dict(u=u, v=v, h=h, a=a, T=T, a0=rnd(a * T), cls=np.concatenate(cls),
                    names=[c[0] for c in CLASSES_2D + (CLUMP,)])
    key = ("mixed", kernel) if window is None and not raw else ("mixed", kernel, window, raw)
    return _cached(key, make)


def strip_ext(name):
    return dict(STRIPS)[name]


def strip_set(oracle, kernel, name, raw=False):
    """The seam set on the strip ``name`` of STRIPS: STRIP_CLASSES about the seam plus the
    clump on it.  Keys, amplitudes (equal peaks, T, a0 = fl32(a T)) and ``raw`` as
    mixed_set; lu, lv are the positions in pixel pitches from the corner, before rounding."""
    def make():
        ext = strip_ext(name)
        psx, psy = (ext[1] - ext[0]) / STRIP_SIZE[0], (ext[3] - ext[2]) / STRIP_SIZE[0]
        pitch = max(psx, psy)
        rnd = (lambda t: np.asarray(t, np.float64)) if raw else f32
        rng = np.random.default_rng(24)
        lu, lv, h, cls = [], [], [], []
        for k, (cname, lo, hi, n) in enumerate(STRIP_CLASSES + (CLUMP,)):
            if k < len(STRIP_CLASSES):
                reach = STRIP_WIDE_REACH if cname == STRIP_WIDE[0] else STRIP_REACH
                lu.append(STRIP_SEAM + rng.uniform(-reach, reach, n))
                lv.append(rng.uniform(-4.0, 20.0, n))
            else:
                lu.append(rng.normal(STRIP_SEAM, 2.0, n))
                lv.append(rng.normal(8.0, 2.0, n))
            h.append(rng.uniform(lo, hi, n) * pitch)
            cls.append(np.full(n, k))
        lu, lv = np.concatenate(lu), np.concatenate(lv)
        u, v, h = rnd(ext[0] + lu * psx), rnd(ext[2] + lv * psy), rnd(np.concatenate(h))
        a = rnd(rng.uniform(0.5, 1.5, h.size) / w0(oracle, kernel, h))
        T = rnd(rng.uniform(1.0, 3.0, h.size))
        return dict(u=u, v=v, h=h, a=a, T=T, a0=rnd(a * T), cls=np.concatenate(cls), lu=lu, lv=lv,
                    names=[c[0] for c in STRIP_CLASSES + (CLUMP,)])
    return _cached(("strip", kernel, name, raw), make)


def cube_ext(shift=None):
    """EXT3D moved by ``shift`` = (sx, sy, sz)."""
    if shift is None:
        return EXT3D
    return tuple(EXT3D[i] + shift[i // 2] for i in range(6))


def cube_set(oracle, kernel, shift=None):
    """The cube set: positions uniform in +-2.2 (footprints clipped at the faces, some
    missing the cube).  Keys x, y, z, h, a, cls, names.  ``shift``: the same draws moved by
    (sx, sy, sz), fp32-rounded after the shift."""
    def make():
        rng = np.random.default_rng(21)
        h, cls = [], []
        for k, (_, lo, hi, n) in enumerate(CLASSES_3D):
            h.append(rng.uniform(lo, hi, n) * PITCH3D)
            cls.append(np.full(n, k))
        h = f32(np.concatenate(h))
        sh = (0.0, 0.0, 0.0) if shift is None else shift
        x, y, z = (f32(rng.uniform(-2.2, 2.2, h.size) + sh[d]) for d in range(3))
        a = f32(rng.uniform(0.5, 1.5, h.size) / w0(oracle, kernel, h))
        return dict(x=x, y=y, z=z, h=h, a=a, cls=np.concatenate(cls),
                    names=[c[0] for c in CLASSES_3D])
    return _cached(("cube", kernel) if shift is None else ("cube", kernel, tuple(shift)), make)


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


def stamp_particle(oracle, kernel, h_px, where, window=None):
    """(u, v, h, a) of one stamp, all fp32-representable.  ``window``: the same position in
    pixel pitches from that window's corner."""
    if window is not None:
        ext = window_ext(window)
        psx, psy = (ext[1] - ext[0]) / SIZE2D[0], (ext[3] - ext[2]) / SIZE2D[0]
        h = float(f32(h_px * max(psx, psy)))
        lu, lv = {"inside": (100.3, 37.6), "corner": (128.0, 128.0), "edge": (0.5, 150.25),
                  "outside": (None, 90.4)}[where]
        u = ext[0] - 1.5 * h if lu is None else ext[0] + lu * psx
        u, v = float(f32(u)), float(f32(ext[2] + lv * psy))
        a = float(f32(1.25 / w0(oracle, kernel, h)[0]))
        return u, v, h, a
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


def term_bound(oracle, kernel, h, a, pitch, extra_ulps=0.0):
    """e_p: the bound on the device's error in ONE term of particle p.  ``extra_ulps``:
    F64_INPUT_ULPS where the device rounds raw fp64 h and a to fp32 itself."""
    h = np.atleast_1d(np.asarray(h, np.float64))
    a = np.atleast_1d(np.asarray(a, np.float64))
    eps = 2.0 ** -21 * (M_PITCHES * pitch + 2.0 * h)
    return np.abs(a) * w0(oracle, kernel, h) * (BETA * eps / h + (ALPHA + extra_ulps) * U24)


def fixed_point_term(oracle, kernel, h, a):
    """F: the upper bound of the int64 fixed-point accumulation's own error."""
    h = np.atleast_1d(np.asarray(h, np.float64))
    return 2.0 ** -37 * h.size * np.max(np.abs(a) * w0(oracle, kernel, h))


def bar2d(oracle, s, a, kernel, size=SIZE2D, ext=EXT2D, chunk=CHUNK, deterministic=False,
          extra_ulps=0.0):
    """(E, by_class): E over the exact neighbour sets, and each class's share of it."""
    e = term_bound(oracle, kernel, s["h"], a, pitch2d(size, ext), extra_ulps)
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


def pass_ulps(passes):
    """The pass rule's extra_ulps for a call of ``passes`` pipeline passes."""
    assert passes >= 1
    return PASS_STORES * (passes - 1)


def peak_sum2d(oracle, s, a, kernel, size=SIZE2D, ext=EXT2D, chunk=CHUNK):
    """S(pixel) = sum |a_p| W(0, h_p) over the pixel's included particles: what one ulp of
    extra_ulps weighs, E(extra_ulps = x) = E(0) + x 2^-24 S (term_bound is linear in it)."""
    return oracle.project_scatter(s["u"], s["v"], s["h"], np.abs(a) * w0(oracle, kernel, s["h"]),
                                  None, size, chunk, *ext, kernel="indicator")[0]


def peak_sum3d(oracle, s, kernel, size=SIZE3D, ext=EXT3D):
    return oracle.project3d(s["x"], s["y"], s["z"], s["h"],
                            np.abs(s["a"]) * w0(oracle, kernel, s["h"]), size, ext,
                            kernel="indicator")


def with_passes(E, S, passes):
    """The bar E of one pass widened by the pass rule."""
    return E + pass_ulps(passes) * U24 * S


def strip_crop(full, row_lo=0):
    """Rows [STRIP_LO, nx) of a strip map whose first row is image row ``row_lo``; the rows
    before them must be 0 (no footprint of the seam set reaches them)."""
    full = np.asarray(full)
    k = STRIP_LO - row_lo
    assert not full[:k].any(), "pixels below STRIP_LO are not 0"
    return np.array(full[k:], np.float64)


def strip_scatter(oracle, s, a0, a1, kernel, ext):
    """The oracle's strip maps of (a0[, a1]), cropped (strip_crop)."""
    o0, o1 = oracle.project_scatter(s["u"], s["v"], s["h"], a0, a1, STRIP_SIZE, CHUNK, *ext,
                                    kernel=kernel)
    return strip_crop(o0), None if o1 is None else strip_crop(o1)


def strip_bar(oracle, s, a, kernel, ext, extra_ulps=0.0):
    """bar2d on the strip, cropped: (E, by_class)."""
    E, by_class = bar2d(oracle, s, a, kernel, STRIP_SIZE, ext, extra_ulps=extra_ulps)
    return strip_crop(E), {n: strip_crop(m) for n, m in by_class.items()}


def ratio_tail_share(r1, E1):
    """The share of the covered pixels (r1 > 0) the ratio rule only requires to be finite."""
    covered = np.count_nonzero(r1 > 0)
    return np.count_nonzero((r1 > 0) & (r1 <= 2.0 * E1)) / max(covered, 1)


def assert_ratio_close(q, r0, r1, E0, E1):
    """The ratio rule (see RATIO_TAIL_SHARE): q == 0 exactly where r1 == 0, |q - r0 / r1| <=
    (E0 + |w| E1) / (r1 - E1) + 2^-23 |w| where r1 > 2 E1, finite elsewhere, and the
    reference's own share of such pixels within RATIO_TAIL_SHARE.  Returns the worst
    err / bar."""
    q = np.asarray(q, np.float64)
    assert q.shape == r0.shape == r1.shape == E0.shape == E1.shape
    assert np.all(r1 >= 0.0), "the ratio rule is stated for non-negative weights"
    assert np.all(np.isfinite(q)), "non-finite pixels"
    share = ratio_tail_share(r1, E1)
    assert share <= RATIO_TAIL_SHARE, f"{share:.2%} of the covered pixels are kernel tails"
    nz = np.count_nonzero(q[r1 == 0])
    assert nz == 0, f"{nz} pixels without weight are not 0"
    ok = r1 > 2.0 * E1
    w = r0[ok] / r1[ok]
    bar = (E0[ok] + np.abs(w) * E1[ok]) / (r1[ok] - E1[ok]) + 2.0 ** -23 * np.abs(w)
    err = np.abs(q[ok] - w)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bar)
    if ratio.size == 0:
        return 0.0
    k = int(np.argmax(ratio))
    if ratio[k] > 1.0:
        pix = tuple(int(i[k]) for i in np.nonzero(ok))
        raise AssertionError(f"worst err/E = {ratio[k]:.3g} at pixel {pix} (q = {q[ok][k]:.9g}, "
                             f"r0 / r1 = {w[k]:.9g}, bar = {bar[k]:.3g}); "
                             f"{np.count_nonzero(ratio > 1.0)} pixels over the ratio bar")
    return float(ratio[k])


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


def _edge_shape_f32(kernel, q, tau):
    """The edge-continuous form of f(q) (edge_shape2) in float32 with the dead
    zone tau: t = clamp(1 - q/2), t^2 <- max(t t - tau^2, 0); cubic 2 (t^2 t - s^3 / 2)
    with s = clamp(1 - q), Wendland (t^2)^2 (1 + 2q)."""
    zero, one, two, half = (np.float32(c) for c in (0.0, 1.0, 2.0, 0.5))
    tau = np.float32(tau)
    t = np.clip(one - half * q, zero, one)
    t2 = np.maximum(t * t - tau * tau, zero)
    if kernel == "cubic":
        sq = np.clip(one - q, zero, one)
        return two * (t2 * t - half * (sq * sq * sq))
    return (t2 * t2) * (one + two * q)


def dead_zone_tau(M, h):
    """tau of a record's dead zone from its decision band, in float32 as the device forms
    it (rec_thr / rec_band / edge_dead2): band / (2 thr) + 2^-20, with M the bound on the
    coordinates of the frame the band is taken for.  0 where the device leaves it off."""
    M, h = np.float32(M), np.asarray(h, np.float32)
    Da = np.abs(np.float32(2.0) * h)
    eps = np.float32(2.0 ** -21) * (M + Da)
    band = (np.float32(4.0) * Da * eps + np.float32(2.0) * eps * eps
            + np.float32(2.0 ** -20) * Da * Da)
    thr = Da * Da
    lo, hi = thr - band, thr + band
    tau = np.float32(0.5) * (hi - lo) / (hi + lo) + np.float32(2.0 ** -20)
    return np.where(tau < np.float32(2.0 ** -4), tau, np.float32(0.0)).astype(np.float32)


def frame_bounds(size, ext, tile=64):
    """(mg, mgl) as the host sets them: the bound on |corner coordinate| in the absolute
    frame, and in the records' local frames (2 tiles of the larger pitch)."""
    nx, ny = size
    psx, psy = (ext[1] - ext[0]) / nx, (ext[3] - ext[2]) / nx
    mgl = 2.0 * tile * max(psx, psy)
    mg = max(abs(ext[0]), abs(ext[0] + nx * psx), abs(ext[2]), abs(ext[2] + ny * psy), mgl)
    return mg * (1.0 + 1e-6), mgl * (1.0 + 1e-6)


def eval_f32_local_2d(s, a, kernel, size=SIZE2D, ext=EXT2D, chunk=CHUNK, taus=(None,), tile=64):
    """The device's arithmetic in float32 NumPy: every pair in a LOCAL frame.  Per 64-pixel
    tile, dx = fl32(u - X_tile_origin), formed in fp64 and rounded once, minus
    fl32(k pitch), k the pixel's index within the tile; the rest as eval_f32_2d (fp32
    operations, fp64 accumulation, the reference's neighbour sets).  One map per entry of
    ``taus``: None is the plain shape, an array of per-particle tau (dead_zone_tau) the
    edge-continuous form with that dead zone.  Returns (maps, neighbour counts)."""
    nx, ny = size
    x_min, x_max, y_min, y_max = ext
    psx, psy, psyc = (x_max - x_min) / nx, (y_max - y_min) / nx, (y_max - y_min) / ny
    ix, iy = np.arange(nx), np.arange(ny)
    X = x_min + ix * psx
    Y = y_min + iy * psy
    X0, Y0 = X[(ix // tile) * tile], Y[(iy // tile) * tile]  # each pixel's tile origin
    offx = ((ix % tile) * psx).astype(np.float32)
    offy = ((iy % tile) * psy).astype(np.float32)
    i0c, j0c = (ix // chunk) * chunk, (iy // chunk) * chunk
    xlo, xhi = x_min + i0c * psx, x_min + np.minimum(i0c + chunk, nx) * psx
    ylo, yhi = y_min + j0c * psyc, y_min + np.minimum(j0c + chunk, ny) * psyc
    outs = [np.zeros((nx, ny)) for _ in taus]
    cnt = np.zeros((nx, ny))
    for p, (u, v, h, ap) in enumerate(zip(s["u"], s["v"], s["h"], a)):
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
        dx32 = ((u - X0[si]).astype(np.float32) - offx[si])[:, None]
        dy32 = ((v - Y0[sj]).astype(np.float32) - offy[sj])[None, :]
        q = np.sqrt(dx32 * dx32 + dy32 * dy32) / np.float32(h)
        coef = _coef_f32(kernel, ap, h)
        for out, tau in zip(outs, taus):
            f = _shape_f32(kernel, q) if tau is None else _edge_shape_f32(kernel, q, tau[p])
            out[si, sj] += np.where(inc, (coef * f).astype(np.float64), 0.0)
        cnt[si, sj] += inc
    return outs, cnt


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
def reference2d(oracle, kernel, size=SIZE2D, window=None, raw=False):
    """The mixed set's oracle maps and bars on ``size``: r0 / r1 (a0 = a T, a1 = a),
    E0 / E1, by_class0 / by_class1, the fixed-point terms F0 / F1 and the neighbour counts
    cnt.  ``window`` / ``raw``: as mixed_set; the raw set's bar carries F64_INPUT_ULPS."""
    def make():
        s = mixed_set(oracle, kernel, window, raw)
        ext = window_ext(window)
        extra = F64_INPUT_ULPS if raw else 0.0
        r0, r1 = oracle.project_scatter(s["u"], s["v"], s["h"], s["a0"], s["a"], size, CHUNK,
                                        *ext, kernel=kernel)
        E0, c0 = bar2d(oracle, s, s["a0"], kernel, size, ext, extra_ulps=extra)
        E1, c1 = bar2d(oracle, s, s["a"], kernel, size, ext, extra_ulps=extra)
        cnt, _ = oracle.project_scatter(s["u"], s["v"], s["h"], np.ones(s["h"].size), None, size,
                                        CHUNK, *ext, kernel="indicator")
        return dict(r0=r0, r1=r1, E0=E0, E1=E1, by_class0=c0, by_class1=c1, cnt=cnt,
                    S0=peak_sum2d(oracle, s, s["a0"], kernel, size, ext),
                    S1=peak_sum2d(oracle, s, s["a"], kernel, size, ext),
                    F0=fixed_point_term(oracle, kernel, s["h"], s["a0"]),
                    F1=fixed_point_term(oracle, kernel, s["h"], s["a"]))
    key = ("ref2d", kernel, size) if window is None and not raw else \
        ("ref2d", kernel, size, window, raw)
    return _cached(key, make)


def strip_reference(oracle, kernel, name, raw=False):
    """reference2d for strip_set on the strip ``name``, every map cropped to the rows from
    STRIP_LO on (strip_crop): r0 / r1, E0 / E1, by_class0 / by_class1, the pass rule's S0 /
    S1 (peak_sum2d), F0 / F1 and the neighbour counts cnt."""
    def make():
        s = strip_set(oracle, kernel, name, raw)
        ext = strip_ext(name)
        extra = F64_INPUT_ULPS if raw else 0.0
        r0, r1 = strip_scatter(oracle, s, s["a0"], s["a"], kernel, ext)
        E0, c0 = strip_bar(oracle, s, s["a0"], kernel, ext, extra)
        E1, c1 = strip_bar(oracle, s, s["a"], kernel, ext, extra)
        cnt, _ = strip_scatter(oracle, s, np.ones(s["h"].size), None, "indicator", ext)
        return dict(r0=r0, r1=r1, E0=E0, E1=E1, by_class0=c0, by_class1=c1, cnt=cnt,
                    S0=strip_crop(peak_sum2d(oracle, s, s["a0"], kernel, STRIP_SIZE, ext)),
                    S1=strip_crop(peak_sum2d(oracle, s, s["a"], kernel, STRIP_SIZE, ext)),
                    F0=fixed_point_term(oracle, kernel, s["h"], s["a0"]),
                    F1=fixed_point_term(oracle, kernel, s["h"], s["a"]))
    return _cached(("strip_ref", kernel, name, raw), make)


def reference3d(oracle, kernel, shift=None):
    def make():
        s = cube_set(oracle, kernel, shift)
        ext = cube_ext(shift)
        r = oracle.project3d(s["x"], s["y"], s["z"], s["h"], s["a"], SIZE3D, ext, kernel=kernel)
        E, c = bar3d(oracle, s, kernel, ext=ext)
        return dict(r=r, E=E, by_class=c, S=peak_sum3d(oracle, s, kernel, ext=ext))
    return _cached(("ref3d", kernel) if shift is None else ("ref3d", kernel, tuple(shift)), make)


def class_map2d(oracle, s, a, kernel, k, size=SIZE2D, ext=EXT2D):
    m = s["cls"] == k
    return oracle.project_scatter(s["u"][m], s["v"][m], s["h"][m], np.asarray(a)[m], None, size,
                                  CHUNK, *ext, kernel=kernel)[0]


def class_map3d(oracle, s, kernel, k):
    m = s["cls"] == k
    return oracle.project3d(s["x"][m], s["y"][m], s["z"][m], s["h"][m], s["a"][m], SIZE3D, EXT3D,
                            kernel=kernel)
