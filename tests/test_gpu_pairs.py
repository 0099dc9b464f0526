"""The kernel_func plug-in's pair lists (asp_pairs_begin / _emit / _end, kernel k_pairs)
against the NumPy reference of tests/pairs_ref.py, PAIR BY PAIR and through the C-ABI:
the CSR layout, the empty slots outside the image, tile_pairs, every (pixel, particle) pair
and the bits of every r2.  Nothing here has a tolerance.

A summed map (the test_plugin_* tests of tests/test_gpu_parity.py) cannot see a wrong
particle index with the right r2, a pair in the neighbouring pixel where the callable is
flat, an r2 taken from the fp32 working copies, a duplicate cancelled by a dropped pair or
a wrong tile_pairs; these comparisons can.  The cases reach the code of the session that
the square G3 fixture does not: the wide loop and the second record stream of k_pairs,
split tiles, non-square grids and mixed axis spellings, windows far from the origin, the
window loop of images above 4096 tiles with its re-bins, device pointers on a caller's
stream, negative / zero / NaN particles and the argument checks.

The reference itself is held to the oracle on the CPU by tests/test_pairs_ref.py.
"""
import ctypes as C

import numpy as np
import pytest

import pairs_cases as pc
import pairs_ref as pr
import value_bar as vb
from test_gpu_path_values import THRESHOLDS, _knobs

pytestmark = pytest.mark.gpu


class Session:
    """One asp_pairs session through ctypes.  Host arrays, or (``device_ptrs``) torch CUDA
    tensors for the inputs and the emit outputs, ordered on ``stream``."""

    def __init__(self, pos, h, axis, size, chunk, ext, device_ptrs=False, stream=None):
        from asp_amd import _lib
        self.lib, self.L = _lib, _lib.lib()
        self.size = (int(size[0]), int(size[1]))
        self.ntx, self.nty = -(-self.size[0] // pr.TILE), -(-self.size[1] // pr.TILE)
        self.ntiles = self.ntx * self.nty
        self.tile_pairs = np.full(self.ntiles, -1, np.int64)
        self.dev = device_ptrs
        self._keep = (pos, h)
        self.handle = C.c_void_p()
        n = 0 if h is None else int(h.shape[0])
        flags = _lib.ASP_F_DEVICE_PTRS if device_ptrs else 0
        rc = self.L.asp_pairs_begin(_lib.ptr(pos, _lib._d), _lib.ptr(h, _lib._d), n, int(axis),
                                    *(float(e) for e in ext), *self.size, int(chunk), flags, 0,
                                    stream, _lib.ptr(self.tile_pairs, _lib._i64),
                                    C.byref(self.handle))
        assert rc == _lib.ASP_OK, self.L.asp_last_error()
        assert self.handle

    @classmethod
    def of(cls, case, **kw):
        return cls(case["pos"], case["h"], case["axis"], case["size"], case["chunk"], case["ext"],
                   **kw)

    def emit_raw(self, t0, t1, offsets, particle, r2):
        p = self.lib.ptr
        return self.L.asp_pairs_emit(self.handle, t0, t1, p(offsets, self.lib._i64),
                                     p(particle, self.lib._i32), p(r2, self.lib._d))

    def emit(self, t0, t1):
        """The decoded pairs of tiles [t0, t1)."""
        tot = int(self.tile_pairs[t0:t1].sum())
        nslots = (t1 - t0) * pr.TILE_PIX
        if self.dev:
            import torch
            offsets = torch.full((nslots + 1,), -7, dtype=torch.int64, device="cuda")
            part = torch.full((max(tot, 1),), -7, dtype=torch.int32, device="cuda")
            r2 = torch.full((max(tot, 1),), -7.0, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
        else:
            offsets = np.full(nslots + 1, -7, np.int64)
            part = np.full(max(tot, 1), -7, np.int32)
            r2 = np.full(max(tot, 1), -7.0)
        rc = self.emit_raw(t0, t1, offsets, part, r2)
        assert rc == self.lib.ASP_OK, self.L.asp_last_error()
        if self.dev:
            offsets, part, r2 = (t.cpu().numpy() for t in (offsets, part, r2))
        return pr.decode_emit(offsets, part[:tot], r2[:tot], t0, t1, self.nty, self.size,
                              self.tile_pairs)

    def close(self):
        if self.handle:
            assert self.L.asp_pairs_end(self.handle) == self.lib.ASP_OK
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):  # (closed in the with statement's implicit finally)
        self.close()


def _check_session(S, ref, ranges):
    assert np.array_equal(S.tile_pairs, pr.tile_counts(ref, S.size)), "tile_pairs"
    first = None
    for t0, t1 in ranges:
        got = S.emit(t0, t1)
        pr.assert_pairs_equal(got, ref)
        first = first or got
    return first


def _fold(emit):
    nx, ny = emit.size
    return np.bincount(emit.pixel, minlength=nx * ny).reshape(nx, ny)


def _native_counts(c):
    """The native indicator map of the case (asp_project2d_f64) and its stats."""
    from asp_amd.device import project2d_f64, stats
    cnt, _ = project2d_f64(c["pos"], c["h"], np.ones(c["h"].size), projection_axis=c["axes"],
                           image_size=c["size"], extent=c["ext"], chunk_size=c["chunk"],
                           kernel="indicator")
    return cnt, stats(0)


# ------------------------------------------------------------------ a. paths, square
@pytest.mark.parametrize("thresholds", list(THRESHOLDS))
@pytest.mark.parametrize("window", [None, "box"])
def test_paths_square(gpu, oracle, monkeypatch, window, thresholds):
    """The mixed set on 256 x 256 under the three threshold settings, with the h40-120
    class wide: all 16 tiles in one emit, as the ranges [0,1) [1,7) [7,7) [7,16) and tile by
    tile.  The session publishes no stats: a native indicator map under the same
    environment shows that the wide path, split tiles and (or not) the large stream ran,
    and equals the emitted per-pixel counts."""
    _knobs(monkeypatch, THRESHOLDS[thresholds], vb.WIDE_TILES)
    c = pc.mixed_case(oracle, window)
    ref = pc.reference(("mixed", window, c["size"], c["chunk"]), c)
    with Session.of(c) as S:
        assert S.ntiles == 16
        whole = _check_session(S, ref, [(0, 16)])
        _check_session(S, ref, [(0, 1), (1, 7), (7, 7), (7, 16)])
        _check_session(S, ref, [(t, t + 1) for t in range(16)])
    cnt, st = _native_counts(c)
    assert st["wide"] > 0, st
    assert st["merges"] > 0, st  # the clump's tile is split over several items
    assert (st["large"] == 0) == (thresholds == "sweep_all"), st
    assert np.array_equal(cnt.astype(np.int64), _fold(whole))


# --------------------------------------------- b. non-square and partial tiles (+ d)
def _nonsquare(oracle, window, size, chunk):
    if size == (200, 150):  # with the edge particles of case d mixed in
        return pc.edge_case(oracle, window, chunk), ("edge", window, chunk)
    return pc.mixed_case(oracle, window, size, chunk), ("mixed", window, size, chunk)


@pytest.mark.parametrize("window", [None, "box"])
@pytest.mark.parametrize("size,chunk", pc.NONSQUARE, ids=lambda s: str(s).replace(" ", ""))
def test_nonsquare_and_partial_tiles(gpu, oracle, monkeypatch, window, size, chunk):
    """192 x 256 (chunk 64) and 200 x 150 (chunks 32 and 7: the v cull's own pitch cuts the
    candidate boxes, partial tiles on both axes), at the origin and on the box window."""
    _knobs(monkeypatch, None, vb.WIDE_TILES)
    c, key = _nonsquare(oracle, window, size, chunk)
    ref = pc.reference(key, c)
    with Session.of(c) as S:
        whole = _check_session(S, ref, [(0, S.ntiles)])
        _check_session(S, ref, [(t, t + 1) for t in range(S.ntiles)])
    cnt, _ = _native_counts(c)
    assert np.array_equal(cnt.astype(np.int64), _fold(whole))


# ------------------------------------------------------------- c. mixed axis spellings
@pytest.mark.parametrize("name", pc.SPELLINGS)
def test_mixed_axis_spellings(gpu, oracle, monkeypatch, name):
    """axis | ASP_AXIS_CULL(c): the cull reads other columns than the pixel test (see
    pairs_cases.spelling_case).  The cull removes at least 5 % of the unculled pairs and
    keeps at least half, so a session culling on the pixel's own columns, or not at all,
    fails."""
    _knobs(monkeypatch, None, vb.WIDE_TILES)
    c = pc.spelling_case(oracle, name)
    ref = pc.reference(("spelling", name), c)
    free = pc.unculled_reference(name, c)
    assert 0.5 * free.pixel.size <= ref.pixel.size <= 0.95 * free.pixel.size
    assert c["axis"] >> 4  # a mixed spelling
    with Session.of(c) as S:
        whole = _check_session(S, ref, [(0, S.ntiles), (2, 9), (9, S.ntiles)])
    cnt, _ = _native_counts(c)
    assert np.array_equal(cnt.astype(np.int64), _fold(whole))


# ---------------------------------------------------------------- d. edge particles
@pytest.mark.parametrize("window", [None, "box"])
def test_edge_particles(gpu, oracle, monkeypatch, window):
    """Negative h (every 50th), h == 0, a NaN coordinate, a NaN h, a particle outside the
    image, one on the last pixel's corner: the particles without pairs in the reference
    have none on the device, the negated ones keep theirs."""
    _knobs(monkeypatch, None, vb.WIDE_TILES)
    c = pc.edge_case(oracle, window, 32)
    ref = pc.reference(("edge", window, 32), c)
    sp = c["special"]
    assert np.isin(sp["negated"], ref.particle).sum() >= 10
    assert sp["last_corner"] in ref.particle[ref.pixel == 200 * 150 - 1]
    with Session.of(c) as S:
        got = _check_session(S, ref, [(0, S.ntiles)])
    for k in ("zero_h", "nan_u", "nan_h", "outside"):
        assert sp[k] not in ref.particle and sp[k] not in got.particle, k
    neg = np.isin(got.particle, sp["negated"])
    assert np.array_equal(got.particle[neg], ref.particle[np.isin(ref.particle, sp["negated"])])


def test_boundary_set(gpu, oracle):
    """test_boundary_pairs_exact's 20 000 particles at 2h +- 0-4 ulp from pixel corners
    (64 x 64, chunk 8): its particle lists and the bits of r2, not only its counts."""
    c = pc.boundary_case()
    ref = pc.reference(("boundary",), c)
    with Session.of(c) as S:
        _check_session(S, ref, [(0, 1)])


# ------------------------------------------------- e. a window far from the origin
def test_far_negative_window(gpu, oracle, monkeypatch):
    """|corner| / pitch ~ 4e6: the candidate boxes grow by several pixels, no pair may be
    gained or lost, and r2 keeps the bits of the reference's absolute-frame expression."""
    for name in ("ASP_GATHER_MIN", "ASP_GATHER_AREA", "ASP_WIDE_TILES"):
        monkeypatch.delenv(name, raising=False)
    c = pc.mixed_case(oracle, "far_negative")
    ref = pc.reference(("mixed", "far_negative", c["size"], c["chunk"]), c)
    assert ref.pixel.size > 500_000
    with Session.of(c) as S:
        _check_session(S, ref, [(0, 16)])


# ------------------------------------------- f. device pointers on a side stream
def test_device_pointers_on_a_side_stream(gpu, oracle, monkeypatch):
    """ASP_F_DEVICE_PTRS: positions / h and the emit outputs are CUDA tensors, the session
    runs on a non-default stream, and an unrelated native projection on the default stream
    runs between two emits (the session owns its buffers)."""
    import torch
    from asp_amd.device import project2d
    _knobs(monkeypatch, None, vb.WIDE_TILES)
    c = pc.mixed_case(oracle, None)
    ref = pc.reference(("mixed", None, c["size"], c["chunk"]), c)
    pos = torch.tensor(c["pos"], dtype=torch.float64, device="cuda")
    h = torch.tensor(c["h"], dtype=torch.float64, device="cuda")
    f32 = [torch.tensor(c[k], dtype=torch.float32, device="cuda") for k in ("u", "v", "h")]
    ones = torch.ones_like(f32[0])
    kw = dict(image_size=c["size"], extent=c["ext"], chunk_size=c["chunk"], kernel="indicator")
    before, _ = project2d(*f32, ones, **kw)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    assert side.cuda_stream != torch.cuda.default_stream().cuda_stream
    with Session(pos, h, c["axis"], c["size"], c["chunk"], c["ext"], device_ptrs=True,
                 stream=side.cuda_stream) as S:
        _check_session(S, ref, [(0, 7)])
        between, _ = project2d(*f32, ones, **kw)
        _check_session(S, ref, [(7, 16), (0, 16)])
        torch.cuda.synchronize()
        assert torch.equal(before, between)


@pytest.mark.parametrize("device_ptrs", [False, True], ids=["host", "device"])
def test_no_particles(gpu, device_ptrs):
    """n == 0 in both pointer modes: tile_pairs and offsets all zero, NULL positions / h
    and NULL particle / r2 accepted."""
    with Session(None, None, 2, (96, 80), 32, (-1.0, 1.0, -1.0, 1.0),
                 device_ptrs=device_ptrs) as S:
        assert S.ntiles == 4 and not S.tile_pairs.any()
        nslots = 4 * pr.TILE_PIX
        if device_ptrs:
            import torch
            offsets = torch.full((nslots + 1,), -7, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
        else:
            offsets = np.full(nslots + 1, -7, np.int64)
        assert S.emit_raw(0, 4, offsets, None, None) == S.lib.ASP_OK, S.L.asp_last_error()
        if device_ptrs:
            offsets = offsets.cpu().numpy()
        assert not offsets.any()


# ------------------------------------------- g. more than 4096 tiles: the window seam
def test_window_seam(gpu, monkeypatch):
    """4160 x 4160 = 65 x 65 tiles: windows of 63 tile rows, the seam at image row 4032.
    tile_pairs of all 4225 tiles, then emits that walk the window loop: a range in the
    second window, one in the first (a re-bin backwards), one across the seam (the base
    carried from one window's launch to the next), and the first again, bit-equal to its
    first emission."""
    monkeypatch.delenv("ASP_GATHER_MIN", raising=False)
    monkeypatch.delenv("ASP_GATHER_AREA", raising=False)
    monkeypatch.setenv("ASP_WIDE_TILES", pc.SEAM_WIDE_TILES)
    c = pc.seam_case()
    ref = pc.reference(("seam",), c)
    nty = 65
    second, first, across = (63 * nty + 2, 63 * nty + 52), (62 * nty + 2, 62 * nty + 52), \
        (62 * nty, 64 * nty)
    # what the case must contain, from the reference alone
    rows = ref.pixel // c["size"][1]
    tiles = pr.tile_of(ref.pixel, c["size"])
    assert (rows < pc.SEAM_ROW).any() and (rows >= pc.SEAM_ROW).any()
    for a, b in (second, first, across):
        assert ((tiles >= a) & (tiles < b)).sum() > 1000, (a, b)
    straddlers = 0
    for p in range(24):  # the h = 30 pitches particles placed at the seam
        m = ref.particle == p
        lo, hi = m & (rows < pc.SEAM_ROW), m & (rows >= pc.SEAM_ROW)
        # over more than ASP_WIDE_TILES tiles of one window: wide there, whatever its box
        wide = max(np.unique(tiles[lo]).size, np.unique(tiles[hi]).size) > int(pc.SEAM_WIDE_TILES)
        straddlers += bool(wide and lo.any() and hi.any())
    assert straddlers >= 8, straddlers
    with Session.of(c) as S:
        assert S.ntiles == 4225
        want = pr.tile_counts(ref, c["size"])
        assert np.array_equal(S.tile_pairs, want), np.nonzero(S.tile_pairs != want)[0][:8]
        one = S.emit(*second)
        pr.assert_pairs_equal(one, ref)
        pr.assert_pairs_equal(S.emit(*first), ref)
        pr.assert_pairs_equal(S.emit(*across), ref)
        again = S.emit(*second)
        pr.assert_pairs_equal(again, ref)
        assert np.array_equal(one.offsets, again.offsets)
        assert np.array_equal(one.particle, again.particle)
        assert np.array_equal(one.r2.view(np.uint64), again.r2.view(np.uint64))


# -------------------------------------------------------------- h. argument errors
def test_argument_errors(gpu, oracle):
    from asp_amd import _lib
    L = _lib.lib()
    INVALID = _lib.ASP_ERR_INVALID
    c = pc.boundary_case()  # one tile, all of it with pairs
    ref = pc.reference(("boundary",), c)
    assert L.asp_pairs_end(None) == _lib.ASP_OK
    off = np.zeros(pr.TILE_PIX + 1, np.int64)
    assert L.asp_pairs_emit(None, 0, 1, _lib.ptr(off, _lib._i64), None, None) == INVALID
    with Session.of(c) as S:
        tot = int(S.tile_pairs.sum())
        assert S.ntiles == 1 and tot > 0
        part, r2 = np.zeros(tot, np.int32), np.zeros(tot)
        for t0, t1 in ((-1, 1), (0, 2), (1, 0)):
            assert S.emit_raw(t0, t1, off, part, r2) == INVALID, (t0, t1)
            assert L.asp_last_error()
        assert S.emit_raw(0, 1, None, part, r2) == INVALID
        assert S.emit_raw(0, 1, off, None, r2) == INVALID
        assert S.emit_raw(0, 1, off, part, None) == INVALID
        assert not off.any() and not part.any() and not r2.any()  # nothing was written
        # an empty range needs no pair arrays, and the session is still usable
        one = np.full(1, -7, np.int64)
        assert S.emit_raw(1, 1, one, None, None) == _lib.ASP_OK and one[0] == 0
        _check_session(S, ref, [(0, 1)])


# --------------------------------------- 4. the host wrapper off the square fixture
def _ones(r, h):
    return np.ones_like(r)


def _cubic(r, hh):  # the NumPy cubic of test_plugin_matches_native_kernels
    q = r / hh
    w = np.where(q < 1.0, 1 - 1.5 * q ** 2 + 0.75 * q ** 3,
                 np.where(q < 2.0, 0.25 * (2 - q) ** 3, 0.0))
    return w / (np.pi * hh ** 3)


@pytest.mark.parametrize("mode,axis", [("per_pixel", 2), ("batch", 2), ("batch", "x")],
                         ids=["per_pixel-z", "batch-z", "batch-strx"])
def test_wrapper_off_the_square_fixture(gpu, oracle, mode, axis):
    """create_image(..., kernel_func=<callable>) at 96 x 80, chunk 32 (2 x 2 tiles, none
    whole), per pixel and in batches, axis 2 and the str "x" (culls on (x, y), measures on
    (y, z)): integer ids under a callable of ones are exact sums, compared with
    array_equal; the NumPy cubic within test_plugin_matches_native_kernels' own bar."""
    from asp_amd._axes import reference_axes
    from asp_amd.tools.projections import create_image
    s = pc.wrapper_set()
    pos, h, ids = s["pos"], s["h"], s["ids"]
    size, cs, ext = pc.WRAPPER_SIZE, pc.WRAPPER_CHUNK, pc.WRAPPER_EXT
    axes = reference_axes(axis)
    assert axes == ((0, 2) if axis == "x" else (2, 2))
    want = oracle.create_image(pos, h, ids, size, cs, axes, *ext, kernel="indicator")
    assert np.count_nonzero(want) > 1000 and want.max() < 2 ** 53
    img = create_image(pos, h, ids, size, cs, axis, *ext, kernel_func=_ones,
                       kernel_func_mode=mode)
    assert img.shape == size and np.array_equal(img, want)
    A = np.linspace(0.5, 1.5, h.size)
    want = oracle.create_image(pos, h, A, size, cs, axes, *ext, kernel="cubic")
    img = create_image(pos, h, A, size, cs, axis, *ext, kernel_func=_cubic,
                       kernel_func_mode=mode)
    np.testing.assert_allclose(img, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
    assert np.array_equal(img != 0, want != 0)
