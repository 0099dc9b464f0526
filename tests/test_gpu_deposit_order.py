"""K4's bank-balanced record order ("LDS bank conflicts in K4"): every wave of
``k_deposit`` takes contiguous pools of 128 records of its item (8 waves: 1024 records per
round of the workgroup), orders each pool by the LDS bank pair of the records' base words
and loads the records by index, 64 per batch (the two-map instantiations; one map keeps
lane t = record base + t, and both are run here).  Every record must still be deposited
exactly once, whatever the item's length and however the bank pairs fall.

One 128 x 128 image of unit pitch (positions in pixels, all fp32-exact), chunk 64: four
64 x 64 tiles.  Pixel-scale particles (h 0.5 .. 1.0 px) placed in [6, 58)^2 give tile
(0, 0) exactly one record each and the other tiles none, which ``stats()`` confirms.

Checks, per case: the indicator kernel's neighbour counts are bit-exact against the oracle
(a record dropped or deposited twice shows there); the values of both kernels, one and two
maps, fp64 and deterministic sums, lie within the per-pixel bar of tests/value_bar.py; two
deterministic calls are bitwise equal.

Split tiles (``it.slab >= 0``, merged by ``k_merge``) are reachable here: a tile's
small/mid stream splits above 2048 records, so N = 2049 and 4097 run 2 and 3 items.
"""
import numpy as np
import pytest

import value_bar as vb

pytestmark = pytest.mark.gpu

SIZE = (128, 128)
EXT = (0.0, 128.0, 0.0, 128.0)
CHUNK = 64
SWEEP_ALL = ("65", str(1 << 30))  # no large stream: k_deposit sweeps every box wider than 4

# one below, at and one above: the batch (64), the pool (128), two and four pools, the
# workgroup's round (8 pools = 1024), the item split (2048), and two splits
COUNTS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047,
          2048, 2049, 4097)


def _dev(*arrs):
    import torch
    return [torch.tensor(np.asarray(a), dtype=torch.float32, device="cuda") for a in arrs]


def _host(t):
    return t.cpu().numpy().astype(np.float64)


def _knobs(monkeypatch, thresholds=None):
    for name in ("ASP_GATHER_MIN", "ASP_GATHER_AREA", "ASP_WIDE_TILES", "ASP_COUNT_EVALS"):
        monkeypatch.delenv(name, raising=False)
    if thresholds is not None:
        monkeypatch.setenv("ASP_GATHER_MIN", thresholds[0])
        monkeypatch.setenv("ASP_GATHER_AREA", thresholds[1])


def _amplitudes(oracle, kernel, h, rng):
    a = vb.f32(rng.uniform(0.5, 1.5, h.size) / vb.w0(oracle, kernel, h))
    T = vb.f32(rng.uniform(1.0, 3.0, h.size))
    return a, vb.f32(a * T)


def _set(u, v, h, cls=None, names=("all",)):
    u, v, h = (vb.f32(np.asarray(t, np.float64)) for t in (u, v, h))
    return dict(u=u, v=v, h=h, cls=np.zeros(h.size, int) if cls is None else np.asarray(cls),
                names=list(names))


def _check_set(oracle, s, size=SIZE, ext=EXT, expect=None, label=""):
    """The set ``s`` through every instantiation of k_deposit that project2d reaches: the
    indicator counts bit-exact, both kernels x one / two maps x fp64 / deterministic within
    the bar, deterministic calls bitwise equal.  ``expect``: what stats() must show."""
    from asp_amd.device import project2d, stats
    u, v, h = _dev(s["u"], s["v"], s["h"])
    kw = dict(image_size=size, extent=ext, chunk_size=CHUNK)
    ones = np.ones(s["h"].size)
    want, _ = oracle.project_scatter(s["u"], s["v"], s["h"], ones, None, size, CHUNK, *ext,
                                     kernel="indicator")
    for det in (False, True):
        cnt, _ = project2d(u, v, h, _dev(ones)[0], kernel="indicator", deterministic=det, **kw)
        st = stats(0)
        for key, val in (expect or {}).items():
            assert st[key] == val, (key, st)
        assert np.array_equal(_host(cnt), want), \
            f"{label}: neighbour counts differ at {np.count_nonzero(_host(cnt) != want)} pixels"
    worst = 0.0
    for kernel in vb.KERNELS:
        a1, a0 = _amplitudes(oracle, kernel, s["h"], np.random.default_rng(5))
        r0, r1 = oracle.project_scatter(s["u"], s["v"], s["h"], a0, a1, size, CHUNK, *ext,
                                        kernel=kernel)
        E0, c0 = vb.bar2d(oracle, s, a0, kernel, size, ext, CHUNK)
        E1, c1 = vb.bar2d(oracle, s, a1, kernel, size, ext, CHUNK)
        F0 = vb.fixed_point_term(oracle, kernel, s["h"], a0)
        F1 = vb.fixed_point_term(oracle, kernel, s["h"], a1)
        d0, d1 = _dev(a0, a1)
        for det in (False, True):
            g, _ = project2d(u, v, h, d1, kernel=kernel, deterministic=det, **kw)
            w = vb.assert_terms_close(_host(g), r1, E1, c1, floor=F1 if det else 0.0)
            g0, g1 = project2d(u, v, h, d0, d1, kernel=kernel, deterministic=det, **kw)
            w0 = vb.assert_terms_close(_host(g0), r0, E0, c0, floor=F0 if det else 0.0)
            w1 = vb.assert_terms_close(_host(g1), r1, E1, c1, floor=F1 if det else 0.0)
            worst = max(worst, w, w0, w1)
            if det:
                h0, h1 = project2d(u, v, h, d0, d1, kernel=kernel, deterministic=True, **kw)
                assert np.array_equal(_host(h0), _host(g0)) and np.array_equal(_host(h1), _host(g1))
                assert np.array_equal(_host(h1), _host(g)), "one map and two maps differ"
    print(f"VALUE_BAR deposit order {label}: worst err/E = {worst:.3f}")


def _uniform(n, seed):
    rng = np.random.default_rng(seed)
    return _set(rng.uniform(6.0, 58.0, n), rng.uniform(6.0, 58.0, n), rng.uniform(0.5, 1.0, n))


@pytest.mark.parametrize("n", COUNTS)
def test_item_lengths(gpu, oracle, monkeypatch, n):
    """N records in one tile, N over the batch, pool, round and split edges."""
    _knobs(monkeypatch)
    items = 3 + (n + 2047) // 2048  # the other three tiles are one empty item each
    _check_set(oracle, _uniform(n, 100 + n),
               expect=dict(records=n, items=items, wide=0, large=0, merges=int(n > 2048)),
               label=f"N = {n}")


@pytest.mark.parametrize("n", (65, 129, 300, 1025))
def test_one_bank_pair_one_pixel(gpu, oracle, monkeypatch, n):
    """All N particles in one pixel: every record has the same base word, so a pool is one
    bank pair with up to 128 records (more than the 64 levels of the per-level table)."""
    _knobs(monkeypatch)
    rng = np.random.default_rng(n)
    s = _set(20.0 + rng.uniform(0.3, 0.7, n), 30.0 + rng.uniform(0.3, 0.7, n),
             rng.uniform(0.55, 0.7, n))
    _check_set(oracle, s, expect=dict(records=n, wide=0, large=0), label=f"one pixel, N = {n}")


@pytest.mark.parametrize("n", (65, 129, 300, 1025))
def test_one_bank_pair_many_words(gpu, oracle, monkeypatch, n):
    """Base words stepping by 16: x0 + y0 = const (mod 16), so one bank pair, different
    words."""
    _knobs(monkeypatch)
    rng = np.random.default_rng(1000 + n)
    i = rng.integers(0, 40, n)
    m = rng.integers(0, 3, n)
    u = 8.0 + i + rng.uniform(0.4, 0.6, n)
    v = 8.0 + ((-i) % 16) + 16 * m + rng.uniform(0.4, 0.6, n)
    s = _set(u, v, np.full(n, 0.625))
    # the box origin of every record: floor(u - 2h) + 1, floor(v - 2h) + 1
    x0 = np.floor(s["u"] - 2 * s["h"]) + 1
    y0 = np.floor(s["v"] - 2 * s["h"]) + 1
    assert np.unique((x0 + y0) % 16).size == 1
    _check_set(oracle, s, expect=dict(records=n, wide=0, large=0), label=f"step 16, N = {n}")


def test_mixed_item(gpu, oracle, monkeypatch):
    """One tile holding 3 x 3 records, 4-wide records (deferred), records with a pixel corner
    at exactly 2h from the particle (r2 == thr: in the error band, deferred, excluded by the
    strict <) and mid-size records swept by a whole wave, in shuffled order."""
    from asp_amd.device import project2d, stats
    _knobs(monkeypatch, SWEEP_ALL)
    rng = np.random.default_rng(7)
    n3, n4, nb, nm = 700, 300, 100, 60
    u = [rng.uniform(8.0, 56.0, n3), rng.uniform(8.0, 56.0, n4)]
    v = [rng.uniform(8.0, 56.0, n3), rng.uniform(8.0, 56.0, n4)]
    h = [rng.uniform(0.5, 0.7, n3), rng.uniform(0.95, 1.05, n4)]
    # band: h = 0.625 (2h = 1.25 exact), the particle 1.25 px from a pixel corner along x
    u.append(rng.integers(10, 50, nb) + 1.25)
    v.append(rng.integers(10, 50, nb).astype(np.float64))
    h.append(np.full(nb, 0.625))
    u.append(rng.uniform(16.0, 48.0, nm))
    v.append(rng.uniform(16.0, 48.0, nm))
    h.append(rng.uniform(2.0, 4.0, nm))
    cls = np.concatenate([np.full(k, c) for c, k in enumerate((n3, n4, nb, nm))])
    order = rng.permutation(cls.size)
    s = _set(np.concatenate(u)[order], np.concatenate(v)[order], np.concatenate(h)[order],
             cls[order], ("3x3", "4x4", "band", "mid"))
    n = cls.size
    _check_set(oracle, s, expect=dict(records=n, wide=0, large=0), label="mixed item")
    # both bodies ran: the small records alone are at most 16 lane-slots each
    monkeypatch.setenv("ASP_COUNT_EVALS", "1")
    project2d(*_dev(s["u"], s["v"], s["h"], np.ones(n)), kernel="cubic", image_size=SIZE,
              extent=EXT, chunk_size=CHUNK)
    st = stats(0)
    assert st["evals_gather"] == 0 and st["evals_wide"] == 0, st
    assert 9 * n3 <= st["evals_small"], st
    assert st["evals_small"] >= 9 * n3 + 64 * nm, st  # every mid record: >= one wave pass


def test_image_edge_and_empty_tile(gpu, oracle, monkeypatch):
    """100 x 100: partial tiles (TW, TH = 36) full of records, tile (0, 1) with none."""
    _knobs(monkeypatch)
    size, ext = (100, 100), (0.0, 100.0, 0.0, 100.0)
    rng = np.random.default_rng(11)
    parts = []
    for (ulo, uhi, vlo, vhi, n) in ((1.0, 63.0, 1.0, 63.0, 900),      # tile (0, 0), to its edges
                                    (64.0, 101.0, 0.0, 63.0, 600),    # tile (1, 0), over the edge
                                    (66.0, 101.0, 66.0, 101.0, 400)):  # tile (1, 1), the corner
        parts.append((rng.uniform(ulo, uhi, n), rng.uniform(vlo, vhi, n), rng.uniform(0.5, 1.0, n)))
    # tile (0, 1) = rows 0..63, columns 64..99 stays empty: a disc that can reach a row
    # below 64 (u < 66) is kept off the columns from 64 on (v + 2h <= 63.5)
    u, v, h = (np.concatenate(t) for t in zip(*parts))
    v = np.where(u < 66.0, np.minimum(v, 61.5), v)
    s = _set(u, v, h)
    want, _ = oracle.project_scatter(s["u"], s["v"], s["h"], np.ones(h.size), None, size, CHUNK,
                                     *ext, kernel="indicator")
    assert want[:64, 64:].sum() == 0 and want[:64, :64].sum() > 0  # empty next to full
    _check_set(oracle, s, size=size, ext=ext, expect=dict(wide=0, large=0), label="100 x 100")


@pytest.mark.parametrize("k", (4, 6))
def test_ext_passes(gpu, oracle, monkeypatch, k):
    """project2d_props with 4 and 6 properties: EXT passes 1 (and 2) load the coefficients
    ``ext[start + idx]`` with the permuted record index."""
    from asp_amd.device import project2d_props, stats
    _knobs(monkeypatch)
    n = 1500
    s = _uniform(n, 77)
    rng = np.random.default_rng(78)
    for kernel in vb.KERNELS:
        base = vb.f32(rng.uniform(0.5, 1.5, n) / vb.w0(oracle, kernel, s["h"]))
        props = [vb.f32(base * rng.uniform(-1.0 if j % 2 else 0.5, 1.5, n)) for j in range(k)]
        outs = project2d_props(*_dev(s["u"], s["v"], s["h"]), _dev(*props), image_size=SIZE,
                               extent=EXT, chunk_size=CHUNK, kernel=kernel)
        st = stats(0)
        assert st["records"] == n and st["large"] == 0 and st["wide"] == 0, st
        for j, (p, o) in enumerate(zip(props, outs)):
            r, _ = oracle.project_scatter(s["u"], s["v"], s["h"], p, None, SIZE, CHUNK, *EXT,
                                          kernel=kernel)
            E, by_class = vb.bar2d(oracle, s, p, kernel, SIZE, EXT, CHUNK)
            w = vb.assert_terms_close(_host(o), r, E, by_class)
            print(f"VALUE_BAR deposit order props k = {k} {kernel} map {j}: worst err/E = {w:.3f}")
