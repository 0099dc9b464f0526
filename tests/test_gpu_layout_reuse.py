"""Layout reuse of the 2-D map: a map of the particle set the previous map
binned skips the count pass and the scans, scatters into the previous layout and lets the
scatter prove that the layout is exact for the arrays' present contents.

The reference of every case is the same call with ``ASP_REUSE_LAYOUT=0`` in the same
process.  Bars:

* deterministic maps (int64 fixed point) are associative sums: bit-identical, whatever the
  order of the particles and of the records (``torch.equal``);
* neighbour counts (indicator kernel, unit property) are sums of ones below 2^24: exact;
* fp64-accumulated maps are the fp32 roundings of fp64 sums of the SAME fp32 terms in
  another order.  The terms here are positive, so two such sums differ by at most
  n 2^-53 of the sum (n <= 5e4 terms: 2^-37), and their roundings by at most one fp32 ulp:
  |g - r| <= 2^-23 |r|; pixels that are 0 are 0 in both;
* a ratio map is a quotient of two such components, divided in fp32 or in fp64 and rounded
  once: each component carries 2^-24, the division and the store 2^-24 each, on either
  side, so |g - r| <= 8 * 2^-24 |r| = 2^-21 |r|.

Sizes: 50 000 Plummer particles (49 count batches, 7 count workgroups, 2 scatter
workgroups, so the per-workgroup runs the proof compares exist) on 256^2 (16 tiles).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G = 256
EXT = (-4.0, 4.0, -4.0, 4.0)
N = 50_000
KW = dict(image_size=(G, G), extent=EXT)


@pytest.fixture
def fresh(gpu):
    """Every test starts without a layout: the workspaces are released."""
    from asp_amd import _lib
    _lib.check(_lib.lib().asp_release(0))
    yield
    _lib.check(_lib.lib().asp_release(0))


def _set(seed=11, law="pixel", n=N):
    from asp_amd.plummer import plummer_torch
    d = plummer_torch(n, seed=seed, h_law=law, extent=4.0, grid=G, device="cuda")
    return d["x"], d["y"], d["h"], (d["m"] * d["T"]).contiguous(), d["m"]


def _reuse():
    from asp_amd.device import stats
    return stats(0)["layout_reuse"]


def _off(monkeypatch, call):
    """The reference: ``call`` with reuse switched off (a counted pass)."""
    monkeypatch.setenv("ASP_REUSE_LAYOUT", "0")
    try:
        out = call()
        assert _reuse() == 0
    finally:
        monkeypatch.delenv("ASP_REUSE_LAYOUT")
    return out


def _same(a, b):
    import torch
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def _close(g, r, ulps):
    g = g.double().cpu().numpy()
    r = r.double().cpu().numpy()
    assert np.array_equal(g == 0, r == 0)
    assert np.all(np.abs(g - r) <= ulps * 2.0 ** -24 * np.abs(r)), \
        float(np.max(np.abs(g - r) / np.maximum(np.abs(r), 1e-300))) / 2.0 ** -24


def _arm(call):
    """Call until the layout is reused (a failed attempt disarms reuse, and two counted
    passes with equal counters re-arm it: at most four calls)."""
    for _ in range(4):
        out = call()
        if _reuse() == 1:
            return out
    raise AssertionError("the layout was never reused")


def test_second_call_reuses_the_layout(fresh, monkeypatch):
    from asp_amd.device import project2d, stats
    s = _set()
    call = lambda: project2d(*s, kernel="cubic", deterministic=True, **KW)  # noqa: E731
    first = call()
    assert _reuse() == 0
    second = call()
    st = stats(0)
    assert st["layout_reuse"] == 1 and st["scatter_path"] == 1, st
    assert st["records"] > N and st["items"] >= 16 and st["records_per_item"] > 0, st
    assert _same(second, first)
    assert _same(second, _off(monkeypatch, call))
    third = call()  # the switched-off pass left a layout as well
    assert _reuse() == 1 and _same(third, first)


def test_properties_kernel_and_flags_share_the_layout(fresh, monkeypatch):
    import torch
    from asp_amd.device import project2d
    x, y, h, a0, a1 = _set()
    project2d(x, y, h, a0, a1, kernel="cubic", deterministic=True, **KW)
    b0, b1 = (a0 * 3.0).contiguous(), torch.ones_like(a1)
    calls = (
        lambda: project2d(x, y, h, b0, b1, kernel="cubic", deterministic=True, **KW),
        lambda: project2d(x, y, h, b0, b1, kernel="wendland_c2", deterministic=True, **KW),
        lambda: project2d(x, y, h, b0, kernel="cubic_column", deterministic=True, **KW),
        lambda: project2d(x, y, h, torch.ones_like(h), kernel="indicator", **KW),
    )
    got = []
    for call in calls:
        got.append(call())
        assert _reuse() == 1
    for call, g in zip(calls, got):
        assert _same(g, _off(monkeypatch, call))
    # fp64 sums and the ratio map (the bars of the module docstring)
    plain = lambda: project2d(x, y, h, a0, a1, kernel="cubic", **KW)  # noqa: E731
    ratio = lambda: project2d(x, y, h, a0, a1, kernel="cubic", ratio=True, **KW)  # noqa: E731
    g = plain()
    assert _reuse() == 1
    q = ratio()
    assert _reuse() == 1
    r = _off(monkeypatch, plain)
    _close(g[0], r[0], 2)
    _close(g[1], r[1], 2)
    rq = _off(monkeypatch, ratio)
    _close(q[0], rq[0], 8)
    _close(q[1], rq[1], 2)


def test_in_place_permutation_is_detected(fresh, monkeypatch):
    """The same particles in another order: every tile total and every counter is the
    same, the runs of the two scatter workgroups are not."""
    from asp_amd.device import project2d, stats
    s = _set()
    call = lambda: project2d(*s, kernel="cubic", deterministic=True, **KW)  # noqa: E731
    first = call()
    before = stats(0)
    call()
    assert _reuse() == 1
    for t in s:
        t.copy_(t.flip(0))
    third = call()
    st = stats(0)
    assert st["layout_reuse"] == 2, st
    for k in ("records", "items", "wide", "merges", "slabs", "large", "records_per_item"):
        assert st[k] == before[k], k
    assert _same(third, first)  # fixed-point sums do not depend on the order
    fourth = call()
    assert _reuse() == 0  # disarmed: counted
    fifth = call()
    assert _reuse() == 1  # equal counters re-armed it
    ref = _off(monkeypatch, call)
    assert _same(third, ref) and _same(fourth, ref) and _same(fifth, ref)


def test_overflowing_runs_stay_inside_the_buffers(fresh, monkeypatch):
    """Positions rewritten in place so that every particle falls into ONE tile -- the last
    of the record buffer's order, whose run the old layout made a few records long -- and
    back: both are detected and nothing is stored outside the buffers; maps, neighbour
    counts and accumulated maps are the counted pass's."""
    import torch
    from asp_amd.device import project2d
    x, y, h, a0, a1 = _set()
    x0, y0 = x.clone(), y.clone()
    ones = torch.ones_like(h)
    base0 = torch.rand(G, G, device=x.device)
    base1 = torch.rand(G, G, device=x.device)
    kinds = {
        "map": lambda: project2d(x, y, h, a0, a1, kernel="cubic", deterministic=True, **KW),
        "count": lambda: project2d(x, y, h, ones, kernel="indicator", **KW),
        "accumulate": lambda: project2d(x, y, h, a0, a1, kernel="cubic", deterministic=True,
                                        accumulate=True, out0=base0.clone(),
                                        out1=base1.clone(), **KW),
    }

    def one_tile():
        x.fill_(3.0)
        y.fill_(3.0)

    def spread():
        x.copy_(x0)
        y.copy_(y0)

    for kind, call in kinds.items():
        for change in (one_tile, spread):
            _arm(kinds["map"])
            change()
            got = call()
            assert _reuse() == 2, (kind, change.__name__)
            assert _same(got, _off(monkeypatch, call)), (kind, change.__name__)
    one_tile()
    cnt, _ = kinds["count"]()
    assert float(cnt.max()) == N and float(cnt.sum()) > 0  # every particle on every pixel it meets
    spread()


def test_physical_h_wide_and_large_records(fresh, monkeypatch):
    import torch
    from asp_amd.device import project2d, stats
    monkeypatch.setenv("ASP_WIDE_TILES", "4")
    x, y, h, a0, a1 = _set(seed=12, law="physical")
    call = lambda: project2d(x, y, h, a0, a1, kernel="wendland_c2", deterministic=True, **KW)  # noqa: E731
    first = call()
    st = stats(0)
    assert st["wide"] > 0 and st["large"] > 0, st
    second = call()
    st2 = stats(0)
    assert st2["layout_reuse"] == 1 and st2["wide"] == st["wide"] and st2["large"] == st["large"]
    assert _same(second, first) and _same(second, _off(monkeypatch, call))
    _arm(call)
    # one wide particle (the largest h well inside the image) shrunk to a pixel: one wide
    # particle fewer, one record more
    inside = (x.abs() < 2.0) & (y.abs() < 2.0)
    k = int(torch.argmax(torch.where(inside, h, torch.zeros_like(h))))
    assert float(h[k]) * 4.0 * G / 8.0 > 3 * 64  # its disc spans more than 4 tiles
    h[k] = 0.75 * 8.0 / G
    third = call()
    st3 = stats(0)
    assert st3["layout_reuse"] == 2 and st3["wide"] == st["wide"] - 1, st3
    assert _same(third, _off(monkeypatch, call))


def test_another_key_is_not_reused(fresh):
    from asp_amd.device import project2d
    x, y, h, a0, a1 = _set()
    kw = dict(kernel="cubic", deterministic=True)
    base = lambda: project2d(x, y, h, a0, a1, **kw, **KW)  # noqa: E731
    others = (
        lambda: project2d(x[:40_000], y[:40_000], h[:40_000], a0[:40_000], a1[:40_000], **kw, **KW),
        lambda: project2d(x, y, h, a0, a1, image_size=(G, G), extent=(-4.0, 4.0, -4.0, 3.5), **kw),
        lambda: project2d(x, y, h, a0, a1, image_size=(128, 128), extent=EXT, **kw),
        lambda: project2d(x, y, h, a0, a1, rows=(0, 128), **kw, **KW),
        lambda: project2d(x, y, h, a0, a1, chunk_size=32, **kw, **KW),
    )
    for other in others:
        base()
        other()
        assert _reuse() == 0
        other()
        assert _reuse() == 1
        base()
        assert _reuse() == 0


def test_other_users_of_the_workspace(fresh, monkeypatch):
    import torch
    from asp_amd.device import project2d, project2d_props, project3d
    from asp_amd.sightlines import sightline_columns
    from asp_amd.tools.projections import create_image
    x, y, h, a0, a1 = _set()
    call = lambda: project2d(x, y, h, a0, a1, kernel="cubic", deterministic=True, **KW)  # noqa: E731
    ref = _off(monkeypatch, call)
    z = torch.zeros_like(x)
    pos = torch.stack((x, y, z), 1).double().cpu().numpy()[:4000]
    hh = h.double().cpu().numpy()[:4000]
    A = np.ones(4000)
    pts = np.random.default_rng(3).uniform(-1.0, 1.0, (64, 2))

    def plugin_ones(r, hs):
        return np.ones_like(r)

    between = {
        "cube": lambda: project3d(x, y, z, h, a1, cube_size=(32, 32, 32), extent=EXT + (-4.0, 4.0)),
        "sample2d": lambda: sightline_columns(pos, hh, A, pts, 2),
        "plugin": lambda: create_image(pos, hh, A, (G, G), 64, 2, *EXT, kernel_func=plugin_ones),
        "props": lambda: project2d_props(x, y, h, [a0, a1, a1], kernel="cubic", **KW),
    }
    for name, other in between.items():
        _arm(call)
        other()
        got = call()
        assert _reuse() in (0, 1), name
        assert _same(got, ref), name


def test_two_streams_keep_their_own_layouts(fresh, monkeypatch):
    import torch
    from asp_amd.device import project2d
    sets = (_set(seed=21), _set(seed=22, n=60_000))
    kw = dict(kernel="cubic", deterministic=True, **KW)
    ref = [_off(monkeypatch, lambda s=s: project2d(*s, **kw)) for s in sets]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in sets]
    outs, reused = [], []
    for k in range(8):
        with torch.cuda.stream(streams[k % 2]):
            outs.append(project2d(*sets[k % 2], **kw))
            reused.append(_reuse())
    torch.cuda.synchronize()
    assert reused[2:] == [1] * 6, reused
    for k, o in enumerate(outs):
        assert _same(o, ref[k % 2]), k


def test_fp64_entry_point(fresh, monkeypatch):
    import torch
    from asp_amd.device import project2d_f64
    x, y, h, a0, a1 = _set()
    pos = torch.stack((x, y, torch.zeros_like(x)), 1).double().contiguous()
    hd, b0, b1 = h.double(), a0.double(), a1.double()
    det = lambda: project2d_f64(pos, hd, b0, b1, kernel="cubic", deterministic=True, **KW)  # noqa: E731
    plain = lambda: project2d_f64(pos, hd, b0, b1, kernel="cubic", **KW)  # noqa: E731
    first = det()
    assert _reuse() == 0
    second = det()
    assert _reuse() == 1 and _same(second, first)
    g = plain()
    assert _reuse() == 1
    r = _off(monkeypatch, plain)
    _close(g[0], r[0], 2)
    _close(g[1], r[1], 2)
    _arm(det)
    pos.copy_(pos.flip(0))  # positions alone: other particles carry these h, a0, a1 now
    third = det()
    assert _reuse() == 2
    assert _same(third, _off(monkeypatch, det))
