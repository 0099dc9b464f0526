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

Rewrites in place (the tests from ``test_slack_set_is_binned_as_predicted`` on).  The cache
can only be wrong when a reuse is ACCEPTED over arrays that no longer hold what was
counted, so these tests rewrite ``layout_ref.slack_set`` -- the same sizes, every box edge
0.05 px or more from the pixel lattice, positive amplitudes distinct per particle -- on
the device between two calls and assert the verdict of the ONE call that follows, with the
knobs of the layout key pinned (``layout_ref.ENV``).  The predictions are those of
``tests/layout_ref.py``, the NumPy statement of the per-(scatter workgroup, column) counts
and the wide count, pinned on the CPU by ``tests/test_layout_ref.py``.

* An accepted rewrite moves particles, smoothing lengths or owners but no count:
  ``layout_reuse == 1`` at once (equal counts => accepted), the maps are the counted
  pass's under the bars above, the host counters are the counted pass's, the neighbour
  counts are the oracle's -- and the maps DIFFER from those before the rewrite, which a
  result computed from anything cached could not.
* A rejected rewrite is the smallest change of its kind -- one particle a tile over, two
  particles across scatter workgroups, one record into the large stream, one particle in
  or out of the wide list (no column moves: only the wide count stands guard), one
  particle without a footprint, a wide list past its capacity: ``layout_reuse == 2``, the
  maps (accumulated ones included) bit-identical to the counted pass's, then a counted
  call (0) and a reused one (1).
* The sweep applies 24 single-particle moves and requires the verdict ``layout_ref``
  computes for each, in both directions.
"""
import numpy as np
import pytest

import layout_ref as lr

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


# ----------------------------------------------------------------------------------
# rewrites in place, accepted and rejected (tests/layout_ref.py predicts which)
# ----------------------------------------------------------------------------------
@pytest.fixture
def pinned(fresh, monkeypatch):
    """The knobs the layout depends on (read per call, held in the layout key)."""
    for k, v in lr.ENV.items():
        monkeypatch.setenv(k, v)


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def _slack(seed=1):
    """``slack_set(seed)`` and its device arrays x, y, h, a0, a1."""
    s = lr.slack_set(seed)
    return s, [_dev(a) for a in (s.u, s.v, s.h, s.a0, s.a1)]


def _rewrite(dev, new):
    """In place: the tensors keep their addresses."""
    for t, a in zip(dev, new):
        t.copy_(_dev(a).to(t.dtype))


def _modes(x, y, h, a0, a1):
    import torch
    from asp_amd.device import project2d
    ones = torch.ones_like(h)
    return {
        "det1": lambda: project2d(x, y, h, a0, kernel="cubic", deterministic=True, **KW),
        "det2": lambda: project2d(x, y, h, a0, a1, kernel="cubic", deterministic=True, **KW),
        "fp64": lambda: project2d(x, y, h, a0, a1, kernel="cubic", **KW),
        "ratio": lambda: project2d(x, y, h, a0, a1, kernel="cubic", ratio=True, **KW),
        "indicator": lambda: project2d(x, y, h, ones, kernel="indicator", **KW),
        "column": lambda: project2d(x, y, h, a0, kernel="cubic_column", deterministic=True, **KW),
    }


def _agree(mode, got, ref):
    """The module's bars: fp64 sums within 2 ulps, the ratio map within 8, all else exact."""
    if mode in ("fp64", "ratio"):
        _close(got[0], ref[0], 8 if mode == "ratio" else 2)
        _close(got[1], ref[1], 2)
    else:
        assert _same(got, ref)


def _differ(got, old):
    """Every map changed: a result made from anything cached would not have."""
    import torch
    return all(not torch.equal(g, o) for g, o in zip(got, old) if g is not None)


def _counters():
    from asp_amd.device import stats
    st = stats(0)
    return {k: st[k] for k in lr.STAT_KEYS}


_oracle_counts = {}


def _neighbour_counts(oracle, name):
    """The oracle's neighbour counts of ``slack_set()`` after rewrite ``name`` (once each)."""
    if name not in _oracle_counts:
        u, v, h, _ = lr.mutated(name)
        _oracle_counts[name] = oracle.project_scatter(u, v, h, np.ones(lr.N), None, (G, G), 64, *EXT,
                                                      kernel="indicator")[0]
    return _oracle_counts[name]


def test_slack_set_is_binned_as_predicted(pinned, monkeypatch):
    """The counted pass's host counters are those of ``layout_ref``'s table, and the set has
    what the rewrites are about: wide particles, a large stream, split tiles."""
    s, dev = _slack()
    call = _modes(*dev)["det2"]
    call()
    assert _reuse() == 0
    st = _counters()
    table, n_wide = lr.layout_counts(s.u, s.v, s.h)
    assert st["records"] == table.sum() and st["large"] == table[:, 16:].sum(), st
    assert st["wide"] == n_wide == lr.N_WIDE and st["large"] > 0, st
    assert st["merges"] > 0 and st["slabs"] > st["merges"], st
    call()
    assert _reuse() == 1 and _counters() == st


# Every accepted rewrite in every mode, but for the indicator mode those under which a map of
# unit amplitudes cannot change (layout_ref.UNIT_MAP_UNCHANGED says why, and
# tests/test_layout_ref.py checks it against the oracle): "differs from before" has nothing
# to see there.
_ACCEPTED_CASES = [(name, mode) for name in lr.ACCEPTED
                   for mode in ("det1", "det2", "fp64", "ratio", "indicator", "column")
                   if not (mode == "indicator" and name in lr.UNIT_MAP_UNCHANGED)]


@pytest.mark.parametrize("name,mode", _ACCEPTED_CASES)
def test_accepted_after_rewrite(pinned, monkeypatch, oracle, name, mode):
    s, dev = _slack()
    call = _modes(*dev)[mode]
    call()
    assert _reuse() == 0
    old = call()
    assert _reuse() == 1
    u, v, h, _ = lr.mutated(name)
    _rewrite(dev[:3], (u, v, h))
    got = call()
    assert _reuse() == 1, name  # equal counts => accepted, on the first call after the rewrite
    st = _counters()
    ref = _off(monkeypatch, call)
    assert st == _counters()
    _agree(mode, got, ref)
    assert _differ(got, old)
    if mode == "indicator":
        assert np.array_equal(got[0].double().cpu().numpy(), _neighbour_counts(oracle, name))


@pytest.mark.parametrize("mode", ("det2", "indicator", "accumulate"))
@pytest.mark.parametrize("name", lr.REJECTED)
def test_rejected_near_misses(pinned, monkeypatch, name, mode):
    import torch
    from asp_amd.device import project2d
    s, dev = _slack()
    x, y, h, a0, a1 = dev
    base0 = torch.rand(G, G, device=x.device)
    base1 = torch.rand(G, G, device=x.device)
    call = _modes(*dev)[mode] if mode != "accumulate" else (
        lambda: project2d(x, y, h, a0, a1, kernel="cubic", deterministic=True, accumulate=True,
                          out0=base0.clone(), out1=base1.clone(), **KW))
    _arm(call)
    before = _counters()
    u, v, hh, _ = lr.mutated(name)
    _rewrite(dev[:3], (u, v, hh))
    got = call()
    assert _reuse() == 2, name
    after = _counters()
    if name == "across_groups":  # nothing coarser than the per-workgroup rows tells
        assert after == before
    if name == "many_wide":
        assert after["wide"] == lr.HEAD + lr.N_WIDE == 2040
    fourth = call()
    assert _reuse() == 0  # disarmed: counted
    fifth = call()
    assert _reuse() == 1  # equal counters re-armed it
    ref = _off(monkeypatch, call)  # (accumulate: the bases were added to exactly once)
    assert _same(got, ref) and _same(fourth, ref) and _same(fifth, ref)


def test_accepted_fp64_entry_point(pinned, monkeypatch):
    """fp64 arrays that fp32 cannot hold, rewritten in place: the fp32 working copies are
    re-derived on every call, or the maps would be the old ones."""
    import torch
    from asp_amd.device import project2d_f64
    s = lr.slack_set()
    rng = np.random.default_rng(5)

    def wide64(a):  # off the fp32 lattice by 2^-30 relative
        return np.asarray(a, dtype=np.float64) * (1.0 + rng.choice([-1.0, 1.0], len(a)) * 2.0 ** -30)

    def arrays(u, v, h):
        return np.stack((wide64(u), wide64(v), np.zeros(lr.N)), 1), wide64(h)

    p0, h0 = arrays(s.u, s.v, s.h)
    assert not np.array_equal(p0[:, 0], p0[:, 0].astype(np.float32))
    pos, hd = _dev(p0), _dev(h0)
    b0, b1 = _dev(s.a0).double(), _dev(s.a1).double()
    call = lambda: project2d_f64(pos, hd, b0, b1, kernel="cubic", deterministic=True, **KW)  # noqa: E731
    call()
    assert _reuse() == 0
    old = call()
    assert _reuse() == 1
    now = (s.u, s.v, s.h)
    for name in ("jitter", "swap_in_batch"):
        u, v, h, _ = lr.mutated(name, base=now)
        _rewrite((pos, hd), arrays(u, v, h))
        got = call()
        assert _reuse() == 1, name
        assert _same(got, _off(monkeypatch, call)), name
        assert _differ(got, old), name
        old, now = got, (u, v, h)


def test_accepted_rows_window(pinned, monkeypatch):
    """A window of image rows has its own key, tile grid and local frames."""
    from asp_amd.device import project2d
    rows = (64, 192)
    s, dev = _slack()
    x, y, h, a0, a1 = dev
    call = lambda: project2d(x, y, h, a0, a1, kernel="cubic", deterministic=True, rows=rows, **KW)  # noqa: E731
    call()
    assert _reuse() == 0
    old = call()
    assert _reuse() == 1
    u, v, hh, _ = lr.mutated("jitter")
    _rewrite(dev[:3], (u, v, hh))
    got = call()
    assert _reuse() == 1
    assert _same(got, _off(monkeypatch, call)) and _differ(got, old)
    _arm(call)
    u = u.copy()
    lr.move_one_tile(u, lr.pick_one_tile_over(s, rows))  # a particle whose box lies in the window
    _rewrite(dev[:1], (u,))
    got = call()
    assert _reuse() == 2
    assert _same(got, _off(monkeypatch, call))


def test_accepted_on_two_slots(pinned, monkeypatch):
    """Two streams, two particle sets: a rewrite of one set is accepted on its slot and
    leaves the other slot's layout and maps alone."""
    import torch
    from asp_amd.device import project2d
    (sa, A), (sb, B) = _slack(seed=5), _slack(seed=6)
    kw = dict(kernel="cubic", deterministic=True, **KW)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]

    def run(k, dev):
        with torch.cuda.stream(streams[k]):
            out = project2d(*dev, **kw)
            return out, _reuse()

    for want in (0, 1):
        old_a, ra = run(0, A)
        old_b, rb = run(1, B)
        assert (ra, rb) == (want, want)
    torch.cuda.synchronize()
    u, v, h, _ = lr.mutated("jitter", seed=5)
    with torch.cuda.stream(streams[0]):
        _rewrite(A[:3], (u, v, h))
    torch.cuda.synchronize()
    got_a, ra = run(0, A)
    got_b, rb = run(1, B)
    again_b, rb2 = run(1, B)
    torch.cuda.synchronize()
    assert (ra, rb, rb2) == (1, 1, 1)
    assert _same(got_b, old_b) and _same(again_b, old_b)
    assert _differ(got_a, old_a)
    assert _same(got_a, _off(monkeypatch, lambda: project2d(*A, **kw)))


def test_verdict_follows_the_counts(pinned, monkeypatch):
    """24 single-particle moves, one after another: the verdict is ``layout_ref``'s for every
    one of them (8 accepted, 16 rejected), the maps the counted pass's."""
    s, dev = _slack()
    x, y, h = dev[:3]
    call = _modes(*dev)["det2"]
    moves = lr.sweep()
    assert len(moves) == 24
    for k, (p, pu, pv, ph, want) in enumerate(moves):
        _arm(call)
        x[p], y[p], h[p] = float(pu), float(pv), float(ph)
        got = call()
        assert _reuse() == want, (k, p, want)
        assert _same(got, _off(monkeypatch, call)), (k, p)
