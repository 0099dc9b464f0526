"""``tests/layout_ref.py`` pinned on the CPU: the particle set, the verdict it predicts for
every rewrite of the catalogue and WHY (which cells of the count table move), so that the
GPU assertions of ``tests/test_gpu_layout_reuse.py`` rest on derived facts."""
import numpy as np
import pytest

import layout_ref as lr


def _cells(before, after):
    """{(scatter workgroup, column): after - before} of the cells that differ."""
    d = after[0] - before[0]
    return {(int(g), int(c)): int(d[g, c]) for g, c in zip(*np.nonzero(d))}


@pytest.fixture(scope="module")
def base():
    s = lr.slack_set()
    return s, lr.boxes(s.u, s.v, s.h), lr.layout_counts(s.u, s.v, s.h)


def _group(p):
    return int(lr.scatter_group(p, lr.N, lr.KNOBS["bin_blocks"], lr.KNOBS["group"]))


def test_the_set_is_what_the_module_says(base):
    s, box, (table, n_wide) = base
    ok, x0, x1, y0, y1 = box
    assert len(s.u) == lr.N and table.shape == (2, 32)
    assert lr.slack(s.u, s.v, s.h) >= 0.15 - 1e-3
    assert n_wide == lr.N_WIDE and not ok[s.cls == lr.OUTSIDE].any()
    assert ok[s.cls != lr.OUTSIDE].all()
    bw, bh = x1 - x0 + 1, y1 - y0 + 1
    inner = (x0 > 0) & (x1 < lr.G - 1) & (y0 > 0) & (y1 < lr.G - 1)
    for c, edge in ((lr.SMALL, 2), (lr.CLUMP, 2), (lr.MID, 8), (lr.LARGE, 24)):
        m = (s.cls == c) & inner
        assert m.any() and (bw[m] == edge).all() and (bh[m] == edge).all(), c
    # the large stream holds records of the LARGE class only, and most of them
    wide, pidx, col = lr.columns(box, 4, 16, lr.KNOBS["wide_tiles"], lr.KNOBS["gather_min"],
                                 lr.KNOBS["gather_area"])
    assert (s.cls[wide] == lr.WIDE).all()
    assert set(s.cls[pidx[col >= 16]]) == {lr.LARGE}
    assert (col[s.cls[pidx] == lr.LARGE] >= 16).mean() > 0.5
    # the clump: one tile, more than the 2048 records of one work item
    t = lr.CLUMP_TILE[0] * 4 + lr.CLUMP_TILE[1]
    assert (col[s.cls[pidx] == lr.CLUMP] == t).all() and table[:, t].sum() > 3 * 2048
    # neither wide nor outside among the first HEAD (many_wide turns exactly those wide)
    assert not np.isin(s.cls[:lr.HEAD], (lr.WIDE, lr.OUTSIDE)).any()
    # the scatter workgroups of the module docstring: 49 batches over 7 count workgroups
    g = lr.scatter_group(np.arange(lr.N), lr.N, 7, 4)
    assert g.max() == 1 and _group(0) == 0 and _group(4 * 1024) == 1 and _group(7 * 1024) == 0
    assert len(np.unique(s.a0)) == lr.N and (s.a0 > 0).all() and (s.a1 > 0).all()


def test_footprint_margin_is_far_below_the_slack(base):
    s = base[0]
    m = s.cls != lr.OUTSIDE
    hd = 2.0 * s.h[m].astype(np.float64)
    margin = (np.abs(s.u[m]) + 4.0 + hd) * 32.0 * 2.0 ** -20 + 2.0 ** -12
    assert margin.max() <= 6.4e-4


@pytest.mark.parametrize("name", lr.ACCEPTED)
def test_accepted_rewrites_move_no_count(base, name):
    s, box, before = base
    u, v, h, info = lr.mutated(name)
    assert lr.verdict(before, lr.layout_counts(u, v, h)) == 1
    assert lr.slack(u, v, h) >= 0.05
    new = lr.boxes(u, v, h)
    perm = np.arange(lr.N)
    if info["swapped"] is not None:
        a, b = info["swapped"]
        perm[a], perm[b] = b, a
    moved = np.zeros(lr.N, bool)
    if name in ("wide_walks",):   # the only accepted rewrite that moves a box: the wide ones
        moved[info["targets"]] = True
        assert new[0][moved].all()
    for o, w in zip(box, new):
        assert np.array_equal(o[perm][~moved], w[~moved])
    t = info["targets"]
    changed = np.zeros(len(t), bool)
    for o, w in ((s.u, u), (s.v, v), (s.h, h)):
        changed |= o[t].view(np.uint32) != w[t].view(np.uint32)
    assert changed.mean() >= 0.9


def test_rejected_rewrites_move_exactly_the_named_cells(base):
    s, box, before = base
    ok, x0, x1, y0, y1 = box
    tile = lambda p: int((x0[p] // 64) * 4 + y0[p] // 64)  # noqa: E731
    got = {}
    for name in lr.REJECTED:
        u, v, h, info = lr.mutated(name)
        after = lr.layout_counts(u, v, h)
        assert lr.verdict(before, after) == 2, name
        got[name] = (_cells(before, after), after[1] - before[1], info["targets"])

    cells, dw, (p,) = got["one_tile_over"]
    assert dw == 0 and cells == {(_group(p), tile(p)): -1, (_group(p), tile(p) + 4): +1}

    cells, dw, (a, b) = got["across_groups"]
    assert dw == 0 and _group(a) != _group(b) and tile(a) != tile(b)
    assert cells == {(_group(a), tile(a)): -1, (_group(a), tile(b)): +1,
                     (_group(b), tile(b)): -1, (_group(b), tile(a)): +1}
    u, v, h, _ = lr.mutated("across_groups")
    assert np.array_equal(before[0].sum(0), lr.layout_counts(u, v, h)[0].sum(0))

    cells, dw, (p,) = got["small_to_large"]
    assert dw == 0 and cells == {(_group(p), tile(p)): -1, (_group(p), tile(p) + 16): +1}

    assert got["outside_to_wide"][:2] == ({}, +1)
    assert got["wide_to_outside"][:2] == ({}, -1)

    for name in ("drops_out", "drops_out_h0"):
        cells, dw, (p,) = got[name]
        assert dw == 0 and cells == {(_group(p), tile(p)): -1}, name

    cells, dw, head = got["many_wide"]
    wide, pidx, col = lr.columns(box, 4, 16, lr.KNOBS["wide_tiles"], lr.KNOBS["gather_min"],
                                 lr.KNOBS["gather_area"])
    m = pidx < lr.HEAD
    want = {}
    for g, c in zip(lr.scatter_group(pidx[m], lr.N, 7, 4), col[m]):
        want[int(g), int(c)] = want.get((int(g), int(c)), 0) - 1
    assert dw == lr.HEAD and np.array_equal(head, np.arange(lr.HEAD)) and cells == want


def test_rows_window_counts(base):
    """The window of image rows 64..192 has its own tile grid and local frames: the jitter
    moves no count there, the one-tile move of a particle inside the window moves two."""
    s = base[0]
    rows = (64, 192)
    before = lr.layout_counts(s.u, s.v, s.h, rows=rows)
    assert before[0].shape == (2, 16)
    u, v, h, _ = lr.mutated("jitter")
    assert lr.verdict(before, lr.layout_counts(u, v, h, rows=rows)) == 1
    p = lr.pick_one_tile_over(s, rows)
    u = s.u.copy()
    lr.move_one_tile(u, p)
    after = lr.layout_counts(u, s.v, s.h, rows=rows)
    ok, x0, x1, y0, y1 = lr.boxes(s.u[p:p + 1], s.v[p:p + 1], s.h[p:p + 1], rows=rows)
    t = int((x0[0] // 64) * 4 + y0[0] // 64)
    assert x0[0] // 64 == 0 and _cells(before, after) == {(_group(p), t): -1, (_group(p), t + 4): +1}


def test_sweep_has_both_verdicts():
    moves = lr.sweep()
    verdicts = [m[4] for m in moves]
    assert len(moves) == lr.SWEEP_MOVES == 24
    assert verdicts.count(1) >= 4 and verdicts.count(2) >= 4, verdicts
    s = lr.slack_set()
    u, v, h = s.uvh()
    for p, pu, pv, ph, _ in moves:
        u[p], v[p], h[p] = pu, pv, ph
    assert lr.slack(u, v, h) >= 0.05


def test_boxes_hold_the_oracles_neighbours(oracle, base):
    """``footprint`` promises a superset: every pixel the oracle's indicator map of ONE
    particle marks lies inside that particle's restated box (200 particles across the
    classes; the outside ones mark nothing)."""
    s, (ok, x0, x1, y0, y1), _ = base
    rng = np.random.default_rng(7)
    sample = np.concatenate([rng.choice(np.nonzero(s.cls == c)[0], k, replace=False)
                             for c, k in ((lr.SMALL, 60), (lr.MID, 50), (lr.LARGE, 40),
                                          (lr.WIDE, 20), (lr.CLUMP, 20), (lr.OUTSIDE, 10))])
    assert len(sample) == 200
    one = np.ones(1)
    for p in sample:
        cnt, _ = oracle.project_scatter(s.u[p:p + 1], s.v[p:p + 1], s.h[p:p + 1], one, None,
                                        (lr.G, lr.G), 64, *lr.EXT, kernel="indicator")
        xs, ys = np.nonzero(cnt)
        if not ok[p]:
            assert len(xs) == 0, p
            continue
        assert len(xs) > 0, p
        assert xs.min() >= x0[p] and xs.max() <= x1[p] and ys.min() >= y0[p] and ys.max() <= y1[p], p


def test_unit_maps_change_under_the_accepted_rewrites(oracle, base):
    """What the GPU module's indicator mode relies on: every accepted rewrite but those of
    ``UNIT_MAP_UNCHANGED`` changes at least one neighbour count."""
    s = base[0]
    ones = np.ones(lr.N)
    cnt = lambda u, v, h: oracle.project_scatter(u, v, h, ones, None, (lr.G, lr.G), 64, *lr.EXT,  # noqa: E731
                                                 kernel="indicator")[0]
    old = cnt(s.u, s.v, s.h)
    for name in lr.ACCEPTED:
        u, v, h, _ = lr.mutated(name)
        assert np.array_equal(cnt(u, v, h), old) == (name in lr.UNIT_MAP_UNCHANGED), name
