"""Cross-snapshot ID matching (asp_match_ids, asp_take_rows, asp_amd.tools._ArrayReorder):
what holds without a GPU.

The definition the device implements is restated in NumPy (tests/reorder_ref.py) and pinned
here, bit for bit, to what the reference's own ArrayReorder / ArrayMapping objects gave
(tests/golden/g12_array_reorder.npz, written by tests/golden/make_golden_reorder.py from
tools/_ArrayReorder.py:815-1171).  tests/test_gpu_reorder.py compares the device with the
restatement.
"""
import ctypes as C

import numpy as np
import pytest
from conftest import golden
from reorder_ref import match_ref, take_ref

REORDER = ("reorder_plain", "reorder_filtered", "reorder_lossless")
MAPPING = ("mapping_plain", "mapping_filtered")


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def filters(g, c):
    if not bool(g[f"{c}_has_filters"]):
        return None, None
    return g[f"{c}_sf"], g[f"{c}_tf"]


def check_direction(g, c, prefix, data, S, T, sf, tf):
    index, matched, counts = match_ref(S, T, sf, tf)
    src_key = "source_filter" if prefix == "fwd" else "rev_source_filter"
    tgt_key = "target_filter" if prefix == "fwd" else "rev_target_filter"
    assert np.array_equal(matched, g[f"{c}_{src_key}"])
    assert np.array_equal(index >= 0, g[f"{c}_{tgt_key}"])
    assert counts[2] == 0
    for k in ("a", "b"):
        d = g[f"{c}_{data}_{k}"]
        assert np.array_equal(raw(take_ref(d, index, default_value=-7)),
                              raw(g[f"{c}_{prefix}_default_{k}"])), (c, prefix, k)
        prior = g[f"{c}_{prefix}_prior_{k}"].copy()
        assert np.array_equal(raw(take_ref(d, index, output_array=prior)),
                              raw(g[f"{c}_{prefix}_output_{k}"])), (c, prefix, k)
    return index, matched, counts


@pytest.mark.parametrize("c", REORDER)
def test_restatement_is_the_references_array_reorder(c):
    g = golden("g12_array_reorder.npz")
    S, T = g[f"{c}_S"], g[f"{c}_T"]
    sf, tf = filters(g, c)
    index, matched, counts = check_direction(g, c, "fwd", "data", S, T, sf, tf)
    rindex, rmatched, rcounts = check_direction(g, c, "rev", "rdata", T, S, tf, sf)
    assert counts[0] == counts[1] == rcounts[0] == rcounts[1]
    for props, n_in, n_out, n in ((g[f"{c}_fwd_props"], S.size, T.size, counts[0]),
                                  (g[f"{c}_rev_props"], T.size, S.size, rcounts[0])):
        want = [n_in, n_out, n, n_in == n, n_out == n, n_in == n and n_out == n, n_in > n,
                n_out > n, n_in > n and n_out == n, n_out > n and n_in == n]
        assert props.tolist() == [int(w) for w in want]


@pytest.mark.parametrize("c", MAPPING)
def test_restatement_is_the_references_array_mapping(c):
    g = golden("g12_array_reorder.npz")
    S, T = g[f"{c}_S"], g[f"{c}_T"]
    sf, tf = filters(g, c)
    index, matched, counts = check_direction(g, c, "fwd", "data", S, T, sf, tf)
    assert g[f"{c}_fwd_props"].tolist() == [S.size, T.size]
    assert counts[0] > counts[1]  # the targets repeat source IDs


def test_restatement_duplicate_rules():
    """A duplicate needs >= 2 filtered sources and >= 1 filtered target; a filtered-out copy
    cannot shadow the kept one."""
    S = np.array([5, 5, 6], np.int64)
    assert match_ref(S, [5, 6])[2][2] == 1
    assert match_ref(S, [5, 6], None, [False, True])[2] == (1, 1, 0)
    index, matched, counts = match_ref(S, [5, 6], [False, True, True])
    assert index.tolist() == [1, 2] and matched.tolist() == [False, True, True] and counts[2] == 0
    assert match_ref(S, [6, 7])[2] == (1, 1, 0)
    u = np.array([2 ** 63 + 5, 7], np.uint64)
    assert match_ref(u, u[::-1].copy())[0].tolist() == [1, 0]


# ---- the C-ABI's argument checks: all before any device work ----

def _match(L, ns=4, nt=4, mode=0, S=True, T=True, index=True, counts=True):
    from asp_amd import _lib
    ids = np.arange(4, dtype=np.int64)
    idx = np.full(4, 9, np.int32)
    cnt = (C.c_int64 * 3)(7, 7, 7)
    rc = L.asp_match_ids(_lib.ptr(ids, _lib._i64) if S else None, None, ns,
                         _lib.ptr(ids, _lib._i64) if T else None, None, nt, mode,
                         _lib.ptr(idx, _lib._i32) if index else None, None,
                         cnt if counts else None, 0, 0, None)
    return rc, L.asp_last_error().decode(), list(cnt)


@pytest.mark.parametrize("kw", [dict(ns=-1), dict(nt=-1), dict(S=False), dict(T=False),
                                dict(index=False), dict(mode=2), dict(mode=-1)],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_match_argument_errors_before_any_device_work(asp, kw):
    from asp_amd import _lib
    rc, msg, _ = _match(_lib.lib(), **kw)
    assert rc == _lib.ASP_ERR_INVALID and msg, (rc, msg)


def test_match_sizes_without_a_device(asp):
    from asp_amd import _lib
    L = _lib.lib()
    assert _match(L, ns=1 << 31)[0] == _lib.ASP_ERR_UNSUPPORTED
    assert _match(L, nt=1 << 31)[0] == _lib.ASP_ERR_UNSUPPORTED
    rc, _, cnt = _match(L, nt=0, T=False, index=False)
    assert rc == _lib.ASP_OK and cnt == [0, 0, 0]
    rc, _, cnt = _match(L, ns=0, nt=0, S=False, T=False, index=False)
    assert rc == _lib.ASP_OK and cnt == [0, 0, 0]


def test_take_rows_argument_errors(asp):
    from asp_amd import _lib
    L = _lib.lib()
    d = np.zeros(4)
    idx = np.zeros(4, np.int32)
    out = np.zeros(4)
    P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    for row_bytes in (0, -8):
        rc = L.asp_take_rows(P(d), 4, row_bytes, _lib.ptr(idx, _lib._i32), 4, None, P(out), 0, 0, None)
        assert rc == _lib.ASP_ERR_INVALID and L.asp_last_error()
    rc = L.asp_take_rows(P(d), 4, 8, _lib.ptr(idx, _lib._i32), 4, None, None, 0, 0, None)
    assert rc == _lib.ASP_ERR_INVALID and b"out" in L.asp_last_error()
    rc = L.asp_take_rows(P(d), 4, 8, None, 4, None, P(out), 0, 0, None)
    assert rc == _lib.ASP_ERR_INVALID
    rc = L.asp_take_rows(None, 4, 8, _lib.ptr(idx, _lib._i32), 4, None, P(out), 0, 0, None)
    assert rc == _lib.ASP_ERR_INVALID
    rc = L.asp_take_rows(P(d), -1, 8, _lib.ptr(idx, _lib._i32), 4, None, P(out), 0, 0, None)
    assert rc == _lib.ASP_ERR_INVALID
    # nothing to gather: valid, no device
    assert L.asp_take_rows(P(d), 4, 8, None, 0, None, None, 0, 0, None) == _lib.ASP_OK


def test_argtypes(asp):
    from asp_amd import _lib
    L = _lib.lib()
    u8, i64, i32 = C.POINTER(C.c_uint8), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    assert L.asp_match_ids.argtypes == [i64, u8, C.c_int64, i64, u8, C.c_int64, C.c_int32, i32, u8,
                                        i64, C.c_int32, C.c_int32, C.c_void_p]
    assert L.asp_take_rows.argtypes == [C.c_void_p, C.c_int64, C.c_int64, i32, C.c_int64,
                                        C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    assert L.asp_match_ids.restype == C.c_int and L.asp_take_rows.restype == C.c_int
    assert {"asp_match_ids", "asp_take_rows"} <= set(_lib.EXPORTS)


# ---- the Python layer's host logic ----

def test_match_ids_refuses_floats_and_bad_filters(asp):
    from asp_amd.tools import match_ids
    ids = np.arange(4, dtype=np.int64)
    with pytest.raises(ValueError, match="integer"):
        match_ids(ids.astype(np.float64), ids)
    with pytest.raises(ValueError, match="integer"):
        match_ids(ids, ids.astype(np.float32))
    with pytest.raises(ValueError, match="boolean"):
        match_ids(ids, ids, np.ones(4, np.int32))
    with pytest.raises(ValueError, match="length 4"):
        match_ids(ids, ids, None, np.ones(3, bool))
    with pytest.raises(ValueError, match="mode"):
        match_ids(ids, ids, mode="both")
    # no targets: valid without a device
    index, matched, counts = match_ids(ids, ids[:0])
    assert index.shape == (0,) and not matched.any() and counts == (0, 0, 0)


def test_hand_built_objects_raise_the_references_errors(asp):
    """Host logic on objects built from a match's three results (no device)."""
    from asp_amd.tools import ArrayMapping, ArrayReorder
    index = np.array([1, -1, 0], np.int32)
    matched = np.array([True, True, False])
    data = np.arange(3.0)
    for cls in (ArrayReorder, ArrayMapping):
        obj = cls(index, matched, (2, 2, 0))
        with pytest.raises(ValueError, match="More output elements expected than matches"):
            obj(data)
        assert obj.input_length == 3 and obj.output_length == 3
    r = ArrayReorder(index, matched, (2, 2, 0))
    assert r.matched_items == 2 and len(r) == 3
    assert r.source_filter.tolist() == [True, True, False]
    assert r.target_filter.tolist() == [True, False, True]
    assert (r.uses_all_inputs, r.all_outputs_matched, r.lossless) == (False, False, False)
    assert (r.matches_are_reduction, r.results_are_expansion) == (True, True)
    assert (r.results_are_subset, r.results_are_superset) == (False, False)
    m = ArrayMapping(index, matched, (2, 2, 0))
    assert m.input_filter.tolist() == [True, True, False]
    assert m.output_filter.tolist() == [True, False, True]
    with pytest.raises(IndexError, match="Duplicate matched detected in filtered source array"):
        ArrayMapping(index, matched, (2, 2, 1))
    with pytest.raises(ValueError, match=r"different number of items \(2 and 3\)"):
        ArrayReorder(index, matched, (3, 2, 0))
    with pytest.raises(ValueError, match="different number of items"):
        ArrayReorder(index, matched, (2, 2, 1))
