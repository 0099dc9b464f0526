"""NumPy restatement of asp_match_ids / asp_take_rows (include/asp.h): the definition the
device implements, pinned bit for bit to the reference's own ArrayReorder / ArrayMapping
objects by tests/test_reorder_host.py (tests/golden/g12_array_reorder.npz) and used by
tests/test_gpu_reorder.py as the expected result.

    index[j]          = the i with sf[i], tf[j] and S[i] == T[j], or -1
    source_matched[i] = sf[i] and some j with tf[j] has T[j] == S[i]
    duplicates        = ID values carried by >= 2 filtered sources and >= 1 filtered target

The search runs over the FILTERED sources, so a filtered-out copy of an ID cannot shadow the
kept one.  With duplicates, ``index`` takes the lowest source position (the device's choice
is unspecified then).
"""
import numpy as np


def as_i64(ids):
    """IDs as int64: uint64 reinterpreted (the same 64 bits), other integers converted."""
    a = np.asarray(ids)
    assert a.dtype.kind in "iu", a.dtype
    if a.dtype == np.uint64:
        return np.ascontiguousarray(a).view(np.int64)
    return a.astype(np.int64)


def match_ref(source_ids, target_ids, source_filter=None, target_filter=None):
    """(index int32, source_matched bool, (targets matched, sources matched, duplicates))."""
    S, T = as_i64(source_ids), as_i64(target_ids)
    sf = np.ones(S.shape[0], bool) if source_filter is None else np.asarray(source_filter, bool)
    tf = np.ones(T.shape[0], bool) if target_filter is None else np.asarray(target_filter, bool)
    keep = np.flatnonzero(sf)
    kept = S[keep]
    order = np.argsort(kept, kind="stable")
    ranked = kept[order]
    index = np.full(T.shape[0], -1, np.int32)
    if ranked.shape[0] > 0:
        at = np.minimum(np.searchsorted(ranked, T, side="left"), ranked.shape[0] - 1)
        hit = (ranked[at] == T) & tf
        index[hit] = keep[order[at[hit]]]
    asked = T[tf]
    source_matched = sf & np.isin(S, asked)
    values, copies = np.unique(kept, return_counts=True)
    duplicates = int(np.isin(values[copies >= 2], asked).sum())
    return index, source_matched, (int((index >= 0).sum()), int(source_matched.sum()), duplicates)


def take_ref(data, index, output_array=None, default_value=None):
    """out[j] = data[index[j]] where index[j] >= 0; elsewhere default_value, or the output's
    prior contents."""
    data = np.asarray(data)
    index = np.asarray(index)
    out = output_array
    if out is None:
        out = np.zeros((index.shape[0],) + data.shape[1:], data.dtype)
    ok = index >= 0
    if default_value is not None:
        out[~ok] = default_value
    out[ok] = data[index[ok]]
    return out
