#!/usr/bin/env python3
"""Generate the golden fixture G12 by RUNNING THE REFERENCE's ArrayReorder and ArrayMapping
(tools/_ArrayReorder.py:815-1038, :1042-1171).

Test infrastructure only; imports the reference file by path at run time (nothing of it is
copied), writes ``g12_array_reorder.npz`` next to this file.  The module imports ``unyt``,
``QuasarCode``, ``QuasarCode.MPI`` and ``numba`` at its top, none installed here: stub
modules stand in for them (``njit`` = identity; the classes and functions named at import
exist and are never called by the NumPy paths recorded here).

Per case ``c`` the file holds the inputs (``c_S``, ``c_T``, ``c_sf``, ``c_tf``; an absent
filter is stored as all true and flagged in ``c_has_filters``), two data arrays
(``c_data_a`` float64 (n,), ``c_data_b`` float32 (n, 3), NaN payloads included; ``c_rdata_*``
for the reverse direction; ``c_*_prior_*``: the output arrays' contents before the call), and what the
reference's object gives: ``c_source_filter``, ``c_target_filter``, ``c_fwd_props`` (the
property lists below, as int64), ``c_fwd_default_{a,b}`` (``default_value`` form), ``c_fwd_output_{a,b}``
(``output_array`` form: the prior contents survive where nothing matches) and, for
ArrayReorder, the same from ``.reverse`` (``c_rev_*``).

Usage:  python tests/golden/make_golden_reorder.py
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("ASP_REFERENCE", "/root/reference")
SRC = os.path.join(REF, "src/astro_sph_tools/tools/_ArrayReorder.py")

REORDER_PROPS = ("input_length", "output_length", "matched_items", "uses_all_inputs",
                 "all_outputs_matched", "lossless", "matches_are_reduction",
                 "results_are_expansion", "results_are_subset", "results_are_superset")
MAPPING_PROPS = ("input_length", "output_length")


def load_reference():
    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    class unyt_array:  # noqa: N801  (singledispatch registers the class; never instantiated)
        pass

    class unyt_quantity:  # noqa: N801
        pass

    class Console:
        @staticmethod
        def print_verbose_warning(*a, **k):
            pass

    def unused(*a, **k):
        raise RuntimeError("MPI helper called by a non-MPI path")

    module("unyt", unyt_array=unyt_array, unyt_quantity=unyt_quantity)
    qc = module("QuasarCode", Console=Console)
    qc.MPI = module("QuasarCode.MPI", MPI_Config=None, mpi_barrier=unused, synchronyse=unused,
                    mpi_gather_array=unused, mpi_scatter_array=unused)
    module("numba", njit=lambda f: f)
    spec = importlib.util.spec_from_file_location("_reference_ArrayReorder", SRC)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    return ref


def ids(rng, n):
    """n distinct IDs over the whole int64 range, a few special values among them."""
    special = np.array([0, 1, -1, np.iinfo(np.int64).min, np.iinfo(np.int64).max, 2 ** 53 + 1,
                        2 ** 53 - 1], np.int64)
    pool = np.unique(np.concatenate([special, rng.integers(np.iinfo(np.int64).min,
                                                           np.iinfo(np.int64).max, 2 * n)]))
    rest = rng.permutation(pool[~np.isin(pool, special)])[: n - special.size]
    return rng.permutation(np.concatenate([special, rest]))


def record(out, c, obj, props, data, n_out, rng, prefix):
    for k, d in data.items():
        out[f"{c}_{prefix}_default_{k}"] = obj(d, default_value=-7)
        prior = rng.standard_normal((n_out,) + d.shape[1:]).astype(d.dtype)
        out[f"{c}_{prefix}_prior_{k}"] = prior.copy()
        out[f"{c}_{prefix}_output_{k}"] = obj(d, output_array=prior)
    out[f"{c}_{prefix}_props"] = np.array([int(getattr(obj, p)) for p in props], np.int64)


def main():
    ref = load_reference()
    rng = np.random.default_rng(12)
    out = {}

    def data_for(n):
        a = rng.standard_normal(n)
        b = rng.standard_normal((n, 3)).astype(np.float32)
        a[::17] = np.nan
        b.view(np.uint32)[::13, 1] = 0x7fc01234  # a NaN payload that a copy must keep
        return {"a": a, "b": b}

    pool = ids(rng, 320)

    def reorder_case(c, S, T, sf, tf):
        obj = ref.ArrayReorder.create(S, T, sf, tf)
        d_fwd, d_rev = data_for(S.size), data_for(T.size)
        out[f"{c}_S"], out[f"{c}_T"] = S, T
        out[f"{c}_sf"] = np.ones(S.size, bool) if sf is None else sf
        out[f"{c}_tf"] = np.ones(T.size, bool) if tf is None else tf
        out[f"{c}_has_filters"] = np.array(sf is not None)
        out[f"{c}_source_filter"], out[f"{c}_target_filter"] = obj.source_filter, obj.target_filter
        out[f"{c}_rev_source_filter"] = obj.reverse.source_filter
        out[f"{c}_rev_target_filter"] = obj.reverse.target_filter
        for k in ("a", "b"):
            out[f"{c}_data_{k}"], out[f"{c}_rdata_{k}"] = d_fwd[k], d_rev[k]
        record(out, c, obj, REORDER_PROPS, d_fwd, T.size, rng, "fwd")
        record(out, c, obj.reverse, REORDER_PROPS, d_rev, S.size, rng, "rev")

    # ---- ArrayReorder: S and T share most IDs, each has some of its own ----
    for c, filtered in (("reorder_plain", False), ("reorder_filtered", True)):
        S = rng.permutation(pool[:200])
        T = rng.permutation(pool[40:270])[:180]
        reorder_case(c, S, T, rng.random(S.size) < 0.85 if filtered else None,
                     rng.random(T.size) < 0.85 if filtered else None)
    # ---- a lossless permutation ----
    S = rng.permutation(pool[:120])
    reorder_case("reorder_lossless", S, rng.permutation(S), None, None)
    # ---- ArrayMapping: the targets repeat source IDs (a membership list) ----
    for c, filtered in (("mapping_plain", False), ("mapping_filtered", True)):
        S = rng.permutation(pool[:160])
        T = rng.choice(pool[30:200], 260)  # with repeats; some IDs are not sources
        sf = rng.random(S.size) < 0.85 if filtered else None
        tf = rng.random(T.size) < 0.85 if filtered else None
        obj = ref.ArrayMapping.create(S, T, sf, tf)
        d_fwd = data_for(S.size)
        out[f"{c}_S"], out[f"{c}_T"] = S, T
        out[f"{c}_sf"] = np.ones(S.size, bool) if sf is None else sf
        out[f"{c}_tf"] = np.ones(T.size, bool) if tf is None else tf
        out[f"{c}_has_filters"] = np.array(filtered)
        out[f"{c}_source_filter"], out[f"{c}_target_filter"] = obj.input_filter, obj.output_filter
        for k in ("a", "b"):
            out[f"{c}_data_{k}"] = d_fwd[k]
        record(out, c, obj, MAPPING_PROPS, d_fwd, T.size, rng, "fwd")
    path = os.path.join(HERE, "g12_array_reorder.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
