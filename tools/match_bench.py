#!/usr/bin/env python3
"""Timing of the cross-snapshot ID matching (asp_match_ids, asp_take_rows; DESIGN.md §18
has the results).

Per configuration one JSON line.  Inputs are device-resident; times are HIP events outside
the library around whole calls, the median of --reps calls after --warmup calls, all in this
one process.  Source IDs: n distinct 64-bit IDs (a bijection of 0..n-1, so no duplicates).
Target: a random 90 % subset of the source in permuted order.  ``skewed``: 1 % of the source
rows carry one ID that no target asks for.

  match_ms            the whole asp_match_ids call (its wait for the counts included)
  count_ms, scatter_ms, join_ms
                      the phases, from calls cut short with ASP_MATCH_STOP (1: count and
                      scans, 2: + scatter): differences of the medians, the three variants
                      alternating inside every repetition
  ids_per_s           (n_source + n_target) / match_ms
  *_bytes, *_fraction the bytes a phase must move over its time, as a fraction of the 6.3 TB/s
                      streaming rate the microarchitecture guide gives for HBM.  Model, per
                      ID unless stated: count reads the 8-byte ID and writes 4 bytes of index
                      per target; scatter reads 8 and writes a 12-byte record; join reads
                      every 12-byte record once, writes 4 bytes of index per matched target and
                      1 byte per matched source, and reads 4 bytes of source position per
                      matched target.  Partition counters and scans are left out (8 bytes per
                      partition, 1/2048 of the IDs).
  take8_ms, take24_ms asp_take_rows of 8- and 24-byte rows by the match's index (10 %
                      of the index -1, filled with a default): bytes = 4 per index + row
                      bytes read per matched row + row bytes written per row; the fraction
                      is again of 6.3 TB/s, the guide's random whole-row gathers (1,152-byte
                      rows, 5.5-5.6 TB/s) being the nearest published figure -- rows of 8-24
                      bytes use a fraction of every 64-byte memory request, so a fraction
                      near row_bytes / 64 of that is the expectation for the read side.
  host_*              (--host-n, default 10^7) the NumPy construction of the same match
                      (tests/reorder_ref.py, the restatement pinned to the reference: argsort,
                      searchsorted, isin, unique) and one fancy-index copy of an 8-byte field,
                      on one CPU core of the machine the tool runs on.
There is no CPU fallback: without a GPU the tool fails.
"""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "astro-sph-tools_amd"))
sys.path.insert(0, str(ROOT / "tests"))

STREAM = 6.3e12  # B/s, achievable HBM streaming rate (microarchitecture guide)
ODD = -7046029254386353131  # 0x9E3779B97F4A7C15 as int64: i -> i * ODD is a bijection mod 2^64


def timed(torch, fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[10_000_000, 100_000_000])
    ap.add_argument("--kinds", nargs="+", default=["subset", "skewed"])
    ap.add_argument("--host-n", type=int, default=10_000_000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()

    import torch
    from asp_amd import _lib
    from asp_amd.tools import match_ids, take_rows
    from reorder_ref import match_ref
    _lib.require_gpu(0)
    gen = torch.Generator(device="cuda").manual_seed(1)

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(text + "\n")

    for n in a.n:
        for kind in a.kinds:
            S = torch.arange(n, dtype=torch.int64, device="cuda") * ODD
            nt = n * 9 // 10
            perm = torch.randperm(n, device="cuda", generator=gen)[:nt]
            T = S[perm]
            if kind == "skewed":  # 1 % of the rows: one ID (that of row n, not in S or T)
                rows = torch.randperm(n, device="cuda", generator=gen)[: n // 100]
                S[rows] = torch.full((1,), n, dtype=torch.int64, device="cuda") * ODD
                del rows
            torch.cuda.synchronize()
            index, matched, counts = match_ids(S, T)
            assert counts[2] == 0, counts
            if kind == "subset":
                assert counts == (nt, nt, 0) and torch.equal(index, perm.to(torch.int32))
            del perm
            # the three variants alternate inside every repetition
            stops = {"1": [], "2": [], "3": []}
            for rep in range(a.warmup + a.reps):
                for stop in stops:
                    os.environ["ASP_MATCH_STOP"] = stop
                    ms = timed(torch, lambda: match_ids(S, T), 0, 1)[0]
                    if rep >= a.warmup:
                        stops[stop].append(ms)
            del os.environ["ASP_MATCH_STOP"]
            t1, t2, t3 = (statistics.median(stops[k]) for k in ("1", "2", "3"))
            hit, src = counts[0], counts[1]
            b_count = 8 * (n + nt) + 4 * nt
            b_scatter = 20 * (n + nt)
            b_join = 12 * (n + nt) + 8 * hit + src
            line = {"tool": "match_bench", "kind": kind, "n_source": n, "n_target": nt,
                    "chunk_keys": os.environ.get("ASP_MATCH_CHUNK_KEYS", "default"),
                    "targets_matched": hit, "sources_matched": src,
                    "match_ms": round(t3, 3),
                    "match_ms_min_max": [round(min(stops["3"]), 3), round(max(stops["3"]), 3)],
                    "ids_per_s": round((n + nt) / (t3 * 1e-3)),
                    "count_ms": round(t1, 3), "scatter_ms": round(t2 - t1, 3),
                    "join_ms": round(t3 - t2, 3),
                    "count_bytes": b_count, "scatter_bytes": b_scatter, "join_bytes": b_join,
                    "count_fraction": round(b_count / (t1 * 1e-3) / STREAM, 4),
                    "scatter_fraction": round(b_scatter / (max(t2 - t1, 1e-6) * 1e-3) / STREAM, 4),
                    "join_fraction": round(b_join / (max(t3 - t2, 1e-6) * 1e-3) / STREAM, 4),
                    "stream_B_per_s": STREAM, "warmup": a.warmup, "reps": a.reps}
            # the gather, by an index with 10 % of -1
            holes = torch.rand(nt, device="cuda", generator=gen) < 0.1
            idx = torch.where(holes, torch.full_like(index, -1), index)
            n_ok = int((idx >= 0).sum())
            del holes
            for cols, name in ((1, "take8"), (3, "take24")):
                data = torch.rand((n, cols) if cols > 1 else (n,), dtype=torch.float64,
                                  device="cuda", generator=gen)
                out = torch.empty((nt, cols) if cols > 1 else (nt,), dtype=torch.float64,
                                  device="cuda")
                ms = timed(torch, lambda: take_rows(data, idx, output_array=out, default_value=0.0),
                           a.warmup, a.reps)
                want = torch.where((idx >= 0).reshape((-1,) + (1,) * (cols > 1)),
                                   data[idx.clamp(min=0).long()], torch.zeros((), dtype=torch.float64,
                                                                               device="cuda"))
                assert torch.equal(out, want)
                del want
                t = statistics.median(ms)
                nbytes = 4 * nt + 8 * cols * (n_ok + nt)
                line.update({f"{name}_ms": round(t, 3), f"{name}_bytes": nbytes,
                             f"{name}_rows_per_s": round(nt / (t * 1e-3)),
                             f"{name}_fraction": round(nbytes / (t * 1e-3) / STREAM, 4)})
                del data, out
            # the host construction, through the restatement
            if n == a.host_n:
                hS, hT = S.cpu().numpy(), T.cpu().numpy()
                t0 = time.perf_counter()
                h_index, h_matched, h_counts = match_ref(hS, hT)
                host_match = time.perf_counter() - t0
                assert np.array_equal(h_index, index.cpu().numpy()) and h_counts == counts
                field = np.random.default_rng(0).standard_normal(n)
                t0 = time.perf_counter()
                moved = np.where(h_index >= 0, field[np.maximum(h_index, 0)], 0.0)
                host_take = time.perf_counter() - t0
                line.update({"host_match_s": round(host_match, 3), "host_take8_s": round(host_take, 3),
                             "match_speedup_vs_host": round(host_match / (t3 * 1e-3), 1)})
                del hS, hT, h_index, h_matched, moved, field
            emit(line)
            del S, T, index, matched, idx
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
