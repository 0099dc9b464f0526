#!/usr/bin/env python3
"""Timing of the periodic nearest-halo search (asp_nearest; DESIGN.md has the results).

Per configuration (queries x centre distribution x sets x query order) one JSON line:
  prep_ms, search_ms  HIP events around the library's own stages (asp_profile_stages:
                      nearest_prep, nearest_search), median of --reps calls after --warmup
                      calls, all in this one process, the query orders alternating;
                      search_ms includes the query sort when ASP_NEAREST_SORT=1
  queries_per_s       queries / (prep + search)
  dists_per_query     from a separate counted run (ASP_NEAREST_COUNT), per set
  floor_fraction      the search's byte floor over search_ms: 24 B read per query plus 12 B
                      written per set per query, at the HBM3E peak of 8.0 TB/s
  scipy_speedup       KDTree(centres[mask], boxsize=L).query(sample, workers=16), one tree
                      per set, timed on the first --scipy-sample queries and scaled linearly
                      to all of them, over (prep + search)
Queries are uniform random in the box (random order: no spatial coherence between
neighbouring rows), device-resident; centres are uniform, or clustered (Plummer spheres
wrapped into the box).  There is no CPU fallback: without a GPU the tool fails.
"""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "astro-sph-tools_amd"))

HBM_PEAK = 8.0e12  # B/s, MI355X HBM3E specification


def centres(kind, m, L, rng):
    if kind == "uniform":
        c = rng.uniform(0.0, L, (m, 3))
    else:  # 64 Plummer spheres of scale radius L / 100, wrapped into the box
        k = 64
        r = (L / 100.0) / np.sqrt(rng.uniform(0.0, 1.0, m) ** (-2.0 / 3.0) - 1.0)
        v = rng.standard_normal((m, 3))
        v /= np.linalg.norm(v, axis=1)[:, None]
        c = rng.uniform(0.0, L, (k, 3))[rng.integers(0, k, m)] + r[:, None] * v
        c = c - np.floor(c / L) * L
    return np.where((c >= L) | (c < 0.0), 0.0, c)


def masks(nsets, m, rng):
    """Nested mass cuts keeping 1, 1/4, 1/16, 1/64 of the centres (a halo mass function)."""
    u = rng.random(m)
    return [u < 4.0 ** -s for s in range(nsets)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, nargs="+", default=[10_000_000, 100_000_000])
    ap.add_argument("--centres", type=int, default=1_000_000)
    ap.add_argument("--kinds", nargs="+", default=["uniform", "clustered"])
    ap.add_argument("--sets", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--orders", nargs="+", default=["0", "1"], help="ASP_NEAREST_SORT values")
    ap.add_argument("--box", type=float, default=100.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scipy-sample", type=int, default=1_000_000)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()

    import torch
    from scipy.spatial import KDTree
    from asp_amd import _lib
    from asp_amd.haloes import nearest_haloes
    _lib.require_gpu(0)
    L = a.box
    rng = np.random.default_rng(0)
    gen = torch.Generator(device="cuda").manual_seed(1)
    for n in a.queries:
        pos = torch.rand((n, 3), dtype=torch.float64, device="cuda", generator=gen) * L
        sample = pos[:min(n, a.scipy_sample)].cpu().numpy()
        torch.cuda.synchronize()
        for kind in a.kinds:
            c = centres(kind, a.centres, L, rng)
            for nsets in a.sets:
                mk = masks(nsets, a.centres, rng)
                t0 = time.perf_counter()
                ref = [KDTree(c[k], boxsize=L).query(sample, workers=16) for k in mk]
                scipy_s = (time.perf_counter() - t0) * n / len(sample)
                # per order: a counted run (checked against scipy on the sample), then warm-up
                evals, same = {}, {}
                for order in a.orders:
                    os.environ["ASP_NEAREST_SORT"] = order
                    os.environ["ASP_NEAREST_COUNT"] = "1"
                    idx, dist = nearest_haloes(pos, c, L, mk)
                    torch.cuda.synchronize()
                    evals[order] = _lib.last_stats(0)["evals"]
                    del os.environ["ASP_NEAREST_COUNT"]
                    same[order] = all(
                        np.array_equal(dist[s, :len(sample)].cpu().numpy().view(np.uint64),
                                       ref[s][0].view(np.uint64)) for s in range(nsets))
                    del idx, dist
                    for _ in range(a.warmup):
                        nearest_haloes(pos, c, L, mk)
                    torch.cuda.synchronize()
                # timed calls, the orders alternating
                prep = {o: [] for o in a.orders}
                search = {o: [] for o in a.orders}
                for _ in range(a.reps):
                    for order in a.orders:
                        os.environ["ASP_NEAREST_SORT"] = order
                        _lib.profile(0, True, stages=("nearest_prep", "nearest_search"))
                        nearest_haloes(pos, c, L, mk)
                        torch.cuda.synchronize()
                        p = _lib.profile_read(0)
                        prep[order].append(p["nearest_prep"][0])
                        search[order].append(p["nearest_search"][0])
                _lib.profile(0, False)
                for order in a.orders:
                    prep_ms = statistics.median(prep[order])
                    search_ms = statistics.median(search[order])
                    floor_ms = n * (24 + 12 * nsets) / HBM_PEAK * 1e3
                    line = {"tool": "nearest_bench", "queries": n, "centres": a.centres,
                            "kind": kind, "sets": nsets, "sort": int(order), "box": L,
                            "prep_ms": round(prep_ms, 3), "search_ms": round(search_ms, 3),
                            "search_ms_min_max": [round(min(search[order]), 3),
                                                  round(max(search[order]), 3)],
                            "queries_per_s": round(n / ((prep_ms + search_ms) * 1e-3)),
                            "dists_per_query_per_set": round(evals[order] / n / nsets, 2),
                            "floor_ms": round(floor_ms, 3),
                            "floor_fraction": round(floor_ms / search_ms, 4),
                            "hbm_peak_B_per_s": HBM_PEAK,
                            "scipy_s_scaled": round(scipy_s, 2),
                            "scipy_speedup": round(scipy_s / ((prep_ms + search_ms) * 1e-3), 1),
                            "distances_bit_identical_on_sample": bool(same[order])}
                    text = json.dumps(line)
                    print(text, flush=True)
                    if a.out:
                        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                        with open(a.out, "a") as f:
                            f.write(text + "\n")
        del pos
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
