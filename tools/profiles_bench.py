#!/usr/bin/env python3
"""Timing of the halo-centred profiles and aperture sums (asp_halo_profiles; DESIGN.md §22 has
the results).

One process per particle count (--particles); per configuration (particle distribution x bins x
properties [x one swept knob]) one JSON line:
  prep_ms, walk_ms   HIP events around the library's own stages, under the stage ids of the
                     other halo entry point (asp_profile_stages: nearest_prep = centre check,
                     keys, sort, cell starts, gather into cell order, candidate count and item
                     scan; nearest_search = the two walk kernels), median of --reps calls after
                     --warmup calls; inputs device-resident
  pairs_tested       (particle, halo) pairs whose d2 was formed, from a separate counted run
                     (ASP_PROFILE_COUNT); pairs_included = sum of count
  tested_per_s       pairs_tested / walk_ms
  floor_fraction     the byte floor over prep_ms + walk_ms: (24 + 8 nprops) B per particle read
                     once at the HBM3E peak of 8.0 TB/s
  scipy_*            (--scipy-sample > 0, particle counts up to --scipy-max) KDTree(particles,
                     boxsize=L).query_ball_point(centres[:sample], r_outer, return_length=True,
                     workers=16): ONE ball count per halo at the outermost edge (a profile of B
                     bins needs B of them, and sums need the index lists), timed on the sample
                     and scaled linearly to all centres -- labelled scaled; the tree's build
                     time is reported apart
Particles: uniform in the box, or clustered (64 Plummer spheres of scale radius L / 100 wrapped
into the box, the centre set of DESIGN.md §17 used as particles).  Centres: uniform in the box.
Radii law (heavy tail): r = r0 u^(-1/3) with u uniform in (0, 1] and r0 = L / 2000, capped at
L / 20 -- N(> r) ~ r^-3, so the volume per decade of radius is constant: most haloes hold a few
particles and a few hold 10^5 and more.  There is no CPU fallback: without a GPU the tool fails.
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


def particles(kind, n, L, gen):
    import torch
    kw = dict(dtype=torch.float64, device="cuda", generator=gen)
    if kind == "uniform":
        return torch.rand((n, 3), **kw) * L
    k = 64
    r = (L / 100.0) / torch.sqrt(torch.rand(n, **kw).clamp_min(1e-12) ** (-2.0 / 3.0) - 1.0 + 1e-300)
    v = torch.randn((n, 3), **kw)
    v /= torch.linalg.norm(v, dim=1, keepdim=True)
    c = (torch.rand((k, 3), **kw) * L)[torch.randint(0, k, (n,), device="cuda", generator=gen)]
    c += r[:, None] * v
    return c - torch.floor(c / L) * L


def radii_law(m, L, rng):
    u = 1.0 - rng.random(m)  # (0, 1]
    return np.minimum((L / 2000.0) * u ** (-1.0 / 3.0), L / 20.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=10_000_000)
    ap.add_argument("--centres", type=int, default=1_000_000)
    ap.add_argument("--kinds", nargs="+", default=["uniform", "clustered"])
    ap.add_argument("--modes", nargs="+", default=["aperture", "profile"],
                    help="aperture: one bin [0, 1]; profile: 20 bins to 3 R")
    ap.add_argument("--props", type=int, nargs="+", default=[0, 4])
    ap.add_argument("--box", type=float, default=100.0)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sweep", nargs="+", default=None,
                    help="an environment knob and the values to time it at, e.g. "
                         "ASP_PROFILE_LIGHT 0 16 64")
    ap.add_argument("--scipy-sample", type=int, default=0)
    ap.add_argument("--scipy-max", type=int, default=10_000_000)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()

    import torch
    from asp_amd import _lib
    from asp_amd.haloes import halo_profiles
    _lib.require_gpu(0)
    L, n, m = a.box, a.particles, a.centres
    rng = np.random.default_rng(0)
    gen = torch.Generator(device="cuda").manual_seed(1)
    centres = rng.uniform(0.0, L, (m, 3))
    centres = np.where(centres >= L, 0.0, centres)
    radii = radii_law(m, L, rng)
    edges = {"aperture": np.array([0.0, 1.0]), "profile": np.linspace(0.0, 3.0, 21)}
    knob, values = (a.sweep[0], a.sweep[1:]) if a.sweep else (None, [None])
    for kind in a.kinds:
        pos = particles(kind, n, L, gen)
        allprops = torch.rand((max(a.props), n), dtype=torch.float64, device="cuda", generator=gen) \
            if max(a.props) else None
        torch.cuda.synchronize()
        scipy = {}
        if a.scipy_sample and n <= a.scipy_max:
            from scipy.spatial import KDTree
            host = pos.cpu().numpy()
            host = np.where(host >= L, 0.0, host)
            t0 = time.perf_counter()
            tree = KDTree(host, boxsize=L)
            build_s = time.perf_counter() - t0
            for mode in a.modes:
                t0 = time.perf_counter()
                got = tree.query_ball_point(centres[:a.scipy_sample],
                                            edges[mode][-1] * radii[:a.scipy_sample],
                                            return_length=True, workers=16)
                scipy[mode] = ((time.perf_counter() - t0) * m / a.scipy_sample, build_s, got)
            del tree, host
        for mode in a.modes:
            for nprops in a.props:
                props = None if nprops == 0 else list(allprops[:nprops])
                for value in values:
                    if knob:
                        os.environ[knob] = value
                    os.environ["ASP_PROFILE_COUNT"] = "1"
                    count, _ = halo_profiles(pos, centres, radii, edges[mode], L, props)
                    torch.cuda.synchronize()
                    tested = _lib.last_stats(0)["evals"]
                    included = int(count.sum())
                    del os.environ["ASP_PROFILE_COUNT"]
                    agree = None
                    if mode in scipy:  # (scipy's test is inclusive; ties have measure zero here)
                        mine = count[:a.scipy_sample].sum(dim=1).cpu().numpy()
                        agree = int((mine != scipy[mode][2]).sum())
                    del count
                    for _ in range(a.warmup):
                        halo_profiles(pos, centres, radii, edges[mode], L, props)
                    torch.cuda.synchronize()
                    prep, walk = [], []
                    for _ in range(a.reps):
                        _lib.profile(0, True, stages=("nearest_prep", "nearest_search"))
                        halo_profiles(pos, centres, radii, edges[mode], L, props)
                        torch.cuda.synchronize()
                        p = _lib.profile_read(0)
                        prep.append(p["nearest_prep"][0])
                        walk.append(p["nearest_search"][0])
                    _lib.profile(0, False)
                    prep_ms, walk_ms = statistics.median(prep), statistics.median(walk)
                    floor_ms = n * (24 + 8 * nprops) / HBM_PEAK * 1e3
                    line = {"tool": "profiles_bench", "particles": n, "centres": m, "kind": kind,
                            "mode": mode, "nbins": len(edges[mode]) - 1, "nprops": nprops, "box": L,
                            "prep_ms": round(prep_ms, 3), "walk_ms": round(walk_ms, 3),
                            "walk_ms_min_max": [round(min(walk), 3), round(max(walk), 3)],
                            "pairs_tested": tested, "pairs_included": included,
                            "tested_per_s": round(tested / (walk_ms * 1e-3)),
                            "floor_ms": round(floor_ms, 3),
                            "floor_fraction": round(floor_ms / (prep_ms + walk_ms), 4),
                            "hbm_peak_B_per_s": HBM_PEAK}
                    if knob:
                        line[knob] = value
                    if mode in scipy:
                        line.update(scipy_sample=a.scipy_sample,
                                    scipy_one_ball_count_s_scaled=round(scipy[mode][0], 2),
                                    scipy_tree_build_s=round(scipy[mode][1], 2),
                                    scipy_count_mismatches_on_sample=agree)
                    text = json.dumps(line)
                    print(text, flush=True)
                    if a.out:
                        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                        with open(a.out, "a") as f:
                            f.write(text + "\n")
                if knob:
                    del os.environ[knob]
        del pos, allprops
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
