#!/usr/bin/env python3
"""Timing of the sightline sampler (asp_sample2d; DESIGN.md §20 has the results).

Per configuration (particles x smoothing-length law x point set) one JSON line:
  prep_ms, deposit_ms   HIP events around the library's own stages (asp_profile_stages:
                        sample_prep, sample_deposit), median of --reps calls after --warmup
                        calls, all in this one process
  pairs_tested          (particle, point) pairs the deposit tested (ASP_SAMPLE_COUNT, from a
                        separate counted call), pairs_included those that passed (the sum of
                        an indicator-kernel call)
  tested_pairs_per_s    pairs_tested / deposit_ms
  floor_ms, floor_fraction
                        the particle stream's byte floor (16 B per particle: u, v, h, a) at
                        the HBM3E peak of 8.0 TB/s, over deposit_ms
  map4096_ms            yardstick 1: the 4096^2 map of the same particles through
                        asp_project2d (device arrays, whole call, torch events, median)
  numpy_s_scaled        yardstick 2: a dense float64 NumPy evaluation of the same sums on
                        --numpy-points points x --numpy-particles particles, scaled linearly
                        in both to the configuration's size
Particles: plummer_torch (float32, device-resident) in the box [-4, 4]^2, h either 0.75
pixel pitches of a 4096^2 map ("pixel") or 1.2 (m / rho)^(1/3) ("physical").  Points:
uniform in the box, or "clustered": 10^6 points that are exact copies of 10^3 positions
drawn in [-1, 1]^2, the Plummer core -- every copy a separate accumulator in one cell, the
contended case.  Configurations run in the order given until --budget-s is used up (a
uniform point set whose cost, scaled from the previous one's first call, would not fit is
left out as well); the rest are reported as skipped.  ASP_SAMPLE_WIDE_POINTS in the
environment is recorded with every line (the A/B of the crowded-cell criterion).  There is
no CPU fallback: without a GPU the tool fails.
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
EXT = 4.0
KERNEL = 3  # cubic spline column: what a sightline column uses


def numpy_dense(u, v, h, a, px, py, block=8):
    """sum_p a W_col(r, h) at every point, every pair formed (the cubic column shape is
    replaced by the 3-D cubic's polynomial: the same mask, comparable arithmetic)."""
    out = np.zeros(px.size)
    thr = (2.0 * h) ** 2
    for i in range(0, px.size, block):
        dx = u[None, :] - px[i:i + block, None]
        dy = v[None, :] - py[i:i + block, None]
        r2 = dx * dx + dy * dy
        k, p = np.nonzero(r2 < thr[None, :])
        q = np.sqrt(r2[k, p]) / h[p]
        t = 2.0 - q
        f = np.where(q < 1.0, 1.0 - 1.5 * q * q + 0.75 * q * q * q, 0.25 * t * t * t)
        out[i:i + block] = np.bincount(k, weights=a[p] * f / (np.pi * h[p] ** 2),
                                       minlength=min(block, px.size - i))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, nargs="+", default=[10_000_000, 100_000_000])
    ap.add_argument("--laws", nargs="+", default=["pixel", "physical"])
    ap.add_argument("--points", nargs="+", default=["10000", "1000000", "10000000", "clustered"])
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--numpy-points", type=int, default=1000)
    ap.add_argument("--numpy-particles", type=int, default=1_000_000)
    ap.add_argument("--budget-s", type=float, default=600.0)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()

    import torch
    from asp_amd import _lib
    from asp_amd.device import project2d
    from asp_amd.plummer import plummer_torch
    _lib.require_gpu(0)
    t_start = time.perf_counter()
    P, D = _lib.ptr, (lambda x: _lib.ptr(x, _lib._d))
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(7)

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(text + "\n")

    def point_set(kind):
        if kind == "clustered":
            c = torch.rand((1000, 2), dtype=torch.float64, device="cuda", generator=gen) * 2.0 - 1.0
            idx = torch.randint(0, 1000, (1_000_000,), device="cuda", generator=gen)
            return c[idx, 0].contiguous(), c[idx, 1].contiguous()
        m = int(kind)
        p = torch.rand((2, m), dtype=torch.float64, device="cuda", generator=gen) * (2 * EXT) - EXT
        return p[0].contiguous(), p[1].contiguous()

    for n in a.particles:
        for law in a.laws:
            if time.perf_counter() - t_start > a.budget_s:
                emit({"tool": "sightline_bench", "particles": n, "h_law": law, "skipped": "budget"})
                continue
            s = plummer_torch(n, seed=3, h_law=law, extent=EXT, grid=4096)
            u, v, h, am = s["x"], s["y"], s["h"], s["m"]
            del s
            one = torch.ones_like(am)
            torch.cuda.synchronize()

            def call(px, py, out, amp=am, kid=KERNEL):
                _lib.check(_lib.lib().asp_sample2d(P(u), P(v), P(h), P(amp), None, n, D(px), D(py),
                                                   px.numel(), kid, _lib.ASP_F_DEVICE_PTRS, P(out),
                                                   None, 0, stream))

            # yardstick 1: the 4096^2 map of the same particles
            map_ms = []
            for r in range(1 + a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                project2d(u, v, h, am, image_size=(4096, 4096), extent=(-EXT, EXT, -EXT, EXT),
                          chunk_size=64, kernel="cubic_column")
                e1.record()
                torch.cuda.synchronize()
                if r:
                    map_ms.append(e0.elapsed_time(e1))
            map_ms = statistics.median(map_ms)
            # yardstick 2: dense NumPy on a sample of points and particles, scaled
            nn, nm = min(n, a.numpy_particles), a.numpy_points
            hu, hv, hh, ha = (t[:nn].double().cpu().numpy() for t in (u, v, h, am))
            hp = np.random.default_rng(5).uniform(-EXT, EXT, (2, nm))
            t0 = time.perf_counter()
            numpy_dense(hu, hv, hh, ha, hp[0], hp[1])
            numpy_s = time.perf_counter() - t0
            del hu, hv, hh, ha

            last = None  # (points, seconds) of the previous uniform set: the next one's estimate
            for kind in a.points:
                base = {"tool": "sightline_bench", "particles": n, "h_law": law, "points": kind,
                        "kernel": "cubic_column", "box": [-EXT, EXT],
                        "wide_points": os.environ.get("ASP_SAMPLE_WIDE_POINTS", "default")}
                left = a.budget_s - (time.perf_counter() - t_start)
                if left < 0:
                    emit(dict(base, skipped="budget"))
                    continue
                if last and kind != "clustered" and last[1] * int(kind) / last[0] * (2 + a.reps) > left:
                    emit(dict(base, skipped="budget", estimated_call_s=round(
                        last[1] * int(kind) / last[0], 1)))
                    continue
                px, py = point_set(kind)
                m = px.numel()
                out = torch.empty(m, dtype=torch.float32, device="cuda")
                os.environ["ASP_SAMPLE_COUNT"] = "1"
                t0 = time.perf_counter()
                call(px, py, out)
                torch.cuda.synchronize()
                first_s = time.perf_counter() - t0
                tested = _lib.last_stats(0)["evals"]
                if kind != "clustered":
                    last = (m, first_s)
                del os.environ["ASP_SAMPLE_COUNT"]
                call(px, py, out, amp=one, kid=2)
                included = int(out.double().sum().item())
                reps = a.reps if first_s < 20.0 else 1  # a very long case is timed once
                for _ in range(a.warmup if reps > 1 else 0):
                    call(px, py, out)
                torch.cuda.synchronize()
                prep, dep = [], []
                for _ in range(reps):
                    _lib.profile(0, True, stages=("sample_prep", "sample_deposit"))
                    call(px, py, out)
                    torch.cuda.synchronize()
                    p = _lib.profile_read(0)
                    prep.append(p["sample_prep"][0])
                    dep.append(p["sample_deposit"][0])
                _lib.profile(0, False)
                prep_ms, dep_ms = statistics.median(prep), statistics.median(dep)
                floor_ms = n * 16 / HBM_PEAK * 1e3
                emit(dict(base, n_points=m, prep_ms=round(prep_ms, 3), deposit_ms=round(dep_ms, 3),
                          deposit_ms_min_max=[round(min(dep), 3), round(max(dep), 3)], reps=reps,
                          pairs_tested=tested, pairs_included=included,
                          tested_pairs_per_s=round(tested / (dep_ms * 1e-3)),
                          points_per_s=round(m / ((prep_ms + dep_ms) * 1e-3)),
                          floor_ms=round(floor_ms, 3), floor_fraction=round(floor_ms / dep_ms, 4),
                          hbm_peak_B_per_s=HBM_PEAK, map4096_ms=round(map_ms, 3),
                          numpy_s_scaled=round(numpy_s * (n / nn) * (m / nm), 1),
                          numpy_sample=[nm, nn],
                          numpy_speedup=round(numpy_s * (n / nn) * (m / nm) / ((prep_ms + dep_ms) * 1e-3))))
                del px, py, out
            del u, v, h, am, one
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
