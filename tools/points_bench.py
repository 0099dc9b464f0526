#!/usr/bin/env python3
"""Timing of the 3-D point sampler (asp_sample3d; DESIGN.md §21 has the results).

Per configuration (particles x smoothing-length law x point set) one JSON line:
  prep_ms, deposit_ms   HIP events around the library's own stages (asp_profile_stages:
                        sample_prep, sample_deposit), median of --reps calls after --warmup
                        calls, all in this one process
  pairs_tested          (particle, point) pairs the deposit tested (ASP_SAMPLE_COUNT, from a
                        separate counted call), pairs_included those that passed (the sum of
                        an indicator-kernel call)
  tested_pairs_per_s    pairs_tested / deposit_ms
  floor_ms, floor_fraction
                        the particle stream's byte floor (20 B per particle: x, y, z, h, a) at
                        the HBM3E peak of 8.0 TB/s, over deposit_ms
  walk                  the wide class's walk in force (ASP_SAMPLE3D_WALK: "flat", the
                        default, or "row"), with the thresholds in force (the environment's,
                        else the library's defaults, by value)
  cube512_ms            yardstick 1: the 512^3 cube of the same particles through
                        asp_project3d (device arrays, whole call, torch events, median)
  sample2d_ms           yardstick 2: asp_sample2d (cubic spline, the same term) on (x, y) of
                        the same particles at the points' (x, y): prep + deposit stages
Particles: plummer_torch (float32, device-resident) in the box [-4, 4]^3, h either 0.75 voxel
pitches of a 512^3 cube ("voxel") or 1.2 (m / rho)^(1/3) ("physical").  Point sets: uniform
in the box (a count), "sightlines" (10^4 sightlines x 10^3 bins, random starts and
directions through the box, asp_amd.points.sightline_points) or "clustered" (10^6 points that
are exact copies of 10^3 positions in [-1, 1]^3).  Configurations run in the order given
until --budget-s is used up; the rest are reported as skipped.  There is no CPU fallback:
without a GPU the tool fails.
"""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "astro-sph-tools_amd"))

HBM_PEAK = 8.0e12  # B/s, MI355X HBM3E specification
EXT = 4.0
KERNEL = 0  # cubic spline
# asp_sample3d's defaults (include/asp_points.h; csrc/asp_sample3d.hip: kWideCells3, kWidePoints3)
LIB_DEFAULTS = {"ASP_SAMPLE_WIDE_CELLS": 27, "ASP_SAMPLE_WIDE_POINTS": 16,
                "ASP_SAMPLE3D_WALK_MIX": 1, "ASP_SAMPLE_CELLS": "ceil(cbrt(m/4)) <= 160"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, nargs="+", default=[10_000_000, 100_000_000])
    ap.add_argument("--laws", nargs="+", default=["voxel", "physical"])
    ap.add_argument("--points", nargs="+",
                    default=["10000", "1000000", "10000000", "sightlines", "clustered"])
    ap.add_argument("--sightlines", type=int, nargs=2, default=[10_000, 1_000],
                    help="sightlines and bins of the 'sightlines' point set")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--budget-s", type=float, default=600.0)
    ap.add_argument("--no-yardsticks", action="store_true")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()

    import torch
    from asp_amd import _lib
    from asp_amd.device import project3d
    from asp_amd.plummer import plummer_torch
    from asp_amd.points import sightline_points
    _lib.require_gpu(0)
    t_start = time.perf_counter()
    P, D = _lib.ptr, (lambda t: _lib.ptr(t, _lib._d))
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(7)
    rand = lambda *shape: torch.rand(shape, dtype=torch.float64, device="cuda", generator=gen)  # noqa: E731
    # the values in force, not the word "default": a results file must say what it measured
    # after the library's defaults move (LIB_DEFAULTS: those of include/asp_points.h)
    knobs = {k: os.environ.get(k, str(v)) for k, v in LIB_DEFAULTS.items()}
    walk = "row" if os.environ.get("ASP_SAMPLE3D_WALK") == "0" else "flat"

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(text + "\n")

    def point_set(kind):
        if kind == "clustered":
            c = rand(1000, 3) * 2.0 - 1.0
            p = c[torch.randint(0, 1000, (1_000_000,), device="cuda", generator=gen)]
        elif kind == "sightlines":
            ns, nb = a.sightlines
            starts = rand(ns, 3) * (2 * EXT) - EXT
            towards = rand(ns, 3) * (2 * EXT) - EXT  # a second point in the box: the direction
            p = sightline_points(starts, towards - starts, EXT, nb).reshape(-1, 3)
        else:
            p = rand(int(kind), 3) * (2 * EXT) - EXT
        return tuple(p[:, d].contiguous() for d in range(3))

    def staged(call):
        """(prep_ms, deposit_ms) medians over --reps profiled calls, and the deposit's range."""
        prep, dep = [], []
        for _ in range(a.reps):
            _lib.profile(0, True, stages=("sample_prep", "sample_deposit"))
            call()
            torch.cuda.synchronize()
            p = _lib.profile_read(0)
            prep.append(p["sample_prep"][0])
            dep.append(p["sample_deposit"][0])
        _lib.profile(0, False)
        return statistics.median(prep), statistics.median(dep), [round(min(dep), 3), round(max(dep), 3)]

    for n in a.particles:
        for law in a.laws:
            if time.perf_counter() - t_start > a.budget_s:
                emit({"tool": "points_bench", "particles": n, "h_law": law, "skipped": "budget"})
                continue
            s = plummer_torch(n, seed=3, h_law="pixel" if law == "voxel" else law, extent=EXT, grid=512)
            x, y, z, h, am = s["x"], s["y"], s["z"], s["h"], s["m"]
            del s
            one = torch.ones_like(am)
            torch.cuda.synchronize()

            def call3(pt, out, amp=am, kid=KERNEL):
                _lib.check(_lib.lib().asp_sample3d(P(x), P(y), P(z), P(h), P(amp), None, n, D(pt[0]),
                                                   D(pt[1]), D(pt[2]), pt[0].numel(), kid,
                                                   _lib.ASP_F_DEVICE_PTRS, P(out), None, 0, stream))

            def call2(pt, out):
                _lib.check(_lib.lib().asp_sample2d(P(x), P(y), P(h), P(am), None, n, D(pt[0]), D(pt[1]),
                                                   pt[0].numel(), KERNEL, _lib.ASP_F_DEVICE_PTRS,
                                                   P(out), None, 0, stream))

            cube_ms = None
            if not a.no_yardsticks:  # yardstick 1: the 512^3 cube of the same particles
                times = []
                for r in range(1 + a.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    cube = project3d(x, y, z, h, am, cube_size=(512, 512, 512),
                                     extent=(-EXT, EXT) * 3, kernel="cubic")
                    e1.record()
                    torch.cuda.synchronize()
                    if r:
                        times.append(e0.elapsed_time(e1))
                    del cube
                cube_ms = round(statistics.median(times), 3)

            for kind in a.points:
                base = dict({"tool": "points_bench", "particles": n, "h_law": law, "points": kind,
                             "kernel": "cubic", "box": [-EXT, EXT], "walk": walk}, **knobs)
                if time.perf_counter() - t_start > a.budget_s:
                    emit(dict(base, skipped="budget"))
                    continue
                pt = point_set(kind)
                m = pt[0].numel()
                out = torch.empty(m, dtype=torch.float32, device="cuda")
                os.environ["ASP_SAMPLE_COUNT"] = "1"
                call3(pt, out)
                torch.cuda.synchronize()
                tested = _lib.last_stats(0)["evals"]
                del os.environ["ASP_SAMPLE_COUNT"]
                call3(pt, out, amp=one, kid=2)
                included = int(out.double().sum().item())
                for _ in range(a.warmup):
                    call3(pt, out)
                torch.cuda.synchronize()
                prep_ms, dep_ms, dep_range = staged(lambda: call3(pt, out))
                s2d_ms = None
                if not a.no_yardsticks:  # yardstick 2: the 2-D sampler at the same M
                    call2(pt, out)
                    p2, d2, _ = staged(lambda: call2(pt, out))
                    s2d_ms = round(p2 + d2, 3)
                floor_ms = n * 20 / HBM_PEAK * 1e3
                emit(dict(base, n_points=m, prep_ms=round(prep_ms, 3), deposit_ms=round(dep_ms, 3),
                          deposit_ms_min_max=dep_range, reps=a.reps, pairs_tested=tested,
                          pairs_included=included,
                          tested_pairs_per_s=round(tested / (dep_ms * 1e-3)),
                          points_per_s=round(m / ((prep_ms + dep_ms) * 1e-3)),
                          floor_ms=round(floor_ms, 3), floor_fraction=round(floor_ms / dep_ms, 4),
                          hbm_peak_B_per_s=HBM_PEAK, cube512_ms=cube_ms, sample2d_ms=s2d_ms))
                del pt, out
            del x, y, z, h, am, one
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
