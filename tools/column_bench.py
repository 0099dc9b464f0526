#!/usr/bin/env python3
"""What the column-integrated kernels cost against the 3-D-normalised ones (DESIGN.md §19
has the results).

In ONE process on one GPU, for each configuration -- by default bench.py's headline map
(10^8 particles -> 4096^2, weighted: sum m T W / sum m W, pixel-scale h) and the
10^7 -> 2048^2 physical-h map, the same Plummer inputs bench.py generates -- the same map
is projected with each kernel of --kernels (default wendland_c2, wendland_c2_column),
the kernels alternating inside every repetition, so a drift of the box moves both alike.
One JSON line per (configuration, kernel):

  map_ms              HIP events outside the library around the whole project2d call: the
                      median of --reps calls after --warmup calls, and [min, max]
  stages_ms           the library's per-stage HIP events (asp_profile), from a pass of their
                      own after the timed one (the events serialise stages the untimed call
                      overlaps): median per stage over --reps calls
  ratio_vs            map_ms and deposit-side stages over those of the first kernel listed
  sum_check           sum(map) * pixel area / sum(m) of the surface-density map (one extra
                      call, one output): the column kernels give the mass fraction inside
                      the image, the 3-D-normalised ones a number with units 1/length

--kernels wendland_c2 alone runs against any build of the library (ASP_LIB=...), which is
how the parent's line is measured on the same box.  There is no CPU fallback.
"""
import argparse
import json
import os
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "astro-sph-tools_amd"))

CONFIGS = {"headline": (100_000_000, 4096, "pixel"), "physical": (10_000_000, 2048, "physical")}
DEPOSIT_SIDE = ("deposit", "gather", "wide", "merge")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=list(CONFIGS), choices=list(CONFIGS))
    ap.add_argument("--kernels", nargs="+", default=["wendland_c2", "wendland_c2_column"])
    ap.add_argument("--scale", type=float, default=1.0, help="multiply the particle counts")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()

    import torch
    from asp_amd import _lib
    from asp_amd.device import project2d
    from asp_amd.plummer import plummer_torch
    _lib.require_gpu(0)

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(text + "\n")

    for name in a.configs:
        n, G, h_law = CONFIGS[name]
        n = int(n * a.scale)
        extent = 4.0
        ext = (-extent, extent, -extent, extent)
        d = plummer_torch(n, seed=0, h_law=h_law, extent=extent, grid=G, device="cuda")
        u, v, h, a1 = d["x"], d["y"], d["h"], d["m"]
        a0 = (d["m"] * d["T"]).contiguous()
        del d
        outs = torch.empty((2, G, G), dtype=torch.float32, device="cuda")
        kw = dict(image_size=(G, G), extent=ext, ratio=True, out0=outs[0], out1=outs[1])

        def run(kernel):
            project2d(u, v, h, a0, a1, kernel=kernel, **kw)

        def event_ms(kernel):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            run(kernel)
            e.record()
            e.synchronize()
            return s.elapsed_time(e)

        times = {k: [] for k in a.kernels}
        for rep in range(a.warmup + a.reps):
            for k in a.kernels:
                ms = event_ms(k)
                if rep >= a.warmup:
                    times[k].append(ms)
        stages = {k: {} for k in a.kernels}
        for rep in range(a.reps):
            for k in a.kernels:
                _lib.profile(0, True)
                run(k)
                torch.cuda.synchronize()
                for st, (ms, launches) in _lib.profile_read(0).items():
                    if launches:
                        stages[k].setdefault(st, []).append(ms)
                _lib.profile(0, False)
        first = None
        for k in a.kernels:
            med = statistics.median(times[k])
            st = {s: round(statistics.median(v), 4) for s, v in stages[k].items()}
            dep = sum(st.get(s, 0.0) for s in DEPOSIT_SIDE)
            one, _ = project2d(u, v, h, a1, kernel=k, image_size=(G, G), extent=ext)
            check = float(one.double().sum()) * (2 * extent / G) ** 2 / float(a1.double().sum())
            line = {"tool": "column_bench", "config": name, "particles": n, "grid": G,
                    "h_law": h_law, "map": "weighted", "kernel": k,
                    "lib": os.environ.get("ASP_LIB", "working build"),
                    "map_ms": round(med, 4),
                    "map_ms_min_max": [round(min(times[k]), 4), round(max(times[k]), 4)],
                    "stages_ms": st, "deposit_side_ms": round(dep, 4),
                    "sum_check": round(check, 6), "warmup": a.warmup, "reps": a.reps}
            if first is None:
                first = (k, med, dep)
            else:
                line["ratio_vs"] = {"kernel": first[0], "map_ms": round(med / first[1], 4),
                                    "deposit_side_ms": round(dep / max(first[2], 1e-9), 4)}
            emit(line)
        del u, v, h, a0, a1, outs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
