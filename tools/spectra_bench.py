#!/usr/bin/env python3
"""Timing of the sightline spectra (asp_spectra2d; DESIGN.md §24 has the results).

Per configuration (particles x smoothing-length law x sightline set x bins x b / dv x walk)
one JSON line:
  prep_ms, deposit_ms   HIP events around the library's own stages (sample_prep,
                        spectra_deposit: zeroing, deposit and finalising pass), median of
                        --reps calls after --warmup calls, all in this one process
  pairs_tested, bin_adds
                        ASP_SAMPLE_COUNT of a separate counted call: (particle, sightline)
                        pairs tested and (pair, bin) adds issued; pairs_included: the sum of
                        an indicator-kernel asp_sample2d call on the same inputs
  bin_adds_per_s, added_bytes_per_s, fraction_of_fp32_rate
                        bin_adds / deposit_ms, 8 bytes each, against the 1.3 TB/s the
                        microarchitecture guide measures for contiguous fp32 atomics
  sample2d_deposit_ms   asp_sample2d (cubic column) on the same particles and points in the
                        same process: the pair-finding floor the deposit sits on
Particles: plummer_torch (float32, device-resident) in the box [-4, 4]^2, h either 0.75 pixel
pitches of a 4096^2 map ("pixel") or 1.2 (m / rho)^(1/3) ("physical").  Sightlines: uniform
in the box, or "copies": 10^4 copies of 10 positions drawn in [-1, 1]^2 (ten rows take every
add).  Velocities: vc uniform over the ring of K bins of width 1, b = (b / dv) for every
particle; ring mode.  ASP_SPECTRA_WALK 1 (the wave walks a pair's bins) and 0 (the lane that
found the pair does) are timed one after the other on the same arrays.  Configurations whose
accumulators (8 m K bytes) exceed --max-acc-gb or m K >= 2^31, or that do not fit --budget-s,
are reported as skipped.  There is no CPU fallback: without a GPU the tool fails.
"""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "astro-sph-tools_amd"))

FP32_ATOMIC_RATE = 1.3e12  # B/s of added bytes, contiguous global fp32 atomics
EXT = 4.0
KERNEL = 3  # cubic spline column


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, nargs="+", default=[10_000_000, 100_000_000])
    ap.add_argument("--laws", nargs="+", default=["pixel", "physical"])
    ap.add_argument("--sightlines", nargs="+", default=["100", "10000", "1000000", "copies"])
    ap.add_argument("--bins", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--b-over-dv", type=float, nargs="+", default=[2.0, 20.0])
    ap.add_argument("--walks", nargs="+", default=["1", "0"])
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--budget-s", type=float, default=600.0)
    ap.add_argument("--max-call-s", type=float, default=20.0,
                    help="a configuration whose counted call took longer is not timed")
    ap.add_argument("--max-acc-gb", type=float, default=16.0)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()

    import torch
    from asp_amd import _lib
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
        if kind == "copies":
            c = torch.rand((10, 2), dtype=torch.float64, device="cuda", generator=gen) * 2.0 - 1.0
            idx = torch.arange(100_000, device="cuda") % 10
            return c[idx, 0].contiguous(), c[idx, 1].contiguous()
        p = torch.rand((2, int(kind)), dtype=torch.float64, device="cuda", generator=gen) * (2 * EXT) - EXT
        return p[0].contiguous(), p[1].contiguous()

    def staged(fn, stages, reps):
        ms = {s: [] for s in stages}
        for _ in range(reps):
            _lib.profile(0, True, stages=stages)
            fn()
            torch.cuda.synchronize()
            p = _lib.profile_read(0)
            for s in stages:
                ms[s].append(p[s][0])
        _lib.profile(0, False)
        return {s: statistics.median(v) for s, v in ms.items()}, ms

    for n in a.particles:
        for law in a.laws:
            if time.perf_counter() - t_start > a.budget_s:
                emit({"tool": "spectra_bench", "particles": n, "h_law": law, "skipped": "budget"})
                continue
            s = plummer_torch(n, seed=3, h_law=law, extent=EXT, grid=4096)
            u, v, h, am = s["x"], s["y"], s["h"], s["m"]
            del s
            one = torch.ones_like(am)
            unit = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen)
            for kind in a.sightlines:
                px, py = point_set(kind)
                m = px.numel()
                col = torch.empty(m, dtype=torch.float32, device="cuda")

                def sample(amp=am, kid=KERNEL):
                    _lib.check(_lib.lib().asp_sample2d(P(u), P(v), P(h), P(amp), None, n, D(px), D(py), m,
                                                       kid, _lib.ASP_F_DEVICE_PTRS, P(col), None, 0, stream))

                t0 = time.perf_counter()
                sample(one, 2)
                included = int(col.double().sum().item())
                sample_s = time.perf_counter() - t0
                sample_ms = None
                if sample_s < a.max_call_s:
                    sample()
                    sample_ms = staged(sample, ("sample_prep", "sample_deposit"), a.reps)[0]
                for K in a.bins:
                    for ratio in a.b_over_dv:
                        base = {"tool": "spectra_bench", "particles": n, "h_law": law, "sightlines": kind,
                                "n_sightlines": m, "bins": K, "b_over_dv": ratio, "ring": True,
                                "kernel": "cubic_column", "pairs_included": included}
                        if m * K >= 2 ** 31 or 8.0 * m * K > a.max_acc_gb * 2 ** 30:
                            emit(dict(base, skipped="accumulators", acc_bytes=8 * m * K))
                            continue
                        if time.perf_counter() - t_start > a.budget_s:
                            emit(dict(base, skipped="budget"))
                            continue
                        vc = unit * float(K)
                        b = torch.full((n,), ratio, dtype=torch.float32, device="cuda")
                        out = torch.empty((m, K), dtype=torch.float32, device="cuda")

                        def call():
                            _lib.check(_lib.lib().asp_spectra2d(
                                P(u), P(v), P(h), P(am), None, D(vc), P(b), n, D(px), D(py), m, 0.0, 1.0, K,
                                1, KERNEL, _lib.ASP_F_DEVICE_PTRS, P(out), None, 0, stream))

                        for walk in a.walks:
                            os.environ["ASP_SPECTRA_WALK"] = walk
                            os.environ["ASP_SAMPLE_COUNT"] = "1"
                            t0 = time.perf_counter()
                            call()
                            torch.cuda.synchronize()
                            first_s = time.perf_counter() - t0
                            st = _lib.last_stats(0)
                            del os.environ["ASP_SAMPLE_COUNT"]
                            line = dict(base, walk=int(walk), pairs_tested=st["evals"],
                                        bin_adds=st["evals_small"], counted_call_s=round(first_s, 3))
                            if first_s > a.max_call_s:
                                emit(dict(line, skipped="call longer than --max-call-s"))
                                continue
                            for _ in range(a.warmup):
                                call()
                            med, ms = staged(call, ("sample_prep", "spectra_deposit"), a.reps)
                            dep = med["spectra_deposit"]
                            adds = st["evals_small"]
                            emit(dict(line, prep_ms=round(med["sample_prep"], 3), deposit_ms=round(dep, 3),
                                      deposit_ms_min_max=[round(min(ms["spectra_deposit"]), 3),
                                                          round(max(ms["spectra_deposit"]), 3)],
                                      reps=a.reps, bin_adds_per_s=round(adds / (dep * 1e-3)),
                                      added_bytes_per_s=round(8 * adds / (dep * 1e-3)),
                                      fraction_of_fp32_rate=round(8 * adds / (dep * 1e-3) / FP32_ATOMIC_RATE, 4),
                                      sample2d_prep_ms=None if sample_ms is None else round(
                                          sample_ms["sample_prep"], 3),
                                      sample2d_deposit_ms=None if sample_ms is None else round(
                                          sample_ms["sample_deposit"], 3)))
                        os.environ.pop("ASP_SPECTRA_WALK", None)
                        del vc, b, out
                del px, py, col
            del u, v, h, am, one, unit
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
