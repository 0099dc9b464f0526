#!/usr/bin/env python3
"""Same-process A/B of the 2-D map's layout reuse: 10^7 particles -> 2048^2,
weighted map, with ASP_REUSE_LAYOUT=0 and =1, per-call milliseconds (HIP events around each
call) for three callers:

  a  identical calls;
  b  the same particles, new a0 / a1 arrays every call;
  c  the positions rewritten in place before every call (another particle set each time;
     the rewrite itself is not timed).

Printed per (pattern, switch): the median and the spread of the steady calls, the calls'
``layout_reuse`` codes and, for c, the first rewritten call on its own -- with reuse on it is
the one call that pays a rejected scatter.  Usage: python tools/layout_reuse_ab.py [n] [grid]"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "astro-sph-tools_amd"))
import torch  # noqa: E402
from asp_amd.device import project2d, stats  # noqa: E402
from asp_amd.plummer import plummer_torch  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
G = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
CALLS = 24
dev = torch.device("cuda:0")
sets = [plummer_torch(n, seed=s, h_law="pixel", extent=4.0, grid=G, device=dev) for s in (0, 1, 2)]
u, v, h = (sets[0][k].clone() for k in ("x", "y", "h"))
props = [((d["m"] * d["T"]).contiguous(), d["m"]) for d in sets]
o = torch.empty((2, G, G), dtype=torch.float32, device=dev)
ext = (-4.0, 4.0, -4.0, 4.0)


def call(a0, a1):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    project2d(u, v, h, a0, a1, image_size=(G, G), extent=ext, kernel="wendland_c2", ratio=True,
              out0=o[0], out1=o[1])
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1), stats(0)["layout_reuse"]


def rewrite(k):
    for t, key in ((u, "x"), (v, "y")):
        t.copy_(sets[k % 3][key])
    torch.cuda.synchronize()


def pattern(p):
    rewrite(0)
    for _ in range(3):  # warm: buffers sized, the record buffer placed, reuse armed
        call(*props[0])
    out = []
    for k in range(CALLS):
        if p == "c":
            rewrite(k + 1)
        out.append(call(*props[k % 3] if p == "b" else props[0]))
    return out


for rep in range(2):
    for p in "abc":
        for switch in ("0", "1"):
            os.environ["ASP_REUSE_LAYOUT"] = switch
            r = pattern(p)
            ms = sorted(t for t, _ in r[1:])
            codes = "".join(str(c) for _, c in r)
            # (pattern c, reuse on: the first rewritten call is the one rejected scatter)
            first = (f", first rewritten call {r[0][0]:.3f} ms" if p == "c" and switch == "1"
                     else "")
            print(f"rep {rep} pattern {p} reuse {switch}: median {ms[len(ms) // 2]:.3f} ms "
                  f"(min {ms[0]:.3f}, max {ms[-1]:.3f}){first}, layout_reuse {codes}",
                  flush=True)
