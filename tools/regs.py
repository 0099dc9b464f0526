#!/usr/bin/env python3
"""Register / LDS / occupancy table of the HIP kernels in one or more source files (gfx950).

Usage: python tools/regs.py SOURCE.hip [SOURCE.hip ...] [name-filter ...]
  e.g. the 2-D map's units:
       python tools/regs.py astro-sph-tools_amd/csrc/asp_map_bin.hip \\
           astro-sph-tools_amd/csrc/asp_map_deposit.hip astro-sph-tools_amd/csrc/asp_project2d.hip \\
           astro-sph-tools_amd/csrc/asp_pairs.hip astro-sph-tools_amd/csrc/asp_probes.hip
Arguments ending in .hip are sources; the rest are substrings a kernel's name must contain.
"""
import re
import subprocess
import sys

srcs = [a for a in sys.argv[1:] if a.endswith(".hip")]
filt = [a for a in sys.argv[1:] if not a.endswith(".hip")]
for src in srcs:
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC",
           "-ffp-contract=off", "-munsafe-fp-atomics", "--cuda-device-only", "-c", "-o", "/dev/null",
           src, "-Rpass-analysis=kernel-resource-usage"]
    if src.endswith("asp_project3d.hip"):
        cmd.append("-fno-slp-vectorize")  # the Makefile's per-file flag
    txt = subprocess.run(cmd, capture_output=True, text=True).stderr
    if len(srcs) > 1:
        print(f"== {src}")
    for b in txt.split("Function Name: ")[1:]:
        name = b.split()[0]
        # k_name<every integer / bool template argument> (or <f> / <d> for a type argument)
        m = re.search(r"_ZN3asp\w*?\d+(k_\w+?)(?:I((?:L[ib]\d+E)+)E|I([fd])E|E)", name)
        targs = re.findall(r"L[ib](\d+)E", m.group(2)) if m and m.group(2) else [m.group(3)] if m and m.group(3) else []
        short = m.group(1) + ("<%s>" % ",".join(targs) if targs else "") if m else name
        if filt and not any(f in short for f in filt):
            continue
        get = lambda k: (re.search(k + r": (\d+)", b) or [None, "?"])[1]  # noqa: E731
        occ, lds = get(r"Occupancy \[waves/SIMD\]"), get(r"LDS Size \[bytes/block\]")
        print(f"{short:30s} vgpr {get('VGPRs'):>4} spill {get('VGPRs Spill'):>3} occ {occ:>2} lds {lds:>6}")
