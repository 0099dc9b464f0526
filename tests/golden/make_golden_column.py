#!/usr/bin/env python3
"""Generate the column-kernel fixtures G13 / G14 by RUNNING THE REFERENCE.

The recipe is make_golden.py's (the reference's sources compiled in a scratch directory
under /tmp, nothing copied into the repository; see that file's header).  The reference's
``create_image`` runs on G3's inputs (Plummer 1e4 -> 256^2, Z axis, +-2, chunk 16, read
back from g3_plummer_1e4_256.npz) with a plain NumPy callable handed to its
``kernel_func`` plug-in point, exactly as G6 does for Wendland C2 -- here the closed-form
column-integrated kernels of tests/column_ref.py:

    g13_cubic_column.npz         img: cubic spline integrated along the line of sight
    g14_wendland_c2_column.npz   img: Wendland C2 integrated along the line of sight

Usage:  python tests/golden/make_golden_column.py   (a few minutes)
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import column_ref  # noqa: E402
import make_golden  # noqa: E402


def main():
    t0 = time.time()
    ref, Axes, _ = make_golden.build_reference()
    create_image = ref["create_image"]
    g3 = np.load(os.path.join(HERE, "g3_plummer_1e4_256.npz"))
    pos, h, A = (g3[k].astype(np.float64) for k in ("pos", "h", "A"))
    size, cs, ext = tuple(int(s) for s in g3["size"]), int(g3["cs"]), tuple(g3["ext"])
    assert int(g3["axis"]) == 2
    for name, kernel in (("g13_cubic_column", "cubic_column"),
                         ("g14_wendland_c2_column", "wendland_c2_column")):
        img = create_image(pos, h, A, size, cs, Axes.Z, *ext,
                           kernel_func=column_ref.CALLABLES[kernel])
        np.savez_compressed(os.path.join(HERE, name + ".npz"), img=img)
        print(f"{name}: sum img * pitch^2 = {img.sum() * ((ext[1] - ext[0]) / size[0]) ** 2:.6g}, "
              f"sum A = {A.sum():.6g}")
    print(f"column fixtures written in {time.time() - t0:.1f}s")


if __name__ == "__main__":
    main()
