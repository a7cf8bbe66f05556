#!/usr/bin/env python
"""Writes tests/golden/g17_grid_diagonals.npz: which diagonal scipy's triangulation of an H x W pixel grid puts into every cell
(motion.grid_diagonals), at the sizes the flow-sampling tests use, so that the GPU tests need no scipy.

    sizes        [n, 2]  (H, W) of every mask
    mask_HxW     np.packbits of the bool [H-1, W-1] mask, row-major: True = the anti-diagonal (x+1, y)-(x, y+1) splits cell (x, y)
    scipy        the version of the scipy that answered

Needs scipy and nothing else beside this package; the masks are Qhull's answer for the points griddata is given.

    python tools/gen_grid_diagonals.py [--out tests/golden/g17_grid_diagonals.npz]
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
SIZES = [(2, 2), (5, 7), (24, 24), (37, 53)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g17_grid_diagonals.npz"))
    a = ap.parse_args()
    import scipy
    motion = importlib.import_module("iclr2025_3d-mom_amd.motion")
    out = {"sizes": np.asarray(SIZES, np.int32), "scipy": np.asarray(scipy.__version__)}
    for H, W in SIZES:
        mask = motion.grid_diagonals(H, W)
        out[f"mask_{H}x{W}"] = np.packbits(mask.reshape(-1))
        print(f"{H} x {W}: {mask.size} cells, {mask.mean():.3f} of them split by the anti-diagonal")
    np.savez(a.out, **out)
    print(f"{a.out}: scipy {scipy.__version__}")


if __name__ == "__main__":
    main()
