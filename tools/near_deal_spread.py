#!/usr/bin/env python3
"""Bytes of near matrix each persistent workgroup of near_spmv_pipe_kernel streams under the static deal (csrc/plan.hip: a leaf's
row block cut into row ranges of <= 256 KB, sorted largest first, item i to workgroup i mod grid).  Needs no GPU: the tree and
the near pairs come from a host-only plan.

  python tools/near_deal_spread.py [--recursions 9] [--spheres 2] [--ncrit 64] [--grid 1280]

Prints max, mean and min bytes per workgroup, the largest item and the item counts: the window over which the workgroups of one
launch finish is (max - min) bytes at what one workgroup streams."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fmm_bem_relaxed_amd as fb  # noqa: E402

ITEM_BYTES = 256 << 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recursions", type=int, default=9)
    ap.add_argument("--spheres", type=int, default=2)
    ap.add_argument("--ncrit", type=int, default=64)
    ap.add_argument("--grid", type=int, default=1280)
    a = ap.parse_args()
    v = np.concatenate([fb.unit_sphere(a.recursions, center=(3.0 * i, 0.0, 0.0)) for i in range(a.spheres)])
    opts = fb.FMMOptions()
    opts.set_max_per_box(a.ncrit)
    pl = fb.FMM_plan(fb.LaplaceSphericalBEM(10, 3), v, opts, host_only=True)
    b, pr = pl.boxes(), pl.pairs("p2p")
    rows = (b["be"] - b["bb"]).astype(np.int64)
    ncols = np.bincount(pr[:, 0], weights=rows[pr[:, 1]], minlength=len(rows)).astype(np.int64)
    items = []
    for box in np.nonzero((b["leaf"] != 0) & (rows > 0) & (ncols > 0))[0]:
        nr, row_bytes = int(rows[box]), int((ncols[box] + 1) & ~1) * 8
        per = max(1, ITEM_BYTES // row_bytes)
        per = per & ~7 if per >= 8 else min(4, nr)
        cnt = (nr + per - 1) // per
        per = (nr + cnt - 1) // cnt
        if per >= 8:
            per = (per + 7) & ~7
        items += [min(per, nr - r0) * row_bytes for r0 in range(0, nr, per)]
    items = np.sort(np.array(items, dtype=np.int64), kind="stable")[::-1]
    grid = min(a.grid, len(items))
    per_wg = np.bincount(np.arange(len(items)) % grid, weights=items, minlength=grid)
    print("N = %d, %d leaves, %d items (%.1f per workgroup), %.3f GB" % (len(v), int((b["leaf"] != 0).sum()), len(items), len(items) / grid, items.sum() / 1e9))
    print("item bytes: max %d, mean %.0f, min %d" % (items.max(), items.mean(), items.min()))
    print("bytes per workgroup of %d: max %d, mean %.0f, min %d; max - min %d, max - mean %.0f" %
          (grid, per_wg.max(), per_wg.mean(), per_wg.min(), per_wg.max() - per_wg.min(), per_wg.max() - per_wg.mean()))


if __name__ == "__main__":
    main()
