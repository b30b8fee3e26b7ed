#!/usr/bin/env python3
"""One execute on each kind of plan whose launchers choose between kernels (csrc/launch_choice.hpp), all at recursion 5, for a
kernel-name census before and after a change of the host code that chooses:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/launch_cases.py
  python tools/launch_cases.py names OUT          -> "calls name" per kernel, sorted by name

Two trees launch the same kernels when the two lists are the same (profiles/r17a_kernel_names_parent_and_new.txt)."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def names(d):
    f = glob.glob(os.path.join(d, "**", "*_kernel_stats.csv"), recursive=True)[0]
    for name, calls in sorted((r["Name"], int(r["Calls"])) for r in csv.DictReader(open(f))):
        print("%6d %s" % (calls, name))


def run():
    import numpy as np
    import torch
    import fmm_bem_relaxed_amd as fb

    rng = np.random.default_rng(17)
    v = np.concatenate([fb.unit_sphere(5), fb.unit_sphere(5, center=(3.0, 0.0, 0.0))])
    o = fb.FMMOptions()
    o.set_max_per_box(64)
    x = torch.from_numpy(rng.standard_normal(len(v))).cuda()

    pl = fb.FMM_plan(fb.LaplaceSphericalBEM(13, 3), v, o)
    for p in (3, 7, 8, 10, 13):
        pl.execute_torch(x, p=p)
    for k in (3, 8):                                          # batched executes
        pl.execute_batch_torch(torch.from_numpy(rng.standard_normal((k, len(v)))).cuda(), p=10)

    rbc = fb.red_blood_cell(4)
    xs = torch.from_numpy(rng.standard_normal(3 * len(rbc))).cuda()
    fb.FMM_plan(fb.StokesSphericalBEM(8, 3, 1e-3), rbc).execute_torch(xs)
    sb = fb.FMM_plan(fb.StokesSphericalBEM(8, 3, 1e-3), rbc, stokes_batch_width=3)
    sb.execute_batch_torch(torch.from_numpy(rng.standard_normal((3, 3 * len(rbc)))).cuda())

    pts = 1.5 * rng.standard_normal((300, 3))
    fb.FMM_plan(fb.LaplaceSphericalBEM(10, 3), fb.unit_sphere(5), targets=pts).execute_torch(
        torch.from_numpy(rng.standard_normal(len(fb.unit_sphere(5)))).cuda())

    f32 = fb.FMM_plan(fb.LaplaceSphericalBEM(8, 3), v, o, near_f32_max_p=5)
    f32.execute_torch(x, p=4)
    assert f32.stats()["last_near_f32"] == 1

    oh = fb.FMMOptions()
    oh.set_max_per_box(64)
    oh.near_stream_fraction = 0.5
    hy = fb.FMM_plan(fb.LaplaceSphericalBEM(10, 3), v, oh)
    hy.execute_torch(x)
    assert hy.stats()["near_recomputed_pairs"] > 0
    torch.cuda.synchronize()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "names":
        names(sys.argv[2])
    else:
        run()
