#!/usr/bin/env python3
"""Time the gradient execute (FMM_plan.execute_gradient_torch, csrc/kernels_grad.hip) beside the potential execute of the same plan.
  python tools/field_gradient_time.py [--recursions 9] [--orders 4,10] [--repeats 10] [--flag 0|1|2]
Workload: the target plan of tools/target_field_time.py -- 2 x UnitSphere(recursions) (N = 1 048 576 panels by default) and a regular
grid of 1 048 576 points over the bounding box of both spheres, theta = 0.5, ncrit 64; --flag 2: the points' flags alternate (both
expansion slots live).  Per order:
  ms_execute, ms_execute_gradient   device time between two events, the mean of --repeats calls after two warm-ups, stage timing off;
  stages_gradient                   fmmbem_plan_stats with stage timing on, in a pass of its own (an event pair per stage lengthens
                                    the execute): ms_near is near_grad_kernel, ms_l2p is l2p_grad_kernel;
  stages_execute                    the same for the potential execute (ms_near: the near-matrix stream, ms_l2p: l2p_kernel).
Prints one JSON document."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fmm_bem_relaxed_amd as fb  # noqa: E402

STAGES = ("ms_gather", "ms_near", "ms_p2m", "ms_m2m", "ms_mh", "ms_m2l", "ms_l2l", "ms_l2p", "ms_scatter", "ms_total")


def grid_targets():
    nx, ny, nz = 256, 64, 64                          # 1 048 576 cell centres over [-1, 4] x [-1, 1] x [-1, 1]
    xs = -1 + 5 * (np.arange(nx) + 0.5) / nx
    ys = -1 + 2 * (np.arange(ny) + 0.5) / ny
    zs = -1 + 2 * (np.arange(nz) + 0.5) / nz
    return np.ascontiguousarray(np.stack(np.meshgrid(xs, ys, zs, indexing="ij"), axis=-1).reshape(-1, 3))


def device_ms(fn, repeats):
    fn()
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(repeats):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / repeats


def staged(plan, fn, repeats):
    plan.set_timing(True)
    for _ in range(repeats):
        fn()
    torch.cuda.synchronize()
    s = plan.stats()
    plan.set_timing(False)
    return {k: round(s[k], 4) for k in STAGES}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recursions", type=int, default=9)
    ap.add_argument("--orders", default="4,10")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--flag", type=int, default=0)
    a = ap.parse_args()
    orders = [int(p) for p in a.orders.split(",")]
    dev = torch.device("cuda", 0)
    v = np.concatenate([fb.unit_sphere(a.recursions), fb.unit_sphere(a.recursions, center=(3.0, 0.0, 0.0))])
    pts = grid_targets()
    flags = (np.arange(len(pts)) % 2).astype(np.uint8) if a.flag == 2 else np.full(len(pts), a.flag, np.uint8)
    K = fb.LaplaceSphericalBEM(max(orders), 3)
    plan = fb.FMM_plan(K, v, p_max=max(orders), targets=pts, target_bc=flags)
    st = plan.stats()
    out = dict(device=torch.cuda.get_device_name(0), n_panels=len(v), n_targets=len(pts), theta=0.5, ncrit=64, flag=a.flag,
               repeats=a.repeats, near_nnz=int(st["near_nnz"]), m2l_pairs=int(st["m2l_pairs"]), target_info=plan.target_info(), orders=[])
    xd = torch.rand(len(v), dtype=torch.float64, generator=torch.Generator().manual_seed(1)).to(dev)
    yd = torch.empty(len(pts), dtype=torch.float64, device=dev)
    gd = torch.empty((len(pts), 3), dtype=torch.float64, device=dev)
    for p in orders:
        K.set_p(p)
        rec = dict(p=p)
        rec["ms_execute"] = device_ms(lambda: plan.execute_torch(xd, out=yd), a.repeats)
        rec["ms_execute_gradient"] = device_ms(lambda: plan.execute_gradient_torch(xd, out=gd), a.repeats)
        rec["stages_execute"] = staged(plan, lambda: plan.execute_torch(xd, out=yd), a.repeats)
        rec["stages_gradient"] = staged(plan, lambda: plan.execute_gradient_torch(xd, out=gd), a.repeats)
        rec["ms_near_grad_kernel"] = rec["stages_gradient"]["ms_near"]
        rec["ms_l2p_grad_kernel"] = rec["stages_gradient"]["ms_l2p"]
        rec["near_pairs_per_s"] = out["near_nnz"] / (rec["ms_near_grad_kernel"] * 1e-3)
        out["orders"].append(rec)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
