#!/usr/bin/env python3
"""Time the velocity-gradient execute (FMM_plan.execute_velocity_gradient_torch, csrc/kernels_velgrad.hip) beside the velocity and
pressure executes of the same plan.
  python tools/field_velocity_gradient_time.py [--recursions 9] [--orders 8,4] [--repeats 10]
Workload: the field plan of tools/field_pressure_time.py -- RedBloodCell(recursions) (N = 524 288 panels by default) and a regular grid
of 1 048 576 points over the cell's bounding box, all VELOCITY targets, theta = 0.5, ncrit 64, K = 4, K_fine = 19.  Per order:
  ms_execute, ms_execute_pressure, ms_execute_velocity_gradient
                                    device time between two events, the mean of --repeats calls after two warm-ups, stage timing off;
  stages_velocity_gradient          fmmbem_plan_stats with stage timing on, in a pass of its own (an event pair per stage lengthens
                                    the execute): ms_near is near_velgrad_kernel, ms_l2p is l2p_velgrad_kernel;
  stages_execute                    the same for the velocity execute (ms_near: the near-matrix stream, ms_l2p: l2p_stokes_kernel).
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


def grid_targets(v, shape=(128, 128, 64)):
    """cell centres of a regular grid over the bounding box of the panels' vertices (tools/stokes_field_time.py)"""
    lo, hi = v.reshape(-1, 3).min(axis=0), v.reshape(-1, 3).max(axis=0)
    axes = [lo[k] + (hi[k] - lo[k]) * (np.arange(shape[k]) + 0.5) / shape[k] for k in range(3)]
    return np.ascontiguousarray(np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3))


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
    ap.add_argument("--orders", default="8,4")
    ap.add_argument("--repeats", type=int, default=10)
    a = ap.parse_args()
    orders = [int(p) for p in a.orders.split(",")]
    dev = torch.device("cuda", 0)
    v = fb.red_blood_cell(a.recursions)
    pts = grid_targets(v)
    K = fb.StokesSphericalBEM(max(orders), 4, 1e-3)
    K.set_Kfine(19)
    plan = fb.FMM_plan(K, v, p_max=max(orders)).field_plan(pts)
    st = plan.stats()
    out = dict(device=torch.cuda.get_device_name(0), n_panels=len(v), n_targets=len(pts), theta=0.5, ncrit=64, repeats=a.repeats,
               near_nnz=int(st["near_nnz"]), m2l_pairs=int(st["m2l_pairs"]), target_info=plan.target_info(), orders=[])
    xd = (torch.rand(3 * len(v), dtype=torch.float64, generator=torch.Generator().manual_seed(1)) - 0.5).to(dev)
    yd = torch.empty((len(pts), 3), dtype=torch.float64, device=dev)
    qd = torch.empty(len(pts), dtype=torch.float64, device=dev)
    gd = torch.empty((len(pts), 3, 3), dtype=torch.float64, device=dev)
    for p in orders:
        K.set_p(p)
        rec = dict(p=p)
        rec["ms_execute"] = device_ms(lambda: plan.execute_torch(xd, out=yd), a.repeats)
        rec["ms_execute_pressure"] = device_ms(lambda: plan.execute_pressure_torch(xd, out=qd), a.repeats)
        rec["ms_execute_velocity_gradient"] = device_ms(lambda: plan.execute_velocity_gradient_torch(xd, out=gd), a.repeats)
        rec["stages_execute"] = staged(plan, lambda: plan.execute_torch(xd, out=yd), a.repeats)
        rec["stages_velocity_gradient"] = staged(plan, lambda: plan.execute_velocity_gradient_torch(xd, out=gd), a.repeats)
        rec["ms_near_velgrad_kernel"] = rec["stages_velocity_gradient"]["ms_near"]
        rec["ms_l2p_velgrad_kernel"] = rec["stages_velocity_gradient"]["ms_l2p"]
        out["orders"].append(rec)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
