#!/usr/bin/env python3
"""Time a field-quantity execute (FMM_plan.execute_gradient_torch, execute_pressure_torch or execute_velocity_gradient_torch,
csrc/kernels_field.hip) beside the potential or velocity execute of the same plan.
  python tools/field_time.py --quantity gradient|pressure|velocity_gradient [--recursions 9] [--orders ...] [--repeats 10] [--flag 0|1|2]
Workloads:
  gradient            the target plan of tools/target_field_time.py -- 2 x UnitSphere(recursions) (N = 1 048 576 panels by default)
                      and a regular grid of 1 048 576 points over the bounding box of both spheres, theta = 0.5, ncrit 64;
                      --flag 2: the points' flags alternate (both expansion slots live).  Orders 4,10.
  pressure,           the field plan of tools/stokes_field_time.py -- RedBloodCell(recursions) (N = 524 288 panels by default) and a
  velocity_gradient   regular grid of 1 048 576 points over the cell's bounding box, all VELOCITY targets, theta = 0.5, ncrit 64,
                      K = 4, K_fine = 19.  Orders 8,4.
Per order, with <q> the quantity and <k> its kernels' short name (grad, pressure, velgrad):
  ms_execute, ms_execute_<q>     device time between two events, the mean of --repeats calls after two warm-ups, stage timing off
                                 (velocity_gradient also times ms_execute_pressure);
  stages_<q>                     fmmbem_plan_stats with stage timing on, in a pass of its own (an event pair per stage lengthens
                                 the execute): ms_near is the quantity's near kernel, ms_l2p its L2P kernel, repeated as
                                 ms_near_<k>_kernel and ms_l2p_<k>_kernel;
  stages_execute                 the same for the potential or velocity execute (ms_near: the near-matrix stream, ms_l2p: l2p_kernel
                                 or l2p_stokes_kernel).
--check M (default 0: off): the Direct quantity (fb.Direct.gradient_torch / pressure_torch / velocity_gradient_torch: all N panels,
every regime) on M points sampled over the whole target set; per order rel_l2_vs_direct_on_sample, the relative L2 of the field
execute against it on those points, and under "check" the sample's size and the device time of that sum.
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
# quantity -> (its kernels' short name, the trailing shape of its result, the default orders)
QUANTITIES = {"gradient": ("grad", (3,), "4,10"), "pressure": ("pressure", (), "8,4"), "velocity_gradient": ("velgrad", (3, 3), "8,4")}


def sphere_grid():
    nx, ny, nz = 256, 64, 64                          # 1 048 576 cell centres over [-1, 4] x [-1, 1] x [-1, 1]
    xs = -1 + 5 * (np.arange(nx) + 0.5) / nx
    ys = -1 + 2 * (np.arange(ny) + 0.5) / ny
    zs = -1 + 2 * (np.arange(nz) + 0.5) / nz
    return np.ascontiguousarray(np.stack(np.meshgrid(xs, ys, zs, indexing="ij"), axis=-1).reshape(-1, 3))


def box_grid(v, shape=(128, 128, 64)):
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
    ap.add_argument("--quantity", choices=sorted(QUANTITIES), required=True)
    ap.add_argument("--recursions", type=int, default=9)
    ap.add_argument("--orders", default=None)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--flag", type=int, default=0)
    ap.add_argument("--check", type=int, default=0)
    a = ap.parse_args()
    q = a.quantity
    if a.flag and q != "gradient":
        ap.error("--flag belongs to --quantity gradient: the Stokes quantities take VELOCITY targets only")
    short, tail, default_orders = QUANTITIES[q]
    orders = [int(p) for p in (a.orders or default_orders).split(",")]
    dev = torch.device("cuda", 0)
    extra = {}
    if q == "gradient":
        v = np.concatenate([fb.unit_sphere(a.recursions), fb.unit_sphere(a.recursions, center=(3.0, 0.0, 0.0))])
        pts = sphere_grid()
        flags = (np.arange(len(pts)) % 2).astype(np.uint8) if a.flag == 2 else np.full(len(pts), a.flag, np.uint8)
        K = fb.LaplaceSphericalBEM(max(orders), 3)
        plan = fb.FMM_plan(K, v, p_max=max(orders), targets=pts, target_bc=flags)
        extra = dict(flag=a.flag)
        xd = torch.rand(len(v), dtype=torch.float64, generator=torch.Generator().manual_seed(1)).to(dev)
        yd = torch.empty(len(pts), dtype=torch.float64, device=dev)
    else:
        v = fb.red_blood_cell(a.recursions)
        pts = box_grid(v)
        K = fb.StokesSphericalBEM(max(orders), 4, 1e-3)
        K.set_Kfine(19)
        plan = fb.FMM_plan(K, v, p_max=max(orders)).field_plan(pts)
        xd = (torch.rand(3 * len(v), dtype=torch.float64, generator=torch.Generator().manual_seed(1)) - 0.5).to(dev)
        yd = torch.empty((len(pts), 3), dtype=torch.float64, device=dev)
    st = plan.stats()
    out = dict(device=torch.cuda.get_device_name(0), n_panels=len(v), n_targets=len(pts), theta=0.5, ncrit=64, **extra, repeats=a.repeats,
               near_nnz=int(st["near_nnz"]), m2l_pairs=int(st["m2l_pairs"]), target_info=plan.target_info(), orders=[])
    od = torch.empty((len(pts),) + tail, dtype=torch.float64, device=dev)
    qd = torch.empty(len(pts), dtype=torch.float64, device=dev) if q == "velocity_gradient" else None
    run = getattr(plan, "execute_%s_torch" % q)
    direct = None
    if a.check > 0:
        # the Direct quantity on a sample spread over the whole target set (tools/stokes_field_time.py does this for the velocity)
        rows = np.sort(np.random.default_rng(2).choice(len(pts), min(a.check, len(pts)), replace=False))
        rows_d, sample = torch.from_numpy(rows).to(dev), torch.from_numpy(pts[rows]).to(dev)
        direct = fb.Direct(K, v)
        args = (xd, sample, torch.from_numpy(flags[rows]).to(dev)) if q == "gradient" else (xd, sample)
        sum_on_sample = getattr(direct, q + "_torch")
        ref = sum_on_sample(*args)
        out["check"] = dict(sample=len(rows), direct_on_sample_ms=device_ms(lambda: sum_on_sample(*args), 1))
        out["check"]["direct_on_all_targets_ms_extrapolated"] = out["check"]["direct_on_sample_ms"] * len(pts) / len(rows)
    for p in orders:
        K.set_p(p)
        rec = dict(p=p)
        rec["ms_execute"] = device_ms(lambda: plan.execute_torch(xd, out=yd), a.repeats)
        if q == "velocity_gradient":
            rec["ms_execute_pressure"] = device_ms(lambda: plan.execute_pressure_torch(xd, out=qd), a.repeats)
        rec["ms_execute_" + q] = device_ms(lambda: run(xd, out=od), a.repeats)
        rec["stages_execute"] = staged(plan, lambda: plan.execute_torch(xd, out=yd), a.repeats)
        rec["stages_" + q] = staged(plan, lambda: run(xd, out=od), a.repeats)
        rec["ms_near_%s_kernel" % short] = rec["stages_" + q]["ms_near"]
        rec["ms_l2p_%s_kernel" % short] = rec["stages_" + q]["ms_l2p"]
        if q == "gradient":
            rec["near_pairs_per_s"] = out["near_nnz"] / (rec["ms_near_grad_kernel"] * 1e-3)
        if direct is not None:
            got = run(xd, out=od)[rows_d]
            rec["rel_l2_vs_direct_on_sample"] = float(torch.linalg.norm(got - ref) / torch.linalg.norm(ref))
        out["orders"].append(rec)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
