#!/usr/bin/env python3
"""A Stokes field plan at the Stokes headline size: the field of a layer on RedBloodCell(9) (N = 524 288 panels, p = 8, theta = 0.5)
on a regular grid of 1 048 576 points over the cell's bounding box (fmmbem_plan_create_field through FMM_plan.field_plan).
  python tools/stokes_field_time.py [--executes 20] [--sample 4096] [--recursions 9] [--classes velocity,traction]
Per flag class (all targets VELOCITY: the single layer, 8 expansion slots; all TRACTION: the double layer, 11): creation time, the
untimed execute time, the mean stage times of the timed executes (fmmbem_plan_set_timing), the near-matrix bytes, and the relative
L2 error against the device Direct sum (fb.Direct) on a random sample of the points -- with, for scale, the time of that Direct sum
on the sample alone.  One JSON document on stdout."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fmm_bem_relaxed_amd as fb  # noqa: E402


def grid_targets(v, shape=(128, 128, 64)):
    """cell centres of a regular grid over the bounding box of the panels' vertices"""
    lo, hi = v.reshape(-1, 3).min(axis=0), v.reshape(-1, 3).max(axis=0)
    axes = [lo[k] + (hi[k] - lo[k]) * (np.arange(shape[k]) + 0.5) / shape[k] for k in range(3)]
    return np.ascontiguousarray(np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--executes", type=int, default=20)
    ap.add_argument("--sample", type=int, default=4096)
    ap.add_argument("--recursions", type=int, default=9)
    ap.add_argument("--classes", default="velocity,traction")
    a = ap.parse_args()
    p = 8
    v = fb.red_blood_cell(a.recursions)
    pts = grid_targets(v)
    K = fb.StokesSphericalBEM(p, 4, 1e-3)
    K.set_Kfine(19)
    dev = torch.device("cuda", 0)
    x = (torch.rand(3 * len(v), dtype=torch.float64, generator=torch.Generator().manual_seed(1)) - 0.5).to(dev)
    res = dict(n_panels=len(v), n_targets=len(pts), p=p, theta=0.5, executes=a.executes, sample=a.sample, classes={})
    rows = np.sort(np.random.default_rng(2).choice(len(pts), min(a.sample, len(pts)), replace=False))
    sample = torch.from_numpy(pts[rows]).to(dev)
    operator = fb.FMM_plan(K, v, p_max=p)                  # the solve's plan: the field plans take its panels and options
    direct = fb.Direct(K, v)

    def timed(fn, reps):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    for name in a.classes.split(","):
        flag = {"velocity": 0, "traction": 1}[name]
        out = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plan = operator.field_plan(pts, np.full(len(pts), flag, np.uint8))
        torch.cuda.synchronize()
        out["create_s"] = time.perf_counter() - t0
        st = plan.stats()
        out.update(build_host_ms=st["build_host_ms"], build_assemble_ms=st["build_assemble_ms"], near_bytes=st["near_bytes"],
                   near_nnz=st["near_nnz"], m2l_pairs=st["m2l_pairs"], expansion_slots=st["expansion_slots"], target_info=plan.target_info())
        y = torch.empty((len(pts), 3), dtype=torch.float64, device=dev)
        out["execute_ms"] = timed(lambda: plan.execute_torch(x, out=y), a.executes)
        plan.set_timing(True)
        for _ in range(a.executes):
            plan.execute_torch(x, out=y)
        torch.cuda.synchronize()
        st = plan.stats()
        out["stages_ms"] = {k[3:]: round(st[k], 4) for k in ("ms_total", "ms_gather", "ms_near", "ms_scatter", "ms_p2m", "ms_m2m",
                                                              "ms_mh", "ms_m2l", "ms_l2l", "ms_l2p")}
        out["timed_executes"] = st["timed_executes"]
        plan.set_timing(False)
        yh = plan.execute_torch(x, out=y)[torch.from_numpy(rows).to(dev)]
        bc = torch.full((len(rows),), flag, dtype=torch.uint8, device=dev)
        ref = direct.matvec_torch(x, sample, bc)
        out["rel_l2_error_vs_direct"] = float(torch.linalg.norm(yh - ref) / torch.linalg.norm(ref))
        out["direct_on_sample_ms"] = timed(lambda: direct.matvec_torch(x, sample, bc), 3)
        out["direct_on_all_targets_ms_extrapolated"] = out["direct_on_sample_ms"] * len(pts) / len(rows)
        plan.close()
        res["classes"][name] = out
    direct.close()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
