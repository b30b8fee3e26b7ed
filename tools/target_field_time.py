#!/usr/bin/env python3
"""A plan over separate target points on the bench workload: the potential of 2 x UnitSphere(9) (N = 1 048 576 panels,
p = 10, theta = 0.5) on a regular grid of 1 048 576 points over the bounding box of both spheres.
  python tools/target_field_time.py [--executes 20] [--sample 4096] [--flag 0|1] [--no-error] [--no-single]
Prints creation time, the mean stage times of the timed executes (fmmbem_plan_set_timing), the untimed execute time beside one
matvec of the single plan on the same panels, the near-matrix bytes, and the relative error against a Direct sum on a random
sample of the targets.  The Direct sum takes every pair in the far regime of the entry functions (the K-point rule,
kernel/LaplaceSphericalBEM.hpp:198-205, 246-258) from one formula over all panels, and the pairs in the near regime
(sqrt(2 A) / dist >= 0.5) from fmmbem_kernel_entries on degenerate target triangles -- the code that assembles the near matrix."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fmm_bem_relaxed_amd as fb  # noqa: E402


def grid_targets():
    nx, ny, nz = 256, 64, 64                          # 1 048 576 cell centres over [-1, 4] x [-1, 1] x [-1, 1]
    xs = -1 + 5 * (np.arange(nx) + 0.5) / nx
    ys = -1 + 2 * (np.arange(ny) + 0.5) / ny
    zs = -1 + 2 * (np.arange(nz) + 0.5) / nz
    g = np.stack(np.meshgrid(xs, ys, zs, indexing="ij"), axis=-1).reshape(-1, 3)
    return np.ascontiguousarray(g)


def direct_sample(v, x, pts, flag, k=3):
    """sum_j K(t, s_j) x_j at the points pts (see the module text)"""
    dev = torch.device("cuda", 0)
    qp, qw = fb.quadrature(k)
    V = torch.from_numpy(np.ascontiguousarray(v)).to(dev)                           # (N, 3, 3)
    Q = torch.einsum("qa,nac->nqc", torch.from_numpy(qp).to(dev), V)              # (N, K, 3)
    e0, e1 = V[:, 2] - V[:, 0], V[:, 1] - V[:, 0]
    c = torch.linalg.cross(e0, e1)
    area = 0.5 * torch.linalg.norm(c, dim=1)
    nrm = c / (2 * area)[:, None]
    cen = (V[:, 0] + V[:, 1] + V[:, 2]) / 3
    w = torch.from_numpy(qw).to(dev)
    xd = torch.from_numpy(x).to(dev)
    K = fb.LaplaceSphericalBEM(10, k)
    out = np.empty(len(pts))
    for c0 in range(0, len(pts), 32):
        t = torch.from_numpy(pts[c0:c0 + 32]).to(dev)                               # (T, 3)
        d = t[:, None, None, :] - Q[None]                                           # (T, N, K, 3)
        r = torch.linalg.norm(d, dim=3)
        if flag == 0:
            kern = (w * area[:, None] / r).sum(dim=2)
        else:
            kern = (w * area[:, None] * (-(d * nrm[None, :, None, :]).sum(dim=3)) / r ** 3).sum(dim=2)
        dist = torch.linalg.norm(t[:, None, :] - cen[None], dim=2)
        near = torch.sqrt(2 * area)[None, :] >= 0.5 * dist
        ti, sj = [a.cpu().numpy() for a in torch.nonzero(near, as_tuple=True)]
        if len(ti):
            tv = np.repeat(pts[c0 + ti][:, None, :], 3, axis=1)
            kern[ti, sj] = torch.from_numpy(fb.kernel_entries(K, tv, v[sj], np.full(len(ti), flag, np.uint8))).to(dev)
        out[c0:c0 + len(t)] = (kern @ xd).cpu().numpy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--executes", type=int, default=20)
    ap.add_argument("--sample", type=int, default=4096)
    ap.add_argument("--flag", type=int, default=0)
    ap.add_argument("--no-error", action="store_true")
    ap.add_argument("--no-single", action="store_true", help="skip the single plan's matvec (a kernel trace of the target plan alone)")
    a = ap.parse_args()
    v = np.concatenate([fb.unit_sphere(9), fb.unit_sphere(9, center=(3.0, 0.0, 0.0))])
    pts = grid_targets()
    K = fb.LaplaceSphericalBEM(10, 3)
    res = dict(n_panels=len(v), n_targets=len(pts), p=10, theta=0.5, flag=a.flag)
    dev = torch.device("cuda", 0)
    x = torch.rand(len(v), dtype=torch.float64, generator=torch.Generator().manual_seed(1)).to(dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    plan = fb.FMM_plan(K, v, targets=pts, target_bc=np.full(len(pts), a.flag, np.uint8))
    torch.cuda.synchronize()
    res["create_s"] = time.perf_counter() - t0
    st = plan.stats()
    res.update(build_host_ms=st["build_host_ms"], build_assemble_ms=st["build_assemble_ms"], near_bytes=st["near_bytes"],
               near_nnz=st["near_nnz"], m2l_pairs=st["m2l_pairs"], target_info=plan.target_info())
    y = torch.empty(len(pts), dtype=torch.float64, device=dev)

    def time_executes(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.executes):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.executes

    res["execute_ms"] = time_executes(lambda: plan.execute_torch(x, out=y))
    plan.set_timing(True)
    for _ in range(a.executes):
        plan.execute_torch(x, out=y)
    torch.cuda.synchronize()
    st = plan.stats()
    res["stages_ms"] = {k[3:]: round(st[k], 4) for k in ("ms_total", "ms_gather", "ms_near", "ms_scatter", "ms_p2m", "ms_m2m",
                                                          "ms_mh", "ms_m2l", "ms_l2l", "ms_l2p")}
    res["timed_executes"] = st["timed_executes"]
    plan.set_timing(False)
    if not a.no_single:
        single = fb.FMM_plan(fb.LaplaceSphericalBEM(10, 3), v)
        ys = torch.empty_like(x)
        res["single_plan_matvec_ms"] = time_executes(lambda: single.execute_torch(x, out=ys))
        res["single_plan_near_bytes"] = single.stats()["near_bytes"]
        single.close()
    if not a.no_error:
        yh = plan.execute_torch(x, out=y).cpu().numpy()
        rows = np.sort(np.random.default_rng(2).choice(len(pts), a.sample, replace=False))
        ref = direct_sample(v, x.cpu().numpy(), pts[rows], a.flag)
        res["sample"] = a.sample
        res["rel_l2_error_vs_direct"] = float(np.linalg.norm(yh[rows] - ref) / np.linalg.norm(ref))
        res["max_rel_error_vs_direct"] = float(np.max(np.abs(yh[rows] - ref)) / np.max(np.abs(ref)))
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
