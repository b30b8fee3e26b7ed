#!/usr/bin/env python3
"""Time the exact block-Jacobi preconditioner (fmmbem_plan_block_inverse_*, csrc/kernels_blockinv.hip) on the two solves of
SURVEY.md section 8d:
  config 5   two disjoint UnitSphere(r), Laplace first kind, b = A_flipped * 1 (examples/LaplaceBEM.cpp:218-232), max_p 12
  config 4   RedBloodCell(r), Stokes, b = (4 pi, 0, 0) per panel (examples/StokesBEM.cpp:262-277), max_p 8
    python tools/block_inverse_time.py [--recursions 9] [--repeats 5] [--tol 1e-5] [--configs 5 4] [--out profiles/block_inverse_time.json]
Per config: the build time of the inverse (wall, the plan's blocks already assembled), the device time of one apply (mean of
--repeats between two events, after one warm-up) with the bytes it streams, and iterations and seconds of the C ABI's solver
(gmres_capi, relaxed p) with the identity, with the reference's block-diagonal inner-solver form (FGMRES, as its drivers run
it) and with the block inverse (GMRES).  Prints one JSON document and, when a GPU ran it, writes it to --out."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fmm_bem_relaxed_amd as fb  # noqa: E402


def config(which, r):
    """(name, panels, kernel factory, right-hand side on the device, stokes?)"""
    dev = torch.device("cuda", 0)
    if which == 5:
        v = np.concatenate([fb.unit_sphere(r, center=(3.0 * i, 0.0, 0.0)) for i in range(2)])
        n = len(v)
        kernel = lambda: fb.LaplaceSphericalBEM(12, 3)       # noqa: E731
        rhs = fb.FMM_plan(kernel(), v, bc=np.ones(n, dtype=np.uint8), p_max=12)
        b = rhs.execute_torch(torch.ones(n, dtype=torch.float64, device=dev))
        rhs.close()
        return "config 5: 2 x UnitSphere(%d), Laplace" % r, v, kernel, b, False

    def kernel():
        K = fb.StokesSphericalBEM(8, 4, 1e-3)
        K.set_Kfine(19)
        return K
    v = fb.red_blood_cell(r)
    b = torch.zeros((len(v), 3), dtype=torch.float64, device=dev)
    b[:, 0] = 4 * math.pi
    return "config 4: RedBloodCell(%d), Stokes" % r, v, kernel, b.reshape(-1), True


def solve(plan, b, so, stokes, M=None, flexible=False):
    torch.cuda.synchronize()
    x, it, res, secs = fb.gmres_capi(plan, torch.zeros_like(b), b, so, M=M, stokes=stokes, flexible=flexible)
    return dict(iterations=it, residual=res, solve_s=secs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recursions", type=int, default=9)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tol", type=float, default=1e-5)
    ap.add_argument("--configs", type=int, nargs="+", default=[5, 4], choices=[4, 5])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "block_inverse_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("block_inverse_time.py needs a GPU: nothing measured, nothing written")
    out = dict(device=torch.cuda.get_device_name(0), recursions=a.recursions, tol=a.tol, cases=[])
    for which in a.configs:
        name, v, kernel, b, stokes = config(which, a.recursions)
        K = kernel()
        plan = fb.FMM_plan(K, v, p_max=K.P)
        t0 = time.perf_counter()
        M = fb.BlockInverse(fb, kernel(), v)
        create_and_build_s = time.perf_counter() - t0
        twin = fb.BlockDiagonal(fb, kernel(), v)              # the reference's form, on a plan of its own
        t0 = time.perf_counter()
        twin.plan.block_inverse_build()                       # the inversion alone: the blocks are assembled
        build_s = time.perf_counter() - t0
        z = torch.empty_like(b)
        M.plan.block_inverse_apply_torch(b, out=z)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.repeats):
            M.plan.block_inverse_apply_torch(b, out=z)
        e1.record()
        torch.cuda.synchronize()
        apply_ms = e0.elapsed_time(e1) / a.repeats
        nbytes = M.plan.block_inverse_bytes()
        so = fb.SolverOptions(residual=a.tol, max_iters=100, restart=100, max_p=K.P)
        solve(plan, b, so, stokes)                            # untimed: the workspace allocation and first launches
        case = dict(config=name, n_panels=len(v), unknowns=b.numel(), plan_and_inverse_s=create_and_build_s, inverse_build_s=build_s,
                    apply_ms=apply_ms, apply_bytes=nbytes, apply_gb_per_s=nbytes / (apply_ms * 1e-3) / 1e9,
                    identity=solve(plan, b, so, stokes),
                    block_diagonal_inner_solver_fgmres=solve(plan, b, so, stokes, M=twin, flexible=True),
                    block_inverse_gmres=solve(plan, b, so, stokes, M=M))
        out["cases"].append(case)
        for pl in (plan, M.plan, twin.plan):
            pl.close()
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
