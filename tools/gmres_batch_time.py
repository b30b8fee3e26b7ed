#!/usr/bin/env python3
"""Multi-right-hand-side GMRES on config 5: 2 x UnitSphere(r) (r = 9: N = 1 048 576), first-kind Laplace, tol 1e-5, max_p 12,
restart 50, Bouras-Fraysse relaxation.  Right-hand sides b_j(i) = 1 / |c_i - q_j| at the panel centroids for charges q_j inside
the spheres (alternating between them, further and further from the centre).
  python tools/gmres_batch_time.py [--ks 2,4,8] [--reps 3] [--recursions 9] [--tol 1e-5] [--once] [--json]
Per k: the k sequential fmmbem_gmres_device solves and the one fmmbem_gmres_batch_device solve, both on a warm workspace (one
untimed run each), wall time around a device synchronisation, the minimum of --reps runs; the ratio; whether every system's
solution and history are bit-equal; and per iteration the order groups, read off the systems' order histories: the systems still
running, counted per order they asked for ("4": four systems at one order, "2+1": two at one order and one at another).  That
is the grouping, not the call count: a group is one fmmbem_plan_execute_batch_device call when its systems are equally spaced
in the workspace, more when a system between them has left, and a call wider than the plan's batch width is several near-field
passes.
--once: one batched solve at the largest k and nothing else (for a kernel trace)."""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="2,4,8")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--recursions", type=int, default=9)
    ap.add_argument("--tol", type=float, default=1e-5)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import fmm_bem_relaxed_amd as fb

    ks = [int(s) for s in a.ks.split(",")]
    kmax = max(ks)
    centers = np.array([[0.0, 0.0, 0.0], [3.0, 0.0, 0.0]])
    v = np.concatenate([fb.unit_sphere(a.recursions, center=tuple(c)) for c in centers])
    n = len(v)
    c = v.mean(axis=1)
    rng = np.random.default_rng(5)
    B = np.empty((kmax, n))
    for j in range(kmax):
        d = rng.normal(size=3)
        q = centers[j % 2] + 0.9 * (j // 2 + 1) / ((kmax + 1) // 2) * d / np.linalg.norm(d)
        B[j] = 1.0 / np.linalg.norm(c - q, axis=1)
    plan = fb.FMM_plan(fb.LaplaceSphericalBEM(12, 3), v, p_max=12)
    so = fb.SolverOptions(residual=a.tol, max_iters=50, restart=50, max_p=12, variable_p=True)
    Bd = torch.from_numpy(B).cuda()

    def batched(k, logs=None):
        X = torch.zeros((k, n), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, its, res, _ = fb.gmres_capi_batch(plan, X, Bd[:k], so, logs=logs)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, X, its, res

    def sequential(k, logs=None):
        X = torch.zeros((k, n), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        its = [fb.gmres_capi(plan, X[j], Bd[j], so, log=None if logs is None else logs[j])[1] for j in range(k)]
        torch.cuda.synchronize()
        return time.perf_counter() - t0, X, its

    if a.once:
        batched(kmax)                                  # the workspace and the batch buffers are allocated here
        dt, _, its, _ = batched(kmax)
        print("one batched solve, k = %d: %.2f ms, iterations %s" % (kmax, dt * 1e3, its))
        return
    rows = []
    for k in ks:
        ls, lb = [[] for _ in range(k)], [[] for _ in range(k)]
        _, Xs, its_s = sequential(k, ls)               # warm-up runs, kept for the comparison
        _, Xb, its_b, res = batched(k, lb)
        equal = bool(torch.equal(Xs, Xb)) and ls == lb and its_s == its_b
        t_seq = min(sequential(k)[0] for _ in range(a.reps))
        t_bat = min(batched(k)[0] for _ in range(a.reps))
        groups = []
        for i in range(max(its_b)):
            ps = [lb[j][i][1] for j in range(k) if i < its_b[j]]
            groups.append("+".join(str(ps.count(p)) for p in sorted(set(ps), reverse=True)))
        rows.append(dict(k=k, sequential_ms=t_seq * 1e3, batched_ms=t_bat * 1e3, ratio=t_bat / t_seq, bit_equal=equal,
                         iterations=its_b, residuals=res, groups=groups,
                         orders=[[p for _, p, _ in lb[j]] for j in range(k)]))
    head = dict(n_panels=n, tol=a.tol, max_p=12, restart=50, batch_width=plan.batch_width(), reps=a.reps)
    if a.json:
        print(json.dumps(dict(head, rows=rows)))
        return
    print("N = %d, tol %g, max_p 12, restart 50, batch width %d; wall ms, minimum of %d warm runs" % (n, a.tol, plan.batch_width(), a.reps))
    print("%3s %14s %12s %7s %9s  %s" % ("k", "sequential ms", "batched ms", "ratio", "bit-equal", "iterations"))
    for r in rows:
        print("%3d %14.2f %12.2f %7.3f %9s  %s" % (r["k"], r["sequential_ms"], r["batched_ms"], r["ratio"], r["bit_equal"], r["iterations"]))
    for r in rows:
        print("k = %d: order groups per iteration (running systems per order): %s" % (r["k"], " ".join(r["groups"])))
        for j, o in enumerate(r["orders"]):
            print("   system %d orders: %s" % (j, " ".join(str(p) for p in o)))


if __name__ == "__main__":
    main()
