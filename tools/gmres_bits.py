#!/usr/bin/env python3
"""Bit record of the device-resident GMRES (csrc/krylov.hip): for a fixed list of small solves the sha256 digest of the raw
solution bytes, the iteration count, the final residual and the p[] / resid[] histories (floats as hex, exact).
  python tools/gmres_bits.py [--out FILE]
The solver fixes the order of every sum and every host operation, so a change that only moves code must leave every entry as
it was: run this on the build before and on the build after (FMMBEM_LIB picks the library) and compare the two files byte for
byte.  Digests are tied to one compiler and one device generation.
The meshes: UnitSphere(4) (2 048 panels, p_max 8) and 2 x UnitSphere(5) with the last panel dropped (an odd n, p_max 10),
first-kind Laplace, right-hand sides 1 / |c - q_j| as in tests/test_gpu_gmres_batch.py.  Per mesh: fmmbem_gmres_device on
three systems under the Bouras-Fraysse and the Simoncini-Szyld relaxation and at fixed p; with restart 5 and max_iters 12;
with the DIAGONAL and the LOCAL preconditioner, each as GMRES and as FGMRES; with graphs on (fmmbem_plan_set_graphs), twice;
fmmbem_gmres with host pointers (plain and DIAGONAL); fmmbem_gmres_batch_device with k = 3.  And one Stokes red blood cell at
recursion 3, velocity, p_min 5."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

_DIRS = np.array([[1.0, 0.0, 0.0], [0.0, 0.6, 0.8], [-0.6, 0.0, 0.8]])
_FRACS = np.array([0.0, 0.9, 0.5])
K = 3


def rhs(v, centers):
    c = v.mean(axis=1)
    return np.stack([1.0 / np.linalg.norm(c - (np.asarray(centers[j % len(centers)]) + _FRACS[j] * _DIRS[j]), axis=1) for j in range(K)])


def entry(x, iterations, residual, log):
    return dict(sha256=hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest(), iterations=int(iterations),
                residual=float(residual).hex(), p=[int(p) for _, p, _ in log], resid=[float(r).hex() for _, _, r in log])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import fmm_bem_relaxed_amd as fb
    from fmm_bem_relaxed_amd import _capi
    from fmm_bem_relaxed_amd.solver import _c_options, _c_preconditioner

    record = {}

    def options(p_max, mode="bouras", **kw):
        args = dict(residual=1e-6, max_iters=100, max_p=p_max)
        args.update(kw)
        so = fb.SolverOptions(**args)
        if mode == "simoncini":
            so.relax_type = fb.SolverOptions.SIMONCINI
        elif mode == "fixed":
            so.variable_p = False
        return so

    def device(name, plan, B, so, systems=range(K), **kw):
        for j in systems:
            x = torch.zeros(B.shape[1], dtype=torch.float64, device="cuda")
            log = []
            _, it, res, _ = fb.gmres_capi(plan, x, torch.from_numpy(B[j]).cuda(), so, log=log, **kw)
            record["%s/system%d" % (name, j)] = entry(x.cpu().numpy(), it, res, log)

    def host(name, plan, B, so, M=None):
        o = _c_options(so, False, False, plan.kernel().P)
        pc = _c_preconditioner(M, "gmres_bits")
        if pc is not None:
            recip = M.recip.cpu().numpy()
            pc.reciprocals = recip.ctypes.data
        cap = so.max_iters + so.restart + 2
        ps, rs = (C.c_int32 * cap)(), (C.c_double * cap)()
        lg = _capi.SolverLog()
        lg.capacity, lg.p, lg.resid = cap, ps, rs
        x, b = np.zeros(B.shape[1]), np.ascontiguousarray(B[1])
        _capi.check(_capi.lib().fmmbem_gmres(plan._h, C.byref(o), x.ctypes.data, b.ctypes.data, C.byref(pc) if pc is not None else None, C.byref(lg)))
        record[name] = entry(x, lg.iterations, lg.residual, [(i + 1, ps[i], rs[i]) for i in range(lg.iterations)])

    def batched(name, plan, B, so, **kw):
        X = torch.zeros(B.shape, dtype=torch.float64, device="cuda")
        logs = [[] for _ in range(len(B))]
        _, its, res, _ = fb.gmres_capi_batch(plan, X, torch.from_numpy(B).cuda(), so, logs=logs, **kw)
        for j in range(len(B)):
            record["%s/system%d" % (name, j)] = entry(X[j].cpu().numpy(), its[j], res[j], logs[j])

    two = np.concatenate([fb.unit_sphere(5), fb.unit_sphere(5, center=(3.0, 0.0, 0.0))])[:-1]
    for mesh, v, p_max, centers in (("sphere4", fb.unit_sphere(4), 8, ((0.0, 0.0, 0.0),)),
                                    ("two5_odd", two, 10, ((0.0, 0.0, 0.0), (3.0, 0.0, 0.0)))):
        kernel = lambda: fb.LaplaceSphericalBEM(p_max, 3)
        plan = fb.FMM_plan(kernel(), v, p_max=p_max)
        B = rhs(v, centers)
        so = options(p_max)
        for mode in ("bouras", "simoncini", "fixed"):
            device("%s/device_%s" % (mesh, mode), plan, B, options(p_max, mode))
        device(mesh + "/device_restart5_max12", plan, B, options(p_max, restart=5, max_iters=12))
        diag, local = fb.Diagonal(plan), fb.LocalInnerSolver(fb, kernel(), v)
        for pc, M in (("diagonal", diag), ("local", local)):
            for flexible in (False, True):
                device("%s/device_%s_%s" % (mesh, pc, "fgmres" if flexible else "gmres"), plan, B, so, systems=(1,), M=M, flexible=flexible)
        host(mesh + "/host", plan, B, so)
        host(mesh + "/host_diagonal", plan, B, so, M=diag)
        batched(mesh + "/batch_device_k3", plan, B, so)
        graphs = fb.FMM_plan(kernel(), v, p_max=p_max)
        graphs.set_graphs(True)
        device(mesh + "/device_graphs", graphs, B, so, systems=(1,))
        device(mesh + "/device_graphs_again", graphs, B, so, systems=(1,))            # the second solve replays
        for p in (plan, local.plan, graphs):
            p.close()

    v = fb.red_blood_cell(3)
    Ks = fb.StokesSphericalBEM(10, 4, 1e-3)
    Ks.set_Kfine(19)
    plan = fb.FMM_plan(Ks, v, p_max=10)
    B = np.zeros((K, len(v), 3))
    B[0, :, 0] = 1.0
    B[1, :, 1] = v.mean(axis=1)[:, 0]
    B[2, :, 2] = v.mean(axis=1)[:, 1] + 0.25
    B = B.reshape(K, -1)
    so = options(10, residual=1e-5, p_min=5)
    device("stokes_rbc3/device", plan, B, so, stokes=True)
    batched("stokes_rbc3/batch_device_k3", plan, B.reshape(K, len(v), 3), so, stokes=True)
    plan.close()

    text = json.dumps(record, indent=1, sort_keys=True) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
