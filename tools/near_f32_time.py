#!/usr/bin/env python3
"""The float near field (fmmbem_options.near_f32_max_p) against the FP64 near field, same build, same process, same run.
  python tools/near_f32_time.py [--kernel laplace|stokes] [--rec 9] [--orders 2,4,8] [--reps 20] [--shape 0..3] [--solve] [--json]
laplace: 2 x UnitSphere(rec) (rec 9: N = 1 048 576, the bench workload); stokes: RedBloodCell(rec), K = 4, K_fine = 19 (rec 9:
config 4).  Two plans of the same panels, one with the option off and one with the threshold at the largest order asked for.  Per
order p and plan: the whole single matvec (ms, HIP events around --reps warm executes) and its near-field kernel alone
(fmmbem_plan_set_timing(2)), with the bytes that kernel streams over its time.  --shape sets FMMBEM_F32_SHAPE (rows x loads x
workgroups per CU of the float kernels, kernels_near.hip launch_near_spmv_f32) for sweeps.
--solve (laplace): the config-5 solve (first-kind GMRES, max_p = 12, restart 50, tol 1e-5) through fmmbem_gmres_device with the
threshold at 0 and at --threshold (default 5, DESIGN.md section 8 "Float near field"): seconds, iterations, the order history."""
import argparse
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", default="laplace", choices=("laplace", "stokes"))
    ap.add_argument("--rec", type=int, default=9)
    ap.add_argument("--orders", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shape", type=int, default=None)
    ap.add_argument("--solve", action="store_true")
    ap.add_argument("--threshold", type=int, default=5)
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    if a.shape is not None:
        os.environ["FMMBEM_F32_SHAPE"] = str(a.shape)  # read once per process, at the first float pass
    import numpy as np
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import fmm_bem_relaxed_amd as fb

    stokes = a.kernel == "stokes"
    orders = [int(s) for s in (a.orders or ("4,8" if stokes else "2,4,8")).split(",")]
    dev = torch.device("cuda", 0)
    if stokes:
        v = fb.red_blood_cell(a.rec)
    else:
        v = np.concatenate([fb.unit_sphere(a.rec), fb.unit_sphere(a.rec, center=(3.0, 0.0, 0.0))])
    n = len(v)

    def kernel(p):
        if not stokes:
            return fb.LaplaceSphericalBEM(p, 3)
        K = fb.StokesSphericalBEM(p, 4, 1e-3)
        K.set_Kfine(19)
        return K

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    out = dict(kernel=a.kernel, n_panels=n, shape_env=os.environ.get("FMMBEM_F32_SHAPE"), rows=[])
    if not a.solve:
        pm = max(orders)
        plans = {"f64": fb.FMM_plan(kernel(pm), v, p_max=pm), "f32": fb.FMM_plan(kernel(pm), v, p_max=pm, near_f32_max_p=pm)}
        st = {k: pl.stats() for k, pl in plans.items()}
        out.update(near_bytes=st["f64"]["near_bytes"], near_f32_bytes=st["f32"]["near_f32_bytes"])
        m = n * plans["f64"].dof
        x = torch.rand(m, dtype=torch.float64, generator=torch.Generator().manual_seed(1)).to(dev)
        y = torch.empty(m, dtype=torch.float64, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        for p in orders:
            for name in ("f64", "f32", "f64", "f32"):      # interleaved, twice: drift of the box shows as a spread
                pl = plans[name]
                ms = timed(lambda: pl.execute_device(x.data_ptr(), y.data_ptr(), stream, p), a.reps)
                pl.set_timing(2)
                for _ in range(a.reps):
                    pl.execute_device(x.data_ptr(), y.data_ptr(), stream, p)
                s = pl.stats()
                pl.set_timing(False)
                nbytes = st["f32"]["near_f32_bytes"] if name == "f32" else st["f64"]["near_bytes"]
                assert s["last_near_f32"] == (1 if name == "f32" else 0)
                out["rows"].append(dict(p=p, near=name, ms_matvec=ms, ms_near=s["ms_near"], near_tbs=nbytes / s["ms_near"] / 1e9))
    else:
        if stokes:
            raise SystemExit("--solve: the Laplace config-5 solve only")
        rhs = fb.FMM_plan(kernel(12), v, bc=np.ones(n, dtype=np.uint8), p_max=12)
        b = rhs.execute_torch(torch.ones(n, dtype=torch.float64, device=dev))
        rhs.close()
        so = fb.SolverOptions(residual=1e-5, max_iters=50, restart=50, max_p=12, variable_p=True)
        sols = {}
        for k in (0, a.threshold):
            plan = fb.FMM_plan(kernel(12), v, p_max=12, near_f32_max_p=k)
            fb.gmres_capi(plan, torch.zeros_like(b), b, so)        # untimed: the workspace allocation and first launches
            secs = []
            for _ in range(5):
                log = []
                xk, it, res, s = fb.gmres_capi(plan, torch.zeros_like(b), b, so, log=log)
                secs.append(s)
            sols[k] = xk
            out["rows"].append(dict(threshold=k, iterations=it, residual=res, solve_s=sorted(secs), p_schedule=[q for _, q, _ in log],
                                    near_f32_bytes=plan.stats()["near_f32_bytes"]))
            plan.close()
        out["rel_diff_solutions"] = float(torch.linalg.vector_norm(sols[a.threshold] - sols[0]) / torch.linalg.vector_norm(sols[0]))
    if a.json:
        print(json.dumps(out))
        return
    print("%s, N = %d%s" % (a.kernel, n, "" if a.shape is None else "  (FMMBEM_F32_SHAPE=%d)" % a.shape))
    if not a.solve:
        print("near matrix %.3f GB FP64, %.3f GB float" % (out["near_bytes"] / 1e9, out["near_f32_bytes"] / 1e9))
        print("%3s %5s %10s %10s %10s" % ("p", "near", "ms/matvec", "near ms", "near TB/s"))
        for r in out["rows"]:
            print("%3d %5s %10.3f %10.3f %10.2f" % (r["p"], r["near"], r["ms_matvec"], r["ms_near"], r["near_tbs"]))
    else:
        for r in out["rows"]:
            print("threshold %2d: %d iterations, residual %.3e, solve s (5 runs, sorted) %s" % (
                r["threshold"], r["iterations"], r["residual"], " ".join("%.4f" % s for s in r["solve_s"])))
            print("   orders: %s" % " ".join(str(q) for q in r["p_schedule"]))
        print("relative difference of the two solutions: %.3e" % out["rel_diff_solutions"])


if __name__ == "__main__":
    main()
