#!/usr/bin/env python3
"""Batched execute on the bench workload: 2 x UnitSphere(9) (N = 1 048 576 panels, theta = 0.5), charges uniform in [0, 1).
  python tools/batch_time.py [--orders 2,4,10] [--ks 1,2,4,8] [--reps 10] [--nv 2|4|8] [--shape 0|1|2] [--json]
Per order p: the single execute (ms, and its near-field kernel alone from fmmbem_plan_set_timing(2)), then per batch size k
the device batch (fmmbem_plan_execute_batch_device, torch's stream): ms per batch, ms per vector, and the near-field pass and P2M
pass per pass of the batch from the plan's stage timing, with the near matrix's bytes over the near pass time.  --nv / --shape
set FMMBEM_BATCH_NV / FMMBEM_BATCH_SHAPE (vectors per pass, rows x loads of the multi-vector SpMV) for sweeps."""
import argparse
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--orders", default="2,4,10")
    ap.add_argument("--ks", default="1,2,4,8")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--nv", type=int, default=None)
    ap.add_argument("--shape", type=int, default=None)
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    if a.nv is not None:
        os.environ["FMMBEM_BATCH_NV"] = str(a.nv)     # read once per process, at the first batch
    if a.shape is not None:
        os.environ["FMMBEM_BATCH_SHAPE"] = str(a.shape)
    import numpy as np
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import fmm_bem_relaxed_amd as fb

    v = np.concatenate([fb.unit_sphere(9), fb.unit_sphere(9, center=(3.0, 0.0, 0.0))])
    n = len(v)
    orders = [int(s) for s in a.orders.split(",")]
    ks = [int(s) for s in a.ks.split(",")]
    plan = fb.FMM_plan(fb.LaplaceSphericalBEM(max(orders), 3), v, p_max=max(10, max(orders)))
    dev = torch.device("cuda", 0)
    kmax = max(ks)
    X = torch.rand((kmax, n), dtype=torch.float64, generator=torch.Generator().manual_seed(1)).to(dev)
    Y = torch.empty((kmax, n), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    near_bytes = plan.stats()["near_bytes"]
    width = plan.batch_width()
    rows = []

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

    for p in orders:
        single = timed(lambda: plan.execute_device(X[0].data_ptr(), Y[0].data_ptr(), stream, p), a.reps)
        plan.set_timing(2)
        for _ in range(a.reps):
            plan.execute_device(X[0].data_ptr(), Y[0].data_ptr(), stream, p)
        near1 = plan.stats()["ms_near"]
        plan.set_timing(False)
        rows.append(dict(p=p, k=0, ms_batch=single, ms_per_vector=single, ms_near_pass=near1,
                         near_gbs=near_bytes / near1 / 1e6))
        for k in ks:
            run = lambda: plan.execute_batch_device(k, X.data_ptr(), n, Y.data_ptr(), n, stream, p)  # noqa: E731
            ms = timed(run, a.reps)
            plan.set_timing(True)
            for _ in range(a.reps):
                run()
            st = plan.stats()
            plan.set_timing(False)
            rows.append(dict(p=p, k=k, ms_batch=ms, ms_per_vector=ms / k, ms_near_pass=st["ms_near"], ms_p2m_pass=st["ms_p2m"],
                             near_gbs=near_bytes / st["ms_near"] / 1e6 if st["ms_near"] > 0 else 0.0))
    head = dict(n_panels=n, theta=0.5, batch_width=width, near_bytes=near_bytes,
                nv_env=os.environ.get("FMMBEM_BATCH_NV"), shape_env=os.environ.get("FMMBEM_BATCH_SHAPE"))
    if a.json:
        print(json.dumps(dict(head, rows=rows)))
        return
    print("N = %d, theta = 0.5, batch width %d, near matrix %.3f GB%s" % (
        n, width, near_bytes / 1e9, "" if not (a.nv or a.shape is not None) else "  (FMMBEM_BATCH_NV=%s FMMBEM_BATCH_SHAPE=%s)" % (
            head["nv_env"], head["shape_env"])))
    print("%3s %3s %10s %10s %12s %12s %9s" % ("p", "k", "ms/batch", "ms/vector", "near ms/pass", "p2m ms/pass", "near GB/s"))
    for r in rows:
        print("%3d %3s %10.3f %10.3f %12.3f %12s %9.0f" % (r["p"], "1*" if r["k"] == 0 else str(r["k"]), r["ms_batch"], r["ms_per_vector"],
                                                       r["ms_near_pass"], "%.3f" % r["ms_p2m_pass"] if "ms_p2m_pass" in r else "-", r["near_gbs"]))
    print("1*: single execute (fmmbem_plan_execute_device); its near ms: the near-field kernel alone")


if __name__ == "__main__":
    main()
