#!/usr/bin/env python3
"""The multi-vector near field of Stokes plans (fmmbem_options.stokes_batch_width) on the stokes_rbc workload of bench.py:
StokesSphericalBEM velocity BC on RedBloodCell(9) (N = 524 288 panels), p = 8, k = 4, K_fine = 19, mu = 1e-3, theta = 0.5.
  python tools/stokes_batch_time.py [--recursions 9] [--p 8] [--widths 1,2,3,4] [--reps 100] [--rounds 3] [--json]
Per width w, on a plan created with that width (1: a plan without the option), a batch of k = w vectors through
fmmbem_plan_execute_batch_device on torch's stream: ms per batch, ms per vector, and the near-field pass per pass of the batch from
the plan's stage timing (width 1: the near-field kernel of the single execute, fmmbem_plan_set_timing(2)), with the near matrix's
bytes over that time.  Times are HIP events around --reps calls after a warm-up call; the widths are visited --rounds times in
turn and the smallest and the largest mean of a width are both reported.  The plans of all widths are alive at once (each holds
its own near matrix, 12.7 GB at the default size), so that the rounds can alternate between them."""
import argparse
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recursions", type=int, default=9)
    ap.add_argument("--p", type=int, default=8)
    ap.add_argument("--widths", default="1,2,3,4")
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import fmm_bem_relaxed_amd as fb

    v = fb.red_blood_cell(a.recursions)
    n = len(v)
    widths = [int(s) for s in a.widths.split(",")]
    dev = torch.device("cuda", 0)
    kmax = max(widths)
    X = torch.rand((kmax, 3 * n), dtype=torch.float64, generator=torch.Generator().manual_seed(1)).to(dev)
    Y = torch.empty((kmax, 3 * n), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def kernel():
        K = fb.StokesSphericalBEM(a.p, 4, 1e-3)
        K.set_Kfine(19)
        return K

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps

    # the plans share one geometry (fmmbem_plan_create recognises it); each holds its own near matrix
    plans = {w: fb.FMM_plan(kernel(), v, p_max=a.p, stokes_batch_width=w) for w in widths}
    near_bytes = plans[widths[0]].stats()["near_bytes"]
    for w, pl in plans.items():
        if pl.batch_width() != max(1, w):
            raise SystemExit("width %d is not active on this plan (batch_width() = %d)" % (w, pl.batch_width()))
    ms = {w: [] for w in widths}
    near = {w: [] for w in widths}
    for _ in range(a.rounds):
        for w in widths:
            pl = plans[w]
            if w <= 1:
                run = lambda: pl.execute_device(X[0].data_ptr(), Y[0].data_ptr(), stream, a.p)  # noqa: E731
            else:
                run = lambda: pl.execute_batch_device(w, X.data_ptr(), 3 * n, Y.data_ptr(), 3 * n, stream, a.p)  # noqa: E731
            ms[w].append(timed(run))
            pl.set_timing(2 if w <= 1 else True)
            for _ in range(a.reps):
                run()
            near[w].append(pl.stats()["ms_near"])
            pl.set_timing(False)
    rows = []
    for w in widths:
        k = max(1, w)
        rows.append(dict(width=w, k=k, ms_batch_min=min(ms[w]), ms_batch_max=max(ms[w]), ms_per_vector_min=min(ms[w]) / k,
                         ms_per_vector_max=max(ms[w]) / k, ms_near_pass_min=min(near[w]), ms_near_pass_max=max(near[w]),
                         near_gbs=near_bytes / min(near[w]) / 1e6 if min(near[w]) > 0 else 0.0))
    head = dict(n_panels=n, p=a.p, theta=0.5, near_bytes=near_bytes, reps=a.reps, rounds=a.rounds)
    if a.json:
        print(json.dumps(dict(head, rows=rows)))
        return
    print("RedBloodCell(%d), N = %d panels, p = %d, near matrix %.3f GB, %d rounds of %d calls" % (
        a.recursions, n, a.p, near_bytes / 1e9, a.rounds, a.reps))
    print("%5s %3s %17s %17s %17s %9s" % ("width", "k", "ms/batch", "ms/vector", "near ms/pass", "near GB/s"))
    for r in rows:
        print("%5d %3d %8.3f-%8.3f %8.3f-%8.3f %8.3f-%8.3f %9.0f" % (
            r["width"], r["k"], r["ms_batch_min"], r["ms_batch_max"], r["ms_per_vector_min"], r["ms_per_vector_max"],
            r["ms_near_pass_min"], r["ms_near_pass_max"], r["near_gbs"]))
    print("width 1: the single execute (fmmbem_plan_execute_device) of a plan without the option; its near ms: the near-field kernel alone")


if __name__ == "__main__":
    main()
