#!/usr/bin/env python3
"""Time the treecode evaluator (FMMOptions.evaluator = "TREECODE", csrc/kernels_far.hip m2p_kernel) beside the FMM evaluator.
  python tools/treecode_time.py [--recursions 9] [--spheres 2] [--orders 4,10] [--repeats 10] [--ncrit 64] [--theta 0.5]
Workload: bench.py's (`--spheres` disjoint unit spheres of UnitSphere(recursions), centres 3 apart; N = 1 048 576 by default), a
treecode plan and an FMM plan of the same panels in one process.  Per order:
  ms per execute       device time of execute_torch between two events, the mean of --repeats calls after two warm-ups, stage
                       timing off;
  stage times          fmmbem_plan_stats with stage timing on, in a pass of its own (an event pair per stage lengthens the
                       execute): ms_m2l is the M2P kernel on the treecode plan and the M2L kernel on the FMM plan;
  m2p_row_sources      (row, source box) evaluations of one treecode execute: the sum over the M2L pairs of the rows of the target box;
  rel_l2_tree_vs_fmm   the two results against each other.
Prints one JSON document."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fmm_bem_relaxed_amd as fb  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recursions", type=int, default=9)
    ap.add_argument("--spheres", type=int, default=2)
    ap.add_argument("--orders", default="4,10")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--ncrit", type=int, default=64)
    ap.add_argument("--theta", type=float, default=0.5)
    a = ap.parse_args()
    orders = [int(p) for p in a.orders.split(",")]
    dev = torch.device("cuda", 0)
    parts = [fb.unit_sphere(a.recursions, center=(3.0 * i, 0.0, 0.0)) for i in range(a.spheres)]
    v = np.concatenate(parts) if len(parts) > 1 else parts[0]
    n = len(v)
    xd = torch.from_numpy(np.random.default_rng(1).random(n)).to(dev)
    out = dict(device=torch.cuda.get_device_name(0), n_panels=n, theta=a.theta, ncrit=a.ncrit, repeats=a.repeats, orders=[])
    plans = {}
    for which in ("TREECODE", "FMM"):
        opts = fb.FMMOptions()
        opts.set_mac_theta(a.theta)
        opts.set_max_per_box(a.ncrit)
        opts.evaluator = which
        K = fb.LaplaceSphericalBEM(max(orders), 3)
        plans[which] = (fb.FMM_plan(K, v, opts, p_max=max(orders)), K)
    tree = plans["TREECODE"][0]
    pairs, bx = tree.pairs("m2l"), tree.boxes()
    st = tree.stats()
    out.update(m2l_pairs=int(len(pairs)), n_leaves=int(st["n_leaves"]), n_levels=int(st["n_levels"]),
               m2p_row_sources=int((bx["be"] - bx["bb"])[pairs[:, 1]].astype(np.int64).sum()))
    for p in orders:
        rec = dict(p=p)
        y = {}
        for which, (plan, K) in plans.items():
            K.set_p(p)
            yd = torch.empty_like(xd)
            rec["ms_execute_" + which.lower()] = device_ms(lambda: plan.execute_torch(xd, out=yd), a.repeats)
            y[which] = yd.cpu().numpy()
            plan.set_timing(True)
            for _ in range(a.repeats):
                plan.execute_torch(xd, out=yd)
            torch.cuda.synchronize()
            s = plan.stats()
            plan.set_timing(False)
            rec["stages_" + which.lower()] = {k: s[k] for k in ("ms_near", "ms_p2m", "ms_m2m", "ms_mh", "ms_m2l", "ms_l2l", "ms_l2p", "ms_scatter", "ms_total")}
        rec["ms_m2p_kernel"] = rec["stages_treecode"]["ms_m2l"]
        rec["m2p_row_sources_per_s"] = out["m2p_row_sources"] / (rec["ms_m2p_kernel"] * 1e-3)
        rec["rel_l2_tree_vs_fmm"] = float(np.linalg.norm(y["TREECODE"] - y["FMM"]) / np.linalg.norm(y["FMM"]))
        out["orders"].append(rec)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
