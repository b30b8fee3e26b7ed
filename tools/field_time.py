#!/usr/bin/env python3
"""Time a field-quantity execute (FMM_plan.execute_gradient_torch, execute_hessian_torch, execute_pressure_torch or
execute_velocity_gradient_torch, csrc/kernels_field.hip) beside the potential or velocity execute of the same plan.
  python tools/field_time.py --quantity gradient|hessian|pressure|velocity_gradient|flow|representation [--recursions 9] [--orders ...] [--repeats 10] [--flag 0|1|2]
Workloads:
  gradient, hessian   the target plan of tools/target_field_time.py -- 2 x UnitSphere(recursions) (N = 1 048 576 panels by default)
                      and a regular grid of 1 048 576 points over the bounding box of both spheres, theta = 0.5, ncrit 64;
                      --flag 2: the points' flags alternate (both expansion slots live).  Orders 4,10.
  pressure,           the field plan of tools/stokes_field_time.py -- RedBloodCell(recursions) (N = 524 288 panels by default) and a
  velocity_gradient   regular grid of 1 048 576 points over the cell's bounding box, all VELOCITY targets, theta = 0.5, ncrit 64,
                      K = 4, K_fine = 19.  Orders 8,4.
Per order, with <q> the quantity and <k> its kernels' short name (grad, hess, pressure, velgrad):
  ms_execute, ms_execute_<q>     device time between two events, the mean of --repeats calls after two warm-ups, stage timing off
                                 (velocity_gradient also times ms_execute_pressure);
  stages_<q>                     fmmbem_plan_stats with stage timing on, in a pass of its own (an event pair per stage lengthens
                                 the execute): ms_near is the quantity's near kernel, ms_l2p its L2P kernel, repeated as
                                 ms_near_<k>_kernel and ms_l2p_<k>_kernel;
  stages_execute                 the same for the potential or velocity execute (ms_near: the near-matrix stream, ms_l2p: l2p_kernel
                                 or l2p_stokes_kernel).
--quantity flow: the flow execute (FMM_plan.execute_flow_device: velocity, pressure and velocity gradient on one far chain) on the
Stokes workload, beside the three single executes in the same process.  Per order, --rounds (default 3) alternating rounds of
{pressure, velocity_gradient, velocity, flow asking q and G, flow asking u, q and G}, each timed as above:
  ms_execute, ms_execute_pressure, ms_execute_velocity_gradient, ms_execute_flow_qg, ms_execute_flow   the means over the rounds;
  rounds                         every round's five figures; spread_ms: the largest (max - min) over the rounds of any of them;
  ms_singles_qg, ms_singles      pressure + velocity_gradient, and that + velocity: what the two flow figures stand against;
  stages_flow, stages_flow_qg, stages_pressure, stages_velocity_gradient, stages_execute    the stage means;
  ms_near_flow_kernel            the one near kernel for q and G alone (stage timing 2: events around the near stage only) and
  ms_near_pressure_kernel, ms_near_velgrad_kernel   the two single near kernels the same way; their sum is what it stands against;
  bits_equal                     every output of both flow forms against the single executes' results (torch.equal).
--quantity representation: the representation execute (FMM_plan.execute_representation_device: both Laplace layers, value and
gradient, on one far chain) on the gradient's workload, beside the four single executes it replaces -- execute and execute_gradient
on an all-0 and an all-1 plan over the same points -- in the same process.  Per order, --rounds alternating rounds of {value of the
single layer, value of the double layer, the two gradients, the representation execute asking both outputs, the value alone, the
gradient alone}, each timed as above:
  ms_execute_single, ms_execute_double, ms_gradient_single, ms_gradient_double, ms_representation, ms_representation_value,
  ms_representation_gradient     the means over the rounds; rounds: every round's figures; spread_ms as for flow;
  ms_four, ms_two_values, ms_two_gradients   the sums the three representation figures stand against;
  stages_representation, stages_gradient_single, stages_gradient_double, stages_execute_single    the stage means;
  ms_near_representation_kernel  the one near kernel (stage timing 2) and ms_near_grad_single_kernel, ms_near_grad_double_kernel the
                                 two gradient passes the same way: their sum is what it stands against;
  rel_l2_value, rel_l2_gradient  the representation execute against the four executes' S - D, relative to |S| + |D|.
--check M (default 0: off): the Direct quantity (fb.Direct.gradient_torch / hessian_torch / pressure_torch / velocity_gradient_torch: all N panels,
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
QUANTITIES = {"gradient": ("grad", (3,), "4,10"), "hessian": ("hess", (3, 3), "4,10"), "pressure": ("pressure", (), "8,4"), "velocity_gradient": ("velgrad", (3, 3), "8,4"),
              "flow": ("flow", (3, 3), "8"), "representation": ("representation", (3,), "4,10")}


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


def near_ms(plan, fn, repeats):
    """ms_near with events around the near stage only (stage timing 2)"""
    plan.set_timing(2)
    for _ in range(repeats):
        fn()
    torch.cuda.synchronize()
    ms = plan.stats()["ms_near"]
    plan.set_timing(False)
    return round(ms, 4)


def flow_orders(plan, K, orders, xd, n_targets, repeats, rounds):
    """the records of --quantity flow, one per order"""
    dev = xd.device
    ud, u1 = (torch.empty((n_targets, 3), dtype=torch.float64, device=dev) for _ in range(2))
    qd, q1 = (torch.empty(n_targets, dtype=torch.float64, device=dev) for _ in range(2))
    gd, g1 = (torch.empty((n_targets, 3, 3), dtype=torch.float64, device=dev) for _ in range(2))
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream
    calls = {
        "ms_execute_pressure": lambda: plan.execute_pressure_torch(xd, out=q1),
        "ms_execute_velocity_gradient": lambda: plan.execute_velocity_gradient_torch(xd, out=g1),
        "ms_execute": lambda: plan.execute_torch(xd, out=u1),
        "ms_execute_flow_qg": lambda: plan.execute_flow_device(xd.data_ptr(), 0, qd.data_ptr(), gd.data_ptr(), stream()),
        "ms_execute_flow": lambda: plan.execute_flow_device(xd.data_ptr(), ud.data_ptr(), qd.data_ptr(), gd.data_ptr(), stream()),
    }
    recs = []
    for p in orders:
        K.set_p(p)
        rec = dict(p=p, rounds=[])
        for _ in range(rounds):
            rec["rounds"].append({k: round(device_ms(fn, repeats), 4) for k, fn in calls.items()})
        for k in calls:
            rec[k] = round(sum(r[k] for r in rec["rounds"]) / rounds, 4)
        rec["spread_ms"] = round(max(max(r[k] for r in rec["rounds"]) - min(r[k] for r in rec["rounds"]) for k in calls), 4)
        rec["ms_singles_qg"] = round(rec["ms_execute_pressure"] + rec["ms_execute_velocity_gradient"], 4)
        rec["ms_singles"] = round(rec["ms_singles_qg"] + rec["ms_execute"], 4)
        for name, key in (("execute", "ms_execute"), ("pressure", "ms_execute_pressure"), ("velocity_gradient", "ms_execute_velocity_gradient"),
                          ("flow_qg", "ms_execute_flow_qg"), ("flow", "ms_execute_flow")):
            rec["stages_" + name] = staged(plan, calls[key], repeats)
        rec["ms_near_flow_kernel"] = near_ms(plan, calls["ms_execute_flow_qg"], repeats)
        rec["ms_near_pressure_kernel"] = near_ms(plan, calls["ms_execute_pressure"], repeats)
        rec["ms_near_velgrad_kernel"] = near_ms(plan, calls["ms_execute_velocity_gradient"], repeats)
        for k in ("ms_execute_pressure", "ms_execute_velocity_gradient", "ms_execute"):
            calls[k]()
        equal = True
        for k, outs in (("ms_execute_flow_qg", ((qd, q1), (gd, g1))), ("ms_execute_flow", ((ud, u1), (qd, q1), (gd, g1)))):
            for t in (ud, qd, gd):
                t.fill_(float("nan"))
            calls[k]()
            torch.cuda.synchronize()
            equal = equal and all(torch.equal(a, b) for a, b in outs)
        rec["bits_equal"] = bool(equal)
        recs.append(rec)
    return recs


def representation_orders(plans, K, orders, sd, md, n_targets, repeats, rounds):
    """the records of --quantity representation, one per order; plans: the all-0 and the all-1 plan over the points"""
    zero, one = plans
    dev = sd.device
    new = lambda *tail: torch.empty((n_targets,) + tail, dtype=torch.float64, device=dev)
    S, D, gS, gD, phi, grad = new(), new(), new(3), new(3), new(), new(3)
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream
    rep = lambda f, g: zero.execute_representation_device(sd.data_ptr(), md.data_ptr(), f, g, stream())
    calls = {
        "ms_execute_single": lambda: zero.execute_torch(sd, out=S),
        "ms_execute_double": lambda: one.execute_torch(md, out=D),
        "ms_gradient_single": lambda: zero.execute_gradient_torch(sd, out=gS),
        "ms_gradient_double": lambda: one.execute_gradient_torch(md, out=gD),
        "ms_representation": lambda: rep(phi.data_ptr(), grad.data_ptr()),
        "ms_representation_value": lambda: rep(phi.data_ptr(), 0),
        "ms_representation_gradient": lambda: rep(0, grad.data_ptr()),
    }
    recs = []
    for p in orders:
        K.set_p(p)
        rec = dict(p=p, rounds=[])
        for _ in range(rounds):
            rec["rounds"].append({k: round(device_ms(fn, repeats), 4) for k, fn in calls.items()})
        for k in calls:
            rec[k] = round(sum(r[k] for r in rec["rounds"]) / rounds, 4)
        rec["spread_ms"] = round(max(max(r[k] for r in rec["rounds"]) - min(r[k] for r in rec["rounds"]) for k in calls), 4)
        rec["ms_two_values"] = round(rec["ms_execute_single"] + rec["ms_execute_double"], 4)
        rec["ms_two_gradients"] = round(rec["ms_gradient_single"] + rec["ms_gradient_double"], 4)
        rec["ms_four"] = round(rec["ms_two_values"] + rec["ms_two_gradients"], 4)
        for name, plan, key in (("execute_single", zero, "ms_execute_single"), ("gradient_single", zero, "ms_gradient_single"),
                                ("gradient_double", one, "ms_gradient_double"), ("representation", zero, "ms_representation")):
            rec["stages_" + name] = staged(plan, calls[key], repeats)
        rec["ms_near_representation_kernel"] = near_ms(zero, calls["ms_representation"], repeats)
        rec["ms_near_representation_gradient_kernel"] = near_ms(zero, calls["ms_representation_gradient"], repeats)
        rec["ms_near_grad_single_kernel"] = near_ms(zero, calls["ms_gradient_single"], repeats)
        rec["ms_near_grad_double_kernel"] = near_ms(one, calls["ms_gradient_double"], repeats)
        for fn in calls.values():
            fn()
        calls["ms_representation"]()
        torch.cuda.synchronize()
        norm = torch.linalg.norm
        rec["rel_l2_value"] = float(norm(phi - (S - D)) / (norm(S) + norm(D)))
        rec["rel_l2_gradient"] = float(norm(grad - (gS - gD)) / (norm(gS) + norm(gD)))
        recs.append(rec)
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quantity", choices=sorted(QUANTITIES), required=True)
    ap.add_argument("--recursions", type=int, default=9)
    ap.add_argument("--orders", default=None)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--flag", type=int, default=0)
    ap.add_argument("--check", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    q = a.quantity
    laplace = q in ("gradient", "hessian")
    if a.flag and not laplace:
        ap.error("--flag belongs to --quantity gradient and hessian: the Stokes quantities take VELOCITY targets only")
    short, tail, default_orders = QUANTITIES[q]
    orders = [int(p) for p in (a.orders or default_orders).split(",")]
    dev = torch.device("cuda", 0)
    extra = {}
    if q == "representation":
        if a.check > 0:
            ap.error("--check belongs to the single quantities: the representation execute is held to the four executes (rel_l2_*)")
        v = np.concatenate([fb.unit_sphere(a.recursions), fb.unit_sphere(a.recursions, center=(3.0, 0.0, 0.0))])
        pts = sphere_grid()
        K = fb.LaplaceSphericalBEM(max(orders), 3)
        plans = [fb.FMM_plan(K, v, p_max=max(orders), targets=pts, target_bc=np.full(len(pts), f, np.uint8)) for f in (0, 1)]
        sd, md = (torch.rand(len(v), dtype=torch.float64, generator=torch.Generator().manual_seed(seed)).to(dev) for seed in (1, 2))
        st = plans[0].stats()
        out = dict(device=torch.cuda.get_device_name(0), n_panels=len(v), n_targets=len(pts), theta=0.5, ncrit=64, repeats=a.repeats,
                   rounds=a.rounds, near_nnz=int(st["near_nnz"]), m2l_pairs=int(st["m2l_pairs"]), target_info=plans[0].target_info())
        out["orders"] = representation_orders(plans, K, orders, sd, md, len(pts), a.repeats, a.rounds)
        print(json.dumps(out, indent=1))
        return
    if laplace:
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
    if q == "flow":
        if a.check > 0:
            ap.error("--check belongs to the single quantities: the flow execute is held to them bit for bit (bits_equal)")
        out["rounds"] = a.rounds
        out["orders"] = flow_orders(plan, K, orders, xd, len(pts), a.repeats, a.rounds)
        print(json.dumps(out, indent=1))
        return
    od = torch.empty((len(pts),) + tail, dtype=torch.float64, device=dev)
    qd = torch.empty(len(pts), dtype=torch.float64, device=dev) if q == "velocity_gradient" else None
    run = getattr(plan, "execute_%s_torch" % q)
    direct = None
    if a.check > 0:
        # the Direct quantity on a sample spread over the whole target set (tools/stokes_field_time.py does this for the velocity)
        rows = np.sort(np.random.default_rng(2).choice(len(pts), min(a.check, len(pts)), replace=False))
        rows_d, sample = torch.from_numpy(rows).to(dev), torch.from_numpy(pts[rows]).to(dev)
        direct = fb.Direct(K, v)
        args = (xd, sample, torch.from_numpy(flags[rows]).to(dev)) if laplace else (xd, sample)
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
        if laplace:
            rec["near_pairs_per_s"] = out["near_nnz"] / (rec["ms_near_%s_kernel" % short] * 1e-3)
        if direct is not None:
            got = run(xd, out=od)[rows_d]
            rec["rel_l2_vs_direct_on_sample"] = float(torch.linalg.norm(got - ref) / torch.linalg.norm(ref))
        out["orders"].append(rec)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
