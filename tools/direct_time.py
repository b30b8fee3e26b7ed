#!/usr/bin/env python3
"""Time the device Direct sum (fb.Direct, csrc/kernels_direct.hip).
  python tools/direct_time.py [--repeats 5] [--no-baseline]
Cases: the symmetric form at N = 8 192 and 32 768 (UnitSphere(6), (7)), Laplace and Stokes; M = 8 exterior points against
N = 524 288 (UnitSphere(9)).  Times are device times of matvec_torch between two events (the mean of --repeats calls after one
warm-up); pairs/s = N M / time.  Unless --no-baseline, each case is also timed on the route the tree had before this sum existed:
  symmetric form   the CPU oracle's Direct (oracle.direct), what tests and bench.py use from Python;
  exterior points  fmmbem_kernel_entries for all 8 N pairs plus the additions on the host -- the calls and the loop of
                   Direct::matvec in include/fmmbem/compat/Direct.hpp, made from Python.
--quantity gradient|pressure|velocity_gradient (default matvec: everything above, unchanged) times that field quantity of the Direct
sum instead (fb.Direct.gradient_torch / pressure_torch / velocity_gradient_torch) at the same sizes -- the sources' own centroids
moved off the surface by 0.05 of their length as explicit points for N = 8 192 and 32 768 (the quantities have no symmetric form, and
a point ON a panel is the caller's business), and the 8 exterior points against N = 524 288 -- and, in the same run, apply on the same
points; ratio_to_apply = the quantity's pairs/s over apply's.  No baseline.
Prints one JSON document."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fmm_bem_relaxed_amd as fb  # noqa: E402


def kernel(kind):
    if kind == "laplace":
        return fb.LaplaceSphericalBEM(5, 3)
    K = fb.StokesSphericalBEM(5, 4, mu=1e-3)
    K.set_Kfine(19)
    return K


def device_ms(fn, repeats):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(repeats):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / repeats


def time_quantity(quantity, repeats):
    """the cases of main() for one field quantity, each beside apply on the same points"""
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    kind = "laplace" if quantity == "gradient" else "stokes"
    dof = 1 if kind == "laplace" else 3
    tail = {"gradient": (3,), "pressure": (), "velocity_gradient": (3, 3)}[quantity]
    out = dict(chunk=fb.lib().fmmbem_direct_chunk(), device=torch.cuda.get_device_name(0), quantity=quantity, cases=[])
    d8 = rng.normal(size=(8, 3))
    for r in (6, 7, 9):
        v = fb.unit_sphere(r)
        n = len(v)
        c = (v[:, 0] + v[:, 1] + v[:, 2]) / 3
        pts = np.ascontiguousarray(1.05 * c if r != 9 else 3 * d8 / np.linalg.norm(d8, axis=1)[:, None])
        m = len(pts)
        x = rng.normal(size=(n,) if dof == 1 else (n, 3))
        D = fb.Direct(kernel(kind), v)
        xd, pd = torch.from_numpy(x).to(dev), torch.from_numpy(pts).to(dev)
        y = torch.empty((m,) if dof == 1 else (m, 3), dtype=torch.float64, device=dev)
        o = torch.empty((m,) + tail, dtype=torch.float64, device=dev)
        ms_apply = device_ms(lambda: D.matvec_torch(xd, pd, out=y), repeats)
        ms = device_ms(lambda: getattr(D, quantity + "_torch")(xd, pd, out=o), repeats)
        D.close()
        out["cases"].append(dict(kernel=kind, form="points off the surface" if r != 9 else "exterior points", n_sources=n, n_targets=m, ms=ms,
                                 pairs_per_s=n * m / (ms * 1e-3), apply_ms=ms_apply, apply_pairs_per_s=n * m / (ms_apply * 1e-3),
                                 ratio_to_apply=ms_apply / ms))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--quantity", choices=("matvec", "gradient", "pressure", "velocity_gradient"), default="matvec")
    a = ap.parse_args()
    if a.quantity != "matvec":
        print(json.dumps(time_quantity(a.quantity, a.repeats), indent=1))
        return
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    out = dict(chunk=fb.lib().fmmbem_direct_chunk(), device=torch.cuda.get_device_name(0), cases=[])
    meshes = {r: fb.unit_sphere(r) for r in (6, 7, 9)}
    for kind in ("laplace", "stokes"):
        dof = 1 if kind == "laplace" else 3
        for r in (6, 7):
            v = meshes[r]
            n = len(v)
            x = rng.normal(size=(n,) if dof == 1 else (n, 3))
            D = fb.Direct(kernel(kind), v)
            xd = torch.from_numpy(x).to(dev)
            y = torch.empty_like(xd)
            ms = device_ms(lambda: D.matvec_torch(xd, out=y), a.repeats)
            case = dict(kernel=kind, form="symmetric", n_sources=n, n_targets=n, ms=ms, pairs_per_s=n * n / (ms * 1e-3))
            if not a.no_baseline:
                from oracle import oracle as O
                O.build()
                ctx = O.Oracle(v, K=3) if kind == "laplace" else O.StokesOracle(v, K=4, K_fine=19, mu=1e-3)
                t0 = time.perf_counter()
                ref = ctx.direct(x)
                case["oracle_direct_ms"] = (time.perf_counter() - t0) * 1e3
                case["oracle_threads"] = O.num_threads()
                case["rel_l2_vs_oracle"] = float(np.linalg.norm(y.cpu().numpy() - ref) / np.linalg.norm(ref))
                ctx.close()
            D.close()
            out["cases"].append(case)
        v = meshes[9]
        n = len(v)
        x = rng.normal(size=(n,) if dof == 1 else (n, 3))
        d = rng.normal(size=(8, 3))
        pts = np.ascontiguousarray(3 * d / np.linalg.norm(d, axis=1)[:, None])
        D = fb.Direct(kernel(kind), v)
        xd, pd = torch.from_numpy(x).to(dev), torch.from_numpy(pts).to(dev)
        y = torch.empty((8,) if dof == 1 else (8, 3), dtype=torch.float64, device=dev)
        ms = device_ms(lambda: D.matvec_torch(xd, pd, out=y), a.repeats)
        t0 = time.perf_counter()
        yh = D.matvec(x, targets=pts)
        case = dict(kernel=kind, form="exterior points", n_sources=n, n_targets=8, ms=ms, pairs_per_s=8 * n / (ms * 1e-3),
                    host_call_ms=(time.perf_counter() - t0) * 1e3)
        D.close()
        if not a.no_baseline:
            t0 = time.perf_counter()
            tri = np.repeat(pts[:, None, :], 3, axis=1)
            E = fb.kernel_entries(kernel(kind), np.repeat(tri, n, axis=0), np.tile(v, (8, 1, 1)))
            ref = np.einsum("ij,j->i", E.reshape(8, n), x) if dof == 1 else np.einsum("ijab,jb->ia", E.reshape(8, n, 3, 3), x)
            case["kernel_entries_route_ms"] = (time.perf_counter() - t0) * 1e3
            case["rel_l2_vs_kernel_entries_route"] = float(np.linalg.norm(yh - ref) / np.linalg.norm(ref))
        out["cases"].append(case)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
