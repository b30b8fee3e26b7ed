#!/usr/bin/env python3
"""Bit record of the near-field kernels: sha256 digests of the raw result bytes of a fixed list of small plans.
  python tools/near_bits.py [--out FILE] [--shapes-only]
The row loops of kernels_near.hip fix the order of every sum, so a change that only moves code must leave every digest as it
was: run this on the build before and on the build after (FMMBEM_LIB picks the library) and compare the two files byte for byte.
Per plan: near_device; execute at p_max and at p = 1; execute_batch with k = 2, 3, 4, 5.
The plans (fixed seeds): Laplace two spheres at recursion 4 and 5 with potential / normal-derivative / mixed flags, each plain,
with near_f32_max_p set and with near_stream_fraction = 0.6; Stokes red blood cell at recursion 4, velocity and traction, with and
without near_f32_max_p; one Laplace and one Stokes plan with max_per_box raised until a leaf has more than 1 024 near columns
(source panels; Stokes at recursion 5), so that the in-place second x chunk runs.
Every plan must hold a work item with fewer than 8 rows (the column-split path) and a leaf with an odd column count; the counts
are worked out from boxes() and near_row with the cutting rule of plan.hip, printed, and asserted after the digests.
--shapes-only: the shape counts from host-only plans (no GPU)."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

P_MAX = 6
F32_P = 3                    # executes at p <= 3 stream the float copy: p = 1 does, p_max does not
KS = (2, 3, 4, 5)


def item_rows(nr, row_bytes, item_bytes):
    """rows of the work items one leaf is cut into (plan.hip: the SpMV work items)"""
    per = max(1, item_bytes // row_bytes)
    per = per & ~7 if per >= 8 else min(4, nr)
    cnt = (nr + per - 1) // per
    per = (nr + cnt - 1) // cnt
    if per >= 8:
        per = (per + 7) & ~7
    return [min(per, nr - r0) for r0 in range(0, nr, per)]


def shapes(plan):
    b, perm, dof = plan.boxes(), plan.perm(), plan.dof
    short = odd = widest = 0
    for leaf, bb, be in zip(b["leaf"], b["bb"], b["be"]):
        if not leaf or be <= bb:
            continue
        ncp = len(plan.near_row(int(perm[bb]) * dof, values=False)[0]) // dof      # source panels of the leaf's rows
        if ncp == 0:
            continue
        rows = item_rows(int(be - bb), 48 * ncp, 512 << 10) if dof == 3 else item_rows(int(be - bb), 8 * ((ncp + 1) & ~1), 256 << 10)
        short += sum(1 for r in rows if r < 8)
        odd += ncp & 1
        widest = max(widest, ncp)
    return dict(items_under_8_rows=short, leaves_odd_columns=odd, widest_leaf_columns=widest)


def cases(fb):
    def two(rec):
        return np.concatenate([fb.unit_sphere(rec), fb.unit_sphere(rec, center=(3.0, 0.0, 0.0))])

    def opts(per_box=None, fraction=None):
        o = fb.FMMOptions()
        if per_box:
            o.set_max_per_box(per_box)
        if fraction:
            o.near_stream_fraction = fraction
        return o

    for rec in (4, 5):
        v = two(rec)
        n = len(v)
        for flags, bc in (("potential", np.zeros(n, np.uint8)), ("normal_deriv", np.ones(n, np.uint8)),
                          ("mixed", (np.arange(n) % 3 == 0).astype(np.uint8))):
            for form, kw in (("plain", {}), ("f32", dict(near_f32_max_p=F32_P)), ("hybrid0.6", dict(opts=opts(fraction=0.6)))):
                yield "laplace_r%d_%s_%s" % (rec, flags, form), False, lambda v=v, bc=bc, kw=kw, **k: fb.FMM_plan(
                    fb.LaplaceSphericalBEM(P_MAX, 3), v, bc=bc, p_max=P_MAX, **kw, **k)
    rbc = fb.red_blood_cell(4)

    def stokes(traction, **kw):
        K = fb.StokesSphericalBEM(P_MAX, 4, 1e-3)
        K.set_Kfine(19)
        bc = np.full(len(rbc), 1 if traction else 0, np.uint8)
        return fb.FMM_plan(K, rbc, bc=bc, p_max=P_MAX, **kw)

    for name, traction in (("velocity", False), ("traction", True)):
        for form, kw in (("plain", {}), ("f32", dict(near_f32_max_p=F32_P))):
            yield "stokes_r4_%s_%s" % (name, form), False, lambda traction=traction, kw=kw, **k: stokes(traction, **kw, **k)
    # a few extra panels beside the big leaves make a leaf's row count leave a short last item and its column count odd
    v4 = np.concatenate([two(4), fb.unit_sphere(2)[:11] * 0.2 + np.array((1.5, 0.0, 0.0))])
    yield "laplace_r4_wide", True, lambda **k: fb.FMM_plan(fb.LaplaceSphericalBEM(P_MAX, 3), v4, opts=opts(per_box=1100), p_max=P_MAX, **k)
    rbc5 = fb.red_blood_cell(5)
    rbc = np.concatenate([rbc5, rbc5[:5] * 0.2 + np.array((0.0, 0.0, 1.0))])
    yield "stokes_r5_wide", True, lambda **k: stokes(False, opts=opts(per_box=500), **k)


def digests(plan, seed):
    import torch
    dev = torch.device("cuda", plan.device)
    m = plan.n * plan.dof
    X = (np.random.default_rng(seed).random((max(KS), m)) - 0.3)
    xd = torch.from_numpy(X).to(dev)
    sha = lambda t: hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()
    out = {}
    y = torch.zeros(m, dtype=torch.float64, device=dev)
    plan.near_device(xd[0].data_ptr(), y.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    out["near_device"] = sha(y)
    for p in (P_MAX, 1):
        out["execute_p%d" % p] = sha(plan.execute_torch(xd[0].contiguous(), p=p))
    for k in KS:
        out["execute_batch_k%d" % k] = sha(plan.execute_batch_torch(xd[:k].contiguous(), p=P_MAX))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes-only", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import fmm_bem_relaxed_amd as fb

    record, bad = {}, []
    for seed, (name, wide, make) in enumerate(cases(fb)):
        plan = make(host_only=True) if a.shapes_only else make()
        s = shapes(plan)
        record[name] = dict(shapes=s) if a.shapes_only else dict(shapes=s, sha256=digests(plan, seed))
        print(name, json.dumps(s), file=sys.stderr)
        if s["items_under_8_rows"] < 1 or s["leaves_odd_columns"] < 1 or (wide and s["widest_leaf_columns"] <= 1024):
            bad.append(name)
        plan.close()
    text = json.dumps(record, indent=1, sort_keys=True) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    assert not bad, "these plans no longer cover the column-split / odd-column / second-chunk paths: %s" % bad


if __name__ == "__main__":
    main()
