#!/usr/bin/env python3
"""Executes on each kind of plan whose host code chooses between kernels or between paths of the execute (csrc/launch_choice.hpp,
fmmbem_plan::run / run_batch / far_chain in csrc/plan.hip), all at recursion 4 or 5, for a kernel census before and after a change
of that host code.  Run it once, alone, under a kernel trace and a time limit:

  timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/launch_cases.py
  python tools/launch_cases.py names OUT          -> "calls name" per kernel, sorted by name
  python tools/launch_cases.py order OUT          -> the kernel names in dispatch order, case by case

Two trees launch the same kernels when the two `names` lists are the same, and launch them in the same order when the two `order`
lists are (profiles/r17a_kernel_names_parent_and_new.txt, profiles/r21a_launches_parent_and_new.txt).  A case ends with a one-element
torch cosine, which `order` turns into the case's heading; the hybrid plan runs two streams side by side, so its case is listed
sorted with counts."""
import collections
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ["laplace p = 3 7 8 10 13, batches of 3 and 8", "stokes, stokes batch of 3", "laplace target plan", "float near field",
         "treecode, treecode batch of 3", "stokes field plans: VELOCITY, TRACTION targets", "graphs: three executes at p = 8",
         "stage timing", "split execute, two shards", "hybrid near field"]
UNORDERED = {"hybrid near field"}
MARK = "cos_kernel"


def _csv(d, suffix):
    return list(csv.DictReader(open(glob.glob(os.path.join(d, "**", "*_" + suffix + ".csv"), recursive=True)[0])))


def names(d):
    for name, calls in sorted((r["Name"], int(r["Calls"])) for r in _csv(d, "kernel_stats")):
        print("%6d %s" % (calls, name))


def order(d):
    rows = _csv(d, "kernel_trace")
    key = "Dispatch_Id" if rows and "Dispatch_Id" in rows[0] else "Start_Timestamp"
    rows.sort(key=lambda r: int(r[key]))
    case, held = 0, []
    for r in rows + [None]:
        if r is not None and MARK not in r["Kernel_Name"]:
            held.append(r["Kernel_Name"])
            continue
        print("== %s" % (CASES[case] if case < len(CASES) else "after the last case"))
        if case < len(CASES) and CASES[case] in UNORDERED:
            for name, calls in sorted(collections.Counter(held).items()):
                print("%6d %s" % (calls, name))
        else:
            for name in held:
                print(name)
        case, held = case + 1, []


def run():
    import numpy as np
    import torch
    import fmm_bem_relaxed_amd as fb

    rng = np.random.default_rng(17)
    done = []

    def end_of(case):
        assert case == CASES[len(done)]
        done.append(case)
        torch.zeros(1, device="cuda").cos_()
        torch.cuda.synchronize()

    def vec(*shape):
        return torch.from_numpy(rng.standard_normal(shape)).cuda()

    v = np.concatenate([fb.unit_sphere(5), fb.unit_sphere(5, center=(3.0, 0.0, 0.0))])
    o = fb.FMMOptions()
    o.set_max_per_box(64)
    x = vec(len(v))

    pl = fb.FMM_plan(fb.LaplaceSphericalBEM(13, 3), v, o)
    for p in (3, 7, 8, 10, 13):
        pl.execute_torch(x, p=p)
    for k in (3, 8):                                          # batched executes
        pl.execute_batch_torch(vec(k, len(v)), p=10)
    end_of(CASES[0])

    rbc = fb.red_blood_cell(4)
    xs = vec(3 * len(rbc))
    fb.FMM_plan(fb.StokesSphericalBEM(8, 3, 1e-3), rbc).execute_torch(xs)
    sb = fb.FMM_plan(fb.StokesSphericalBEM(8, 3, 1e-3), rbc, stokes_batch_width=3)
    sb.execute_batch_torch(vec(3, 3 * len(rbc)))
    end_of(CASES[1])

    sphere = fb.unit_sphere(5)
    pts = 1.5 * rng.standard_normal((300, 3))
    fb.FMM_plan(fb.LaplaceSphericalBEM(10, 3), sphere, targets=pts).execute_torch(vec(len(sphere)))
    end_of(CASES[2])

    f32 = fb.FMM_plan(fb.LaplaceSphericalBEM(8, 3), v, o, near_f32_max_p=5)
    f32.execute_torch(x, p=4)
    assert f32.stats()["last_near_f32"] == 1
    end_of(CASES[3])

    ot = fb.FMMOptions()
    ot.set_max_per_box(64)
    ot.evaluator = "TREECODE"
    tc = fb.FMM_plan(fb.LaplaceSphericalBEM(8, 3), sphere, ot)
    tc.execute_torch(vec(len(sphere)))
    assert tc.batch_width() > 1
    tc.execute_batch_torch(vec(3, len(sphere)))
    end_of(CASES[4])

    base = fb.FMM_plan(fb.StokesSphericalBEM(6, 3, 1e-3), rbc)
    for flag in (0, 1):                                       # VELOCITY: the single layer; TRACTION: the double layer
        base.field_plan(pts, target_bc=np.full(len(pts), flag, dtype=np.uint8)).execute_torch(xs)
    end_of(CASES[5])

    gr = fb.FMM_plan(fb.LaplaceSphericalBEM(8, 3), sphere)
    gr.set_graphs(True)
    for _ in range(3):                                        # launch by launch, captured, replayed
        gr.execute_torch(vec(len(sphere)))
    end_of(CASES[6])

    tm = fb.FMM_plan(fb.LaplaceSphericalBEM(8, 3), sphere)
    tm.set_timing(1)
    tm.execute_torch(vec(len(sphere)))
    assert tm.stats()["ms_total"] >= 0
    end_of(CASES[7])

    shards = [fb.FMM_plan(fb.LaplaceSphericalBEM(8, 3), v, shard=(r, 2), shard_upward=True) for r in range(2)]
    buf = torch.zeros((2, shards[0].exchange_doubles(8)), dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    for r, sh in enumerate(shards):
        sh.upward_device(x.data_ptr(), buf[r].data_ptr(), s, 8)
    for r, sh in enumerate(shards):
        y = torch.empty_like(x)
        if r == 0:                                            # the near field while the all-gather would be in flight, then the rest
            sh.near_split_device(y.data_ptr(), s)
        sh.downward_device(buf.data_ptr(), y.data_ptr(), s, 8)
    torch.cuda.synchronize()
    end_of(CASES[8])

    oh = fb.FMMOptions()
    oh.set_max_per_box(64)
    oh.near_stream_fraction = 0.5
    hy = fb.FMM_plan(fb.LaplaceSphericalBEM(10, 3), v, oh)
    hy.execute_torch(x)
    assert hy.stats()["near_recomputed_pairs"] > 0
    end_of(CASES[9])


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] in ("names", "order"):
        (names if sys.argv[1] == "names" else order)(sys.argv[2])
    else:
        run()
