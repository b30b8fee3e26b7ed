"""The float near field (fmmbem_options.near_f32_max_p) on the GPU.

Above the threshold a plan is bit for bit the plan without the option.  At or below it the near field streams a float copy of
the assembled matrix into FP64 sums: the far field is the same kernels on the same data, so the difference to the FP64 plan is
the near field's alone, and every row obeys

    |dy_i| <= (2^-24 + 2^-40) (|A| |x|)_i,

|A| from the FP64 plan's fmmbem_plan_get_near_row.  The bound is derived, not measured: 2^-24 is the unit roundoff of the one
float rounding per entry, 2^-40 covers the FP64 summation-order noise of both kernels for rows of up to a few thousand entries.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

BOUND = 2.0 ** -24 + 2.0 ** -40
RECOMMENDED = 5          # DESIGN.md section 8 "Float near field": the largest measured order whose error against Direct is >= 100 x 2^-24


def two_spheres(fb, rec):
    return np.concatenate([fb.unit_sphere(rec), fb.unit_sphere(rec, center=(3.0, 0.0, 0.0))])


def _flags(n, which):
    return {"potential": np.zeros(n, np.uint8), "normal_deriv": np.ones(n, np.uint8),
            "mixed": (np.arange(n) % 3 == 0).astype(np.uint8)}[which]


def _run(plan, x, p):
    import torch
    xd = torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).to("cuda:%d" % plan.device)
    y = plan.execute_torch(xd, p=p)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def abs_row_sums(plan, x):
    """(|A_near| |x|) per unknown, in the caller's order, from every near row of (the FP64 values of) `plan`"""
    dof = plan.dof
    perm = plan.perm().astype(np.int64)
    xt = np.abs(np.asarray(x).reshape(plan.n, dof))[perm].reshape(-1)            # tree order, dof per panel
    out = np.zeros(plan.n * dof)
    for row in range(plan.n * dof):
        cols, vals = plan.near_row(row)
        out[perm[row // dof] * dof + row % dof] = np.abs(vals) @ xt[cols.astype(np.int64)]
    return out


def assert_row_bound(y32, y64, bound_rows, what):
    d = np.abs(y32 - y64)
    worst = float((d / np.maximum(bound_rows, 1e-300)).max())
    print("%s: max |dy_i| / (|A||x|)_i = %.3e (2^-24 = %.3e), rows changed %d of %d" % (what, worst, 2.0 ** -24, int((d > 0).sum()), d.size))
    assert (d <= BOUND * bound_rows).all(), (what, worst)


def check_pair(p64, p32, x, k, p_max, what):
    """p32 = p64's plan with threshold k: unchanged above k; float, repeatable, different and within the row bound up to k"""
    s64 = p64.stats()
    assert s64["near_f32_bytes"] == 0
    nb = p32.stats()["near_bytes"]
    assert nb == s64["near_bytes"] and p32.stats()["near_f32_bytes"] > 0
    rows = abs_row_sums(p64, x)
    for p in sorted({k + 1, p_max}):
        if p > k:
            assert np.array_equal(_run(p32, x, p), _run(p64, x, p)), (what, p)
            st = p32.stats()
            assert st["last_near_f32"] == 0 and st["near_bytes"] == nb
    for p in sorted({1, k}):
        y32 = _run(p32, x, p)
        st = p32.stats()
        assert st["last_near_f32"] == 1 and st["near_f32_bytes"] > 0 and st["near_bytes"] == nb
        assert np.array_equal(_run(p32, x, p), y32), (what, p, "two executes differ")
        y64 = _run(p64, x, p)
        assert p64.stats()["last_near_f32"] == 0
        assert not np.array_equal(y32, y64), (what, p)
        assert_row_bound(y32, y64, rows, "%s p=%d" % (what, p))


@pytest.mark.parametrize("rec", [4, 5, 6])
@pytest.mark.parametrize("flags", ["potential", "normal_deriv", "mixed"])
def test_laplace(fb, rec, flags):
    v = two_spheres(fb, rec)
    n = len(v)
    bc = _flags(n, flags)
    x = np.random.default_rng(rec).random(n) - 0.3
    p64 = fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), v, bc=bc, p_max=8)
    p32 = fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), v, bc=bc, p_max=8, near_f32_max_p=4)
    # a quarter of the FP64 bytes plus the padding of the rows to four columns
    assert p32.stats()["near_f32_bytes"] >= p32.stats()["near_bytes"] // 2
    check_pair(p64, p32, x, 4, 8, "laplace r=%d %s" % (rec, flags))


@pytest.mark.parametrize("rec", [4, 5])
def test_stokes_velocity(fb, rec):
    v = fb.red_blood_cell(rec)
    n = len(v)
    x = np.random.default_rng(10 + rec).random((n, 3)) - 0.3

    def kernel():
        K = fb.StokesSphericalBEM(6, 4, 1e-3)
        K.set_Kfine(19)
        return K
    p64 = fb.FMM_plan(kernel(), v, p_max=8)
    p32 = fb.FMM_plan(kernel(), v, p_max=8, near_f32_max_p=5)
    check_pair(p64, p32, x, 5, 8, "stokes rbc r=%d" % rec)


@pytest.mark.parametrize("evaluator", ["local", "block_diagonal"])
def test_local_and_block_diagonal(fb, evaluator):
    v = two_spheres(fb, 5)
    o = fb.FMMOptions()
    o.lazy_evaluation = False
    o.local_evaluation = evaluator == "local"
    o.block_diagonal = evaluator == "block_diagonal"
    x = np.random.default_rng(20).random(len(v)) - 0.3
    p64 = fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), v, o, p_max=8)
    p32 = fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), v, o, p_max=8, near_f32_max_p=4)
    check_pair(p64, p32, x, 4, 8, evaluator)


def test_create_like_carries_the_mode_and_its_own_values(fb):
    v = two_spheres(fb, 5)
    n = len(v)
    x = np.random.default_rng(21).random(n) - 0.3
    flipped = (np.arange(n) % 2).astype(np.uint8)
    base32 = fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), v, p_max=8, near_f32_max_p=4)
    like32 = base32.like(flipped)
    base64 = fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), v, p_max=8)
    like64 = base64.like(flipped)
    assert like32.stats()["near_f32_bytes"] == base32.stats()["near_f32_bytes"] > 0
    assert like32.batch_width() == 1 and like64.batch_width() > 1
    check_pair(like64, like32, x, 4, 8, "create_like")
    check_pair(base64, base32, x, 4, 8, "create_like base")     # the base plan's copy is untouched by the like plan's
    # fmmbem_plan_create recognising the geometry of a live plan: the same
    again32 = fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), v, bc=flipped, p_max=8, near_f32_max_p=4)
    assert again32.stats()["geometry_shared"] > 1
    assert np.array_equal(_run(again32, x, 3), _run(like32, x, 3))
    assert again32.stats()["last_near_f32"] == 1


def test_fmm_plan_without_a_far_field_takes_the_option_as_off(fb):
    """Eight leaves that are all neighbours (UnitSphere(4), 512 panels): no M2L pair, the result is exact at every order and there
    is no truncation error for the rounding to hide under -- the FMM evaluator ignores the option there; the near-field-only
    evaluators (no far field by definition) keep it."""
    v = fb.unit_sphere(4)
    x = np.random.default_rng(27).random(len(v)) - 0.3
    off = fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), v, p_max=8)
    on = fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), v, p_max=8, near_f32_max_p=8)
    assert off.stats()["m2l_pairs"] == 0 and on.stats()["near_f32_bytes"] == 0
    for p in (1, 4, 8):
        assert np.array_equal(_run(on, x, p), _run(off, x, p))
        assert on.stats()["last_near_f32"] == 0
    assert np.array_equal(_run(off, x, 1), _run(off, x, 8))     # the order changes nothing on this plan
    o = fb.FMMOptions()
    o.lazy_evaluation, o.local_evaluation = False, True
    loc = fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), v, o, p_max=8, near_f32_max_p=8)
    assert loc.stats()["near_f32_bytes"] > 0
    # one leaf more than that (two spheres: M2L pairs between them) and the FMM evaluator takes it
    v2 = two_spheres(fb, 4)
    on2 = fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), v2, p_max=8, near_f32_max_p=8)
    assert on2.stats()["m2l_pairs"] > 0 and on2.stats()["near_f32_bytes"] > 0


def _fallback_plans(fb, v, k):
    o_h = fb.FMMOptions()
    o_h.near_stream_fraction = 0.5
    o_m = fb.FMMOptions()
    o_m.sparse_local = False
    pts = np.random.default_rng(22).normal(size=(500, 3)) * 2.0 + np.array([1.5, 0.0, 0.0])
    K = lambda: fb.LaplaceSphericalBEM(5, 3)
    return {
        "hybrid": fb.FMM_plan(K(), v, o_h, p_max=8, near_f32_max_p=k),
        "matrix_free": fb.FMM_plan(K(), v, o_m, p_max=8, near_f32_max_p=k),
        "device_list": fb.FMM_plan(K(), v, p_max=8, devices=[0, 0], near_f32_max_p=k),
        "targets": fb.FMM_plan(K(), v, p_max=8, targets=pts, near_f32_max_p=k),
    }


def test_fallbacks_are_the_plans_without_the_option(fb):
    v = two_spheres(fb, 6)
    x = np.random.default_rng(23).random(len(v)) - 0.3
    on, off = _fallback_plans(fb, v, 4), _fallback_plans(fb, v, 0)
    assert off["hybrid"].stats()["near_recomputed_pairs"] > 0
    for name in on:
        assert on[name].stats()["near_f32_bytes"] == 0, name
        for p in (2, 4, 8):
            assert np.array_equal(_run(on[name], x, p), _run(off[name], x, p)), (name, p)
            assert on[name].stats()["last_near_f32"] == 0, name
    # a Stokes hybrid plan
    vs = fb.red_blood_cell(5)
    xs = np.random.default_rng(24).random((len(vs), 3))
    o_h = fb.FMMOptions()
    o_h.near_stream_fraction = 0.5
    a = fb.FMM_plan(fb.StokesSphericalBEM(6, 3, 1e-3), vs, o_h, p_max=8, near_f32_max_p=4)
    b = fb.FMM_plan(fb.StokesSphericalBEM(6, 3, 1e-3), vs, o_h, p_max=8)
    if b.stats()["near_recomputed_pairs"] > 0:
        assert a.stats()["near_f32_bytes"] == 0
        assert np.array_equal(_run(a, xs, 3), _run(b, xs, 3))


@pytest.mark.parametrize("kernel", ["laplace", "stokes"])
def test_batch_runs_vector_by_vector(fb, kernel):
    import torch
    if kernel == "laplace":
        v = two_spheres(fb, 5)
        plan = fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), v, p_max=8, near_f32_max_p=4)
    else:
        v = fb.red_blood_cell(4)
        plan = fb.FMM_plan(fb.StokesSphericalBEM(6, 3, 1e-3), v, p_max=8, near_f32_max_p=4)
    assert plan.stats()["near_f32_bytes"] > 0 and plan.batch_width() == 1
    k, m = 5, plan.n * plan.dof
    X = np.random.default_rng(25).random((k, m)) - 0.3
    for p in (3, 5):                                            # one order below and one above the threshold
        xb = torch.from_numpy(X).cuda()
        yb = torch.empty_like(xb)
        plan.execute_batch_device(k, xb.data_ptr(), m, yb.data_ptr(), m, torch.cuda.current_stream().cuda_stream, p)
        torch.cuda.synchronize()
        assert plan.stats()["last_near_f32"] == (1 if p <= 4 else 0)
        got = yb.cpu().numpy()
        for j in range(k):
            assert np.array_equal(got[j], _run(plan, X[j], p)), (kernel, p, j)


def test_graph_replay_keeps_the_kernel_of_its_order(fb):
    v = two_spheres(fb, 5)
    x = np.random.default_rng(26).random(len(v)) - 0.3
    plain = fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), v, p_max=8, near_f32_max_p=4)
    graphed = fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), v, p_max=8, near_f32_max_p=4)
    graphed.set_graphs(True)
    for _ in range(3):                                          # launch by launch, captured, replayed
        for p in (2, 6, 4, 5):
            assert np.array_equal(_run(graphed, x, p), _run(plain, x, p)), p
            assert graphed.stats()["last_near_f32"] == (1 if p <= 4 else 0)


def _first_kind(fb, r, p, k):
    import torch
    v = fb.unit_sphere(r)
    n = len(v)
    plan = fb.FMM_plan(fb.LaplaceSphericalBEM(p, 3), v, p_max=p, near_f32_max_p=k)
    rhs = fb.FMM_plan(fb.LaplaceSphericalBEM(p, 3), v, bc=np.ones(n, dtype=np.uint8), p_max=p)
    b = rhs.execute_torch(torch.ones(n, dtype=torch.float64, device="cuda"))
    rhs.close()
    return plan, b


@pytest.mark.parametrize("r", [4, 5, 6])
def test_relaxed_gmres_is_blind_to_the_float_near_field(fb, r):
    """The systems of tests/golden/gmres_ref_r<r>.json through fmmbem_gmres_device with the threshold at 0, at the recommended
    value and at 4: the same iteration count and order history, and a solution that moves by at most twice what relaxation
    itself moves it (threshold-0 relaxed solve against the fixed-p_max solve of the same system, measured here on the FP64
    path) -- the option's perturbation is far below the truncation error at the orders it touches.

    Measured on the MI355X (|x_k - x_0| / |x_0| for threshold 5 / 4, against the relaxation's own effect; iterations and
    order histories identical in every run of every fixture):
      r = 6: tol 1e-5  5.7e-11 / 5.7e-11 against 8.0e-5;   tol 1e-10  1.2e-14 / 3.1e-15 against 1.6e-9
      r = 5: tol 1e-5  2.6e-10 / 1.0e-10 against 9.8e-6;   tol 1e-10  3.1e-15 / 3.1e-15 against 1.3e-10
    r = 4: UnitSphere(4) is 512 panels in eight level-1 leaves that are all neighbours -- no M2L pair, no far field, the order
    changes nothing and the relaxed solve equals the fixed-p solve bit for bit (baseline exactly 0).  The option's premise
    (rounding hidden under the far field's truncation error) does not hold on such a plan and the library takes it as 0 there
    (near_f32_bytes == 0, include/fmmbem.h), so the three solves are the same bits."""
    import torch
    runs = json.load(open(os.path.join(ROOT, "tests", "golden", "gmres_ref_r%d.json" % r)))["runs"]
    bad = []                                                    # every run is measured and printed before anything is asserted
    for run in runs:
        p, tol = run["max_p"], run["tol"]
        so = fb.SolverOptions(residual=tol, max_iters=500, max_p=p)
        fixed = fb.SolverOptions(residual=tol, max_iters=500, max_p=p, variable_p=False)
        plan0, b = _first_kind(fb, r, p, 0)
        log0 = []
        x0, it0, res0, _ = fb.gmres_capi(plan0, torch.zeros_like(b), b, so, log=log0)
        xf, itf, resf, _ = fb.gmres_capi(plan0, torch.zeros_like(b), b, fixed)
        base = float(torch.linalg.vector_norm(x0 - xf) / torch.linalg.vector_norm(xf))
        assert plan0.stats()["near_f32_bytes"] == 0
        plan0.close()
        for k in (RECOMMENDED, 4):
            plank, bk = _first_kind(fb, r, p, k)
            assert torch.equal(bk, b)
            logk = []
            xk, itk, resk, _ = fb.gmres_capi(plank, torch.zeros_like(b), b, so, log=logk)
            diff = float(torch.linalg.vector_norm(xk - x0) / torch.linalg.vector_norm(x0))
            used = sum(1 for _, q, _ in logk if q <= k)
            print("r=%d max_p=%d tol=%.0e threshold=%d: iterations %d / %d, float matvecs %d, |x_k - x_0| / |x_0| = %.3e, relaxation's own %.3e"
                  % (r, p, tol, k, itk, it0, used, diff, base))
            stk = plank.stats()
            assert (stk["near_f32_bytes"] > 0) == (stk["m2l_pairs"] > 0)      # active wherever the plan has a far field
            first = [(a, c) for a, c in zip(log0, logk) if a[1] != c[1]][:1]
            if itk != it0 or [q for _, q, _ in logk] != [q for _, q, _ in log0]:
                bad.append(("history", p, tol, k, itk, it0, first))
            if not resk < tol:
                bad.append(("residual", p, tol, k, resk))
            if not diff <= 2.0 * base:
                bad.append(("solution", p, tol, k, diff, base))
            plank.close()
    assert not bad, bad


def _build_cpp(tmp_path):
    exe = str(tmp_path / "near_f32")
    libdir = os.path.join(ROOT, "fmm-bem-relaxed_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "near_f32.cpp"), "-o", exe,
                           "-L" + libdir, "-lfmmbem_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_adapter_sets_the_option(tmp_path, fb):
    exe = _build_cpp(tmp_path)
    out = {}
    for k in (0, 4):
        r = subprocess.run([exe, "5", str(k)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = r.stdout.splitlines()
        head = lines[0].split()
        assert head[:3] == ["near_f32", str(2 * 4 ** 5), str(k)] and (int(head[3]) > 0) == (k > 0)
        rows = [ln.split() for ln in lines[1:9]]
        assert [int(w[1]) for w in rows] == list(range(1, 9))
        assert [int(w[3]) for w in rows] == [1 if p <= k else 0 for p in range(1, 9)]
        out[k] = [float(w[5]) for w in rows]
    for p in range(1, 9):
        if p <= 4:
            assert out[4][p - 1] != out[0][p - 1] and abs(out[4][p - 1] - out[0][p - 1]) <= 1e-6 * abs(out[0][p - 1])
        else:
            assert out[4][p - 1] == out[0][p - 1]


def _driver(name, args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", name)] + args, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.splitlines()


def _without_times(lines):
    skip = ("Flipping BC", "Creating plan", "Executing plan", "\tsetup", "\tsolve", "float near field")
    return [ln for ln in lines if not ln.startswith(skip)]


def test_laplace_driver_reports_the_same_lines(fb):
    args = ["-recursions", "6", "-p", "10", "-solver_tol", "1e-5"]
    off, on = _driver("LaplaceBEM.py", args), _driver("LaplaceBEM.py", args + ["-near_f32", str(RECOMMENDED)])
    assert sum(ln.startswith("float near field: matvecs at p <= %d" % RECOMMENDED) for ln in on) == 1
    assert not any(ln.startswith("float near field") for ln in off)
    a, b = _without_times(off), _without_times(on)
    its = [ln for ln in a if ln.startswith("it: ")]
    assert its and [ln.split(", res")[0] + ln.split("fmm_req_p")[1] for ln in its] == \
        [ln.split(", res")[0] + ln.split("fmm_req_p")[1] for ln in b if ln.startswith("it: ")]      # iterations and orders
    for key in ("Final residual", "external phi", "relative error"):
        la, lb = [ln for ln in a if ln.startswith(key)], [ln for ln in b if ln.startswith(key)]
        assert len(la) == 1 and len(lb) == 1
        if key == "Final residual":
            assert la[0].split("after")[1] == lb[0].split("after")[1]                                 # the iteration count
        else:
            # the printed error within the driver's printed precision: every printed digit but the last (%.4e / %.3e)
            ea, eb = float(la[0].split()[-1]), float(lb[0].split()[-1])
            assert abs(ea - eb) <= (1e-3 if key == "external phi" else 1e-2) * abs(ea), (la, lb)
    assert [ln for ln in a if not ln.startswith(("it: ", "Final residual", "external phi", "relative error"))] == \
        [ln for ln in b if not ln.startswith(("it: ", "Final residual", "external phi", "relative error"))]


def test_stokes_driver_reports_the_same_lines(fb):
    args = ["-recursions", "5", "-p", "8", "-pmin", "3", "-solver_tol", "1e-4"]      # UnitSphere(5): a plan with a far field
    off, on = _driver("StokesBEM.py", args), _driver("StokesBEM.py", args + ["-near_f32", "8"])      # every matvec of the solve
    assert sum(ln.startswith("float near field: matvecs at p <= 8") for ln in on) == 1
    assert float([ln for ln in on if ln.startswith("float near field")][0].split("stream")[1].split()[0]) > 0     # active
    a, b = _without_times(off), _without_times(on)
    ia, ib = [ln for ln in a if ln.startswith("it: ")], [ln for ln in b if ln.startswith("it: ")]
    assert ia and len(ia) == len(ib)
    assert [ln.split("fmm_req_p")[1] for ln in ia] == [ln.split("fmm_req_p")[1] for ln in ib]
    for key in ("Fx:", "error on a sphere"):
        la, lb = [ln for ln in a if ln.startswith(key)], [ln for ln in b if ln.startswith(key)]
        assert len(la) == 1 and len(lb) == 1
        ea = float(la[0].split(",")[0].split()[-1])
        eb = float(lb[0].split(",")[0].split()[-1])
        # every printed digit but the last: Fx is printed %.5f, the drag error %.5e
        assert abs(ea - eb) <= (1e-4 if key == "Fx:" else 1e-4 * abs(ea)), (la, lb)
