"""fmmbem_gmres_batch(_device): k right-hand sides on one plan, solved in lockstep (include/fmmbem.h; csrc/krylov.hip).  The
contract is an equality: for every system the solution vector, the iteration count, the final residual and the p[] / resid[]
histories are bit for bit (np.array_equal, ==) what fmmbem_gmres_device gives for that system alone on the same plan.

Right-hand sides that need no oracle: on a first-kind Laplace plan (all panels POTENTIAL) b_j(i) = 1 / |c_i - q_j| at the panel
centroids c_i for a charge q_j inside the surface.  q at the centre of a single sphere makes b nearly constant (few
iterations), q at 0.9 of the radius converges slowly; the tests assert, from the single solves' logs, that their systems do
take different numbers of iterations and do ask for different orders at the same iteration."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678
KS = (1, 2, 3, 4, 5, 7)
# charge positions as fractions of the radius along fixed directions; system 0 at the centre, system 1 far out
_DIRS = np.array([[1.0, 0.0, 0.0], [0.0, 0.6, 0.8], [-0.6, 0.0, 0.8], [0.48, -0.6, 0.64], [0.0, -1.0, 0.0], [0.36, 0.48, -0.8], [-0.8, 0.6, 0.0]])
_FRACS = np.array([0.0, 0.9, 0.5, 0.8, 0.3, 0.7, 0.6])


def two_spheres(fb, rec):
    return np.concatenate([fb.unit_sphere(rec), fb.unit_sphere(rec, center=(3.0, 0.0, 0.0))])


def rhs(v, k, centers=((0.0, 0.0, 0.0),)):
    """(k, n): b_j = 1 / |c - q_j|, q_j inside the sphere round centers[j % len(centers)]"""
    c = v.mean(axis=1)
    B = np.empty((k, len(v)))
    for j in range(k):
        q = np.asarray(centers[j % len(centers)]) + _FRACS[j % 7] * _DIRS[j % 7]
        B[j] = 1.0 / np.linalg.norm(c - q, axis=1)
    return B


_MESHES = {}


def mesh_plan(fb, name, p_max=10):
    """(vertices, plan, right-hand sides for 7 systems), one plan per mesh for the whole module"""
    if name not in _MESHES:
        if name == "sphere5":
            v = fb.unit_sphere(5)
            B = rhs(v, 7)
        else:
            v = two_spheres(fb, 6)
            B = rhs(v, 7, centers=((0.0, 0.0, 0.0), (3.0, 0.0, 0.0)))
        _MESHES[name] = (v, fb.FMM_plan(fb.LaplaceSphericalBEM(p_max, 3), v, p_max=p_max), B)
    return _MESHES[name]


def options(fb, mode="bouras", **kw):
    args = dict(residual=1e-6, max_iters=100, max_p=10)
    args.update(kw)
    so = fb.SolverOptions(**args)
    if mode == "simoncini":
        so.relax_type = fb.SolverOptions.SIMONCINI
    elif mode == "fixed":
        so.variable_p = False
    return so


def singles(fb, plan, X0, B, so, M=None, stokes=False, flexible=False):
    """k separate fmmbem_gmres_device solves -> (X, [iterations], [residual], [log])"""
    import torch
    dev = "cuda:%d" % plan.device
    X, its, res, logs = [], [], [], []
    for j in range(len(B)):
        x = torch.from_numpy(np.ascontiguousarray(X0[j])).to(dev)
        b = torch.from_numpy(np.ascontiguousarray(B[j])).to(dev)
        log = []
        _, it, r, _ = fb.gmres_capi(plan, x, b, so, M=M, log=log, stokes=stokes, flexible=flexible)
        X.append(x.cpu().numpy())
        its.append(it)
        res.append(r)
        logs.append(log)
    return np.stack(X), its, res, logs


def batch(fb, plan, X0, B, so, M=None, stokes=False, flexible=False, gx=0, gb=0, host=False, with_logs=True):
    """one fmmbem_gmres_batch(_device) call with leading dimensions n + gx / n + gb, the gaps holding a sentinel that must
    survive -> (X, [iterations], [residual], [log])"""
    import torch
    from fmm_bem_relaxed_amd import _capi
    from fmm_bem_relaxed_amd.solver import _c_options, _c_preconditioner
    k, n = B.shape
    o = _c_options(so, stokes, flexible, plan.kernel().P)
    cap = so.max_iters + so.restart + 2
    ps, rs = [(C.c_int32 * cap)() for _ in range(k)], [(C.c_double * cap)() for _ in range(k)]
    lg = (_capi.SolverLog * k)()
    for j in range(k):
        lg[j].capacity, lg[j].p, lg[j].resid = cap, C.cast(ps[j], C.POINTER(C.c_int32)), C.cast(rs[j], C.POINTER(C.c_double))
    xb = np.full((k, n + gx), SENTINEL)
    xb[:, :n] = X0
    bb = np.full((k, n + gb), SENTINEL)
    bb[:, :n] = B
    L = _capi.lib()
    if host:
        pc = None
        if M is not None:
            pc = _c_preconditioner(M, "test")
            if pc.kind == _capi.PC_DIAGONAL:
                recip = M.recip.cpu().numpy()
                pc.reciprocals = recip.ctypes.data
        _capi.check(L.fmmbem_gmres_batch(plan._h, C.byref(o), k, xb.ctypes.data, n + gx, bb.ctypes.data, n + gb,
                                         C.byref(pc) if pc is not None else None, lg if with_logs else None))
        xo, bo = xb, bb
    else:
        dev = "cuda:%d" % plan.device
        xd, bd = torch.from_numpy(xb).to(dev), torch.from_numpy(bb).to(dev)
        pc = _c_preconditioner(M, "test")
        _capi.check(L.fmmbem_gmres_batch_device(plan._h, C.byref(o), k, xd.data_ptr(), n + gx, bd.data_ptr(), n + gb,
                                                C.byref(pc) if pc is not None else None, lg if with_logs else None,
                                                torch.cuda.current_stream(dev).cuda_stream))
        xo, bo = xd.cpu().numpy(), bd.cpu().numpy()
    assert (xo[:, n:] == SENTINEL).all() and (bo[:, n:] == SENTINEL).all(), "a gap between the vectors was written"
    assert np.array_equal(bo[:, :n], B), "a right-hand side was written"
    its = [lg[j].iterations for j in range(k)]
    logs = [[(i + 1, int(ps[j][i]), float(rs[j][i])) for i in range(min(its[j], cap))] for j in range(k)]
    return xo[:, :n].copy(), its, [lg[j].residual for j in range(k)], logs


def assert_same(got, ref, k=None, what=""):
    Xg, ig, rg, lg = got
    Xr, ir, rr, lr = ref
    k = len(ig) if k is None else k
    for j in range(k):
        assert ig[j] == ir[j], (what, j, ig[j], ir[j])
        assert lg[j] == lr[j], (what, j, "order / residual history")
        assert rg[j] == rr[j], (what, j, rg[j], rr[j])
        assert np.array_equal(Xg[j], Xr[j]), (what, j, float(np.abs(Xg[j] - Xr[j]).max()))


def hard_cases(ref, k):
    """from the single solves' logs: (different iteration counts among the first k systems, some iteration at which two systems
    still running ask for different orders)"""
    _, its, _, logs = ref
    counts = len(set(its[:k])) > 1
    orders = False
    for i in range(max(its[:k])):
        ps = {logs[j][i][1] for j in range(k) if i < its[j]}
        orders = orders or len(ps) > 1
    return counts, orders


_SINGLES = {}


@pytest.mark.parametrize("mode", ["bouras", "simoncini", "fixed"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("mesh", ["sphere5", "two6"])
def test_every_system_equals_its_single_solve(fb, mesh, k, mode):
    v, plan, B = mesh_plan(fb, mesh)
    so = options(fb, mode)
    X0 = np.zeros_like(B)
    if (mesh, mode) not in _SINGLES:
        _SINGLES[(mesh, mode)] = singles(fb, plan, X0, B, so)
        print(mesh, mode, "iterations", _SINGLES[(mesh, mode)][1])
    ref = _SINGLES[(mesh, mode)]
    assert all(r < so.residual for r in ref[2])
    if k > 1:
        counts, orders = hard_cases(ref, k)
        assert counts, "the systems must not all take the same number of iterations"
        if mode != "fixed":
            assert orders, "two running systems must ask for different orders at some iteration"
    assert_same(batch(fb, plan, X0[:k], B[:k], so), ref, k, (mesh, k, mode))


def test_restart_cycles_and_iteration_limit(fb):
    v, plan, B = mesh_plan(fb, "two6")
    X0 = np.zeros_like(B[:4])
    # restart = 5, several cycles, the systems leaving in different ones
    so = options(fb, restart=5, residual=1e-3)
    ref = singles(fb, plan, X0, B[:4], so)
    print("restart 5, tol 1e-3:", ref[1], ref[2])
    # GMRES(5) stagnates on the slow systems: some leave in the first cycle, some in a later one, some never
    assert any(r < so.residual for r in ref[2]) and max(ref[1]) > 2 * so.restart and len(set(ref[1])) > 2
    assert_same(batch(fb, plan, X0, B[:4], so), ref, what="restart 5")
    # max_iters reached before convergence: in the middle of a cycle, at the end of one, in the first one, with one column
    for so in (options(fb, restart=5, max_iters=12), options(fb, restart=5, max_iters=10), options(fb, max_iters=4),
               options(fb, restart=1, max_iters=3), options(fb, restart=3, max_iters=0)):
        ref = singles(fb, plan, X0, B[:4], so)
        print("restart", so.restart, "max_iters", so.max_iters, ref[1], ref[2])
        assert any(r > so.residual for r in ref[2])
        assert_same(batch(fb, plan, X0, B[:4], so), ref, what=(so.restart, so.max_iters))


def test_zero_right_hand_side_and_solved_initial_guess(fb):
    v, plan, B = mesh_plan(fb, "sphere5")
    so = options(fb)
    first = singles(fb, plan, np.zeros_like(B[:3]), B[:3], so)
    Bm = B[:4].copy()
    Bm[1] = 0.0                                       # b = 0: x0 comes back untouched after 0 iterations
    X0 = np.zeros_like(Bm)
    X0[1] = 3.0
    X0[2] = first[0][2]                               # the solution of an earlier solve as the initial guess
    ref = singles(fb, plan, X0, Bm, so)
    assert ref[1][1] == 0 and (ref[0][1] == 3.0).all() and ref[1][2] < ref[1][3]
    assert_same(batch(fb, plan, X0, Bm, so), ref)
    # every system trivial: nothing to iterate on
    Z = np.zeros_like(Bm)
    got = batch(fb, plan, X0, Z, so)
    assert got[1] == [0] * 4 and np.array_equal(got[0], X0)


@pytest.mark.parametrize("flexible", [False, True])
@pytest.mark.parametrize("pc", ["diagonal", "local", "block_diagonal"])
def test_preconditioners(fb, pc, flexible):
    v, plan, B = mesh_plan(fb, "two6")
    so = options(fb)
    if pc == "diagonal":
        M = fb.Diagonal(plan)
    else:
        M = (fb.LocalInnerSolver if pc == "local" else fb.BlockDiagonal)(fb, fb.LaplaceSphericalBEM(10, 3), v)
    k = 4
    X0 = np.zeros_like(B[:k])
    ref = singles(fb, plan, X0, B[:k], so, M=M, flexible=flexible)
    print(pc, flexible, ref[1])
    assert all(r < so.residual for r in ref[2]) and len(set(ref[1])) > 1
    assert_same(batch(fb, plan, X0, B[:k], so, M=M, flexible=flexible), ref, what=(pc, flexible))
    assert_same(batch(fb, plan, X0, B[:k], so, M=M, flexible=flexible, host=True, gx=3, gb=1), ref, what=(pc, flexible, "host"))


def test_leading_dimensions_and_odd_panel_count(fb):
    v = two_spheres(fb, 5)[:-1]                       # an odd number of unknowns: the workspace stride is n + 1
    assert len(v) % 2 == 1
    plan = fb.FMM_plan(fb.LaplaceSphericalBEM(10, 3), v, p_max=10)
    B = rhs(v, 5, centers=((0.0, 0.0, 0.0), (3.0, 0.0, 0.0)))
    so = options(fb)
    X0 = np.zeros_like(B)
    ref = singles(fb, plan, X0, B, so)
    assert len(set(ref[1])) > 1
    assert_same(batch(fb, plan, X0, B, so), ref, what="ld = n, odd")
    assert_same(batch(fb, plan, X0, B, so, gx=5, gb=2), ref, what="odd gaps")
    assert_same(batch(fb, plan, X0, B, so, gx=1, gb=64), ref, what="even ldx")
    assert_same(batch(fb, plan, X0, B, so, gx=7, gb=3, host=True), ref, what="host")


def test_stokes_velocity_plan(fb):
    v = fb.red_blood_cell(3)
    K = fb.StokesSphericalBEM(10, 4, 1e-3)
    K.set_Kfine(19)
    plan = fb.FMM_plan(K, v, p_max=10)
    assert plan.batch_width() == 1
    n = len(v)
    B = np.zeros((3, n, 3))
    B[0, :, 0] = 1.0                                  # a uniform velocity, a shear, a rotation-like field
    B[1, :, 1] = v.mean(axis=1)[:, 0]
    B[2, :, 2] = v.mean(axis=1)[:, 1] + 0.25
    B = B.reshape(3, 3 * n)
    so = options(fb, residual=1e-5, p_min=5)
    X0 = np.zeros_like(B)
    ref = singles(fb, plan, X0, B, so, stokes=True)
    print("stokes", ref[1])
    assert min(p for lg in ref[3] for _, p, _ in lg) >= 5
    assert_same(batch(fb, plan, X0, B, so, stokes=True, gx=3), ref, what="stokes")
    assert_same(batch(fb, plan, X0, B, so, stokes=True, flexible=True), singles(fb, plan, X0, B, so, stokes=True, flexible=True), what="stokes fgmres")


@pytest.mark.parametrize("kind", ["hybrid", "matrix_free"])
def test_plans_that_batch_vector_by_vector(fb, kind):
    v = two_spheres(fb, 6)
    o = fb.FMMOptions()
    if kind == "hybrid":
        o.near_stream_fraction = 0.5
    else:
        o.sparse_local = False
    plan = fb.FMM_plan(fb.LaplaceSphericalBEM(10, 3), v, o, p_max=10)
    if kind == "matrix_free":
        assert plan.batch_width() == 1
    B = rhs(v, 3, centers=((0.0, 0.0, 0.0), (3.0, 0.0, 0.0)))
    so = options(fb)
    X0 = np.zeros_like(B)
    ref = singles(fb, plan, X0, B, so)
    assert len(set(ref[1])) > 1
    assert_same(batch(fb, plan, X0, B, so), ref, what=kind)


def test_host_form_side_stream_and_python_wrapper(fb):
    import torch
    v, plan, B = mesh_plan(fb, "two6")
    so = options(fb)
    k = 4
    X0 = np.zeros_like(B[:k])
    ref = singles(fb, plan, X0, B[:k], so)
    dev = batch(fb, plan, X0, B[:k], so)
    assert_same(dev, ref, what="device")
    assert_same(batch(fb, plan, X0, B[:k], so, host=True), ref, what="host")
    nolog = batch(fb, plan, X0, B[:k], so, with_logs=False)                            # logs = NULL
    assert np.array_equal(nolog[0], ref[0])
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        side = batch(fb, plan, X0, B[:k], so, gx=2)
        # gmres_capi_batch: (k, n) tensors, a row stride larger than n, torch's current stream
        Xt = torch.zeros((k, B.shape[1] + 6), dtype=torch.float64, device="cuda")[:, :B.shape[1]]
        Bt = torch.from_numpy(B[:k]).cuda()
        logs = [[] for _ in range(k)]
        Xo, its, res, secs = fb.gmres_capi_batch(plan, Xt, Bt, so, logs=logs)
        wrapped = (Xo.cpu().numpy(), its, res, logs)
    assert_same(side, ref, what="side stream")
    assert_same(wrapped, ref, what="gmres_capi_batch")
    assert secs > 0
    with pytest.raises(ValueError):
        fb.gmres_capi_batch(plan, Xt.float(), Bt.float(), so)
    with pytest.raises(ValueError):
        fb.gmres_capi_batch(plan, Xt[:, :-1], Bt[:, :-1], so)


def test_single_solves_around_a_batched_solve(fb):
    """a single fmmbem_gmres_device before and after a batched solve on the same plan gives the bits it gives on a fresh plan"""
    v = two_spheres(fb, 6)
    B = rhs(v, 3, centers=((0.0, 0.0, 0.0), (3.0, 0.0, 0.0)))
    so = options(fb)
    X0 = np.zeros_like(B)
    fresh = fb.FMM_plan(fb.LaplaceSphericalBEM(10, 3), v, p_max=10)
    want = singles(fb, fresh, X0[1:2], B[1:2], so)
    fresh.close()
    plan = fb.FMM_plan(fb.LaplaceSphericalBEM(10, 3), v, p_max=10)
    before = singles(fb, plan, X0[1:2], B[1:2], so)
    got = batch(fb, plan, X0, B, so)
    after = singles(fb, plan, X0[1:2], B[1:2], so)
    again = batch(fb, plan, X0[:2], B[:2], so)          # fewer systems in the workspace of more
    assert_same(before, want, what="before")
    assert_same(after, want, what="after")
    assert_same(([got[0][1]], [got[1][1]], [got[2][1]], [got[3][1]]), want, what="batch")
    assert_same(again, got, 2, what="second batch")


def test_single_solve_on_a_plan_with_graphs_on(fb):
    """fmmbem_plan_set_graphs(plan, 1): a single fmmbem_gmres_device runs its matvecs through fmmbem_plan_execute_device, which
    captures and replays the plan's graphs (the batched execute never does), and gives the bits of the same solve on a
    graphs-off plan.  fmmbem_plan_stats reports nothing about graphs, so the replay is observed as a repeat of the solve -- every
    order it asks for captured by now -- returning the same bits.  A k = 3 solve on that plan afterwards equals its singles."""
    v = fb.unit_sphere(4)
    B = rhs(v, 3)
    so = options(fb, max_p=8)
    X0 = np.zeros_like(B)
    off = fb.FMM_plan(fb.LaplaceSphericalBEM(8, 3), v, p_max=8)
    want = singles(fb, off, X0, B, so)
    off.close()
    assert all(r < so.residual for r in want[2]) and len(set(want[1])) > 1
    plan = fb.FMM_plan(fb.LaplaceSphericalBEM(8, 3), v, p_max=8)
    plan.set_graphs(True)
    one = tuple([part[1]] for part in want)
    assert_same(singles(fb, plan, X0[1:2], B[1:2], so), one, what="graphs on")
    assert_same(singles(fb, plan, X0[1:2], B[1:2], so), one, what="graphs on, repeat")
    assert_same(batch(fb, plan, X0, B, so), want, what="k = 3 after the graphed single solves")
    assert_same(singles(fb, plan, X0[1:2], B[1:2], so), one, what="graphs on, after the batched solve")
    plan.close()


def test_host_entry_refuses_bad_options_before_staging(fb):
    """fmmbem_gmres with restart = 0, and with a DIAGONAL preconditioner without reciprocals: FMMBEM_ERR_INVALID, x untouched"""
    from fmm_bem_relaxed_amd import _capi
    from fmm_bem_relaxed_amd.solver import _c_options
    v, plan, B = mesh_plan(fb, "sphere5")
    x, b = np.full(B.shape[1], 2.0), B[1].copy()
    L = _capi.lib()
    o = _c_options(options(fb, restart=0), False, False, plan.kernel().P)
    assert L.fmmbem_gmres(plan._h, C.byref(o), x.ctypes.data, b.ctypes.data, None, None) == 1
    assert b"restart >= 1" in L.fmmbem_last_error()
    o = _c_options(options(fb), False, False, plan.kernel().P)
    pc = _capi.Preconditioner()
    pc.kind, pc.reciprocals = _capi.PC_DIAGONAL, None
    assert L.fmmbem_gmres(plan._h, C.byref(o), x.ctypes.data, b.ctypes.data, C.byref(pc), None) == 1
    assert b"without reciprocals" in L.fmmbem_last_error()
    assert (x == 2.0).all()


def test_fgmres_without_a_preconditioner_is_gmres(fb):
    """FGMRES with the identity keeps Z_j = V_j: the same operations as GMRES, so fmmbem_gmres_device with flexible = 1 and
    M = NULL gives the bits of flexible = 0 and M = NULL (the Laplace order rules coincide: max(1, predict_p)) -- on a plan whose
    workspace an earlier preconditioned FGMRES left full of other Z vectors, and through the batched solver as well"""
    v, plan, B = mesh_plan(fb, "two6")
    so = options(fb, restart=8, max_iters=30)
    X0 = np.zeros_like(B[:3])
    singles(fb, plan, X0, B[:3], so, M=fb.Diagonal(plan), flexible=True)                  # Z now holds M(V_j) of another solve
    plain = singles(fb, plan, X0, B[:3], so)
    assert max(plain[1]) > so.restart                                                   # more than one update
    assert_same(singles(fb, plan, X0, B[:3], so, flexible=True), plain, what="fgmres, M = NULL")
    assert_same(batch(fb, plan, X0, B[:3], so, flexible=True), plain, what="batched fgmres, M = NULL")


_ALLOC_RETRY = r"""
import sys
import numpy as np, torch
sys.path.insert(0, %r)
import fmm_bem_relaxed_amd as fb
v = fb.unit_sphere(4); n = len(v)
plan = fb.FMM_plan(fb.LaplaceSphericalBEM(8, 3), v, p_max=8)
c = v.mean(axis=1)
B = torch.from_numpy(np.stack([1.0 / np.linalg.norm(c - np.array([f, 0.0, 0.0]), axis=1) for f in (0.0, 0.8, 0.4)])).cuda()
so = fb.SolverOptions(residual=1e-6, max_iters=40, max_p=8)
try:
    fb.gmres_capi_batch(plan, torch.zeros_like(B), B, so)
    print("NOFAIL")
except fb.FmmBemError as e:
    print("FAILED", e.status, str(e)[:200].replace("\n", " "))
x1, it1, res1, _ = fb.gmres_capi(plan, torch.zeros_like(B[1]), B[1].contiguous(), so)      # the next single solve on the SAME plan
X, its, res, _ = fb.gmres_capi_batch(plan, torch.zeros_like(B), B, so)                     # and the next batched one
print("RETRY", it1, its[1], int(torch.equal(X[1], x1)), float(max(res)), len(set(its)))
"""


@pytest.mark.parametrize("k", [1, 2, 3, 5, 6])
def test_batched_workspace_survives_a_failed_allocation(k, tmp_path):
    """the k-th allocation of the batched workspace fails (injected, FMMBEM_KRYLOV_FAIL_GROW): the call returns FMMBEM_ERR_ALLOC,
    the workspace is left empty, and the next single solve and the next batched solve on the same plan succeed"""
    script = tmp_path / "retry.py"
    script.write_text(_ALLOC_RETRY % ROOT)
    r = subprocess.run([sys.executable, str(script)], env=dict(os.environ, FMMBEM_KRYLOV_FAIL_GROW=str(k)), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert lines[0].startswith("FAILED 4") and "injected" in lines[0], lines
    tag, it1, itb, same, res, distinct = lines[1].split()
    assert tag == "RETRY" and it1 == itb and same == "1" and float(res) < 1e-6 and int(distinct) > 1
