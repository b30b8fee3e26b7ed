"""The exact block-Jacobi preconditioner (include/fmmbem.h fmmbem_plan_block_inverse_*; csrc/kernels_blockinv.hip): the leaf
blocks of a BLOCK_DIAGONAL plan inverted on the device, held to LAPACK's explicit inverse of the SAME blocks (read back through
the near-row getter) on the host, and preconditioner kind 3 of the C ABI's solver.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -52

# case: (mesh, recursions, kernel, flag of every panel, ncrit)
CASES = {
    1: ("sphere", 3, "laplace", 0, 64),
    2: ("sphere", 3, "laplace", 1, 64),
    3: ("sphere", 4, "laplace", 0, 7),          # odd and small leaves
    4: ("sphere", 3, "laplace", 0, 1),          # every block 1 x 1
    5: ("rbc", 3, "stokes", 0, 64),
    6: ("rbc", 3, "stokes", 0, 1),              # every block 3 x 3
    7: ("sphere", 3, "stokes", 1, 64),          # TRACTION
}


def _bd_options(fb, ncrit):
    o = fb.FMMOptions()
    o.local_evaluation, o.lazy_evaluation, o.sparse_local, o.block_diagonal = False, False, True, True
    o.set_max_per_box(ncrit)
    return o


_cache = {}


def _case(fb, c):
    """Built once per case and shared, never modified: the plan with its inverse, its leaf blocks on the host, a random v,
    z = apply(v), LAPACK's answer and the per-leaf bound."""
    if c in _cache:
        return _cache[c]
    mesh, r, kern, flag, ncrit = CASES[c]
    panels = fb.unit_sphere(r) if mesh == "sphere" else fb.red_blood_cell(r)
    n = len(panels)
    K = fb.LaplaceSphericalBEM(5, 3) if kern == "laplace" else fb.StokesSphericalBEM(5, 3)
    plan = fb.FMM_plan(K, panels, _bd_options(fb, ncrit), bc=np.full(n, flag, dtype=np.uint8))
    assert plan.block_inverse_bytes() == 0
    plan.block_inverse_build()
    plan.block_inverse_build()                                   # a second build: a no-op
    dof = plan.dof
    perm = plan.perm().astype(np.int64)
    bx = plan.boxes()
    leaves = sorted((int(bx["bb"][b]), int(bx["be"][b])) for b in range(len(bx["leaf"])) if bx["leaf"][b])   # the plan's leaf order
    assert sum(e - b for b, e in leaves) == n and all(e > b for b, e in leaves)
    blocks, index = [], []
    for bb, be in leaves:
        m = dof * (be - bb)
        A = np.empty((m, m))
        for i in range(m):
            cols, vals = plan.near_row(dof * bb + i)
            assert cols.tolist() == list(range(dof * bb, dof * be))
            A[i] = vals
        blocks.append(A)
        # positions of the leaf's unknowns in a flattened vector in the caller's order
        index.append((perm[bb:be, None] * dof + np.arange(dof)[None, :]).reshape(-1))
    assert plan.block_inverse_bytes() == 8 * sum(A.size for A in blocks)
    rng = np.random.default_rng(100 + c)
    v = rng.standard_normal((n,) if dof == 1 else (n, dof))
    z = plan.block_inverse_apply(v)
    vf, zf = v.reshape(-1), z.reshape(-1)
    ratios, bounds = [], []
    for A, ix in zip(blocks, index):
        m = len(ix)
        nA = np.linalg.norm(A, 2)
        zl, vl = zf[ix], vf[ix]
        zr = np.linalg.inv(A) @ vl                               # the yardstick: LAPACK's explicit inverse
        dev = np.linalg.norm(A @ zl - vl) / (nA * np.linalg.norm(zl))
        ref = np.linalg.norm(A @ zr - vl) / (nA * np.linalg.norm(zr))
        bound = 4.0 * max(ref, m * U)
        ratios.append(dev / (bound / 4.0))
        bounds.append((dev, bound, nA * np.linalg.norm(zl)))
    _cache[c] = dict(plan=plan, n=n, dof=dof, blocks=blocks, index=index, v=v, z=z, bounds=bounds, ratios=ratios, perm=perm, leaves=leaves)
    return _cache[c]


@pytest.mark.parametrize("c", sorted(CASES))
def test_residual_against_the_plans_own_blocks(fb, c):
    d = _case(fb, c)
    print("case %d: %d leaves, largest block %d, max residual ratio to max(LAPACK, m u): %.3g" %
          (c, len(d["blocks"]), max(len(ix) for ix in d["index"]), max(d["ratios"])))
    for leaf, (dev, bound, _) in enumerate(d["bounds"]):
        assert dev <= bound, (c, leaf, dev, bound)


@pytest.mark.parametrize("c", sorted(CASES))
def test_execute_of_apply_returns_v(fb, c):
    """plan.execute applies the blocks themselves: execute(apply(v)) = v leaf by leaf -- the rows land where the operator expects them"""
    d = _case(fb, c)
    y = d["plan"].execute(d["z"]).reshape(-1)
    vf = d["v"].reshape(-1)
    worst = 0.0
    for leaf, (ix, (_, bound, scale)) in enumerate(zip(d["index"], d["bounds"])):
        err = np.linalg.norm(y[ix] - vf[ix])
        worst = max(worst, err / (bound * scale))
        assert err <= bound * scale, (c, leaf, err, bound * scale)
    print("case %d: max |execute(apply(v)) - v| over its bound: %.3g" % (c, worst))


@pytest.mark.parametrize("c", sorted(CASES))
def test_unit_vectors_stay_in_their_leaf(fb, c):
    d = _case(fb, c)
    n, dof = d["n"], d["dof"]
    nd = n * dof
    picks = sorted({0, nd // 3 + 1, nd // 2, nd - 1})
    E = np.zeros((len(picks), nd))
    for j, u in enumerate(picks):
        E[j, u] = 1.0
    Z = d["plan"].block_inverse_apply(E.reshape((len(picks), n) if dof == 1 else (len(picks), n, dof))).reshape(len(picks), nd)
    for j, u in enumerate(picks):
        own = [ix for ix in d["index"] if u in ix]
        assert len(own) == 1
        outside = np.ones(nd, dtype=bool)
        outside[own[0]] = False
        assert (Z[j][outside] == 0.0).all()
        assert Z[j][u] != 0.0


def test_one_by_one_blocks_divide_by_the_diagonal(fb):
    d = _case(fb, 4)
    assert all(A.shape == (1, 1) for A in d["blocks"])
    want = d["v"] / d["plan"].diagonal()
    assert (np.abs(d["z"] - want) <= 2 * np.spacing(np.abs(want))).all()


@pytest.mark.parametrize("c", [3, 5])
def test_same_bits_every_run_every_k_host_and_device(fb, c):
    import torch
    d = _case(fb, c)
    plan, n, dof = d["plan"], d["n"], d["dof"]
    assert np.array_equal(plan.block_inverse_apply(d["v"]), d["z"])
    rng = np.random.default_rng(7)
    V = rng.standard_normal((5, n) if dof == 1 else (5, n, dof))
    V[2] = d["v"]
    Z = plan.block_inverse_apply(V)
    for j in range(5):
        assert np.array_equal(Z[j], plan.block_inverse_apply(V[j])), j
    assert np.array_equal(Z[2], d["z"])
    Vd = torch.from_numpy(V.reshape(5, -1)).cuda()
    Zd = plan.block_inverse_apply_torch(Vd)
    assert np.array_equal(Zd.cpu().numpy().reshape(Z.shape), Z)
    out = torch.full_like(Vd[0], float("nan"))
    plan.block_inverse_apply_torch(Vd[3].contiguous(), out=out)            # every entry of z is written
    assert np.array_equal(out.cpu().numpy().reshape(Z[3].shape), Z[3])


def test_singular_block_is_refused_and_the_plan_stays_usable(fb):
    """Two identical panels in a two-panel leaf: the 2 x 2 Laplace POTENTIAL block holds one value four times"""
    def tri(c):
        c = np.asarray(c, dtype=np.float64)
        return np.array([c + [0.1, 0.0, 0.0], c + [0.0, 0.1, 0.0], c + [0.0, 0.0, 0.1]])
    panels = np.array([tri([1, 1, 1]), tri([-1, -1, -1]), tri([1, 1, 1]), tri([1, -1, -1]), tri([-1, 1, 1])])
    plan = fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), panels, _bd_options(fb, 2))
    x = np.arange(1.0, 6.0)
    y0 = plan.execute(x)
    with pytest.raises(fb.FmmBemError) as e:
        plan.block_inverse_build()
    assert e.value.status == 1
    perm = plan.perm()
    bx = plan.boxes()
    leaves = sorted((int(bx["bb"][b]), int(bx["be"][b])) for b in range(len(bx["leaf"])) if bx["leaf"][b])   # the plan's leaf order
    assert all(e > b for b, e in leaves)
    two = [k for k, (bb, be) in enumerate(leaves) if sorted(perm[bb:be].tolist()) == [0, 2]]
    assert len(two) == 1
    assert "leaf %d " % two[0] in str(e.value) and "singular" in str(e.value)
    assert plan.block_inverse_bytes() == 0
    with pytest.raises(fb.FmmBemError) as e:
        plan.block_inverse_apply(x)
    assert e.value.status == 1
    assert np.array_equal(plan.execute(x), y0) and np.isfinite(y0).all()
    c, vals = plan.near_row(int(np.nonzero(perm == 0)[0][0]))
    assert len(vals) == 2 and vals[0] == vals[1]


# ---- the solver: preconditioner kind 3 -------------------------------------------------------------------------------------

TOL = 1e-6


def _laplace_operator(fb):
    if "lap" not in _cache:
        import torch
        panels = fb.unit_sphere(5)
        K = fb.LaplaceSphericalBEM(10, 3)
        plan = fb.FMM_plan(K, panels, p_max=10)
        b = torch.from_numpy(np.random.default_rng(11).standard_normal((3, len(panels)))).cuda()
        _cache["lap"] = (panels, K, plan, b)
    return _cache["lap"]


def _true_residual(plan, x, b, p):
    import torch
    r = b - plan.execute_torch(x.contiguous(), p=p)
    return float(torch.linalg.vector_norm(r) / torch.linalg.vector_norm(b))


def test_solver_laplace_and_iteration_counts(fb):
    import torch
    panels, K, plan, B = _laplace_operator(fb)
    b = B[0].contiguous()
    so = fb.SolverOptions(residual=TOL, max_iters=500, max_p=10, variable_p=False)
    M = fb.BlockInverse(fb, fb.LaplaceSphericalBEM(10, 3), panels)
    log = []
    x, it, res, _ = fb.gmres_capi(plan, torch.zeros_like(b), b, so, M=M, log=log)
    assert res <= TOL and all(p == 10 for _, p, _ in log)
    true = _true_residual(plan, x, b, 10)
    _, it0, _, _ = fb.gmres_capi(plan, torch.zeros_like(b), b, so)
    _, it2, _, _ = fb.gmres_capi(plan, torch.zeros_like(b), b, so, M=fb.BlockDiagonal(fb, fb.LaplaceSphericalBEM(10, 3), panels), flexible=True)
    print("unit_sphere(5), random b, tol %g: iterations identity %d, block-diagonal inner solver (FGMRES) %d, block inverse %d; "
          "estimate %.3e, recomputed %.3e" % (TOL, it0, it2, it, res, true))
    assert true <= 2 * TOL
    # the flexible solver and solver.py's loops take the functor as well
    xf, itf, resf, _ = fb.gmres_capi(plan, torch.zeros_like(b), b, so, M=M, flexible=True)
    assert resf <= TOL and _true_residual(plan, xf, b, 10) <= 2 * TOL
    K.set_p(10)
    xs, its, ress = fb.gmres(plan, torch.zeros_like(b), b, so, M=M)
    assert its == it and float(torch.linalg.vector_norm(xs - x) / torch.linalg.vector_norm(x)) <= 1e-9


@pytest.mark.parametrize("flexible", [False, True])
def test_solver_stokes(fb, flexible):
    import torch
    panels = fb.red_blood_cell(3)
    K = fb.StokesSphericalBEM(10, 3)
    plan = fb.FMM_plan(K, panels, p_max=10)
    M = fb.BlockInverse(fb, fb.StokesSphericalBEM(10, 3), panels)
    b = torch.from_numpy(np.random.default_rng(12).standard_normal(3 * len(panels))).cuda()
    so = fb.SolverOptions(residual=TOL, max_iters=500, max_p=10, variable_p=False)
    log = []
    x, it, res, _ = fb.gmres_capi(plan, torch.zeros_like(b), b, so, M=M, log=log, stokes=True, flexible=flexible)
    orders = {p for _, p, _ in log}
    assert res <= TOL and len(orders) == 1                      # variable_p = 0: one order, the Stokes rule's (GMRES: max_p - 1)
    true = _true_residual(plan, x, b, orders.pop())
    _, it0, _, _ = fb.gmres_capi(plan, torch.zeros_like(b), b, so, stokes=True, flexible=flexible)
    print("red_blood_cell(3) Stokes, %s: iterations identity %d, block inverse %d; estimate %.3e, recomputed %.3e" %
          ("FGMRES" if flexible else "GMRES", it0, it, res, true))
    assert true <= 2 * TOL


def test_batch_solver_gives_each_systems_single_solve_bits(fb):
    import torch
    panels, K, plan, B = _laplace_operator(fb)
    so = fb.SolverOptions(residual=TOL, max_iters=500, max_p=10)
    M = fb.BlockInverse(fb, fb.LaplaceSphericalBEM(10, 3), panels)
    for flexible in (False, True):
        logs = [[], [], []]
        X, its, ress, _ = fb.gmres_capi_batch(plan, torch.zeros_like(B), B, so, M=M, logs=logs, flexible=flexible)
        for j in range(3):
            log = []
            x, it, res, _ = fb.gmres_capi(plan, torch.zeros_like(B[j]), B[j].contiguous(), so, M=M, log=log, flexible=flexible)
            assert it == its[j] and res == ress[j] and log == logs[j]
            assert torch.equal(x, X[j]), (flexible, j)


def test_other_kinds_do_not_move(fb):
    """Kinds 0-2: the same iteration counts, histories and solution bits before any inverse exists and after one has been built
    (on the inner-solver form's own plan too) and used by a kind-3 solve on the same operator"""
    import torch
    panels, K, plan, B = _laplace_operator(fb)
    b = B[1].contiguous()
    so = fb.SolverOptions(residual=TOL, max_iters=500, max_p=10)
    diag = fb.Diagonal(plan)
    inner_a = fb.BlockDiagonal(fb, fb.LaplaceSphericalBEM(10, 3), panels)

    def run(M, flexible):
        log = []
        x, it, res, _ = fb.gmres_capi(plan, torch.zeros_like(b), b, so, M=M, log=log, flexible=flexible)
        return x.clone(), it, res, log

    before = [run(None, False), run(diag, False), run(inner_a, False), run(inner_a, True)]
    inner_b = fb.BlockDiagonal(fb, fb.LaplaceSphericalBEM(10, 3), panels)
    inner_b.plan.block_inverse_build()
    M3 = fb.BlockInverse(fb, fb.LaplaceSphericalBEM(10, 3), panels)
    run(M3, False)
    run(M3, True)
    with pytest.raises(fb.FmmBemError):                          # the twin plan shares the geometry, not the inverse
        inner_a.plan.block_inverse_apply(np.zeros(len(panels)))
    after = [run(None, False), run(diag, False), run(inner_b, False), run(inner_b, True)]
    for (x0, it0, r0, l0), (x1, it1, r1, l1) in zip(before, after):
        assert it0 == it1 and r0 == r1 and l0 == l1
        assert torch.equal(x0, x1)
    # a plan without an inverse is refused as kind 3, and so is the operator itself
    from fmm_bem_relaxed_amd import solver
    fake = solver.BlockInverse.__new__(solver.BlockInverse)
    for pl in (inner_a.plan, plan):
        fake.plan = pl
        with pytest.raises(fb.FmmBemError) as e:
            fb.gmres_capi(plan, torch.zeros_like(b), b, so, M=fake)
        assert e.value.status == 1
