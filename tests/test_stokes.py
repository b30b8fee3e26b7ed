"""StokesSphericalBEM, velocity boundary condition: oracle known answer
and GPU-vs-oracle parity."""
import numpy as np
import pytest

from conftest import drand48, rel_l2
from own_geometry import plan_under


@pytest.fixture(scope="module")
def stokes5(oracle_mod):
    v = oracle_mod.unit_sphere(5)
    o = oracle_mod.StokesOracle(v, K=4, K_fine=19, mu=1e-3)
    return v, o


def test_oracle_reproduces_reference_error_level(stokes5):
    """StokesBEM (velocity BC) N=2048, p=8, k=4, kfine=19: rel L2 vs Direct 1.43e-5."""
    v, o = stokes5
    x = np.tile([1.0, 0.0, 0.0], (o.n, 1))            # charges of examples/StokesBEM.cpp:257
    err = rel_l2(o.matvec(x, 8), o.direct(x))
    assert abs(err - 1.43e-5) / 1.43e-5 < 0.01, err


def test_oracle_faithful_equals_tuned(stokes5):
    v, o = stokes5
    x = drand48(3 * o.n, seed=2).reshape(o.n, 3)
    assert rel_l2(o.matvec(x, 6, faithful=True), o.matvec(x, 6)) < 1e-14


def test_oracle_sphere_drag_identity(stokes5):
    """Uniform traction 1.5 mu U / R on the unit sphere moves it with U (Stokes drag 6 pi mu R U,
    examples/StokesBEM.cpp:344-361); the single-layer operator here carries no 1/(8 pi): u * 4 pi."""
    v, o = stokes5
    f = np.tile([1.5 * o.mu, 0.0, 0.0], (o.n, 1))
    u = o.direct(f).mean(axis=0)
    assert abs(u[0] - 4 * np.pi) / (4 * np.pi) < 1e-2 and abs(u[1]) < 1e-10 and abs(u[2]) < 1e-10


@pytest.mark.gpu
def test_gpu_stokes_vs_oracle(fb, stokes5):
    v, o = stokes5
    K = fb.StokesSphericalBEM(8, 4, 1e-3)
    K.set_Kfine(19)
    pl = fb.FMM_plan(K, v, p_max=10)
    rp, col, val = o.near_csr()
    for row in (0, o.n // 2, o.n - 1):                  # 3x3 near blocks: three rows of unknowns per panel row
        for a in range(3):
            cols, vals = pl.near_row(3 * row + a)
            ref = val[rp[row]:rp[row + 1], a, :].reshape(-1)
            assert np.array_equal(cols // 3, np.repeat(col[rp[row]:rp[row + 1]], 3))
            assert np.max(np.abs(vals - ref)) / np.abs(ref).max() <= 1e-13
    for x in (np.tile([1.0, 0.0, 0.0], (o.n, 1)), drand48(3 * o.n, seed=9).reshape(o.n, 3)):
        for p in (8, 4, 10):
            K.set_p(p)
            y = pl.execute(x)
            assert y.shape == (o.n, 3)
            assert rel_l2(y, o.matvec(x, p)) <= 1e-12
    K.set_p(8)
    x = np.tile([1.0, 0.0, 0.0], (o.n, 1))
    y8, yo8 = pl.execute(x), o.matvec(x, 8)
    for which in ("M", "L"):
        E, Eo = pl.expansions(which, 8), o.expansions(8, which)
        assert np.max(np.abs(E[:, :4] - Eo[:, :4])) / np.abs(Eo).max() <= 1e-12
    err = rel_l2(y8, o.direct(x))
    assert abs(err - 1.43e-5) / 1.43e-5 < 0.01


@pytest.mark.gpu
def test_gpu_stokes_red_blood_cell(fb, oracle_mod):
    """Config-4 geometry (RedBloodCell), small: N=2048."""
    v = oracle_mod.red_blood_cell(5)
    o = oracle_mod.StokesOracle(v, K=4, K_fine=19, mu=1e-3)
    K = fb.StokesSphericalBEM(8, 4, 1e-3)
    K.set_Kfine(19)
    pl = fb.FMM_plan(K, v)
    x = drand48(3 * o.n, seed=4).reshape(o.n, 3)
    y = pl.execute(x)
    assert rel_l2(y, o.matvec(x, 8)) <= 1e-12
    assert rel_l2(y, o.direct(x)) < 1e-3


@pytest.mark.gpu
def test_gpu_stokes_traction_far_field_against_direct(fb, oracle_mod):
    """TRACTION targets through the FMM evaluator: near blocks as before, far field by the double-layer decomposition of
    kernels_far.hip (seven dipole potentials: t_i = x_k d_i Psi_k - d_i Psi_0 - Theta_i).  The reference's own far field for
    this operator is wrong, so the answer is the Direct sum over the reference's entries
    (oracle: orc_stokes_entry, kernel/StokesSphericalBEM.hpp:160-258): the error must fall with the order like that of the
    velocity operator, for all-traction targets and for mixed flags (the target's flag picks the row's operator)."""
    v = np.concatenate([oracle_mod.unit_sphere(5), oracle_mod.unit_sphere(4, center=(2.6, 0.2, -0.3))])
    n = len(v)
    x = drand48(3 * n, seed=21).reshape(n, 3)
    rows = (0, 96)
    for name, bc in (("traction", np.ones(n, dtype=np.uint8)), ("mixed", (np.arange(n) % 2).astype(np.uint8))):
        o = oracle_mod.StokesOracle(v, K=4, K_fine=19, mu=1e-3, bc=bc)
        ref = o.direct(x, rows=rows)
        errs = []
        for p in (4, 8, 12):
            K = fb.StokesSphericalBEM(p, 4, 1e-3)
            K.set_Kfine(19)
            pl = fb.FMM_plan(K, v, bc=bc)
            assert pl.stats()["m2l_pairs"] > 0
            y = pl.execute(x)[rows[0]:rows[1]]
            errs.append(rel_l2(y, ref))
            pl.close()
        # measured: 7.6e-3, 5.0e-4, 6.8e-5 at p = 4, 8, 12 (a factor ~0.55 per order, one derivative worse than the single layer)
        assert errs[0] < 2e-2 and errs[1] < 1e-3 and errs[2] < 1.5e-4 and errs[2] < errs[1] < errs[0], (name, errs)
        # the rows of velocity targets of the mixed operator are the velocity operator's rows, bit for bit
        if name == "mixed":
            K = fb.StokesSphericalBEM(8, 4, 1e-3)
            K.set_Kfine(19)
            ym = fb.FMM_plan(K, v, bc=bc).execute(x)
            yv = fb.FMM_plan(K, v).execute(x)
            assert np.array_equal(ym[bc == 0], yv[bc == 0])
        o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("p", [6, 14])
def test_gpu_stokes_traction_p2m_without_stored_gradient_records(fb, monkeypatch, p):
    """The double layer's P2M without its gradient records (FMMBEM_P2M_TABLE=0; a plan whose records would pass 16 GB takes
    the same path instead of being refused): the seven dipole multipoles from the harmonic recurrences, slot by slot
    (`p2m_kernel<1>` with wmode 5..11).  Every M of every box as with the stored records, and the result; mixed target
    flags so that the velocity group's recurrence P2M runs beside it."""
    v = np.concatenate([fb.unit_sphere(5), fb.unit_sphere(4, center=(2.6, 0.2, -0.3))])
    n = len(v)
    bc = (np.arange(n) % 3 == 0).astype(np.uint8)
    x = (drand48(3 * n, seed=5) - 0.5).reshape(n, 3)
    K = fb.StokesSphericalBEM(p, 4, 1.0)
    K.set_Kfine(7)
    ref_plan = fb.FMM_plan(K, v, bc=bc)
    y_ref, M_ref = ref_plan.execute(x), ref_plan.expansions("M", p)
    monkeypatch.setenv("FMMBEM_P2M_TABLE", "0")
    pl = fb.FMM_plan(K, v, bc=bc)
    y, M = pl.execute(x), pl.expansions("M", p)
    scale = np.abs(M_ref).max(axis=2, keepdims=True) + 1e-300
    assert np.abs(M_ref[:, 4:]).max() > 0                      # the dipole slots are live
    assert np.max(np.abs(M - M_ref) / scale) <= 1e-12
    assert rel_l2(y, y_ref) <= 1e-12


@pytest.mark.gpu
def test_gpu_stokes_traction_far_field_above_the_rotation_orders(fb, oracle_mod, monkeypatch):
    """Orders 13 ... 16 (the reference accepts any p, StokesSphericalBEM.hpp:131-141): the eleven slots of a mixed operator
    go through the double-sum M2L one slot per pass.  Against Direct the error keeps falling (p = 12: 6.8e-5); at p <= 12 the
    two M2L kernels give the same operator to rounding (FMMBEM_M2L_ROT=0)."""
    v = np.concatenate([oracle_mod.unit_sphere(4), oracle_mod.unit_sphere(3, center=(2.6, 0.2, -0.3))])
    n = len(v)
    x = drand48(3 * n, seed=23).reshape(n, 3)
    bc = (np.arange(n) % 3 != 0).astype(np.uint8)
    o = oracle_mod.StokesOracle(v, K=4, K_fine=19, mu=1e-3, bc=bc)
    ref = o.direct(x)
    K = fb.StokesSphericalBEM(16, 4, 1e-3)
    K.set_Kfine(19)
    pl = fb.FMM_plan(K, v, bc=bc)
    errs = {}
    for p in (10, 12, 13, 14, 16):
        K.set_p(p)
        errs[p] = rel_l2(pl.execute(x), ref)
    assert errs[16] < errs[14] < errs[13] < errs[12] < errs[10] and errs[16] < 0.3 * errs[12], errs
    K.set_p(12)
    y_rot = pl.execute(x)
    assert pl.stats()["m2l_kernel"] == 1
    K2 = fb.StokesSphericalBEM(12, 4, 1e-3)
    K2.set_Kfine(19)
    pl2 = plan_under(fb, monkeypatch, {"FMMBEM_M2L_ROT": "0"}, K2, v, bc=bc)      # which M2L a plan runs is its geometry's
    assert rel_l2(pl2.execute(x), y_rot) <= 1e-13
    assert pl2.stats()["m2l_kernel"] == 2
    o.close()


@pytest.mark.gpu
def test_gpu_stokes_sphere_drag_solve(fb):
    """examples/StokesBEM.cpp:255-361: unit sphere moving with U = (1,0,0); the driver overwrites its right-hand side
    with the analytic (4 pi, 0, 0) per panel (:273-276), solves the first-kind (stokeslet) system with the relaxed
    GMRES of GMRES_Stokes.hpp (p = max(p_min, predict_p - 1)) and reports the drag against 6 pi mu."""
    import torch
    mu = 1e-3
    v = fb.unit_sphere(4)
    n = len(v)
    K = fb.StokesSphericalBEM(10, 4, mu)
    K.set_Kfine(19)
    plan = fb.FMM_plan(K, v, p_max=10)
    b = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    b[:, 0] = 4 * np.pi
    so = fb.SolverOptions(residual=1e-5, max_iters=100, max_p=10, p_min=5)
    log = []
    x, it, res = fb.gmres(plan, torch.ones(3 * n, dtype=torch.float64, device="cuda"), b.reshape(-1), so, log=log, stokes=True)
    assert res < 1e-5 and min(p for _, p, _ in log) >= 5 and log[0][1] == 9          # max(p_min, 10 - 1)
    t = x.reshape(n, 3).cpu().numpy()
    e0, e1 = v[:, 2] - v[:, 0], v[:, 1] - v[:, 0]
    area = 0.5 * np.linalg.norm(np.cross(e0, e1), axis=1)
    fx, fy, fz = (t * area[:, None]).sum(axis=0)
    drag_error = abs(6 * np.pi * mu - fx) / (6 * np.pi * mu)
    assert drag_error < 2e-2 and abs(fy) < 1e-6 * abs(fx) + 1e-12 and abs(fz) < 1e-6 * abs(fx) + 1e-12
    assert np.sqrt(((t[:, 0] - 1.5 * mu) ** 2).mean()) / (1.5 * mu) < 0.1               # traction 1.5 mu U / R pointwise


@pytest.mark.gpu
def test_gpu_stokes_diagonal_and_rows_from_symmetric_blocks(fb, stokes5):
    """The Stokes near blocks are held in their symmetric 6-value form only: the introspection row and the diagonal
    (Preconditioners::Diagonal, examples/BEM/Preconditioner.hpp:19-42) are expanded from it."""
    v, o = stokes5
    K = fb.StokesSphericalBEM(8, 4, 1e-3)
    K.set_Kfine(19)
    pl = fb.FMM_plan(K, v)
    diag = pl.diagonal().reshape(o.n, 3)
    perm = pl.perm()
    rp, col, val = o.near_csr()
    for row in (0, 17, o.n - 1):
        k = rp[row] + int(np.nonzero(col[rp[row]:rp[row + 1]] == row)[0][0])        # the self block of tree row `row`
        for a in range(3):
            assert abs(diag[perm[row], a] - val[k, a, a]) <= 1e-13 * abs(val[k, a, a])
            cols, vals = pl.near_row(3 * row + a)
            assert np.max(np.abs(vals - val[rp[row]:rp[row + 1], a, :].reshape(-1))) <= 1e-13 * np.abs(val).max()


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"FMMBEM_P2M_TABLE": "0"}, {"FMMBEM_STOKES_SYM": "0"}])
def test_gpu_stokes_alternative_paths(fb, stokes5, monkeypatch, env):
    """Recurrence P2M instead of the stored moments; the 9-value near rows instead of the symmetric blocks."""
    v, o = stokes5
    K = fb.StokesSphericalBEM(8, 4, 1e-3)
    K.set_Kfine(19)
    pl = plan_under(fb, monkeypatch, env, K, v)                # the storage form is the geometry's; the P2M table is the plan's own
    x = drand48(3 * o.n, seed=5).reshape(o.n, 3)
    assert rel_l2(pl.execute(x), o.matvec(x, 8)) <= 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("k,kfine", [(4, 79), (13, 25), (79, 79)])
def test_gpu_stokes_other_rules(fb, oracle_mod, k, kfine):
    """The other keys of GaussQuadrature.hpp as K and K_fine, up to the 79-point rule (:186-272): near blocks and matvec."""
    v = oracle_mod.unit_sphere(3)
    o = oracle_mod.StokesOracle(v, K=k, K_fine=kfine, mu=1e-3)
    K = fb.StokesSphericalBEM(6, k, 1e-3)
    K.set_Kfine(kfine)
    pl = fb.FMM_plan(K, v)
    rp, col, val = o.near_csr()
    for row in (0, o.n - 1):
        for a in range(3):
            _, vals = pl.near_row(3 * row + a)
            ref = val[rp[row]:rp[row + 1], a, :].reshape(-1)
            assert np.max(np.abs(vals - ref)) / np.abs(ref).max() <= 1e-13
    x = drand48(3 * o.n, seed=12).reshape(o.n, 3)
    assert rel_l2(pl.execute(x), o.matvec(x, 6)) <= 1e-12


@pytest.mark.gpu
def test_gpu_stokes_high_orders(fb, oracle_mod):
    """p = 13..16: the Stokes L2P stages 8 leaves x 4 potentials x S(p) coefficients per wavefront, 69.6 KB at p = 16 --
    above the 64 KB a kernel gets without hipFuncAttributeMaxDynamicSharedMemorySize."""
    v = oracle_mod.unit_sphere(4)
    o = oracle_mod.StokesOracle(v, K=4, K_fine=19, mu=1e-3)
    K = fb.StokesSphericalBEM(16, 4, 1e-3)
    K.set_Kfine(19)
    pl = fb.FMM_plan(K, v, p_max=16)
    x = drand48(3 * o.n, seed=6).reshape(o.n, 3)
    for p in (13, 15, 16):
        K.set_p(p)
        assert rel_l2(pl.execute(x), o.matvec(x, p)) <= 1e-12


@pytest.mark.gpu
def test_gpu_stokes_traction_entries_and_near_field_operators(fb, oracle_mod):
    """TRACTION targets (kernel/StokesSphericalBEM.hpp:160-258, 377-389): the 3x3 blocks -3 int (d.n) d d^T / r^5 against the
    oracle's restatement (self 2 pi I, near K_fine, far K points), through fmmbem_kernel_entries and through the assembled
    near matrix of the near-field-only evaluators.  The oracle's Direct sum over the same entries reproduces the double-layer identity
    sum_j T_ij c = 4 pi c on a closed surface (12.5664)."""
    v = oracle_mod.unit_sphere(5)
    n = len(v)
    bc = np.ones(n, dtype=np.uint8)
    K = fb.StokesSphericalBEM(6, 4, 1e-3)
    K.set_Kfine(19)
    o = oracle_mod.StokesOracle(v, K=4, K_fine=19, mu=1e-3, bc=bc, evaluator=1)
    rng = np.random.default_rng(13)
    ti = np.concatenate([np.arange(30), rng.integers(0, n, 300)]).astype(np.int32)
    sj = np.concatenate([np.arange(30), np.clip(ti[30:] + rng.integers(-40, 41, 300), 0, n - 1)]).astype(np.int32)
    ref = o.kernel_entries(ti, sj)
    got = fb.kernel_entries(K, v[ti], v[sj], target_bc=bc[ti])
    assert np.max(np.abs(got - ref)) <= 1e-12 * np.max(np.abs(ref))
    u = o.direct(np.tile([1.0, 0.0, 0.0], (n, 1)), rows=(0, 64))
    assert np.max(np.abs(u[:, 0] - 4 * np.pi)) < 2e-2 and np.max(np.abs(u[:, 1:])) < 2e-2
    x = drand48(3 * n, seed=8).reshape(n, 3)
    for name, ev in (("local", 1), ("block", 2)):
        oe = oracle_mod.StokesOracle(v, K=4, K_fine=19, mu=1e-3, bc=bc, evaluator=ev)
        fo = fb.FMMOptions()
        fo.lazy_evaluation = False
        fo.local_evaluation, fo.block_diagonal = (ev == 1), (ev == 2)
        pl = fb.FMM_plan(K, v, fo, bc=bc)
        assert rel_l2(pl.execute(x), oe.matvec(x, 6)) <= 1e-13, name
        oe.close()
    # mixed flags: the target's flag picks the integral row by row
    mixed = (np.arange(n) % 3 == 0).astype(np.uint8)
    om = oracle_mod.StokesOracle(v, K=4, K_fine=19, mu=1e-3, bc=mixed, evaluator=1)
    fo = fb.FMMOptions()
    fo.lazy_evaluation, fo.local_evaluation = False, True
    assert rel_l2(fb.FMM_plan(K, v, fo, bc=mixed).execute(x), om.matvec(x, 6)) <= 1e-13
    om.close()
    o.close()


@pytest.mark.gpu
def test_gpu_stokes_matrix_free_near_field(fb, stokes5, monkeypatch):
    """StokesBEM -disable_sparse (examples/StokesBEM.cpp:197; EvalInteractionLazy.hpp:239-252): the near field recomputed
    every matvec equals the assembled one."""
    v, o = stokes5
    K = fb.StokesSphericalBEM(8, 4, 1e-3)
    K.set_Kfine(19)
    fo = fb.FMMOptions()
    fo.sparse_local = False
    pl = fb.FMM_plan(K, v, fo)
    st = pl.stats()
    assert st["near_bytes"] == 0 and 0 < st["near_side_entries"] < 0.2 * st["near_nnz"]     # the near-regime pairs, kept; no matrix
    x = drand48(3 * o.n, seed=11).reshape(o.n, 3)
    y = pl.execute(x)
    assert rel_l2(y, o.matvec(x, 8)) <= 1e-12
    assert rel_l2(y, fb.FMM_plan(K, v).execute(x)) <= 1e-14                                  # the assembled operator
    # a rule of more than four points takes the literal kernel (every block recomputed by stokes_entry): K = 13
    K13 = fb.StokesSphericalBEM(8, 13, 1e-3)
    K13.set_Kfine(19)
    assert rel_l2(fb.FMM_plan(K13, v, fo).execute(x), fb.FMM_plan(K13, v).execute(x)) <= 1e-14


@pytest.mark.gpu
def test_gpu_stokes_traction_shards_and_matrix_free(fb, oracle_mod):
    """The double-layer operator through the other routes of the plan: shards over target leaves sum to the whole operator bit
    for bit (a shard builds gradient records for its own P2M rows only when the upward pass is sharded too), and the
    matrix-free near field gives the assembled operator."""
    v = np.concatenate([oracle_mod.unit_sphere(4), oracle_mod.unit_sphere(4, center=(2.4, 0.0, 0.3))])
    n = len(v)
    bc = (np.arange(n) % 3 != 0).astype(np.uint8)                       # mostly TRACTION targets, some velocity
    x = drand48(3 * n, seed=33).reshape(n, 3)
    K = fb.StokesSphericalBEM(7, 4, 1e-3)
    K.set_Kfine(19)
    y = fb.FMM_plan(K, v, bc=bc).execute(x)
    total = np.zeros_like(y)
    for rank in range(3):
        part = fb.FMM_plan(K, v, bc=bc, shard=(rank, 3))
        total += part.execute(x)
        part.close()
    assert np.array_equal(total, y)
    fo = fb.FMMOptions()
    fo.sparse_local = False
    ymf = fb.FMM_plan(K, v, fo, bc=bc).execute(x)
    assert rel_l2(ymf, y) <= 1e-13
