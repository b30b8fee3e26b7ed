"""fmmbem_plan_block_inverse_* and preconditioner kind 3 on host-only plans: the order of the refusals (include/fmmbem.h),
and the handles stay usable."""
import ctypes as C

import numpy as np

OK, INVALID, NO_DEVICE, UNSUPPORTED = 0, 1, 2, 6


def _block_diagonal_options(fb, sparse=True):
    o = fb.FMMOptions()
    o.local_evaluation, o.lazy_evaluation, o.sparse_local, o.block_diagonal = False, False, sparse, True
    return o


def test_symbols_and_constants(fb):
    from fmm_bem_relaxed_amd import _capi
    L = fb.lib()
    for name in ("fmmbem_plan_block_inverse_build", "fmmbem_plan_block_inverse_apply_device", "fmmbem_plan_block_inverse_apply",
                 "fmmbem_plan_block_inverse_bytes"):
        assert name in fb.SYMBOLS and getattr(L, name)
    assert _capi.PC_BLOCK_INVERSE == 3
    assert L.fmmbem_version() == 1                                        # additive: the ABI version does not move


def test_build_status_order_on_host_only_plans(fb):
    L = fb.lib()
    v = fb.unit_sphere(3)
    K = fb.LaplaceSphericalBEM(5, 3)
    assert L.fmmbem_plan_block_inverse_build(None) == INVALID             # 1. null
    fmm = fb.FMM_plan(K, v, host_only=True)
    assert L.fmmbem_plan_block_inverse_build(fmm._h) == INVALID           # 2. another evaluator ...
    assert b"BLOCK_DIAGONAL" in L.fmmbem_last_error()
    loc = fb.FMMOptions()
    loc.local_evaluation, loc.lazy_evaluation = True, False
    assert L.fmmbem_plan_block_inverse_build(fb.FMM_plan(K, v, loc, host_only=True)._h) == INVALID
    pts = np.random.default_rng(3).normal(size=(40, 3)) * 2.0
    tp = fb.FMM_plan(K, v, host_only=True, targets=pts)
    assert L.fmmbem_plan_block_inverse_build(tp._h) == INVALID            # ... or a target plan
    mf = fb.FMM_plan(K, v, _block_diagonal_options(fb, sparse=False), host_only=True)
    assert L.fmmbem_plan_block_inverse_build(mf._h) == UNSUPPORTED        # 3. matrix-free, before host-only
    sh = fb.FMM_plan(K, v, _block_diagonal_options(fb), host_only=True, shard=(0, 2))
    assert L.fmmbem_plan_block_inverse_build(sh._h) == UNSUPPORTED        #    a shard
    bd = fb.FMM_plan(K, v, _block_diagonal_options(fb), host_only=True)
    assert L.fmmbem_plan_block_inverse_build(bd._h) == NO_DEVICE          # 4. host-only
    assert L.fmmbem_plan_block_inverse_build(bd._h) == NO_DEVICE
    st = fb.FMM_plan(fb.StokesSphericalBEM(5, 3), v, _block_diagonal_options(fb), host_only=True)
    assert L.fmmbem_plan_block_inverse_build(st._h) == NO_DEVICE
    for pl in (fmm, tp, mf, sh, bd, st):                                   # the handles are still usable
        assert pl.stats()["n_panels"] == pl.n
        assert pl.block_inverse_bytes() == 0


def test_apply_before_build_and_argument_checks(fb):
    L = fb.lib()
    v = fb.unit_sphere(3)
    bd = fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), v, _block_diagonal_options(fb), host_only=True)
    n = bd.n
    x, z = np.full(2 * n, 2.0), np.full(2 * n, 3.0)
    xp, zp = x.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p)
    for host in (True, False):
        def call(h, k, vv, ldv, zz, ldz):
            if host:
                return L.fmmbem_plan_block_inverse_apply(h, k, vv, ldv, zz, ldz)
            return L.fmmbem_plan_block_inverse_apply_device(h, k, vv, ldv, zz, ldz, None)
        assert call(bd._h, 1, xp, n, zp, n) == INVALID                    # no inverse built
        assert b"no inverse built" in L.fmmbem_last_error()
        assert call(bd._h, 2, xp, n, zp, n) == INVALID
        assert call(None, 1, xp, n, zp, n) == INVALID                     # as execute_batch refuses them
        assert call(bd._h, 0, xp, n, zp, n) == INVALID
        assert call(bd._h, -1, xp, n, zp, n) == INVALID
        assert call(bd._h, 1, None, n, zp, n) == INVALID
        assert call(bd._h, 1, xp, n, None, n) == INVALID
        assert call(bd._h, 2, xp, n - 1, zp, n) == INVALID
        assert call(bd._h, 2, xp, n, zp, n - 1) == INVALID
        assert b"leading dimension" in L.fmmbem_last_error()
    assert (x == 2.0).all() and (z == 3.0).all()                           # nothing written
    assert L.fmmbem_plan_block_inverse_bytes(None, None) == INVALID
    assert bd.stats()["n_panels"] == n


def test_gmres_validates_kind_3_before_the_plan(fb):
    """A block-inverse preconditioner without a plan of its own is refused with the null arguments, before the operator plan's
    own refusal; with one, the host-only operator answers as for every other kind."""
    from fmm_bem_relaxed_amd import _capi
    L = fb.lib()
    v = fb.unit_sphere(3)
    K = fb.LaplaceSphericalBEM(5, 3)
    op = fb.FMM_plan(K, v, host_only=True)
    bd = fb.FMM_plan(K, v, _block_diagonal_options(fb), host_only=True)
    n = op.n
    k = 2
    x, b = np.full(k * n, 2.0), np.ones(k * n)
    xp, bp = x.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)
    o = _capi.SolverOpts()
    L.fmmbem_solver_options_default(C.byref(o))
    o.max_p = 5
    pc = _capi.Preconditioner()
    pc.kind = _capi.PC_BLOCK_INVERSE
    calls = (lambda: L.fmmbem_gmres(op._h, C.byref(o), xp, bp, C.byref(pc), None),
             lambda: L.fmmbem_gmres_device(op._h, C.byref(o), xp, bp, C.byref(pc), None, None),
             lambda: L.fmmbem_gmres_batch(op._h, C.byref(o), k, xp, n, bp, n, C.byref(pc), None),
             lambda: L.fmmbem_gmres_batch_device(op._h, C.byref(o), k, xp, n, bp, n, C.byref(pc), None, None))
    pc.inner_plan = None
    for call in calls:
        assert call() == INVALID
        assert b"plan of its own" in L.fmmbem_last_error()
    pc.inner_plan = op._h
    for call in calls:
        assert call() == INVALID
    pc.inner_plan = bd._h
    for call in calls:
        assert call() == NO_DEVICE
    pc.kind = 4                                                            # an unknown kind: the plan's refusal first, as before
    assert L.fmmbem_gmres(op._h, C.byref(o), xp, bp, C.byref(pc), None) == NO_DEVICE
    assert (x == 2.0).all() and (b == 1.0).all()


def test_python_surface(fb):
    import pytest
    assert fb.BlockInverse is not None
    bd = fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), fb.unit_sphere(3), _block_diagonal_options(fb), host_only=True)
    with pytest.raises(fb.FmmBemError) as e:
        bd.block_inverse_build()
    assert e.value.status == NO_DEVICE
    with pytest.raises(ValueError):
        bd.block_inverse_apply(np.zeros(bd.n + 1))
    with pytest.raises(fb.FmmBemError) as e:
        bd.block_inverse_apply(np.zeros(bd.n))
    assert e.value.status == INVALID


# ---- the pivoting inputs of tests/test_gpu_block_inverse_pivot.py: their property holds on the oracle's blocks -------------

def test_pivoting_inputs_exchange_rows_on_the_oracles_blocks(oracle_mod):
    """The GPU tests count exchanges on the blocks they read back from the plan; here the same count on the CPU oracle's
    entries, so that the inputs are known to pivot wherever the suite runs."""
    import block_inverse_cases as bic
    for name, beyond in (("laplace-257-f1", 256), ("stokes-86-vel", 256)):
        (A,) = bic.oracle_blocks(oracle_mod, name)
        assert A.shape[0] == (257 if name.startswith("laplace") else 258)
        inv, piv, bad = bic.gauss_jordan(A)
        assert bad is None
        print("%s: %d exchanges, %d with a pivot row >= %d" % (name, bic.exchanges(piv), bic.exchanges(piv, beyond), beyond))
        assert bic.exchanges(piv) > 0 and bic.exchanges(piv, beyond) > 0
        assert np.abs(inv @ A - np.eye(len(A))).max() <= 1e-8            # the restatement inverts
    blocks = bic.oracle_blocks(oracle_mod, "multi-mixed")
    assert sorted(len(A) for A in blocks) == [1, 1, 31, 270, 297]
    counts = {len(A): bic.exchanges(bic.gauss_jordan(A)[1]) for A in blocks}
    print("multi-mixed: exchanges by leaf size", counts)
    assert counts[297] > 0 and counts[270] > 0                           # both leaves of more than 256 rows
