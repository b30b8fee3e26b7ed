"""fmmbem_gmres_batch(_device) on host-only plans: the argument checks come first, then exactly the refusals of fmmbem_gmres on
the same handle (include/fmmbem.h), and the handle stays usable."""
import ctypes as C

import numpy as np
import pytest

OK, INVALID, NO_DEVICE, UNSUPPORTED = 0, 1, 2, 6


def _plans(fb):
    v = fb.unit_sphere(3)
    pts = np.random.default_rng(3).normal(size=(40, 3)) * 2.0
    return {
        "laplace": fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), v, host_only=True),
        "stokes": fb.FMM_plan(fb.StokesSphericalBEM(5, 3), v, host_only=True),
        "targets": fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), v, host_only=True, targets=pts),
    }


def _options():
    from fmm_bem_relaxed_amd import _capi
    o = _capi.SolverOpts()
    _capi.lib().fmmbem_solver_options_default(C.byref(o))
    o.max_p = 5
    return o


@pytest.mark.parametrize("which", ["laplace", "stokes", "targets"])
def test_invalid_arguments_then_gmres_refusals(fb, which):
    from fmm_bem_relaxed_amd import _capi
    pl = _plans(fb)[which]
    L = fb.lib()
    n = pl.n * pl.dof
    k = 3
    x, b = np.full(k * (n + 4), 2.0), np.ones(k * (n + 4))
    xp, bp = x.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)
    o = _options()
    logs = (_capi.SolverLog * k)()
    single = L.fmmbem_gmres(pl._h, C.byref(o), xp, bp, None, None)
    assert single == (UNSUPPORTED if which == "targets" else NO_DEVICE)
    for host in (True, False):
        def call(h, oo, kk, xx, ldx, bb, ldb, lg=None):
            if host:
                return L.fmmbem_gmres_batch(h, oo, kk, xx, ldx, bb, ldb, None, lg)
            return L.fmmbem_gmres_batch_device(h, oo, kk, xx, ldx, bb, ldb, None, lg, None)
        ob = C.byref(o)
        assert call(None, ob, k, xp, n, bp, n) == INVALID             # null plan, options, vectors
        assert call(pl._h, None, k, xp, n, bp, n) == INVALID
        assert call(pl._h, ob, k, None, n, bp, n) == INVALID
        assert call(pl._h, ob, k, xp, n, None, n) == INVALID
        assert call(pl._h, ob, 0, xp, n, bp, n) == INVALID            # k < 1
        assert call(pl._h, ob, -2, xp, n, bp, n) == INVALID
        assert call(pl._h, ob, k, xp, n - 1, bp, n) == INVALID        # leading dimensions shorter than a vector
        assert call(pl._h, ob, k, xp, n, bp, n - 1) == INVALID
        assert b"leading dimension" in L.fmmbem_last_error()
        assert call(pl._h, ob, k, xp, n, bp, n) == single             # otherwise: what fmmbem_gmres says
        assert call(pl._h, ob, k, xp, n + 4, bp, n + 3) == single
        assert call(pl._h, ob, k, xp, n, bp, n, logs) == single       # with logs and without (above)
        assert call(pl._h, ob, 1, xp, n, bp, n) == single
    assert (x == 2.0).all() and (b == 1.0).all()                       # nothing written
    # the handle is still usable
    assert pl.stats()["n_panels"] == pl.n
    assert L.fmmbem_gmres(pl._h, C.byref(o), xp, bp, None, None) == single


def test_single_entry_refusals_on_a_host_only_plan(fb):
    """fmmbem_gmres on a host-only plan: null arguments are INVALID; after them the plan's own refusal comes before the checks
    of the options (restart = 0) and of the preconditioner (DIAGONAL without reciprocals), and nothing is written"""
    from fmm_bem_relaxed_amd import _capi
    pl = _plans(fb)["laplace"]
    L = fb.lib()
    x, b = np.full(pl.n, 2.0), np.ones(pl.n)
    xp, bp = x.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)
    o = _options()
    assert L.fmmbem_gmres(None, C.byref(o), xp, bp, None, None) == INVALID
    assert L.fmmbem_gmres(pl._h, None, xp, bp, None, None) == INVALID
    assert L.fmmbem_gmres(pl._h, C.byref(o), None, bp, None, None) == INVALID
    assert L.fmmbem_gmres(pl._h, C.byref(o), xp, None, None, None) == INVALID
    assert b"fmmbem_gmres: null argument" in L.fmmbem_last_error()
    o.restart = 0
    assert L.fmmbem_gmres(pl._h, C.byref(o), xp, bp, None, None) == NO_DEVICE
    o = _options()
    pc = _capi.Preconditioner()
    pc.kind, pc.reciprocals = _capi.PC_DIAGONAL, None
    log = _capi.SolverLog()
    assert L.fmmbem_gmres(pl._h, C.byref(o), xp, bp, C.byref(pc), C.byref(log)) == NO_DEVICE
    assert (x == 2.0).all() and (b == 1.0).all() and log.iterations == 0
    assert pl.stats()["n_panels"] == pl.n


def test_python_wrapper_is_exported_and_checks_shapes(fb):
    import torch
    assert fb.gmres_capi_batch is not None
    pl = _plans(fb)["laplace"]
    so = fb.SolverOptions(max_p=5)
    X = torch.zeros((2, pl.n), dtype=torch.float64)
    with pytest.raises(ValueError):                                     # CPU tensors: the solver is resident on the device
        fb.gmres_capi_batch(pl, X, X.clone(), so)
    with pytest.raises(ValueError):
        fb.gmres_capi_batch(pl, X[0], X[0].clone(), so)
