"""fmmbem_plan_execute_batch(_device) and fmmbem_plan_batch_width on host-only plans: argument checks first, then exactly the
refusals of fmmbem_plan_execute on the same handle (include/fmmbem.h)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

OK, INVALID, NO_DEVICE, UNSUPPORTED = 0, 1, 2, 6


def _plans(fb):
    v = fb.unit_sphere(3)
    rng = np.random.default_rng(3)
    pts = rng.normal(size=(40, 3)) * 2.0
    return {
        "laplace": fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), v, host_only=True),
        "stokes": fb.FMM_plan(fb.StokesSphericalBEM(5, 3), v, host_only=True),
        "targets": fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), v, host_only=True, targets=pts),
    }


def _sizes(pl):
    nx = pl.n * pl.dof
    return nx, (nx if pl.n_targets is None else pl.n_targets)


@pytest.mark.parametrize("which", ["laplace", "stokes", "targets"])
def test_invalid_arguments_then_execute_refusals(fb, which):
    pl = _plans(fb)[which]
    L = fb.lib()
    nx, ny = _sizes(pl)
    k = 3
    x = np.ones(k * nx)
    y = np.zeros(k * ny)
    xp, yp = x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p)
    single = L.fmmbem_plan_execute(pl._h, 5, xp, yp)
    assert single == (UNSUPPORTED if which == "targets" else NO_DEVICE)
    for host in (True, False):
        def call(h, kk, xx, ldx, yy, ldy):
            if host:
                return L.fmmbem_plan_execute_batch(h, 5, kk, xx, ldx, yy, ldy)
            return L.fmmbem_plan_execute_batch_device(h, 5, kk, xx, ldx, yy, ldy, None)
        assert call(None, k, xp, nx, yp, ny) == INVALID            # null plan
        assert call(pl._h, k, None, nx, yp, ny) == INVALID         # null vectors
        assert call(pl._h, k, xp, nx, None, ny) == INVALID
        assert call(pl._h, 0, xp, nx, yp, ny) == INVALID           # k < 1
        assert call(pl._h, -1, xp, nx, yp, ny) == INVALID
        assert call(pl._h, k, xp, nx - 1, yp, ny) == INVALID       # leading dimensions shorter than a vector
        assert call(pl._h, k, xp, nx, yp, ny - 1) == INVALID
        assert call(pl._h, k, xp, nx, yp, ny) == single            # otherwise: what execute says
        assert call(pl._h, k, xp, nx + 5, yp, ny + 2) == single
    assert not y.any()                                              # nothing written


def test_batch_width_host_only(fb):
    L = fb.lib()
    w = C.c_int(-1)
    assert L.fmmbem_plan_batch_width(None, C.byref(w)) == INVALID
    for pl in _plans(fb).values():
        assert L.fmmbem_plan_batch_width(pl._h, None) == INVALID
        assert pl.batch_width() == 1                                # nothing runs on a host-only plan


def test_execute_batch_shapes_and_status(fb):
    pls = _plans(fb)
    lap, sto, tgt = pls["laplace"], pls["stokes"], pls["targets"]
    n = lap.n
    for pl, bad in ((lap, np.ones(n)), (lap, np.ones((2, n + 1))), (lap, np.ones((0, n))), (lap, np.ones((2, n, 3))),
                    (sto, np.ones((2, n))), (sto, np.ones((2, n, 2))), (sto, np.ones((2, 3 * n))), (tgt, np.ones((2, n, 1)))):
        with pytest.raises(ValueError):
            pl.execute_batch(bad)
    for pl, x in ((lap, np.ones((3, n))), (sto, np.ones((2, n, 3)))):
        with pytest.raises(fb.FmmBemError) as e:
            pl.execute_batch(x)
        assert e.value.status == NO_DEVICE
    with pytest.raises(fb.FmmBemError) as e:
        tgt.execute_batch(np.ones((2, n)))
    assert e.value.status == UNSUPPORTED


def test_adapter_program_compiles_with_gxx(tmp_path):
    exe = str(tmp_path / "batch")
    libdir = os.path.join(ROOT, "fmm-bem-relaxed_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "batch.cpp"), "-o", exe,
                           "-L" + libdir, "-lfmmbem_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.isfile(exe)
