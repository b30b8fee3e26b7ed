"""The device Direct sum (fmmbem_direct_*), host side: the symbols, the chunk length, and the status codes -- every invalid call is
refused by one host pass before any device is touched, so all of this runs without a GPU.  (The invalid calls of apply need a handle,
which only a device gives: a NaN in a target point and n_targets != n_sources are in test_gpu_direct.py.)"""
import ctypes

import numpy as np
import pytest

VP = ctypes.c_void_p


def options(fb, **kw):
    o = fb.Options()
    fb.lib().fmmbem_options_default(ctypes.byref(o))
    for k, val in kw.items():
        setattr(o, k, val)
    return o


def create(fb, o, v, n=None, out=True):
    """(status, handle value or None): the handle is seeded with garbage so that `left NULL` is an observation"""
    h = VP(0xdead)
    rc = fb.lib().fmmbem_direct_create(ctypes.byref(o) if o is not None else None, (0 if v is None else len(v)) if n is None else n,
                                       v.ctypes.data_as(VP) if v is not None else None, ctypes.byref(h) if out else None)
    return rc, h.value


def test_symbols_and_chunk(fb):
    L = fb.lib()
    for name in ("fmmbem_direct_create", "fmmbem_direct_apply", "fmmbem_direct_apply_device", "fmmbem_direct_chunk",
                 "fmmbem_direct_destroy"):
        assert name in fb.SYMBOLS
        getattr(L, name)
    assert L.fmmbem_direct_chunk() > 0
    L.fmmbem_direct_destroy(None)                      # a null handle is a no-op


def test_create_invalid_arguments_leave_out_null(fb):
    v = np.ascontiguousarray(fb.unit_sphere(3)).reshape(-1, 9)
    cases = {
        "null options": (None, v, None),
        "null vertices": (options(fb), None, 5),
        "no sources": (options(fb), v, 0),
        "bad quadrature key": (options(fb, quad_k=5), v, None),
        "bad K_fine": (options(fb, kernel=1, quad_k=4, quad_k_fine=5, mu=1.0), v, None),
        "mu = 0": (options(fb, kernel=1, quad_k=4, quad_k_fine=19, mu=0.0), v, None),
    }
    for what, (o, vv, n) in cases.items():
        rc, h = create(fb, o, vv, n)
        assert rc == 1, what
        assert h is None, what
    for bad_value in (np.nan, np.inf):
        bad = v.copy()
        bad[7, 4] = bad_value
        rc, h = create(fb, options(fb), bad)
        assert rc == 1 and h is None
    assert create(fb, options(fb), v, out=False)[0] == 1
    rc, h = create(fb, options(fb, kernel=7), v)
    assert rc == 6 and h is None                       # an unknown kernel id, as everywhere in the C ABI


def test_apply_rejects_null_handle(fb):
    L = fb.lib()
    buf = np.zeros(16)
    bp = buf.ctypes.data_as(VP)
    assert L.fmmbem_direct_apply(None, 4, bp, None, bp, bp) == 1
    assert L.fmmbem_direct_apply_device(None, 4, bp, None, bp, bp, None) == 1


def test_create_on_valid_input_reports_the_device(fb, gpu_available):
    """valid input passes the host checks; what comes back then says whether a device is there"""
    v = np.ascontiguousarray(fb.unit_sphere(3)).reshape(-1, 9)
    for o in (options(fb), options(fb, kernel=1, quad_k=4, quad_k_fine=19, mu=1e-3)):
        rc, h = create(fb, o, v)
        if gpu_available:
            assert rc == 0 and h
            fb.lib().fmmbem_direct_destroy(VP(h))
        else:
            assert rc == 2 and h is None
            assert "no HIP device" in fb.lib().fmmbem_last_error().decode()
    if not gpu_available:
        for K in (fb.LaplaceSphericalBEM(5, 3), fb.StokesSphericalBEM(5, 4)):
            with pytest.raises(fb.FmmBemError) as e:
                fb.Direct(K, fb.unit_sphere(3))
            assert e.value.status == 2


def test_python_argument_checks(fb):
    with pytest.raises(fb.FmmBemError) as e:
        fb.Direct(fb.LaplaceSphericalBEM(5, 5), fb.unit_sphere(2))         # quadrature key 5 does not exist
    assert e.value.status == 1
    with pytest.raises(fb.FmmBemError) as e:
        fb.Direct(fb.LaplaceSphericalBEM(5, 3), np.zeros((0, 3, 3)))
    assert e.value.status == 1
