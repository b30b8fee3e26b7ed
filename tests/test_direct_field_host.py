"""The field quantities of the device Direct sum (fmmbem_direct_gradient / _pressure / _velocity_gradient and their _device forms), host
side: the symbols, the refusal of a null handle -- the first check, made before any device is touched -- and the Python methods.  All
of this runs without a GPU; what needs a handle is in test_gpu_direct_field.py."""
import ctypes
import inspect

import numpy as np
import pytest

VP = ctypes.c_void_p
HOST = ("fmmbem_direct_gradient", "fmmbem_direct_pressure", "fmmbem_direct_velocity_gradient")
DEVICE = tuple(name + "_device" for name in HOST)


def test_symbols_are_declared_and_exported(fb):
    L = fb.lib()
    for name in HOST + DEVICE:
        assert name in fb.SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    assert fb.lib().fmmbem_version() == 1              # entry points only: the ABI version stays


def test_null_handle_is_refused(fb):
    L = fb.lib()
    buf = np.zeros(64)
    before = buf.copy()
    bp = buf.ctypes.data_as(VP)
    assert L.fmmbem_direct_gradient(None, 4, bp, None, bp, bp) == 1
    assert L.fmmbem_direct_gradient_device(None, 4, bp, None, bp, bp, None) == 1
    assert L.fmmbem_direct_pressure(None, 4, bp, bp, bp) == 1
    assert L.fmmbem_direct_pressure_device(None, 4, bp, bp, bp, None) == 1
    assert L.fmmbem_direct_velocity_gradient(None, 4, bp, bp, bp) == 1
    assert L.fmmbem_direct_velocity_gradient_device(None, 4, bp, bp, bp, None) == 1
    assert "null" in L.fmmbem_last_error().decode()
    assert np.array_equal(buf, before)


def test_direct_class_has_the_methods(fb):
    want = {"gradient": ["x", "targets", "target_bc"], "pressure": ["x", "targets"], "velocity_gradient": ["x", "targets"],
            "stress": ["x", "targets"], "gradient_torch": ["x", "targets", "target_bc", "out"], "pressure_torch": ["x", "targets", "out"],
            "velocity_gradient_torch": ["x", "targets", "out"]}
    for name, args in want.items():
        fn = getattr(fb.Direct, name)
        assert list(inspect.signature(fn).parameters)[1:] == args, name


def test_without_a_device_direct_still_reports_it(fb, gpu_available):
    if gpu_available:
        D = fb.Direct(fb.LaplaceSphericalBEM(5, 3), fb.unit_sphere(2))
        with pytest.raises(ValueError):
            D.gradient(np.ones(len(fb.unit_sphere(2)) - 1), np.zeros((3, 3)))     # shape errors are ValueError, as in matvec
        with pytest.raises(ValueError):
            D.gradient(np.ones(len(fb.unit_sphere(2))), None)                     # no symmetric form
        D.close()
        return
    for K in (fb.LaplaceSphericalBEM(5, 3), fb.StokesSphericalBEM(5, 4)):
        with pytest.raises(fb.FmmBemError) as e:
            fb.Direct(K, fb.unit_sphere(3))
        assert e.value.status == 2
