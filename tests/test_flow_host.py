"""The flow execute (fmmbem_plan_execute_flow), host side: the symbols, the refusals of the C ABI in the order include/fmmbem.h
states them -- one probe per rung, each arranged so that only that rung can fire --, the outputs untouched and the handles usable
after every refusal, and the argument checks of the Python forms.  No device needed."""
import ctypes

import numpy as np
import pytest


def test_symbols_present(fb):
    L = fb.lib()
    for name in ("fmmbem_plan_execute_flow", "fmmbem_plan_execute_flow_device"):
        assert name in fb.SYMBOLS
        getattr(L, name)
    assert L.fmmbem_version() == 1
    for name in ("execute_flow", "execute_flow_device", "execute_flow_torch", "execute_stress"):
        assert hasattr(fb.FMM_plan, name)


@pytest.fixture(scope="module")
def plans(fb):
    v = fb.unit_sphere(3)
    pts = np.random.default_rng(1).normal(size=(50, 3)) * 2
    KS, KL = fb.StokesSphericalBEM(5, 3), fb.LaplaceSphericalBEM(5, 3)
    flags = np.zeros(50, np.uint8)
    flags[7] = 1
    return dict(v=v, pts=pts,
                field=fb.FMM_plan(KS, v, host_only=True).field_plan(pts),
                single=fb.FMM_plan(KS, v, host_only=True),
                laplace=fb.FMM_plan(KL, v, host_only=True).field_plan(pts),
                traction=fb.FMM_plan(KS, v, host_only=True).field_plan(pts, flags))


def test_refusals_in_order_and_the_handle_stays_usable(fb, plans):
    L = fb.lib()
    v, pts = plans["v"], plans["pts"]
    tp, single, laplace, traction = plans["field"], plans["single"], plans["laplace"], plans["traction"]
    buf = np.zeros(3 * len(v) + 9 * len(pts))
    bp, null = buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p()
    before = tp.pairs("m2l").copy()
    forms = (lambda h, p, x, u, q, g: L.fmmbem_plan_execute_flow(h, p, x, u, q, g),
             lambda h, p, x, u, q, g: L.fmmbem_plan_execute_flow_device(h, p, x, u, q, g, null))
    err = lambda: L.fmmbem_last_error().decode()
    subsets = [(bp, bp, bp), (bp, None, None), (None, bp, None), (None, None, bp), (None, bp, bp), (bp, None, bp), (bp, bp, None)]
    for call in forms:
        assert call(None, 5, bp, bp, bp, bp) == 1 and "null plan" in err()          # 1 null plan (everything else in order)
        assert call(tp._h, 5, None, bp, bp, bp) == 1                                # 2 null x ...
        assert call(tp._h, 5, bp, None, None, None) == 1 and "no output" in err()   #   ... or all three outputs null
        for h in (single._h, laplace._h, traction._h):                             #   before p and before the kind of plan
            assert call(h, 0, None, bp, bp, bp) == 1 and call(h, 0, bp, None, None, None) == 1 and "p_max" not in err()
        assert call(tp._h, 0, bp, bp, bp, bp) == 1 and "p_max" in err()            # 3 p = 0 and p_max + 1
        assert call(tp._h, 6, bp, bp, bp, bp) == 1 and "p_max" in err()
        assert call(single._h, 0, bp, bp, bp, bp) == 1 and call(laplace._h, 6, bp, bp, bp, bp) == 1      #   before the kind of plan
        assert call(traction._h, 6, bp, bp, bp, bp) == 1
        assert call(single._h, 5, bp, bp, bp, bp) == 6 and "separate targets" in err()    # 4 not over separate targets
        assert call(laplace._h, 5, bp, bp, bp, bp) == 6 and "Stokes" in err()             # 5 a Laplace plan (a target plan)
        for u, q, g in subsets:                                                           # 6 a TRACTION target, whichever outputs
            assert call(traction._h, 5, bp, u, q, g) == 6 and "VELOCITY" in err()         #   (host-only too: TRACTION comes first)
        for u, q, g in subsets:                                                           # 7 host-only, every other rung passed
            assert call(tp._h, 5, bp, u, q, g) == 6 and "host-only" in err()
    assert np.all(buf == 0)                                   # no refusal touched a pointer
    # the handles are still usable
    assert np.array_equal(tp.pairs("m2l"), before)
    assert tp.stats()["n_panels"] == len(v) and tp.target_info()["n_targets"] == 50
    assert single.stats()["n_panels"] == len(v)
    assert laplace.target_info()["n_targets"] == 50 and traction.target_info()["n_targets"] == 50


def test_python_forms_check_their_arguments(fb, plans):
    v = plans["v"]
    tp = plans["field"]
    for plan, x in ((tp, np.ones((len(v), 3))), (plans["single"], np.ones(3 * len(v))), (plans["laplace"], np.ones(len(v))),
                    (plans["traction"], np.ones((len(v), 3)))):
        with pytest.raises(fb.FmmBemError) as e:
            plan.execute_flow(x)
        assert e.value.status == 6
        with pytest.raises(fb.FmmBemError) as e:
            plan.execute_stress(x)                            # as before the flow execute carried it
        assert e.value.status == 6
    for bad in (np.ones(len(v)), np.ones(3 * len(v) + 1), np.ones((len(v), 2)), np.ones((3, len(v)))):
        with pytest.raises(ValueError):
            tp.execute_flow(bad)
    with pytest.raises(ValueError):
        tp.execute_flow(np.ones((len(v), 3)), velocity=False, pressure=False, velocity_gradient=False)
    with pytest.raises(ValueError):
        tp.execute_flow(np.full((len(v), 3), "a"))            # not numbers
    import torch
    for bad in (torch.ones(3 * len(v), dtype=torch.float64), torch.ones(3 * len(v), dtype=torch.float32)):      # not on a device / float
        with pytest.raises(ValueError):
            tp.execute_flow_torch(bad)
    with pytest.raises(ValueError):
        tp.execute_flow_torch(torch.ones(3 * len(v), dtype=torch.float64), velocity=False, pressure=False, velocity_gradient=False)
    with pytest.raises(fb.FmmBemError) as e:                  # the device form reaches the library's refusal
        tp.execute_flow_device(8, 8, 0, 0)
    assert e.value.status == 6
    with pytest.raises(fb.FmmBemError) as e:
        tp.execute_flow_device(8, 0, 0, 0)
    assert e.value.status == 1
