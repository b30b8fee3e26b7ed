"""The representation execute (fmmbem_plan_execute_representation), host side: the symbols, the refusals of the C ABI in the order
include/fmmbem.h states them -- one probe per rung, each arranged so that only that rung can fire --, the buffers untouched and the
handles usable after every refusal, and the argument checks of the Python forms.  No device needed."""
import ctypes

import numpy as np
import pytest


def test_symbols_present(fb):
    L = fb.lib()
    for name in ("fmmbem_plan_execute_representation", "fmmbem_plan_execute_representation_device"):
        assert name in fb.SYMBOLS
        getattr(L, name)
    assert L.fmmbem_version() == 1
    for name in ("execute_representation", "execute_representation_device", "execute_representation_torch"):
        assert hasattr(fb.FMM_plan, name)


@pytest.fixture(scope="module")
def plans(fb):
    v = fb.unit_sphere(3)
    pts = np.random.default_rng(1).normal(size=(50, 3)) * 2
    KS, KL = fb.StokesSphericalBEM(5, 3), fb.LaplaceSphericalBEM(5, 3)
    flags = (np.arange(50) % 2).astype(np.uint8)
    return dict(v=v, pts=pts,
                field=fb.FMM_plan(KL, v, host_only=True).field_plan(pts, flags),          # Laplace, over separate targets, host-only
                single=fb.FMM_plan(KL, v, host_only=True),                                # over its own panels
                stokes=fb.FMM_plan(KS, v, host_only=True).field_plan(pts))                # a Stokes field plan


def test_refusals_in_order_and_the_handle_stays_usable(fb, plans):
    L = fb.lib()
    v, pts = plans["v"], plans["pts"]
    tp, single, stokes = plans["field"], plans["single"], plans["stokes"]
    buf = np.zeros(3 * len(v) + 3 * len(pts))
    bp, null = buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p()
    before = tp.pairs("m2l").copy()
    forms = (lambda h, p, s, m, f, g: L.fmmbem_plan_execute_representation(h, p, s, m, f, g),
             lambda h, p, s, m, f, g: L.fmmbem_plan_execute_representation_device(h, p, s, m, f, g, null))
    err = lambda: L.fmmbem_last_error().decode()
    some = [(bp, bp), (bp, None), (None, bp)]                 # the combinations of two pointers that are not both null
    for call in forms:
        assert call(None, 5, bp, bp, bp, bp) == 1 and "null plan" in err()          # 1 null plan (everything else in order)
        assert call(tp._h, 5, None, None, bp, bp) == 1 and "no layer" in err()      # 2 both inputs null ...
        assert call(tp._h, 5, bp, bp, None, None) == 1 and "no output" in err()     #   ... or both outputs null
        for h in (single._h, stokes._h):                                            #   before p and before the kind of plan
            assert call(h, 0, None, None, bp, bp) == 1 and call(h, 0, bp, bp, None, None) == 1 and "p_max" not in err()
        assert call(tp._h, 0, bp, bp, bp, bp) == 1 and "p_max" in err()             # 3 p = 0 and p_max + 1
        assert call(tp._h, 6, bp, bp, bp, bp) == 1 and "p_max" in err()
        assert call(single._h, 0, bp, bp, bp, bp) == 1 and call(stokes._h, 6, bp, bp, bp, bp) == 1      #   before the kind of plan
        assert call(single._h, 5, bp, bp, bp, bp) == 6 and "separate targets" in err()    # 4 not over separate targets
        assert call(stokes._h, 5, bp, bp, bp, bp) == 6 and "Laplace" in err()             # 5 a Stokes plan (host-only too: Stokes first)
        for s, m in some:                                                                 # 6 host-only, every other rung passed
            for f, g in some:
                assert call(tp._h, 5, s, m, f, g) == 6 and "host-only" in err()
    assert np.all(buf == 0)                                   # no refusal touched a pointer
    # the handles are still usable
    assert np.array_equal(tp.pairs("m2l"), before)
    assert tp.stats()["n_panels"] == len(v) and tp.target_info()["n_targets"] == 50
    assert single.stats()["n_panels"] == len(v) and stokes.target_info()["n_targets"] == 50


def test_python_forms_check_their_arguments(fb, plans):
    v = plans["v"]
    tp = plans["field"]
    ones = np.ones(len(v))
    for plan, x in ((tp, ones), (plans["single"], ones), (plans["stokes"], np.ones((len(v), 3)))):
        with pytest.raises(fb.FmmBemError) as e:
            plan.execute_representation(x, x)
        assert e.value.status == 6
    for bad in (np.ones(len(v) + 1), np.ones((len(v), 2)), np.ones((2, len(v)))):
        with pytest.raises(ValueError):
            tp.execute_representation(bad, ones)
        with pytest.raises(ValueError):
            tp.execute_representation(ones, bad)
        with pytest.raises(ValueError):
            tp.execute_representation(None, bad)
    with pytest.raises(ValueError):
        tp.execute_representation(None, None)
    with pytest.raises(ValueError):
        tp.execute_representation(ones, ones, value=False, gradient=False)
    with pytest.raises(ValueError):
        tp.execute_representation(np.full(len(v), "a"), ones)       # not numbers
    for s, m in ((ones, None), (None, ones)):                       # one layer alone passes the checks and reaches the library
        with pytest.raises(fb.FmmBemError) as e:
            tp.execute_representation(s, m)
        assert e.value.status == 6
    import torch
    for bad in (torch.ones(len(v), dtype=torch.float64), torch.ones(len(v), dtype=torch.float32)):      # not on a device / float
        with pytest.raises(ValueError):
            tp.execute_representation_torch(bad, None)
        with pytest.raises(ValueError):
            tp.execute_representation_torch(None, bad)
    with pytest.raises(ValueError):
        tp.execute_representation_torch(None, None)
    with pytest.raises(ValueError):
        tp.execute_representation_torch(torch.ones(len(v), dtype=torch.float64), None, value=False, gradient=False)
    with pytest.raises(fb.FmmBemError) as e:                  # the device form reaches the library's refusal
        tp.execute_representation_device(8, 8, 8, 0)
    assert e.value.status == 6
    with pytest.raises(fb.FmmBemError) as e:
        tp.execute_representation_device(0, 0, 8, 8)
    assert e.value.status == 1
    with pytest.raises(fb.FmmBemError) as e:
        tp.execute_representation_device(8, 0, 0, 0)
    assert e.value.status == 1
