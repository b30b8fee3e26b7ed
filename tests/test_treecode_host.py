"""The treecode evaluator (FMMBEM_EVAL_TREECODE = 4, `-eval TREE`) without a device: the value is accepted where the issue says
so and refused with FMMBEM_ERR_UNSUPPORTED (6) elsewhere, a host-only plan holds the FMM plan's lists, and the C++ and Python
option classes map to it.  The value 3 stays "no such evaluator" (tests/test_capi_host.py::test_error_codes)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

UNSUPPORTED = 6
LIST_COUNTS = ("n_panels", "n_boxes", "n_leaves", "n_levels", "near_nnz", "near_nnz_total", "p2p_pairs", "m2l_pairs", "m2l_pairs_owned",
               "m2m_ops", "l2l_ops", "p2m_leaves", "l2p_leaves", "m2l_classes")


def options(fb, **kw):
    o = fb.Options()
    fb.lib().fmmbem_options_default(ctypes.byref(o))
    o.host_only = 1
    for k, val in kw.items():
        setattr(o, k, val)
    return o


def create(fb, o, v):
    h = ctypes.c_void_p()
    rc = fb.lib().fmmbem_plan_create(ctypes.byref(o), len(v), v.ctypes.data_as(ctypes.c_void_p), None, ctypes.byref(h))
    if rc == 0:
        fb.lib().fmmbem_plan_destroy(h)
    return rc


def test_constant(fb):
    from fmm_bem_relaxed_amd import _capi
    assert _capi.EVAL_TREECODE == 4


def test_host_only_plan_holds_the_fmm_plans_lists(fb):
    v = fb.unit_sphere(4)
    opts = fb.FMMOptions()
    opts.set_max_per_box(16)
    fmm = fb.FMM_plan(fb.LaplaceSphericalBEM(8, 3), v, opts, host_only=True)
    opts_t = fb.FMMOptions()
    opts_t.set_max_per_box(16)
    opts_t.evaluator = "TREECODE"
    tree = fb.FMM_plan(fb.LaplaceSphericalBEM(8, 3), v, opts_t, host_only=True)
    a, b = fmm.stats(), tree.stats()
    assert a["m2l_pairs"] > 0
    for k in LIST_COUNTS:
        assert a[k] == b[k], k
    assert np.array_equal(fmm.perm(), tree.perm())
    for which in ("p2p", "m2l", "m2m"):
        assert np.array_equal(fmm.pairs(which), tree.pairs(which)), which


def test_refusals(fb):
    from fmm_bem_relaxed_amd import _capi
    v = np.ascontiguousarray(fb.unit_sphere(3))
    assert create(fb, options(fb, evaluator=4), v) == 0
    assert create(fb, options(fb, evaluator=4, sparse_local=0, near_stream_fraction=0.5, near_f32_max_p=4, l2l_rule=1), v) == 0
    assert create(fb, options(fb, evaluator=4, kernel=_capi.KERNEL_STOKES_BEM), v) == UNSUPPORTED
    assert "Stokes" in fb.lib().fmmbem_last_error().decode()
    assert create(fb, options(fb, evaluator=4, shard_rank=1, shard_world=2), v) == UNSUPPORTED
    assert "shard_world" in fb.lib().fmmbem_last_error().decode()
    o = options(fb, evaluator=4, n_devices=2)
    o.devices[0], o.devices[1] = 0, 1
    assert create(fb, o, v) == UNSUPPORTED
    assert "device list" in fb.lib().fmmbem_last_error().decode()
    assert create(fb, options(fb, evaluator=3), v) == 1               # still no such evaluator


def test_device_list_from_the_environment_is_refused(fb, monkeypatch):
    v = np.ascontiguousarray(fb.unit_sphere(3))
    monkeypatch.setenv("FMMBEM_DEVICES", "0,1")
    assert create(fb, options(fb, evaluator=4, host_only=0), v) == UNSUPPORTED


def test_target_plans_refuse_it(fb):
    v = np.ascontiguousarray(fb.unit_sphere(3))
    pts = np.ascontiguousarray(np.random.default_rng(0).normal(size=(50, 3)) * 3)
    o = options(fb, evaluator=4)
    h = ctypes.c_void_p()
    rc = fb.lib().fmmbem_plan_create_targets(ctypes.byref(o), len(v), v.ctypes.data_as(ctypes.c_void_p), None, len(pts),
                                             pts.ctypes.data_as(ctypes.c_void_p), None, ctypes.byref(h))
    assert rc == UNSUPPORTED


def test_python_options_round_trip(fb):
    v = fb.unit_sphere(3)
    opts = fb.FMMOptions()
    assert opts.evaluator == "FMM"
    opts.evaluator = "TREECODE"
    plan = fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), v, opts, host_only=True)
    assert plan.options().evaluator == "TREECODE"
    opts.lazy_evaluation, opts.local_evaluation = False, True       # no far field to choose: the LOCAL evaluator as ever
    local = fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), v, opts, host_only=True)
    assert local.stats()["m2l_pairs"] == 0
    opts.evaluator = "TREE"
    with pytest.raises(ValueError):
        fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), v, opts, host_only=True)
    with pytest.raises(fb.FmmBemError) as e:                          # Stokes: the library's refusal
        so = fb.FMMOptions()
        so.evaluator = "TREECODE"
        fb.FMM_plan(fb.StokesSphericalBEM(5, 4, 1e-3), v, so, host_only=True)
    assert e.value.status == UNSUPPORTED


def test_cpp_adapter_maps_eval_tree(tmp_path):
    exe = str(tmp_path / "treecode_options")
    libdir = os.path.join(ROOT, "fmm-bem-relaxed_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "treecode_options.cpp"),
                           "-o", exe, "-L" + libdir, "-lfmmbem_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, "3", "-eval", "TREE"], capture_output=True, text=True, check=True).stdout.splitlines()
    assert out[0].split() == ["evaluator", "4", "1", "2"]
    hp = out[1].split()
    assert hp[0] == "host_plan" and hp[1] == "0" and int(hp[2]) > 0 and hp[2:4] == hp[4:6]
    assert out[2].split() == ["stokes", str(UNSUPPORTED)]
    out = subprocess.run([exe, "3"], capture_output=True, text=True, check=True).stdout.splitlines()
    assert out[0].split() == ["evaluator", "0", "1", "2"]
