"""fmmbem_options.near_f32_max_p (the float near field) without a device: the default, the range check, the Python mirror of the
structs, and the plans on which the option is accepted without effect (include/fmmbem.h)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

OK, INVALID = 0, 1


def _default_options(fb):
    from fmm_bem_relaxed_amd import _capi
    o = _capi.Options()
    fb.lib().fmmbem_options_default(C.byref(o))
    return o


def test_default_is_off_and_mirror_round_trips(fb):
    from fmm_bem_relaxed_amd import _capi
    o = _default_options(fb)
    assert o.near_f32_max_p == 0
    # the field is the LAST of fmmbem_options and fills the padding behind devices[8]: the C struct's size is what it was
    assert _capi.Options.near_f32_max_p.offset == _capi.Options.devices.offset + 32
    o.near_f32_max_p = 6
    o.host_only = 1
    o.p_max = 8
    v = np.ascontiguousarray(fb.unit_sphere(3), dtype=np.float64).reshape(-1, 9)
    h = C.c_void_p()
    assert fb.lib().fmmbem_plan_create(C.byref(o), len(v), v.ctypes.data_as(C.c_void_p), None, C.byref(h)) == OK
    s = _capi.Stats()
    assert fb.lib().fmmbem_plan_stats(h, C.byref(s)) == OK
    d = s.as_dict()
    assert d["near_f32_bytes"] == 0 and d["last_near_f32"] == 0
    assert d["n_panels"] == len(v) and d["n_devices"] == 1     # the fields in front of the new ones still line up
    fb.lib().fmmbem_plan_destroy(h)


@pytest.mark.parametrize("bad", [-1, 17])
@pytest.mark.parametrize("targets", [False, True])
def test_out_of_range_is_invalid(fb, bad, targets):
    o = _default_options(fb)
    o.host_only = 1
    o.near_f32_max_p = bad
    v = np.ascontiguousarray(fb.unit_sphere(2), dtype=np.float64).reshape(-1, 9)
    pts = np.ascontiguousarray(np.random.default_rng(1).normal(size=(10, 3)) * 2.0)
    h = C.c_void_p()
    if targets:
        rc = fb.lib().fmmbem_plan_create_targets(C.byref(o), len(v), v.ctypes.data_as(C.c_void_p), None, len(pts),
                                                 pts.ctypes.data_as(C.c_void_p), None, C.byref(h))
    else:
        rc = fb.lib().fmmbem_plan_create(C.byref(o), len(v), v.ctypes.data_as(C.c_void_p), None, C.byref(h))
    assert rc == INVALID and not h.value
    with pytest.raises(fb.FmmBemError) as e:
        fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), fb.unit_sphere(2), host_only=True, near_f32_max_p=bad,
                    targets=pts if targets else None)
    assert e.value.status == INVALID


@pytest.mark.parametrize("k", [1, 16])
def test_range_ends_are_accepted(fb, k):
    pl = fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), fb.unit_sphere(2), host_only=True, near_f32_max_p=k)
    assert pl.stats()["near_f32_bytes"] == 0


@pytest.mark.parametrize("kernel", ["laplace", "stokes"])
def test_host_only_plan_builds_and_reports_zero(fb, kernel):
    K = fb.LaplaceSphericalBEM(5, 3) if kernel == "laplace" else fb.StokesSphericalBEM(5, 3)
    v = fb.unit_sphere(3)
    pl = fb.FMM_plan(K, v, host_only=True, near_f32_max_p=4)
    ref = fb.FMM_plan(K, v, host_only=True)
    s, r = pl.stats(), ref.stats()
    assert s["near_f32_bytes"] == 0 and s["last_near_f32"] == 0
    assert r["near_f32_bytes"] == 0 and r["last_near_f32"] == 0
    for key in ("n_panels", "n_boxes", "n_leaves", "near_nnz", "m2l_pairs", "p2p_pairs"):
        assert s[key] == r[key]                                  # the option does not touch the tree or the lists
    assert pl.batch_width() == 1


def test_target_plan_with_the_option_builds_and_reports_zero(fb):
    v = fb.unit_sphere(3)
    pts = np.random.default_rng(2).normal(size=(50, 3)) * 2.0
    pl = fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), v, host_only=True, targets=pts, near_f32_max_p=5)
    s = pl.stats()
    assert s["near_f32_bytes"] == 0 and s["last_near_f32"] == 0
    assert s["n_panels"] == len(v)


def test_adapter_program_compiles_with_gxx(tmp_path):
    exe = str(tmp_path / "near_f32")
    libdir = os.path.join(ROOT, "fmm-bem-relaxed_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "near_f32.cpp"), "-o", exe,
                           "-L" + libdir, "-lfmmbem_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, "3", "4"], capture_output=True, text=True, timeout=300)
    # without a device the program reports the refusal of the plan (FMMBEM_ERR_NO_DEVICE) and exits 2; with one it runs
    assert (r.returncode == 2 and r.stdout.startswith("error 2")) or r.returncode == 0, r.stdout + r.stderr
