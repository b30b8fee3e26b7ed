"""PlanAdapter::execute_velocity_gradient and execute_stress of the header-only adapter (include/fmmbem/FMM_plan.hpp) on the plan
field_plan returns, compiled with plain g++ against the C ABI (tests/cpp/field_velocity_gradient.cpp)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def _build(tmp_path):
    exe = str(tmp_path / "field_velocity_gradient")
    libdir = os.path.join(ROOT, "fmm-bem-relaxed_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "field_velocity_gradient.cpp"), "-o", exe,
                           "-L" + libdir, "-lfmmbem_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def _points(tmp_path):
    rng = np.random.default_rng(12)
    d = rng.normal(size=(300, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    pts = d * np.concatenate([0.8 * rng.random(60), 1.05 + 3 * rng.random(240)])[:, None]
    pts[-5:] = pts[0]                                   # coincident points
    path = str(tmp_path / "points.bin")
    with open(path, "wb") as f:
        f.write(np.int64(len(pts)).tobytes())
        f.write(np.ascontiguousarray(pts).tobytes())
    return path, pts


def test_program_compiles_and_reports(tmp_path, gpu_available):
    exe = _build(tmp_path)
    path, _ = _points(tmp_path)
    r = subprocess.run([exe, "4", path], capture_output=True, text=True, timeout=300)
    if not gpu_available:
        assert r.returncode == 2 and "no HIP device" in r.stdout


@pytest.mark.gpu
def test_adapter_matches_python(tmp_path, fb):
    exe = _build(tmp_path)
    path, pts = _points(tmp_path)
    r = subprocess.run([exe, "4", path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == "single 6" and lines[1] == "traction 6"      # Error(FMMBEM_ERR_UNSUPPORTED), both
    v = fb.unit_sphere(4)
    i = np.arange(len(v))
    x = np.stack([1.0 + (i % 7) / 4, (i % 5) / 8 - 0.25, 0.5 - (i % 3) / 4], axis=1)
    K = fb.StokesSphericalBEM(8, 4, 1e-3)
    K.set_Kfine(19)
    opts = fb.FMMOptions()
    plan = fb.FMM_plan(K, v, opts, p_max=10).field_plan(pts)
    at = 2
    for p in (8, 10):
        K.set_p(p)
        for word, method in (("gradient", plan.execute_velocity_gradient), ("stress", plan.execute_stress)):
            assert lines[at] == "%s %d %d %d" % (word, len(v), len(pts), p)
            got = np.array([[float(t) for t in ln.split()] for ln in lines[at + 1: at + 1 + len(pts)]]).reshape(len(pts), 3, 3)
            at += 1 + len(pts)
            assert np.array_equal(got, method(x)), (word, p)         # the same library calls, the same combination: the same bits
    assert at == len(lines)
