"""PlanAdapter::execute_flow and execute_stress on top of it (include/fmmbem/FMM_plan.hpp) on the plan field_plan returns, compiled
with plain g++ against the C ABI (tests/cpp/flow.cpp): the flow execute equals the three adapter executes, every combination of
null outputs, execute_stress equals the composition of the two single executes it was, and a refusal surfaces as Error and leaves
the caller's vectors alone."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def _build(tmp_path):
    exe = str(tmp_path / "flow")
    libdir = os.path.join(ROOT, "fmm-bem-relaxed_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "flow.cpp"), "-o", exe,
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
def test_adapter_flow_equals_the_adapter_executes(tmp_path, fb):
    exe = _build(tmp_path)
    path, pts = _points(tmp_path)
    r = subprocess.run([exe, "4", path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    v = fb.unit_sphere(4)
    # Error(FMMBEM_ERR_UNSUPPORTED) twice, the caller's vectors as they were, Error(FMMBEM_ERR_INVALID) with no output asked
    assert lines[:4] == ["single 6", "traction 6", "traction kept 1", "none 1"]
    at = 4
    for p in (8, 10):
        assert lines[at] == "flow %d %d %d 1 1 1" % (len(v), len(pts), p)
        assert lines[at + 1] == "subsets %d 9 9" % p
        assert lines[at + 2] == "stress %d 1" % p
        at += 3
    # and from outside: the adapter's G is the Python form's
    assert lines[at] == "gradient %d %d 10" % (len(v), len(pts))
    got = np.array([[float(t) for t in ln.split()] for ln in lines[at + 1: at + 1 + len(pts)]]).reshape(len(pts), 3, 3)
    assert at + 1 + len(pts) == len(lines)
    i = np.arange(len(v))
    x = np.stack([1.0 + (i % 7) / 4, (i % 5) / 8 - 0.25, 0.5 - (i % 3) / 4], axis=1)
    K = fb.StokesSphericalBEM(10, 4, 1e-3)
    K.set_Kfine(19)
    plan = fb.FMM_plan(K, v, fb.FMMOptions(), p_max=10).field_plan(pts)
    u, q, g = plan.execute_flow(x)
    assert np.array_equal(got, g) and np.array_equal(g, plan.execute_velocity_gradient(x))
