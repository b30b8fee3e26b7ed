"""PlanAdapter::execute_representation (include/fmmbem/FMM_plan.hpp) on the plan field_plan returns, compiled with plain g++ against
the C ABI (tests/cpp/representation.cpp): the representation execute against the adapter's two executes and two gradient executes on
an all-POTENTIAL and an all-NORMAL_DERIV plan over the same points (each row within 1e-11 of the larger of the two layers' largest
entries, the bound of tests/test_gpu_representation.py), every combination of null layers and outputs, and refusals that surface as
Error and leave the caller's vectors alone."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def _build(tmp_path):
    exe = str(tmp_path / "representation")
    libdir = os.path.join(ROOT, "fmm-bem-relaxed_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "representation.cpp"), "-o", exe,
                           "-L" + libdir, "-lfmmbem_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def _points(tmp_path):
    rng = np.random.default_rng(12)
    d = rng.normal(size=(300, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    pts = d * np.concatenate([0.8 * rng.random(60), 1.05 + 3 * rng.random(240)])[:, None]
    pts[-5:] = pts[0]                                   # coincident points (their flags differ in the program's mixed plan)
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
def test_adapter_representation_equals_the_adapter_executes(tmp_path, fb):
    exe = _build(tmp_path)
    path, pts = _points(tmp_path)
    r = subprocess.run([exe, "4", path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    v = fb.unit_sphere(4)
    # Error(FMMBEM_ERR_UNSUPPORTED), the caller's vectors as they were, Error(FMMBEM_ERR_INVALID) with no layer and with no output
    assert lines[:4] == ["single 6", "single kept 1", "no layer 1", "no output 1"]
    at = 4
    for p in (8, 12):
        head = lines[at].split()
        assert head[:4] == ["representation", str(len(v)), str(len(pts)), str(p)], lines[at]
        print(lines[at])
        assert float(head[4]) <= 1e-11 and float(head[5]) <= 1e-11, lines[at]
        assert lines[at + 1] == "subsets %d 10 10" % p
        at += 2
    # and from outside: the adapter's gradient is the Python form's
    assert lines[at] == "gradient %d %d 12" % (len(v), len(pts))
    got = np.array([[float(t) for t in ln.split()] for ln in lines[at + 1: at + 1 + len(pts)]])
    assert at + 1 + len(pts) == len(lines)
    i = np.arange(len(v))
    sigma, mu = 1.0 + (i % 7) / 4, (i % 5) / 8 - 0.25
    K = fb.LaplaceSphericalBEM(12, 3)
    flags = np.zeros(len(pts), np.uint8)
    flags[::3] = 1
    plan = fb.FMM_plan(K, v, fb.FMMOptions(), p_max=12).field_plan(pts, flags)
    phi, grad = plan.execute_representation(sigma, mu)
    assert np.array_equal(got, grad)
