"""PlanAdapter::execute_batch through the header-only adapter (include/fmmbem/FMM_plan.hpp), compiled with plain g++ against the
C ABI (tests/cpp/batch.cpp)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def _build(tmp_path):
    exe = str(tmp_path / "batch")
    libdir = os.path.join(ROOT, "fmm-bem-relaxed_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "batch.cpp"), "-o", exe,
                           "-L" + libdir, "-lfmmbem_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def _charges(n, k):
    i = np.arange(n)
    return np.stack([1.0 + ((i + 3 * j) % 7) / 4 for j in range(k)])


def test_program_compiles_and_reports(tmp_path, gpu_available):
    exe = _build(tmp_path)
    r = subprocess.run([exe, "4", "3", "8"], capture_output=True, text=True, timeout=300)
    if not gpu_available:
        assert r.returncode == 2 and r.stdout.startswith("error 2"), r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("k,p", [(3, 8), (5, 10)])
def test_adapter_batch_matches_python_and_singles(tmp_path, fb, k, p):
    exe = _build(tmp_path)
    r = subprocess.run([exe, "4", str(k), str(p)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == "mismatch 1"                    # FMMBEM_ERR_INVALID: a vector of the wrong length
    v = fb.unit_sphere(4)
    n = len(v)
    assert lines[1] == "batch %d %d %d" % (n, k, p)
    assert lines[2] == "equal 1"
    got = np.array([float(s) for s in lines[3:3 + k * n]]).reshape(k, n)
    K = fb.LaplaceSphericalBEM(p, 3)
    plan = fb.FMM_plan(K, v)
    assert np.array_equal(got, plan.execute_batch(_charges(n, k)))
