"""The reference's four-argument constructor FMM_plan(K, sources, targets, opts) (include/FMM_plan.hpp:45-55) through the
header-only adapter (include/fmmbem/FMM_plan.hpp), compiled with plain g++ against the C ABI (tests/cpp/target_plan.cpp)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def _build(tmp_path):
    exe = str(tmp_path / "target_plan")
    libdir = os.path.join(ROOT, "fmm-bem-relaxed_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "target_plan.cpp"), "-o", exe,
                           "-L" + libdir, "-lfmmbem_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def _targets(tmp_path):
    rng = np.random.default_rng(12)
    d = rng.normal(size=(500, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    pts = d * np.concatenate([0.8 * rng.random(100), 1.05 + 3 * rng.random(400)])[:, None]
    flags = (rng.random(500) < 0.5).astype(np.float64)
    path = str(tmp_path / "targets.bin")
    with open(path, "wb") as f:
        f.write(np.int64(len(pts)).tobytes())
        f.write(np.ascontiguousarray(pts).tobytes())
        f.write(flags.tobytes())
    return path, pts, flags.astype(np.uint8)


def test_constructor_compiles_and_reports(tmp_path, gpu_available):
    exe = _build(tmp_path)
    path, _, _ = _targets(tmp_path)
    r = subprocess.run([exe, "4", path], capture_output=True, text=True)
    lines = r.stdout.splitlines()
    assert lines[0] == "stokes 6"                      # StokesSphericalBEM: Error(FMMBEM_ERR_UNSUPPORTED)
    if not gpu_available:
        assert r.returncode == 2 and "no HIP device" in r.stdout


@pytest.mark.gpu
def test_adapter_matches_python(tmp_path, fb):
    exe = _build(tmp_path)
    path, pts, flags = _targets(tmp_path)
    r = subprocess.run([exe, "4", path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == "stokes 6"
    v = fb.unit_sphere(4)
    x = 1.0 + (np.arange(len(v)) % 7) / 4
    K = fb.LaplaceSphericalBEM(10, 3)
    plan = fb.FMM_plan(K, v, p_max=12, targets=pts, target_bc=flags)
    at = 1
    for p in (10, 12):
        assert lines[at] == "targets %d %d %d" % (len(v), len(pts), p)
        got = np.array([float(s) for s in lines[at + 1: at + 1 + len(pts)]])
        at += 1 + len(pts)
        K.set_p(p)
        ref = plan.execute(x)
        assert np.linalg.norm(got - ref) <= 1e-15 * np.linalg.norm(ref), p
