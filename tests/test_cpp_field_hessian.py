"""PlanAdapter::execute_hessian of the header-only adapter (include/fmmbem/FMM_plan.hpp) on a plan over separate targets and on a
field plan, compiled with plain g++ against the C ABI (tests/cpp/field_hessian.cpp)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def _build(tmp_path):
    exe = str(tmp_path / "field_hessian")
    libdir = os.path.join(ROOT, "fmm-bem-relaxed_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "field_hessian.cpp"), "-o", exe,
                           "-L" + libdir, "-lfmmbem_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def _targets(tmp_path):
    rng = np.random.default_rng(13)
    d = rng.normal(size=(300, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    pts = d * np.concatenate([0.8 * rng.random(60), 1.05 + 3 * rng.random(240)])[:, None]
    pts[-5:] = pts[0]                                   # coincident targets
    flags = (rng.random(300) < 0.5).astype(np.float64)
    path = str(tmp_path / "targets.bin")
    with open(path, "wb") as f:
        f.write(np.int64(len(pts)).tobytes())
        f.write(np.ascontiguousarray(pts).tobytes())
        f.write(flags.tobytes())
    return path, pts, flags.astype(np.uint8)


def test_program_compiles_and_reports(tmp_path, gpu_available):
    exe = _build(tmp_path)
    path, _, _ = _targets(tmp_path)
    r = subprocess.run([exe, "4", path], capture_output=True, text=True, timeout=300)
    if not gpu_available:
        assert r.returncode == 2 and "no HIP device" in r.stdout


@pytest.mark.gpu
def test_adapter_matches_python(tmp_path, fb):
    exe = _build(tmp_path)
    path, pts, flags = _targets(tmp_path)
    r = subprocess.run([exe, "4", path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == "single 6"                       # a plan over its own panels: Error(FMMBEM_ERR_UNSUPPORTED)
    v = fb.unit_sphere(4)
    x = 1.0 + (np.arange(len(v)) % 7) / 4
    K = fb.LaplaceSphericalBEM(10, 3)
    plan = fb.FMM_plan(K, v, p_max=12, targets=pts, target_bc=flags)
    at = 1
    for kind, p in (("targets", 10), ("targets", 12), ("field", 12)):
        assert lines[at] == "%s %d %d %d" % (kind, len(v), len(pts), p)
        got = np.array([[float(s) for s in ln.split()] for ln in lines[at + 1: at + 1 + len(pts)]]).reshape(len(pts), 3, 3)
        at += 1 + len(pts)
        K.set_p(p)
        want = plan.execute_hessian(x)
        assert np.array_equal(got, want), (kind, p)        # the same library call: the same bits
        assert np.array_equal(want, want.transpose(0, 2, 1))
    assert at == len(lines)
