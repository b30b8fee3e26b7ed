"""PlanAdapter::field_plan of the header-only adapter (include/fmmbem/FMM_plan.hpp), compiled with plain g++ against the C ABI
(tests/cpp/field_plan.cpp): a Laplace and a Stokes field plan, an order above the operator plan's p_max (the field plan grows), and
execute_batch -- against FMM_plan.field_plan of the Python surface on the GPU."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def _build(tmp_path):
    exe = str(tmp_path / "field_plan")
    libdir = os.path.join(ROOT, "fmm-bem-relaxed_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "field_plan.cpp"), "-o", exe,
                           "-L" + libdir, "-lfmmbem_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def _points(tmp_path):
    rng = np.random.default_rng(12)
    d = rng.normal(size=(500, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    pts = d * np.concatenate([0.8 * rng.random(100), 1.05 + 3 * rng.random(400)])[:, None]
    pts[480:] = pts[479]                                   # coincident points
    flags = (rng.random(500) < 0.5).astype(np.float64)
    path = str(tmp_path / "points.bin")
    with open(path, "wb") as f:
        f.write(np.int64(len(pts)).tobytes())
        f.write(np.ascontiguousarray(pts).tobytes())
        f.write(flags.tobytes())
    return path, pts, flags.astype(np.uint8)


def test_field_plan_compiles_and_the_constructor_keeps_refusing(tmp_path, gpu_available):
    exe = _build(tmp_path)
    path, _, _ = _points(tmp_path)
    r = subprocess.run([exe, "4", path], capture_output=True, text=True)
    lines = r.stdout.splitlines()
    assert lines[0] == "four-argument stokes 6"            # StokesSphericalBEM: Error(FMMBEM_ERR_UNSUPPORTED), as before
    if not gpu_available:
        assert r.returncode == 2 and "no HIP device" in r.stdout


@pytest.mark.gpu
def test_adapter_matches_python(tmp_path, fb):
    exe = _build(tmp_path)
    path, pts, flags = _points(tmp_path)
    r = subprocess.run([exe, "4", path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == "four-argument stokes 6"
    v = fb.unit_sphere(4)
    n, m = len(v), len(pts)
    i = np.arange(n)
    q = 1.0 + (i % 7) / 4
    g = np.stack([q, -0.5 + (i % 5) / 8, 0.25 * (i % 3)], axis=1)
    KS = fb.StokesSphericalBEM(6, 4, 1e-3)
    KS.set_Kfine(19)
    at = 1
    for name, K, x, orders, dof in (("laplace", fb.LaplaceSphericalBEM(8, 3), q, (8, 11), 1), ("stokes", KS, g, (6, 9), 3)):
        assert lines[at] == "field of field 6"
        at += 1

        def block(at):
            return np.array([[float(s) for s in ln.split()] for ln in lines[at:at + m]]).reshape((m,) if dof == 1 else (m, 3))

        for p in orders:
            assert lines[at] == "%s %d %d %d" % (name, n, m, p)
            got = block(at + 1)
            at += 1 + m
            K.set_p(p)
            field = fb.FMM_plan(K, v, p_max=p).field_plan(pts, flags)      # sized as the adapter's plan is at this point
            ref = field.execute(x)
            assert np.linalg.norm(got - ref) <= 1e-15 * np.linalg.norm(ref), (name, p)
        assert lines[at] == "batch 2"
        ref = field.execute(x)                             # the last order set
        for sign in (1.0, -1.0):
            got = block(at + 1)
            at += m
            assert np.linalg.norm(got - sign * ref) <= 1e-15 * np.linalg.norm(ref), (name, "batch", sign)
        at += 1
    assert at == len(lines)
