"""fmmbem::DirectSum and fmmbem::direct_matvec (include/fmmbem/Direct.hpp) through plain g++ against the C ABI
(tests/cpp/direct_sum.cpp), beside the reference-named Direct::matvec of the compat header, which keeps its own route."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def _build(tmp_path):
    exe = str(tmp_path / "direct_sum")
    libdir = os.path.join(ROOT, "fmm-bem-relaxed_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "direct_sum.cpp"), "-o", exe,
                           "-L" + libdir, "-lfmmbem_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def _targets(tmp_path):
    rng = np.random.default_rng(12)
    d = rng.normal(size=(400, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    pts = d * np.concatenate([0.8 * rng.random(100), 1.01 + 2 * rng.random(300)])[:, None]
    flags = (rng.random(400) < 0.5).astype(np.float64)
    path = str(tmp_path / "targets.bin")
    with open(path, "wb") as f:
        f.write(np.int64(len(pts)).tobytes())
        f.write(np.ascontiguousarray(pts).tobytes())
        f.write(flags.tobytes())
    return path, pts, flags.astype(np.uint8)


def test_adapter_compiles_and_reports(tmp_path, gpu_available):
    exe = _build(tmp_path)
    path, _, _ = _targets(tmp_path)
    r = subprocess.run([exe, "4", path], capture_output=True, text=True)
    if not gpu_available:
        assert r.returncode == 2 and "no HIP device" in r.stdout
    else:
        assert r.returncode == 0, r.stdout + r.stderr


def _sections(text):
    out, name = {}, None
    for line in text.splitlines():
        if line[0].isalpha():
            name = line.split()[0]
            out[name] = []
        else:
            out[name].append(float(line))
    return {k: np.array(v) for k, v in out.items()}


@pytest.mark.gpu
def test_adapter_matches_python(tmp_path, fb):
    exe = _build(tmp_path)
    path, pts, flags = _targets(tmp_path)
    r = subprocess.run([exe, "4", path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = _sections(r.stdout)
    v = fb.unit_sphere(4)
    n, m = len(v), len(pts)
    i = np.arange(n)
    x = 1.0 + (i % 7) / 4

    def close(a, b):
        return np.linalg.norm(a - b) <= 1e-14 * np.linalg.norm(b)

    K = fb.LaplaceSphericalBEM(5, 3)
    D = fb.Direct(K, v)
    y = D.matvec(x, targets=pts, target_bc=flags)
    assert got["laplace"].shape == (m,) and close(got["laplace"], y)
    assert close(got["laplace_add"] - 1.5, y) and not close(got["laplace_add"], y)       # added to, not overwritten
    bc = (i % 3 == 0).astype(np.uint8)
    assert close(got["laplace_sym"], D.matvec(x, target_bc=bc))
    D.close()
    # the compat header's Direct::matvec: its own entries (fmmbem_kernel_entries) added on the host in source order, as before
    tri = np.repeat(pts[:16, None, :], 3, axis=1)
    E = fb.kernel_entries(K, np.repeat(tri, n, axis=0), np.tile(v, (16, 1, 1)), target_bc=np.repeat(flags[:16], n)).reshape(16, n)
    old = np.zeros(16)
    for j in range(n):
        old += E[:, j] * x[j]
    assert np.array_equal(got["laplace_compat"], old)
    assert np.linalg.norm(old - y[:16]) <= 1e-13 * np.linalg.norm(y[:16])                  # and the two routes agree to rounding

    KS = fb.StokesSphericalBEM(5, 4, mu=1e-3)
    KS.set_Kfine(19)
    xs = np.stack([1.0 + (i % 7) / 4, -0.5 + (i % 3), 0.25 * (i % 5)], axis=1)
    DS = fb.Direct(KS, v)
    ys = DS.matvec(xs, targets=pts, target_bc=flags)
    DS.close()
    assert got["stokes"].shape == (3 * m,) and close(got["stokes"].reshape(m, 3), ys)
    assert close(got["stokes_add"].reshape(m, 3) - 1.5, ys)
