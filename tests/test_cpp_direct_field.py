"""fmmbem::DirectSum's field quantities (include/fmmbem/Direct.hpp: gradient, pressure, velocity_gradient, stress) through plain g++
against the C ABI (tests/cpp/direct_field.cpp): each equals the C ABI's result at the same 64 points bit for bit, and the other
kernel's methods throw the library's refusal (status 6)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

M = 64


def _build(tmp_path):
    exe = str(tmp_path / "direct_field")
    libdir = os.path.join(ROOT, "fmm-bem-relaxed_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "direct_field.cpp"), "-o", exe,
                           "-L" + libdir, "-lfmmbem_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def _targets(tmp_path):
    rng = np.random.default_rng(12)
    d = rng.normal(size=(M, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    pts = np.ascontiguousarray(d * np.concatenate([0.8 * rng.random(16), 1.01 + 2 * rng.random(M - 16)])[:, None])
    flags = (rng.random(M) < 0.5).astype(np.float64)
    path = str(tmp_path / "targets.bin")
    with open(path, "wb") as f:
        f.write(np.int64(len(pts)).tobytes())
        f.write(pts.tobytes())
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
def test_adapter_equals_the_c_abi_bit_for_bit(tmp_path, fb):
    exe = _build(tmp_path)
    path, pts, flags = _targets(tmp_path)
    r = subprocess.run([exe, "4", path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = _sections(r.stdout)
    v = fb.unit_sphere(4)
    n = len(v)
    i = np.arange(n)
    L, vp = fb.lib(), ctypes.c_void_p
    ptr = lambda a: a.ctypes.data_as(vp)                                                         # noqa: E731

    x = 1.0 + (i % 7) / 4
    D = fb.Direct(fb.LaplaceSphericalBEM(5, 3), v)
    g = np.empty((M, 3))
    assert L.fmmbem_direct_gradient(D._h, M, ptr(pts), ptr(flags), ptr(x), ptr(g)) == 0
    D.close()
    assert np.any(flags == 1) and np.any(flags == 0)
    assert got["gradient"].shape == (3 * M,) and np.array_equal(got["gradient"].reshape(M, 3), g)
    assert got["laplace_refuses"].tolist() == [6, 6, 6]

    KS = fb.StokesSphericalBEM(5, 4, mu=1e-3)
    KS.set_Kfine(19)
    xs = np.ascontiguousarray(np.stack([1.0 + (i % 7) / 4, -0.5 + (i % 3), 0.25 * (i % 5)], axis=1))
    DS = fb.Direct(KS, v)
    q, G = np.empty(M), np.empty((M, 3, 3))
    assert L.fmmbem_direct_pressure(DS._h, M, ptr(pts), ptr(xs), ptr(q)) == 0
    assert L.fmmbem_direct_velocity_gradient(DS._h, M, ptr(pts), ptr(xs), ptr(G)) == 0
    DS.close()
    assert got["pressure"].shape == (M,) and np.array_equal(got["pressure"], q)
    assert got["velocity_gradient"].shape == (9 * M,) and np.array_equal(got["velocity_gradient"].reshape(M, 3, 3), G)
    sigma = -q[:, None, None] * np.eye(3)[None] + 1e-3 * (G + G.transpose(0, 2, 1))
    assert got["stress"].shape == (9 * M,) and np.array_equal(got["stress"].reshape(M, 3, 3), sigma)
    assert got["stokes_refuses"].tolist() == [6]
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(q)) and np.all(np.isfinite(G)) and np.abs(G).max() > 0
