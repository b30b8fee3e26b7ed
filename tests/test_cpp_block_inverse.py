"""fmmbem::BlockInversePC through the header-only adapter (include/fmmbem/FMM_plan.hpp), compiled with plain g++ against the C
ABI (tests/cpp/block_inverse.cpp): its operator() against FMM_plan.block_inverse_apply, and fmmbem::GMRES with it against
gmres_capi with solver.BlockInverse on the same mesh."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def _build(tmp_path):
    exe = str(tmp_path / "block_inverse")
    libdir = os.path.join(ROOT, "fmm-bem-relaxed_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "block_inverse.cpp"), "-o", exe,
                           "-L" + libdir, "-lfmmbem_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_program_compiles_and_reports(tmp_path, gpu_available):
    exe = _build(tmp_path)
    r = subprocess.run([exe, "3"], capture_output=True, text=True, timeout=300)
    if not gpu_available:
        assert r.returncode == 2 and r.stdout.startswith("error 2"), r.stdout + r.stderr
    else:
        assert r.returncode == 0 and r.stdout.startswith("block_inverse 128 "), r.stdout[:300] + r.stderr


@pytest.mark.gpu
def test_adapter_equals_python_calls(fb, tmp_path):
    import torch
    r = 4
    exe = _build(tmp_path)
    out = subprocess.run([exe, str(r)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[:300] + out.stderr
    lines = out.stdout.splitlines()
    n = 2 * 4 ** r
    head = lines[0].split()
    assert head[:2] == ["block_inverse", str(n)]
    iv, iz, ig = lines.index("v"), lines.index("z"), lines.index("gmres")
    v = np.array([float(t) for t in lines[iv + 1:iz]])
    z = np.array([float(t) for t in lines[iz + 1:ig]])
    rep = lines[ig + 1].split()
    iters, resid = int(rep[1]), float(rep[3])
    ps = [int(ln.split()[1]) for ln in lines[ig + 2:ig + 2 + iters]]
    x = np.array([float(t) for t in lines[ig + 2 + iters:]])
    assert v.shape == z.shape == x.shape == (n,)

    panels = fb.unit_sphere(r)
    K = fb.LaplaceSphericalBEM(10, 3)
    o = fb.FMMOptions()
    o.sparse_local = True
    plan = fb.FMM_plan(K, panels, o)
    M = fb.BlockInverse(fb, fb.LaplaceSphericalBEM(10, 3), panels)
    assert int(head[2]) == M.plan.block_inverse_bytes() > 0
    zp = M.plan.block_inverse_apply(v)
    assert np.linalg.norm(z - zp) <= 1e-15 * np.linalg.norm(zp)
    so = fb.SolverOptions(residual=1e-6, max_iters=60, max_p=10, restart=60)
    log = []
    b = torch.from_numpy(v).cuda()
    xp, it, res, _ = fb.gmres_capi(plan, torch.zeros_like(b), b, so, M=M, log=log)
    assert it == iters and [p for _, p, _ in log] == ps
    assert abs(res - resid) <= 1e-12 * resid
    xp = xp.cpu().numpy()
    assert np.linalg.norm(x - xp) <= 1e-13 * np.linalg.norm(xp)
