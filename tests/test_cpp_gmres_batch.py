"""fmmbem::GMRES_batch / FGMRES_batch through the header-only adapter (include/fmmbem/FMM_plan.hpp), compiled with plain g++
against the C ABI (tests/cpp/gmres_batch.cpp): every system's report and solution, printed with %.17g, equal as text to what
fmmbem::GMRES / FGMRES print for that system alone."""
import os
import subprocess

import pytest

from conftest import ROOT


def _build(tmp_path):
    exe = str(tmp_path / "gmres_batch")
    libdir = os.path.join(ROOT, "fmm-bem-relaxed_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "gmres_batch.cpp"), "-o", exe,
                           "-L" + libdir, "-lfmmbem_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def _blocks(lines, tag):
    """{system: lines of its block} for the blocks that start with '<tag> <j>'"""
    out, cur = {}, None
    for ln in lines:
        head = ln.split()
        if len(head) == 2 and head[0] in ("single", "batch"):
            cur = int(head[1]) if head[0] == tag else None
            if cur is not None:
                out[cur] = []
        elif cur is not None:
            out[cur].append(ln)
    return out


def test_program_compiles_and_reports(tmp_path, gpu_available):
    exe = _build(tmp_path)
    r = subprocess.run([exe, "4", "3", "gmres"], capture_output=True, text=True, timeout=300)
    if not gpu_available:
        assert r.returncode == 2 and r.stdout.startswith("error 2"), r.stdout + r.stderr
    else:
        assert r.returncode == 0 and r.stdout.startswith("systems 512 3 gmres"), r.stdout[:300] + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("k,mode", [(3, "gmres"), (4, "fgmres"), (5, "gmres_diag"), (2, "fgmres_diag")])
def test_adapter_batch_equals_single_solves_as_text(tmp_path, k, mode):
    exe = _build(tmp_path)
    r = subprocess.run([exe, "4", str(k), mode], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    n = 2 * 4 ** 4
    assert lines[0] == "systems %d %d %s" % (n, k, mode)
    single, batch = _blocks(lines[1:], "single"), _blocks(lines[1:], "batch")
    assert sorted(single) == sorted(batch) == list(range(k))
    iters = set()
    for j in range(k):
        assert len(single[j]) >= n + 2                  # the report, at least one iteration, the solution
        assert single[j] == batch[j], (j, single[j][0], batch[j][0])
        iters.add(single[j][0].split()[1])
    if k > 2:
        assert len(iters) > 1, "the systems should not all take the same number of iterations"
