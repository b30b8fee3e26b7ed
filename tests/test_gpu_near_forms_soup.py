"""Every form of the near field on ragged triangle soups (tests/near_form_cases.py), row by row against the CPU oracle's own near
matrix summed in np.longdouble -- never against another device plan:

    |y_i - r_i| <= (eps_entry + m_i 2^-53) (|A| |x|)_i            (the float form: + 2^-24)

with m_i the stored entries of the row and eps_entry = 1e-13 (TOL_ENTRY) for POTENTIAL rows; 4.8e-11 for NORMAL_DERIV rows and
6.8e-11 for Stokes rows, whose entries are cancelling sums on which the oracle itself is 6e-11 from a long-double evaluation
(measured: 4 x the worst |device - oracle| / |oracle|, 1.20e-11 and 1.70e-11; tests/near_form_cases.py).  The inputs: a normal
vector, a vector with one entry 1e8 above the rest, and three unit vectors (a row is then ONE entry: a wrong column -- swizzle,
padding, chunk edge -- cannot hide in a sum).  The forms: streamed (near_spmv_pipe, near_spmv_sym3, the Stokes 9-value rows of near_spmv_kernel), matrix-free, hybrid, the
float copy, the multi-vector passes; each test reads from stats() that its form ran.  Then whole executes against the oracle's
matvec, batches bit for bit against single executes, and -- in child processes, one at a time -- the kernel shapes only a
process-wide switch selects (FMMBEM_BATCH_NV, FMMBEM_BATCH_SHAPE, FMMBEM_F32_SHAPE, FMMBEM_HYB_WG_*).

Fallbacks the code states, and what is done about them here:
  * a plan without any M2L pair takes near_f32_max_p as 0 under the FMM evaluator (plan.hip, f32_premise): cases (105), (106),
    (202) and (203) run the float form under the LOCAL evaluator, which keeps the option and lists the same near field
    (tests/test_near_form_cases_host.py), so the float kernels do meet those inputs;
  * nothing else falls back on any case: a form that reports it did not run fails its test.

Batch shapes (FMMBEM_BATCH_SHAPE 1 / 2, FMMBEM_BATCH_NV 2 / 8): spmv_rows keeps ONE accumulator per row and lane, and a lane
meets its columns lane, lane + 64, ... in ascending order whatever the number of loads in flight (kVecs) or rows in flight
(kRows); the column-split quarters do not depend on either.  The shape does not change the order of a row's additions, so the
children assert bitwise equality with the single execute.

Worst measured ratios to the bound are printed by every test (pytest -s) and tabulated in DESIGN.md section 8.  On the MI355X:
streamed, matrix-free and hybrid forms 0.021 of the bound at the most (under a unit vector), the float form 0.99 (one
round-to-nearest float per entry: at its bound by construction), whole executes 3.3e-15 against the oracle's matvec."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import near_form_cases as nfc
from conftest import ROOT

pytestmark = pytest.mark.gpu

TOL_ENTRY = nfc.EPS_ENTRY
TOL_MATVEC = 1e-11                                 # tests/test_random_meshes.py: whole matvec against the oracle on soups
LAPLACE = sorted(nfc.LAPLACE)
STOKES = sorted(nfc.STOKES)


def _tag(case, mixed):
    return "(%d) %s" % (case, ("mixed" if mixed else "velocity" if nfc.is_stokes(case) else "potential"))


def _assert_rows(plan, R, what, extra=0.0):
    q = nfc.near_ratios(plan, R, extra=extra)
    print("%s: worst row / bound: %s" % (what, ", ".join("%s %.3g" % kv for kv in q.items())))
    assert max(q.values()) <= 1.0, (what, q)
    return max(q.values())


def _assert_execute(plan, R, p, what):
    """the whole matvec at order p against the oracle's, complete L2L list, 1e-11 relative L2 as on the random soups"""
    o, x = R["o"], R["X"][0]
    dof = plan.dof
    plan.kernel().set_p(p)
    y = plan.execute(x.reshape((o.n, 3)) if dof == 3 else x)
    yo = o.matvec(x.reshape((o.n, 3)) if dof == 3 else x, p)
    assert np.all(np.isfinite(y)), what
    err = float(np.linalg.norm(y - yo) / np.linalg.norm(yo))
    print("%s: execute p=%d rel. L2 against the oracle %.3g" % (what, p, err))
    assert err <= TOL_MATVEC, (what, err)


def _order(case):
    return 6 if nfc.is_stokes(case) else 8


# ------------------------------------------------------------------ the entries themselves
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("case", LAPLACE + STOKES)
def test_every_entry_of_the_default_plan(fb, oracle_mod, case, mixed):
    """plan.near_row against near_csr on EVERY row: identical columns, every value within the eps_entry of its row (1e-13 for
    POTENTIAL targets; the measured tolerances of tests/near_form_cases.py for the cancelling sums), and a Stokes row within
    1e-13 of its LARGEST entry, as tests/test_stokes.py holds it"""
    R = nfc.case_reference(oracle_mod, case, mixed)
    o = R["o"]
    rp, col, val = o.near_csr()
    plan = nfc.make_plan(fb, case, mixed)
    perm = o.perm().astype(np.int64)
    assert np.array_equal(plan.perm(), o.perm())
    worst = worst_row = worst_ratio = 0.0
    for t in range(o.n):
        ref_cols = col[rp[t]:rp[t + 1]]
        for a in range(plan.dof):
            cols, vals = plan.near_row(plan.dof * t + a)
            if plan.dof == 1:
                assert np.array_equal(cols, ref_cols), (case, t)
                ref = val[rp[t]:rp[t + 1]]
            else:
                assert np.array_equal(cols, (3 * ref_cols.astype(np.int64)[:, None] + np.arange(3)).reshape(-1)), (case, t, a)
                ref = val[rp[t]:rp[t + 1], a, :].reshape(-1)
                worst_row = max(worst_row, float(np.max(np.abs(vals - ref)) / np.abs(ref).max()))
            zero = ref == 0                              # the off-diagonal values of a TRACTION self block, 2 pi I
            assert np.all(vals[zero] == 0), (case, t, a)
            rel = float(np.max(np.abs(vals - ref)[~zero] / np.abs(ref[~zero])))
            worst = max(worst, rel)
            worst_ratio = max(worst_ratio, rel / R["eps"][plan.dof * perm[t] + a])
    print("%s: worst entry against the oracle's %.3g, %.3g of its row's eps_entry; against the row's largest entry %.3g"
          % (_tag(case, mixed), worst, worst_ratio, worst_row))
    assert worst_ratio <= 1.0, (worst, worst_ratio)
    assert worst_row <= TOL_ENTRY, worst_row


# ------------------------------------------------------------------ the near field alone, form by form
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("case", LAPLACE + STOKES)
def test_streamed(fb, oracle_mod, case, mixed):
    R = nfc.case_reference(oracle_mod, case, mixed)
    plan = nfc.make_plan(fb, case, mixed)
    st = plan.stats()
    assert st["near_bytes"] > 0 and st["near_recomputed_pairs"] == 0 and st["near_f32_bytes"] == 0
    _assert_rows(plan, R, "streamed " + _tag(case, mixed))
    assert plan.stats()["last_near_f32"] == 0
    if not (mixed and nfc.is_stokes(case)):            # the oracle's far field is velocity only
        _assert_execute(plan, R, _order(case), "streamed " + _tag(case, mixed))


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("case", STOKES)
def test_streamed_stokes_nine_value_rows(fb, oracle_mod, monkeypatch, case, mixed):
    """FMMBEM_STOKES_SYM=0 (read while the plan is created): near_spmv_kernel on 9-value rows, half as many bytes again"""
    R = nfc.case_reference(oracle_mod, case, mixed)
    sym_bytes = nfc.make_plan(fb, case, mixed).stats()["near_bytes"]
    monkeypatch.setenv("FMMBEM_STOKES_SYM", "0")
    monkeypatch.setenv("FMMBEM_PLAN_SHARE", "0")       # a live plan of the same panels would lend its geometry, symmetric blocks included
    plan = nfc.make_plan(fb, case, mixed)
    assert plan.stats()["geometry_shared"] == 1
    assert plan.stats()["near_bytes"] > 1.4 * sym_bytes
    _assert_rows(plan, R, "streamed, 9-value rows " + _tag(case, mixed))
    if not mixed:
        _assert_execute(plan, R, 6, "streamed, 9-value rows " + _tag(case, mixed))


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("case,K", [(c, k) for c in LAPLACE for k in (1, 3, 4)] + [(c, None) for c in STOKES])
def test_matrix_free(fb, oracle_mod, case, K, mixed):
    R = nfc.case_reference(oracle_mod, case, mixed, K=K)
    plan = nfc.make_plan(fb, case, mixed, K=K, sparse_local=False)
    st = plan.stats()
    assert st["near_bytes"] == 0 and st["near_side_entries"] > 0, st
    what = "matrix-free K=%s %s" % (K, _tag(case, mixed))
    _assert_rows(plan, R, what)
    if not (mixed and nfc.is_stokes(case)):
        _assert_execute(plan, R, _order(case), what)


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("f", [0.5, 0.0])
@pytest.mark.parametrize("case,K", [(c, k) for c in LAPLACE for k in (1, 3)] + [(c, None) for c in STOKES])
def test_hybrid(fb, oracle_mod, case, K, f, mixed):
    R = nfc.case_reference(oracle_mod, case, mixed, K=K)
    plan = nfc.make_plan(fb, case, mixed, K=K, near_stream_fraction=f)
    st = plan.stats()
    assert st["near_recomputed_pairs"] > 0, st
    if f == 0.0:
        assert st["near_recomputed_pairs"] == st["near_nnz"] and st["near_bytes"] == 0
    else:
        assert 0 < st["near_recomputed_pairs"] <= st["near_nnz"]
    what = "hybrid f=%.1f K=%s %s" % (f, K, _tag(case, mixed))
    _assert_rows(plan, R, what)
    if not (mixed and nfc.is_stokes(case)):
        _assert_execute(plan, R, _order(case), what)


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("case", LAPLACE + STOKES)
def test_float(fb, oracle_mod, case, mixed):
    """near_f32_max_p = 4: the near field alone (an execute at p = 1) streams the float copy; an execute above the threshold is
    bit for bit the plain plan's.  The cases without a far field: the LOCAL evaluator keeps the option there (module docstring)."""
    local = case in nfc.NO_FAR_FIELD
    R = nfc.case_reference(oracle_mod, case, mixed, evaluator=1 if local else 0)
    how = dict(evaluator="local") if local else {}
    plan = nfc.make_plan(fb, case, mixed, near_f32_max_p=4, **how)
    assert plan.stats()["near_f32_bytes"] > 0
    _assert_rows(plan, R, "float " + _tag(case, mixed), extra=nfc.EPS_F32)
    assert plan.stats()["last_near_f32"] == 1
    plain = nfc.make_plan(fb, case, mixed, **how)
    x = R["X"][0].reshape((-1, 3)) if plan.dof == 3 else R["X"][0]
    for p in (5, 8):
        plan.kernel().set_p(p)
        plain.kernel().set_p(p)
        assert np.array_equal(plan.execute(x), plain.execute(x)), p
        assert plan.stats()["last_near_f32"] == 0
    if local:                                           # under the FMM evaluator the option is taken as 0 on these two, as the code says
        assert nfc.make_plan(fb, case, mixed, near_f32_max_p=4).stats()["near_f32_bytes"] == 0


# ------------------------------------------------------------------ batches and the combined launch: the same bits
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("case", [101, 102, 107])
def test_laplace_batches_are_their_single_executes(fb, case, mixed):
    """k = 1 ... 9 vectors: passes of 4 + 4 + 1, 4 + 2, ... through near_spmv_pipe_multi_kernel; the single execute is pinned above"""
    plan = nfc.make_plan(fb, case, mixed)
    assert plan.batch_width() == 4
    X = np.random.default_rng(case).standard_normal((9, plan.n))
    single = np.stack([plan.execute(x) for x in X])
    for k in range(1, 10):
        got = plan.execute_batch(X[:k])
        for j in range(k):
            assert np.array_equal(got[j], single[j]), (case, k, j, float(np.abs(got[j] - single[j]).max()))


@pytest.mark.parametrize("width", [2, 3, 4])
@pytest.mark.parametrize("case", STOKES)
def test_stokes_batches_are_their_single_executes(fb, case, width):
    plan = nfc.make_plan(fb, case, False, p_max=6, stokes_batch_width=width)
    assert plan.batch_width() == width
    X = np.random.default_rng(case).standard_normal((width + 1, plan.n, 3))
    single = np.stack([plan.execute(x) for x in X])
    got = plan.execute_batch(X)
    for j in range(width + 1):
        assert np.array_equal(got[j], single[j]), (case, width, j, float(np.abs(got[j] - single[j]).max()))
    plain = nfc.make_plan(fb, case, False, p_max=6)
    assert plain.batch_width() == 1 and np.array_equal(plain.execute(X[0]), single[0])


@pytest.mark.parametrize("case", [101, 107])
def test_separate_near_and_p2m_launches_give_the_same_bits(fb, oracle_mod, monkeypatch, case):
    """FMMBEM_NEAR_P2M (read at every execute) = 0 against the default at p = 8"""
    R = nfc.case_reference(oracle_mod, case, False)
    plan = nfc.make_plan(fb, case, False)
    y = plan.execute(R["X"][0])
    monkeypatch.setenv("FMMBEM_NEAR_P2M", "2")         # one launch or an error: the default did take the combined launch
    assert np.array_equal(plan.execute(R["X"][0]), y)
    monkeypatch.setenv("FMMBEM_NEAR_P2M", "0")
    assert np.array_equal(plan.execute(R["X"][0]), y)


# ------------------------------------------------------------------ the shapes only a process-wide switch selects
_CHILD = r"""
import json, sys
import numpy as np
sys.path[:0] = [%(root)r, %(tests)r]
import fmm_bem_relaxed_amd as fb
import near_form_cases as nfc
from oracle import oracle as O
O.build()
mode = sys.argv[1]
out = dict(mode=mode, worst=0.0, runs=[])

def rows(plan, case, mixed, K, extra, evidence):
    R = nfc.case_reference(O, case, mixed, K=K)
    q = max(nfc.near_ratios(plan, R, extra=extra).values())
    out["runs"].append(dict(case=case, mixed=mixed, worst=q, ran=bool(evidence(plan.stats()))))
    out["worst"] = max(out["worst"], q)

if mode == "batch":
    out["bitwise"], out["widths"] = True, []
    for case in (101, 102, 107):
        plan = nfc.make_plan(fb, case, False)
        out["widths"].append(plan.batch_width())
        R = nfc.case_reference(O, case, False)
        X = np.random.default_rng(case).standard_normal((9, plan.n))
        single = np.stack([plan.execute(x) for x in X])
        s = np.abs(X).astype(np.longdouble) @ np.abs(nfc.dense_near(R["o"])[0]).T
        bound = 2.0 * R["m"] * nfc.U53 * s.astype(np.float64)
        for k in range(1, 10):
            got = plan.execute_batch(X[:k])
            for j in range(k):
                out["bitwise"] = out["bitwise"] and bool(np.array_equal(got[j], single[j]))
                out["worst"] = max(out["worst"], float((np.abs(got[j] - single[j]) / bound[j]).max()))
elif mode == "f32":
    for case in (101, 102, 107, 201, 203):
        for mixed in (False, True):
            local = case in nfc.NO_FAR_FIELD               # no far field: the LOCAL evaluator keeps the option
            plan = nfc.make_plan(fb, case, mixed, near_f32_max_p=4, evaluator="local" if local else "fmm")
            rows(plan, case, mixed, None, nfc.EPS_F32, lambda st: st["last_near_f32"] == 1 and st["near_f32_bytes"] > 0)
elif mode == "hybrid":
    for case in (101, 102, 107, 201, 203):
        for mixed in (False, True):
            plan = nfc.make_plan(fb, case, mixed, near_stream_fraction=0.5)
            rows(plan, case, mixed, None, 0.0, lambda st: st["near_recomputed_pairs"] > 0)
print("RESULT " + json.dumps(out))
"""


def _child(tmp_path, mode, env):
    script = tmp_path / "near_forms_child.py"
    script.write_text(_CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, str(script), mode], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0][len("RESULT "):])
    print("%s %s: worst row / bound %.3g" % (mode, env, out["worst"]))
    return out


@pytest.mark.parametrize("env,width", [({"FMMBEM_BATCH_NV": "2"}, 2), ({"FMMBEM_BATCH_NV": "8"}, 8),
                                       ({"FMMBEM_BATCH_SHAPE": "1"}, 4), ({"FMMBEM_BATCH_SHAPE": "2"}, 4)])
def test_batch_shapes_of_a_process(tmp_path, env, width):
    """near_spmv_pipe_multi_kernel<.., 2 / 8> and its 2x8 and 4x4 shapes: k = 1 ... 9 vectors on (101), (102), (107).  The shape
    does not change the order of a row's additions (module docstring): every vector is bit for bit its single execute.  The
    child also reports |batch - single|_i over 2 m_i 2^-53 (|A||x|)_i, 0 when the bits agree."""
    out = _child(tmp_path, "batch", env)
    assert out["widths"] == [width] * 3, out
    assert out["bitwise"] and out["worst"] == 0.0, out


@pytest.mark.parametrize("shape", [0, 1, 2, 3])
def test_float_shapes_of_a_process(tmp_path, shape):
    """near_spmv_pipe_f32_kernel and near_spmv_sym3_f32_kernel, the four shapes of each, under the near-only row bound"""
    out = _child(tmp_path, "f32", {"FMMBEM_F32_SHAPE": str(shape)})
    assert len(out["runs"]) == 10 and all(r["ran"] for r in out["runs"]), out
    assert out["worst"] <= 1.0, out


def test_hybrid_grids_of_a_process(tmp_path):
    """one workgroup per CU of each kernel of the hybrid pass instead of 3 + 1 (Laplace) and 2 + 2 (Stokes)"""
    out = _child(tmp_path, "hybrid", {"FMMBEM_HYB_WG_STREAM": "1", "FMMBEM_HYB_WG_RECOMPUTE": "1"})
    assert len(out["runs"]) == 10 and all(r["ran"] for r in out["runs"]), out
    assert out["worst"] <= 1.0, out
