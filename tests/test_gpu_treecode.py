"""The treecode evaluator on the GPU (FMMBEM_EVAL_TREECODE, `-eval TREE`): near field + M2P of every long-range pair at the bodies
of its target box (EvalInteractionLazySparse<Context, false>, kernel/LaplaceSphericalBEM.hpp:395-422).

The CPU oracle has no treecode, so the reference is COMPOSED from oracle pieces (compose_treecode below; no product code in it):
the oracle's near field, its multipoles M of the upward pass at order p, its M2L pair list, its box ranges and permutation, its
cart2sph and evalLocal.  Composed treecode against the oracle's own FMM matvec, relative L2, measured on the CPU:

    case         panels  settings            flags       M2L pairs                              p=4     p=8     p=12    p=16
    two_r3       256     ncrit 16, th 0.5    i % 3 == 0  638, 56 with an inner target box       3.1e-4  1.4e-5  1.2e-6  9.8e-8
    r4_ncrit8    512     ncrit 8                         4 688, 840 onto inner boxes            2.7e-4  5.9e-6  3.3e-7  1.7e-8
    r2_ncrit1    32      ncrit 1                         608                                                    6.6e-7  1.4e-8
    three_balls  1 536   ncrit 600           i % 2       2, onto a level-3 and a level-1 leaf           4.7e-8          1.1e-9

Bounds against the composed reference are the project's own (tests/test_gpu_target_plan_oracle.py::check): per flag class
relative L2 <= 1e-12 and every row within 1e-11 of the class's max |y|.  Against the FMM plan at p = 16: 1e-6, ten times the
oracle's own figures above -- it catches a wrong sign or slot that a shared mistake in the composition would hide."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def check(y, yo, flags, what, rel_tol=1e-12, row_tol=1e-11):
    """the bounds of tests/test_gpu_target_plan_oracle.py::check, per flag class (restated: that one also keeps a record of its own)"""
    assert y.shape == yo.shape and np.all(np.isfinite(y)), what
    for f in (0, 1):
        s = flags == f
        if not s.any():
            continue
        err = np.abs(y[s] - yo[s])
        scale = np.max(np.abs(yo[s]))
        rel = float(np.linalg.norm(y[s] - yo[s]) / np.linalg.norm(yo[s]))
        assert rel <= rel_tol, (what, f, rel)
        worst_row = int(np.argmax(err))
        assert err[worst_row] <= row_tol * scale, (what, f, worst_row, float(err[worst_row]), float(scale))


def two_spheres(rec, dist):
    a = O.unit_sphere(rec)
    return np.concatenate([a, O.unit_sphere(rec, center=(dist, 0.0, 0.0))])


def three_balls():
    s = O.unit_sphere(4) * 0.2
    return np.concatenate([s + np.array(c)[None, None, :] for c in ((0.0, 0.0, 0.0), (1.5, 0.0, 0.0), (12.0, 0.0, 0.0))])


def make_case(name):
    if name == "two_r3":
        v = two_spheres(3, 3.0)
        return dict(v=v, bc=(np.arange(len(v)) % 3 == 0).astype(np.uint8), ncrit=16, theta=0.5)
    if name == "r4_ncrit8":
        v = O.unit_sphere(4)
        return dict(v=v, bc=np.zeros(len(v), dtype=np.uint8), ncrit=8, theta=0.5)
    if name == "r2_ncrit1":
        v = O.unit_sphere(2)
        return dict(v=v, bc=np.zeros(len(v), dtype=np.uint8), ncrit=1, theta=0.5)
    if name == "three_balls":
        v = three_balls()
        return dict(v=v, bc=(np.arange(len(v)) % 2).astype(np.uint8), ncrit=600, theta=0.5)
    if name == "no_far":
        v = O.unit_sphere(2)
        return dict(v=v, bc=np.zeros(len(v), dtype=np.uint8), ncrit=64, theta=0.5)
    raise KeyError(name)


# case -> the order it is checked at: the five cases cover 4, 8, 12, 13 and 16 (every order on two_r3 below)
ORDER = {"two_r3": 13, "r4_ncrit8": 4, "r2_ncrit1": 12, "three_balls": 16, "no_far": 8}


def compose_treecode(orc, x, p):
    """y_i = (A_near x)_i + sum over long-range pairs (s, t) with i under t of M2P(M_s, c_s, centroid_i)"""
    orc.matvec(x, p)
    M = orc.expansions(p, "M")                                        # [boxes, 2, S]
    bx, perm, cen = orc.boxes(), orc.perm(), orc.panels()["center"]
    T = O.Tables(p)
    y = orc.near_only(x).copy()
    n_of = np.concatenate([np.full(n + 1, n) for n in range(p)])      # stored index -> n, m
    m_of = np.concatenate([np.arange(n + 1) for n in range(p)])
    full = n_of * n_of + n_of + m_of                                  # ... -> index n^2 + n + m of evalLocal's Ynm
    w = np.where(m_of == 0, 1.0, 2.0)
    for s, t in orc.pairs("m2l"):
        for pos in range(bx["bb"][t], bx["be"][t]):
            i = perm[pos]
            r, th, ph = O.cart2sph(cen[i] - bx["center"][s])
            Y, _ = T.eval_local(r, th, ph)
            acc = (w[None, :] * (M[s] * Y[full][None, :]).real).sum(axis=1)
            y[i] += acc[0] if orc.bc[i] == 0 else -acc[1]
    return y


class Fixture:
    def __init__(self, fb, name, evaluator="TREECODE", sparse_local=True):
        self.name = name
        self.c = make_case(name)
        self.opts = fb.FMMOptions()
        self.opts.set_mac_theta(self.c["theta"])
        self.opts.set_max_per_box(self.c["ncrit"])
        self.opts.sparse_local = sparse_local
        self.opts.evaluator = evaluator
        self.K = fb.LaplaceSphericalBEM(ORDER[name], 3)
        self.plan = fb.FMM_plan(self.K, self.c["v"], self.opts, bc=self.c["bc"], p_max=16)
        self.x = np.random.default_rng(len(name)).standard_normal(len(self.c["v"]))

    def run(self, p, x=None):
        self.K.set_p(p)
        return self.plan.execute(self.x if x is None else x)


class Store:
    """plans and composed references, built once per module and shared"""

    def __init__(self, fb):
        self.fb = fb
        self.fix, self.orc, self.refs = {}, {}, {}

    def get(self, name, evaluator="TREECODE", sparse_local=True):
        key = (name, evaluator, sparse_local)
        if key not in self.fix:
            self.fix[key] = Fixture(self.fb, name, evaluator, sparse_local)
        return self.fix[key]

    def oracle(self, name):
        if name not in self.orc:
            c = make_case(name)
            self.orc[name] = O.Oracle(c["v"], bc=c["bc"], K=3, theta=c["theta"], ncrit=c["ncrit"])
        return self.orc[name]

    def ref(self, name, p, x=None, tag=None):
        F = self.get(name)
        key = (name, p, tag)
        if key not in self.refs:
            self.refs[key] = compose_treecode(self.oracle(name), F.x if x is None else x, p)
        return self.refs[key]


@pytest.fixture(scope="module")
def store(fb):
    return Store(fb)


# ---- 1. equals the composed reference ----
@pytest.mark.parametrize("name", ["two_r3", "r4_ncrit8", "r2_ncrit1", "three_balls", "no_far"])
def test_case_equals_composed_reference(store, name):
    F = store.get(name)
    p = ORDER[name]
    st = F.plan.stats()
    pairs = store.oracle(name).pairs("m2l")
    assert st["m2l_pairs"] == len(pairs)
    if name == "no_far":
        assert st["m2l_pairs"] == 0
    check(F.run(p), store.ref(name, p), F.c["bc"], (name, p))
    x2 = np.random.default_rng(99).standard_normal(len(F.x))          # a second vector on the same plan
    check(F.run(p, x2), store.ref(name, p, x2, "second"), F.c["bc"], (name, p, "second vector"))


def test_case_shapes(store):
    """the cases hold what they are chosen for: inner target boxes, one-row leaves, leaves of more than 64 rows"""
    bx = store.oracle("two_r3").boxes()
    assert np.any(bx["leaf"][store.oracle("two_r3").pairs("m2l")[:, 1]] == 0)
    bx = store.oracle("r2_ncrit1").boxes()
    assert np.all((bx["be"] - bx["bb"])[bx["leaf"] != 0] == 1)
    bx = store.oracle("three_balls").boxes()
    rows = np.sort((bx["be"] - bx["bb"])[bx["leaf"] != 0])
    assert rows.tolist() == [440, 512, 584]
    assert len(store.oracle("three_balls").pairs("m2l")) == 2


def test_every_order_on_one_plan(store):
    F = store.get("two_r3")
    for p in range(1, 17):
        check(F.run(p), store.ref("two_r3", p), F.c["bc"], ("order", p))


def test_relaxed_sequence(store):
    F = store.get("two_r3")
    for p in (16, 3, 1, 12, 13):
        check(F.run(p), store.ref("two_r3", p), F.c["bc"], ("relaxed", p))


def test_matrix_free_near_field(store):
    F = store.get("two_r3", sparse_local=False)
    for p in (5, 13):
        check(F.run(p), store.ref("two_r3", p), F.c["bc"], ("sparse_local = 0", p))


# ---- 2. M, the permutation and the lists are the FMM plan's ----
@pytest.mark.parametrize("name", ["two_r3", "r4_ncrit8"])
def test_multipoles_and_lists_are_the_fmm_plans(store, name):
    T, F = store.get(name), store.get(name, evaluator="FMM")
    for p in (7, 10, 14):
        T.run(p)
        F.run(p)
        assert np.array_equal(T.plan.expansions("M", p), F.plan.expansions("M", p)), p
    assert np.array_equal(T.plan.perm(), F.plan.perm())
    for which in ("p2p", "m2l", "m2m"):
        assert np.array_equal(T.plan.pairs(which), F.plan.pairs(which)), which
    with pytest.raises(store.fb.FmmBemError) as e:
        T.plan.expansions("L", 7)
    assert e.value.status == 6


# ---- 3. against the FMM plan ----
@pytest.mark.parametrize("name", ["two_r3", "r4_ncrit8", "r2_ncrit1"])
def test_against_the_fmm_plan(store, name):
    T, F = store.get(name), store.get(name, evaluator="FMM")
    yt, yf = T.run(16), F.run(16)
    rel = float(np.linalg.norm(yt - yf) / np.linalg.norm(yf))
    print("\n%s p = 16: treecode vs FMM plan, relative L2 %.2e" % (name, rel))
    assert rel <= 1e-6, (name, rel)
    assert rel > 0                                                    # two evaluators, not one


# ---- 4. the same bits ----
def test_two_executes_agree(store):
    F = store.get("r4_ncrit8")
    for p in (4, 10, 14):
        assert np.array_equal(F.run(p), F.run(p)), p


def test_graph_replays(store):
    F = store.get("two_r3")
    p = 11
    plain = F.run(p)
    x2 = -0.5 * F.x + 1.0
    plain2 = F.run(p, x2)
    F.plan.set_graphs(True)
    try:
        for rep in range(3):
            assert np.array_equal(F.run(p), plain), rep
            assert np.array_equal(F.run(p, x2), plain2), rep
    finally:
        F.plan.set_graphs(False)
    check(plain, store.ref("two_r3", p), F.c["bc"], "graph")


@pytest.mark.parametrize("sparse_local", [True, False])
def test_execute_batch(store, sparse_local):
    F = store.get("two_r3", sparse_local=sparse_local)
    p = 12
    F.K.set_p(p)
    X = np.random.default_rng(5).standard_normal((5, len(F.x)))
    X[0] = F.x
    X[3] *= 1e3
    X[4] = 0.0
    single = [F.plan.execute(X[j]) for j in range(5)]
    check(single[0], store.ref("two_r3", p), F.c["bc"], "batch row 0")
    for k in (1, 2, 3, 5):
        Y = F.plan.execute_batch(X[:k])
        for j in range(k):
            assert np.array_equal(Y[j], single[j]), ("batch vs execute", k, j)
        if k == 5:
            assert np.all(Y[4] == 0)


def test_execute_torch_on_a_side_stream(store):
    import torch
    F = store.get("r4_ncrit8")
    p = 9
    host = F.run(p)
    xd = torch.from_numpy(F.x).to("cuda:0")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        y = F.plan.execute_torch(xd)
    s.synchronize()
    assert np.array_equal(y.cpu().numpy(), host)


# ---- 5. no far field ----
def test_no_far_pair_gives_exactly_the_near_field(store):
    import torch
    F = store.get("no_far")
    assert F.plan.stats()["m2l_pairs"] == 0
    xd = torch.from_numpy(F.x).to("cuda:0")
    near = torch.empty_like(xd)
    F.plan.near_device(xd.data_ptr(), near.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for p in (3, 8, 13):
        assert np.array_equal(F.run(p), near.cpu().numpy()), p


# ---- 6. solver and drivers ----
def test_gmres_capi_on_a_treecode_plan(fb):
    import torch
    v = fb.unit_sphere(4)
    n = len(v)
    opts = fb.FMMOptions()
    opts.evaluator = "TREECODE"
    K = fb.LaplaceSphericalBEM(12, 3)
    plan = fb.FMM_plan(K, v, opts, bc=np.zeros(n, dtype=np.uint8), p_max=12)
    rhs = plan.like(np.ones(n, dtype=np.uint8), K=fb.LaplaceSphericalBEM(12, 3))     # the drivers' right-hand-side plan
    assert rhs.stats()["geometry_shared"] >= 2
    dev = torch.device("cuda", 0)
    b = rhs.execute_torch(torch.ones(n, dtype=torch.float64, device=dev))
    so = fb.SolverOptions()
    so.residual, so.variable_p, so.max_p = 1e-6, False, 12
    so.max_iters = so.restart = 200
    x, it, res, _ = fb.gmres_capi(plan, torch.zeros(n, dtype=torch.float64, device=dev), b, so)
    assert 0 < it < 200 and res <= 1e-6, (it, res)
    r = plan.execute_torch(x) - b                                     # the reported residual is the operator's
    assert float(r.norm() / b.norm()) <= 1e-5
    assert plan.stats()["m2l_kernel"] == 4


def _driver_error(flag):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "LaplaceBEM.py"), "-recursions", "4", "-p", "12", "-fixed_p",
                        "-eval", flag], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"relative error: ([0-9.eE+-]+)", r.stdout)
    assert m, r.stdout[-2000:]
    return float(m.group(1))


def test_driver_eval_tree():
    """the operators differ by about 1e-6 and the discretisation error is about 1e-2: a larger gap means a bug"""
    tree, fmm = _driver_error("TREE"), _driver_error("FMM")
    print("\nLaplaceBEM.py -recursions 4 -p 12 -fixed_p: relative error TREE %.4e, FMM %.4e" % (tree, fmm))
    assert abs(tree - fmm) <= 0.1 * fmm, (tree, fmm)


# ---- 7. stats ----
def test_stats_after_a_timed_execute(store):
    F = store.get("r4_ncrit8")
    F.plan.set_timing(True)
    try:
        F.run(10)
        F.run(10)
        st = F.plan.stats()
    finally:
        F.plan.set_timing(False)
    assert st["m2l_kernel"] == 4 and st["last_p"] == 10
    assert st["ms_m2l"] > 0 and st["ms_near"] > 0 and st["ms_p2m"] > 0
    assert st["ms_l2l"] == 0 and st["ms_l2p"] == 0 and st["ms_mh"] == 0
    fm = store.get("r4_ncrit8", evaluator="FMM").plan.stats()
    for k in ("p2p_pairs", "m2l_pairs", "m2m_ops", "l2l_ops", "p2m_leaves", "l2p_leaves", "near_nnz"):
        assert st[k] == fm[k], k
