"""The flow execute (fmmbem_plan_execute_flow, FMM_plan.execute_flow): velocity, pressure and velocity gradient of a Stokes field
plan from one gather, one P2M and one far chain, the pressure's and the gradient's near pairs in ONE kernel.  Its contract is
equality of bits with the three single executes, so that is what is tested, on the small cases of the pressure's and the gradient's
own tests (field_pressure_reference.CASES; all points VELOCITY targets):
  two_r3      both regimes among the near pairs, ten coincident targets (the per-point buffers are live)
  r4_ncrit8   targets exactly on centroids (self pairs add 0), batches that end inside runs
  big_leaves  target leaves of more than 64 rows, runs longer than one 64-panel batch
  one_row     one-row leaves
  far_only    no near pair: zeros stored to both buffers
  no_far      no M2L pair
1 equality at p = 1, 2, 8, 12, 13, 16 (the gradient's far half not launched, its first order, an unrolled order, the last unrolled
  order, the first run-time order, p_max), every subset of outputs, the torch form, a second vector and a relaxed sequence of orders
2 q and G of the flow execute against the composed references of the pressure and of the gradient at p = 12, relative L2 <= 1e-12,
  the bound test_gpu_field_quantities.py holds these kernels to on this case
3 the neighbours keep their bits around flow executes, graphs on and off; two fresh plans that meet the flow execute and the single
  executes in opposite orders agree call by call
4 the stage times of a timed flow execute    5 which near kernel ran (fmmbem_stats.last_near_f32: 2 the one kernel for q and G)"""
import itertools

import numpy as np
import pytest
import torch

import field_pressure_reference as Q
import field_velocity_gradient_reference as V

pytestmark = pytest.mark.gpu

CASES = ("two_r3", "r4_ncrit8", "big_leaves", "one_row", "far_only", "no_far")
ORDERS = (1, 2, 8, 12, 13, 16)
SUBSETS = [s for s in itertools.product((False, True), repeat=3) if any(s)]       # (velocity, pressure, velocity_gradient)

_PLANS = {}


def fresh(fb, name):
    ref = Q.reference(name)
    K, plan = Q.host_plan(fb, ref.v, ref.pts, ref.c["ncrit"], p_max=16, host_only=False)
    return ref, K, plan


def get(fb, name):
    if name not in _PLANS:
        _PLANS[name] = fresh(fb, name)
    return _PLANS[name]


def singles(K, plan, x, p):
    K.set_p(p)
    return plan.execute(x), plan.execute_pressure(x), plan.execute_velocity_gradient(x)


def same(got, want, what):
    for name, a, b in zip(("u", "q", "G"), got, want):
        assert a.shape == b.shape and np.array_equal(a, b), (what, name, float(np.abs(a - b).max()))


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_flow_equals_the_single_executes(fb, name):
    ref, K, plan = get(fb, name)
    x = ref.vector("x")
    xd = torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).to("cuda:0")
    n = len(ref.pts)
    for p in ORDERS:
        want = singles(K, plan, x, p)
        assert want[0].shape == (n, 3) and want[1].shape == (n,) and want[2].shape == (n, 3, 3)
        got = plan.execute_flow(x)
        same(got, want, (name, p, "all"))
        for sub in SUBSETS:
            out = plan.execute_flow(x, *sub)
            for k in range(3):
                assert (out[k] is None) == (not sub[k]), (name, p, sub)
            same([o for o in out if o is not None], [w for w, s in zip(want, sub) if s], (name, p, sub))
        assert np.array_equal(plan.execute_flow(x.reshape(-1))[2], want[2])           # (3N,) as (N, 3)
        for sub in ((True, True, True), (False, True, True), (True, False, False), (False, False, True)):
            out = plan.execute_flow_torch(xd, *sub)
            same([o.cpu().numpy() for o in out if o is not None], [w for w, s in zip(want, sub) if s], (name, p, sub, "torch"))
        assert np.array_equal(plan.execute_flow_torch(xd, p=p)[1].cpu().numpy(), want[1])
    if name == "two_r3":                                      # the ten copies: equal values, and not their neighbour's
        K.set_p(8)
        u, q, g = plan.execute_flow(x)
        copies = np.arange(n - 10, n)
        assert np.all(g[copies] == g[copies[0]]) and np.all(q[copies] == q[copies[0]]) and np.all(u[copies] == u[copies[0]])
        assert np.all(g[copies[0]] != g[copies[0] - 1]) and q[copies[0]] != q[copies[0] - 1]


def test_second_vector_and_relaxed_orders_equal_fresh_plans(fb):
    ref, K, plan = get(fb, "two_r3")
    for p, key in ((16, "x"), (4, "x2"), (10, "x")):
        K.set_p(p)
        got = plan.execute_flow(ref.vector(key))
        _, K2, other = fresh(fb, "two_r3")
        K2.set_p(p)
        same(got, other.execute_flow(ref.vector(key)), (p, key, "fresh flow"))
        _, K3, third = fresh(fb, "two_r3")
        same(got, singles(K3, third, ref.vector(key), p), (p, key, "fresh singles"))


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
def test_flow_meets_the_composed_references(fb):
    ref, K, plan = get(fb, "two_r3")
    x = ref.vector("x")
    assert np.array_equal(V.reference("two_r3").vector("x"), x)
    K.set_p(12)
    want = {"pressure": ref.pressure(12), "velocity_gradient": V.reference("two_r3").gradient(12)}
    for sub in ((False, True, True), (True, True, True)):
        _, q, g = plan.execute_flow(x, *sub)
        for what, got in (("pressure", q), ("velocity_gradient", g)):
            rel = float(np.linalg.norm(got - want[what]) / np.linalg.norm(want[what]))
            print("flow%r, %s at p = 12: rel L2 %.2e" % (sub, what, rel))
            assert rel <= 1e-12, (sub, what, rel)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
def test_neighbours_keep_their_bits(fb):
    ref, K, plan = fresh(fb, "two_r3")
    p = 10
    x, xb = ref.vector("x"), np.stack([ref.x, ref.x2])
    K.set_p(p)
    y0, yb0, q0, g0, s0 = plan.execute(x), plan.execute_batch(xb), plan.execute_pressure(x), plan.execute_velocity_gradient(x), plan.execute_stress(x)
    assert np.array_equal(s0, -q0[:, None, None] * np.eye(3)[None] + K.Mu * (g0 + g0.transpose(0, 2, 1)))

    def others_unchanged(what):
        K.set_p(p)
        assert np.array_equal(plan.execute(x), y0), what
        assert np.array_equal(plan.execute_batch(xb), yb0), what
        assert np.array_equal(plan.execute_pressure(x), q0), what
        assert np.array_equal(plan.execute_velocity_gradient(x), g0), what
        assert np.array_equal(plan.execute_stress(x), s0), what

    def flows(what):
        K.set_p(p)
        same(plan.execute_flow(x), (y0, q0, g0), what)
        K.set_p(7)
        a, b = plan.execute_flow(ref.x2), plan.execute_flow(ref.x2, velocity=False)      # another order and vector in between
        same(a[1:], b[1:], what)
        K.set_p(p)
        same(plan.execute_flow(x, pressure=False)[::2], (y0, g0), what)

    others_unchanged("before")
    flows("graphs off")
    others_unchanged("graphs off")
    plan.set_graphs(True)
    try:
        for rep in range(3):
            others_unchanged(("graphs on", rep))
            flows(("graphs on", rep))
        others_unchanged("graphs on, after")
    finally:
        plan.set_graphs(False)
    others_unchanged("graphs off again")
    flows("graphs off again")


def record(fb, flow_first):
    """A fresh plan of two_r3 that meets the flow execute before or after the single executes; every result by name"""
    ref, K, plan = fresh(fb, "two_r3")
    x = ref.vector("x")
    calls = {"flow": lambda: plan.execute_flow(x), "flow_qg": lambda: plan.execute_flow(x, velocity=False)[1:],
             "pressure": lambda: (plan.execute_pressure(x),), "velocity_gradient": lambda: (plan.execute_velocity_gradient(x),),
             "velocity": lambda: (plan.execute(x),)}
    rec = {}
    K.set_p(8)
    first = ("flow", "pressure", "velocity_gradient", "velocity") if flow_first else ("velocity_gradient", "velocity", "pressure", "flow")
    for name in first:                                        # allocation order
        rec["first", name] = calls[name]()
    for sweep in range(2):
        for p in (2, 12, 13):
            K.set_p(p)
            for k, name in enumerate(("pressure", "flow_qg", "velocity_gradient", "velocity", "flow", "pressure")):
                out = calls[name]()
                if (p, name) in rec:
                    same(out, rec[p, name], (flow_first, sweep, p, k, name))
                rec[p, name] = out
    return rec


def test_flow_and_singles_interleaved_on_two_plans(fb):
    a, b = record(fb, True), record(fb, False)
    assert a.keys() == b.keys()
    for key in a:
        same(a[key], b[key], key)
    for p in (2, 12, 13):                                     # and the flow execute is the singles on either
        same(a[p, "flow"], a[p, "velocity"] + a[p, "pressure"] + a[p, "velocity_gradient"], p)
        same(a[p, "flow_qg"], a[p, "pressure"] + a[p, "velocity_gradient"], p)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
def test_timed_flow_execute_is_one_execute(fb):
    ref, K, plan = get(fb, "r4_ncrit8")
    x = ref.vector("x")
    K.set_p(8)
    want = plan.execute_flow(x)
    plan.set_timing(True)
    try:
        got = plan.execute_flow(x)
        st = plan.stats()
    finally:
        plan.set_timing(False)
    assert st["timed_executes"] == 1 and st["last_p"] == 8
    assert st["ms_near"] > 0 and st["ms_l2p"] > 0 and st["ms_m2l"] > 0 and st["ms_total"] >= st["ms_near"]
    same(got, want, "timed")
    same(plan.execute_flow(x), want, "after timing")


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
def test_which_near_kernel_ran(fb):
    """fmmbem_stats.last_near_f32 after a flow execute: 2 the one near kernel for q and G, 3 a single quantity's kernel, 0 neither;
    an execute sets it back"""
    ref, K, plan = get(fb, "two_r3")
    x = ref.vector("x")
    K.set_p(8)
    for sub, code in (((True, True, True), 2), ((False, True, True), 2), ((True, True, False), 3), ((False, False, True), 3),
                      ((True, False, False), 0)):
        plan.execute(x)
        assert plan.stats()["last_near_f32"] == 0
        plan.execute_flow(x, *sub)
        assert plan.stats()["last_near_f32"] == code, sub
    plan.execute_stress(x)                                    # the stress takes the one kernel
    assert plan.stats()["last_near_f32"] == 2
    plan.execute_pressure(x)                                  # a single field execute leaves the record alone
    assert plan.stats()["last_near_f32"] == 2
