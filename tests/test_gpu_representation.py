"""The representation execute on the GPU (fmmbem_plan_execute_representation, FMM_plan.execute_representation): phi = S[sigma] -
D[mu] and its gradient at the points of a Laplace target plan from one gather, one far chain on the two layers FOLDED into one
multipole set, and one kernel over the near pairs; the points' own flags ignored.  The shapes are those of
tests/field_gradient_reference.py (K = 3, theta = 0.5; x the density sigma, x2 the surface potential mu, independent seeds).

The bounds (those of tests/test_gpu_target_plan_oracle.py::check, with the scale the contract names): an output is within 1e-12
relative L2 of the reference S - D, MEASURED AGAINST |S part| + |D part| so that cancellation of the two layers can neither hide nor
fake an error, and every row within 1e-11 of the larger of the two parts' largest entries.

1 against the four existing executes (execute and execute_gradient on an all-0 and an all-1 plan over the same points): every case,
  p = 1, 2, 8, 12, 13, 16 spread over them, every order 1..16 on two_r3; awkward's on-axis rows within 10 x ON_AXIS_DEVIATION
2 against references with no product code: TargetOracle.matvec and the composed gradient with the flags all 0 / all 1
3 the flags do not enter: the mixed-flag plan gives the all-0 plan's result; coincident copies of both flags receive equal rows
4 the nine combinations of null inputs and outputs against the full call
5 quad_k = 13, where a batch of the near kernel holds fewer than 64 panels
6 bits and state: repeats, a side stream, a relaxed sequence against fresh plans, the neighbours around it with graphs on and off,
  the torch form, the stage times, a plan whose own targets are all flag 1
7 the driver's -field_one_pass"""
import os
import subprocess
import sys

import numpy as np
import pytest

import double_layer_reference as D
import field_gradient_reference as G
import field_representation_reference as RR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# case -> the orders it is checked at: 1 (the gradient's chain has one term), 2, an unrolled order, the last unrolled order, the first
# run-time order, p_max
ORDERS = {"two_r3": (13,), "r4_ncrit8": (2, 12), "big_leaves": (16,), "one_row": (1, 12), "far_only": (8,), "no_far": (8,), "awkward": (12, 13)}
WORST = {}


def options(fb, ncrit):
    opts = fb.FMMOptions()
    opts.set_mac_theta(G.THETA)
    opts.set_max_per_box(ncrit)
    return opts


class Fixture:
    """A case's all-0 plan (the representation execute runs on it) and all-1 plan, which give the four single executes"""

    def __init__(self, fb, name, quad_k=G.K):
        self.fb, self.name = fb, name
        self.R = R = G.reference(name)
        self.sigma, self.mu = R.x, R.x2
        self.K = fb.LaplaceSphericalBEM(8, quad_k)
        m = len(R.pts)
        self.zero = self.plan_with(np.zeros(m, np.uint8))
        self.one = self.plan_with(np.ones(m, np.uint8))

    def plan_with(self, flags):
        return self.fb.FMM_plan(self.K, self.R.v, options(self.fb, self.R.c["ncrit"]), p_max=16, targets=self.R.pts, target_bc=flags)

    def four(self, p):
        """dict(S, D, gS, gD): the four single executes at order p"""
        self.K.set_p(p)
        return dict(S=self.zero.execute(self.sigma), D=self.one.execute(self.mu), gS=self.zero.execute_gradient(self.sigma),
                    gD=self.one.execute_gradient(self.mu))

    def run(self, p, plan=None, **kw):
        self.K.set_p(p)
        return (plan or self.zero).execute_representation(self.sigma, self.mu, **kw)


_FIX = {}


def get(fb, name):
    if name not in _FIX:
        _FIX[name] = Fixture(fb, name)
    return _FIX[name]


def check_one(got, ref, s_part, d_part, what, exempt=None):
    """got against ref: relative L2 <= 1e-12 of |s_part| + |d_part|, rows within 1e-11 of the two parts' largest entry"""
    assert got.shape == ref.shape and np.all(np.isfinite(got)), what
    keep = np.ones(len(ref), bool) if exempt is None else ~exempt
    scale_l2 = np.linalg.norm(s_part[keep]) + np.linalg.norm(d_part[keep])
    top = max(np.abs(s_part).max(), np.abs(d_part).max())
    rel = float(np.linalg.norm(got[keep] - ref[keep]) / scale_l2)
    row = float(np.abs(got[keep] - ref[keep]).max() / top)
    WORST[what[0]] = max(WORST.get(what[0], 0.0), rel)
    print("%s: rel L2 %.2e of the two layers' norms, worst row %.2e of the largest entry" % (what, rel, row))
    assert rel <= 1e-12, (what, rel)
    assert row <= 1e-11, (what, row)


def check(got, parts, what, exempt=None):
    """(phi, grad) against S - D and gS - gD of parts"""
    phi, grad = got
    check_one(phi, parts["S"] - parts["D"], parts["S"], parts["D"], ("phi",) + tuple(what), exempt)
    check_one(grad, parts["gS"] - parts["gD"], parts["gS"], parts["gD"], ("grad",) + tuple(what), exempt)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in G.CASES if n != "awkward"])
def test_equals_the_four_executes(fb, name):
    F = get(fb, name)
    for p in ORDERS[name]:
        phi, grad = F.run(p)
        assert phi.shape == (len(F.R.pts),) and grad.shape == (len(F.R.pts), 3)
        check((phi, grad), F.four(p), (name, p))
    if name == "big_leaves":
        tb = F.zero.target_boxes()
        assert (tb["be"] - tb["bb"])[tb["leaf"] != 0].max() > 64
    if name == "far_only":                                  # no near pair: the near kernel stores zeros, the result is the fold's
        st = F.zero.stats()
        assert st["p2p_pairs"] == 0 and st["m2l_pairs"] >= 1
    if name == "no_far":                                    # no M2L: the near sums, the same bits at every order
        assert F.zero.stats()["m2l_pairs"] == 0
        phi8, grad8 = F.run(8)
        for p2 in (3, 13):
            phi, grad = F.run(p2)
            assert np.array_equal(phi, phi8) and np.array_equal(grad, grad8), p2


def test_every_order_on_one_plan(fb):
    F = get(fb, "two_r3")
    for p in range(1, 17):
        check(F.run(p), F.four(p), ("order", p))


@pytest.mark.parametrize("p", ORDERS["awkward"])
def test_targets_on_the_axis_of_their_leaf(fb, p):
    """The 16 added rows (a leaf's centre and 0.3 side above it) within 10 x ON_AXIS_DEVIATION of the scale, as the gradient's own
    test has them; every other row keeps the bounds"""
    F = get(fb, "awkward")
    exempt = np.zeros(len(F.R.pts), bool)
    exempt[-G.N_AWKWARD:] = True
    got, parts = F.run(p), F.four(p)
    check(got, parts, ("awkward, the other rows", p), exempt=exempt)
    for out, s_part, d_part in ((got[0], parts["S"], parts["D"]), (got[1], parts["gS"], parts["gD"])):
        top = max(np.abs(s_part).max(), np.abs(d_part).max())
        err = np.abs(out[exempt] - (s_part - d_part)[exempt]).max()
        print("awkward rows p = %d: %.3e of the scale" % (p, float(err / top)))
        assert np.all(np.isfinite(out[exempt])) and err <= 10 * D.ON_AXIS_DEVIATION * top, (p, float(err / top))


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,p", [("two_r3", 8), ("r4_ncrit8", 12)])
def test_equals_references_without_product_code(fb, name, p):
    F = get(fb, name)
    check(F.run(p), RR.parts(name, p), (name, p, "oracle and composed reference"))


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
def test_flags_do_not_enter(fb):
    F = get(fb, "two_r3")
    R = F.R
    mixed = F.plan_with(R.flags)
    p = 12
    want = F.four(p)
    phi, grad = F.run(p, plan=mixed)
    check((phi, grad), want, ("mixed flags", p))
    phi0, grad0 = F.run(p)
    check_one(phi, phi0, want["S"], want["D"], ("phi", "mixed against all-0", p))
    check_one(grad, grad0, want["gS"], want["gD"], ("grad", "mixed against all-0", p))
    copies = np.arange(len(R.pts) - 10, len(R.pts))        # ten copies of one point, five per flag: separate bodies, identical bits
    assert set(R.flags[copies].tolist()) == {0, 1}
    for out in (phi, grad):
        assert all(np.array_equal(out[k], out[copies[0]]) for k in copies)
    assert not np.array_equal(grad[copies[0]], grad[copies[0] - 1])
    mixed.close()


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
def test_null_inputs_and_outputs(fb):
    F = get(fb, "two_r3")
    p = 12
    F.K.set_p(p)
    plan, zeros = F.zero, np.zeros(len(F.R.v))
    want = F.four(p)
    no_layer = {k: np.zeros_like(a) for k, a in want.items()}
    for sigma, mu, parts, with_zeros in ((F.sigma, F.mu, want, (F.sigma, F.mu)),
                                         (F.sigma, None, dict(want, D=no_layer["D"], gD=no_layer["gD"]), (F.sigma, zeros)),
                                         (None, F.mu, dict(want, S=no_layer["S"], gS=no_layer["gS"]), (zeros, F.mu))):
        full = plan.execute_representation(sigma, mu)
        check(full, parts, ("layers", sigma is not None, mu is not None))
        filled = plan.execute_representation(*with_zeros)                 # a missing layer is a zero vector
        check_one(full[0], filled[0], parts["S"], parts["D"], ("phi", "against a zero vector"))
        check_one(full[1], filled[1], parts["gS"], parts["gD"], ("grad", "against a zero vector"))
        phi_only = plan.execute_representation(sigma, mu, gradient=False)  # a missing output leaves the other's bits
        grad_only = plan.execute_representation(sigma, mu, value=False)
        assert phi_only[1] is None and grad_only[0] is None
        assert np.array_equal(phi_only[0], full[0]) and np.array_equal(grad_only[1], full[1])


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
def test_quad_k_13(fb):
    """K = 13: 9 + 39 doubles per panel record, 24 panels per batch of the near kernel -- batches that end inside runs"""
    F = Fixture(fb, "r4_ncrit8", quad_k=13)
    check(F.run(8), F.four(8), ("quad_k 13", 8))
    F.zero.close()
    F.one.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
def test_bits_and_neighbours(fb):
    import torch
    F = get(fb, "two_r3")
    R = F.R
    plan = F.plan_with(R.flags)                             # a plan with both slots live: execute reads what the fold wrote over
    p = 10
    F.K.set_p(p)
    X = np.stack([R.x, R.x2, -R.x])
    y0, Y0, g0 = plan.execute(R.x), plan.execute_batch(X), plan.execute_gradient(R.x)
    phi0, grad0 = F.run(p, plan=plan)
    for rep in range(2):                                     # the same bits on every run
        phi, grad = F.run(p, plan=plan)
        assert np.array_equal(phi, phi0) and np.array_equal(grad, grad0)
    assert np.array_equal(plan.execute(R.x), y0) and np.array_equal(plan.execute_batch(X), Y0)
    assert np.array_equal(plan.execute_gradient(R.x), g0)
    plan.set_graphs(True)                                    # launched plainly whatever set_graphs says; the graphs keep their bits
    try:
        for rep in range(3):
            F.K.set_p(p)
            assert np.array_equal(plan.execute(R.x), y0), rep
            phi, grad = F.run(p, plan=plan)
            assert np.array_equal(phi, phi0) and np.array_equal(grad, grad0), rep
            F.run(7, plan=plan)                              # another order in between
            F.K.set_p(p)
            assert np.array_equal(plan.execute_batch(X), Y0) and np.array_equal(plan.execute_gradient(R.x), g0), rep
    finally:
        plan.set_graphs(False)
    F.K.set_p(p)
    assert np.array_equal(plan.execute(R.x), y0)
    # the torch form on a side stream, every subset of outputs and layers that is not empty
    sd, md = (torch.from_numpy(a).to("cuda:0") for a in (F.sigma, F.mu))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        both = plan.execute_representation_torch(sd, md)
        phi_only = plan.execute_representation_torch(sd, md, gradient=False, p=p)
        grad_only = plan.execute_representation_torch(sd, md, value=False)
        double_layer = plan.execute_representation_torch(None, md)
    s.synchronize()
    assert tuple(both[0].shape) == (len(R.pts),) and tuple(both[1].shape) == (len(R.pts), 3)
    assert np.array_equal(both[0].cpu().numpy(), phi0) and np.array_equal(both[1].cpu().numpy(), grad0)
    assert phi_only[1] is None and np.array_equal(phi_only[0].cpu().numpy(), phi0)
    assert grad_only[0] is None and np.array_equal(grad_only[1].cpu().numpy(), grad0)
    want = plan.execute_representation(None, F.mu)
    assert np.array_equal(double_layer[0].cpu().numpy(), want[0]) and np.array_equal(double_layer[1].cpu().numpy(), want[1])
    plan.close()


def test_relaxed_sequence_against_fresh_plans(fb):
    F = get(fb, "two_r3")
    for p in (16, 3, 12, 13):
        got = F.run(p)
        fresh = F.plan_with(np.zeros(len(F.R.pts), np.uint8))
        want = F.run(p, plan=fresh)
        fresh.close()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), p


def test_timed_execute_reports_its_kernels(fb):
    F = get(fb, "r4_ncrit8")
    F.zero.set_timing(True)
    try:
        got = F.run(8)
        st = F.zero.stats()
    finally:
        F.zero.set_timing(False)
    assert st["timed_executes"] == 1 and st["last_p"] == 8
    assert st["ms_near"] > 0 and st["ms_l2p"] > 0 and st["ms_p2m"] > 0 and st["ms_m2l"] > 0 and st["ms_total"] >= st["ms_near"]
    again = F.run(8)
    assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1])


def test_plan_whose_targets_are_all_flag_1(fb):
    """Slot 0 is not live on this plan: its moment table is built at the call, and its far chain runs on a slot the plan never uses"""
    F = get(fb, "two_r3")
    for p in (8, 13):                                        # a rotation order and a double-sum order of M2L
        want = F.four(p)
        y1 = F.one.execute(F.mu)
        check(F.run(p, plan=F.one), want, ("all-1 plan", p))
        assert np.array_equal(F.one.execute(F.mu), y1)


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
def driver(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "LaplaceBEM.py")] + list(args), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.splitlines()


TIMED = ("Flipping BC:", "Creating plan:", "Executing plan:", "\tsetup :", "\tsolve :")      # wall-clock figures: they differ run to run
FIELD = ("field:", "field gradient:")


def test_driver_one_pass():
    args = ["-recursions", "4", "-p", "12", "-fixed_p", "-field", "200", "-field_grad"]
    two_plans, one_pass = driver(*args), driver(*args, "-field_one_pass")
    for head in FIELD:
        a, b = ([ln for ln in out if ln.startswith(head)] for out in (two_plans, one_pass))
        assert len(a) == 1 and len(b) == 1, (head, two_plans, one_pass)
        print(a[0], "|", b[0])
        assert "200 points at r = 3" in b[0]
        for key in ("max error:", "rms error:"):
            ea, eb = (float(ln.split(key)[1].split(",")[0]) for ln in (a[0], b[0]))
            assert abs(ea - eb) <= 1e-3 * ea, (head, key, ea, eb)

    def rest(out):
        return [next((t for t in TIMED if ln.startswith(t)), ln) for ln in out if not ln.startswith(FIELD)]
    assert rest(two_plans) == rest(one_pass)


def test_report_worst_errors():
    print("\nrepresentation execute, worst relative L2: phi %.2e, grad %.2e" % (WORST.get("phi", 0.0), WORST.get("grad", 0.0)))
