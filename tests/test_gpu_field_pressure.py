"""The field pressure on the GPU (fmmbem_plan_execute_pressure) against the composed CPU reference of
tests/field_pressure_reference.py: the near pairs by pi_entry in numpy over the plan's own p2p list, the far half by the oracle's P2M
and translations and the long-double gradients of the local expansions.

1 composed reference: every case at every order 1 .. p_max of its plan, relative L2 <= 1e-12 and every row within 1e-11 of the case's
  scale max_i sum_j |pi_ij| |x_j| (the gradient tests' bounds for the same arithmetic); the rows added on the axis of their leaf
  (awkward) within 1e-9 of the scale; no_far the same bits at every order; far_only exact zeros from the near kernel; a relaxed
  sequence of orders and a second vector on one plan
2 bits: repeats, host and device forms, coincident copies, execute around a pressure execute with graphs on and off, a side stream
3 kernel_pressure_entries against pi_entry in numpy in all three regimes and on a fine-rule point, to 1e-13 of sum_q |w_q A d_q| / |d_q|^3
4 stage times of a timed pressure execute    5 the translating sphere, end to end    6 the driver's -field_pressure line"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import field_gradient_reference as G
import field_plan_reference as R
import field_pressure_reference as Q

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# case -> p_max of its plan.  Every order 1 .. 16 (the twelve unrolled instantiations and the generic kernel) runs on six cases;
# r4_ncrit8 -- the deep tree with the self rule, 4 287 M2L pairs, whose reference costs 3.5 s at p = 16 -- stops at 10.
P_MAX = {"two_r3": 16, "r4_ncrit8": 10, "big_leaves": 16, "one_row": 16, "far_only": 16, "no_far": 16, "awkward": 16}
ON_AXIS = 1e-9                                           # the gradient tests' bound of the rows on the axis of their leaf
WORST = {"rel": 0.0, "row": 0.0, "axis": 0.0}


class Fixture:
    def __init__(self, fb, name):
        self.R = ref = Q.reference(name)
        self.K, self.plan = Q.host_plan(fb, ref.v, ref.pts, ref.c["ncrit"], p_max=P_MAX[name], host_only=False)
        # the reference sums over the host-only plan's lists: they are this plan's
        for which in ("p2p", "m2l", "m2m", "l2l"):
            assert np.array_equal(self.plan.pairs(which), ref.lists[which]), which
        assert np.array_equal(self.plan.target_perm()[0], ref.tree) and np.array_equal(self.plan.perm(), ref.perm)

    def run(self, p, key="x"):
        self.K.set_p(p)
        return self.plan.execute_pressure(self.R.vector(key))


_FIX = {}


def get(fb, name):
    if name not in _FIX:
        _FIX[name] = Fixture(fb, name)
    return _FIX[name]


def check(q, ref, scale, what, exempt=None):
    assert q.shape == ref.shape and q.ndim == 1 and np.all(np.isfinite(q)), what
    s = np.ones(len(q), bool) if exempt is None else ~exempt
    top = float(np.linalg.norm(ref[s]))                      # (far_only at p = 1: the gradient of a constant, reference and result 0)
    rel = float(np.linalg.norm(q[s] - ref[s]) / top) if top > 0 else float(np.any(q[s] != 0))
    row = float(np.abs(q[s] - ref[s]).max() / scale)
    WORST["rel"], WORST["row"] = max(WORST["rel"], rel), max(WORST["row"], row)
    print("%s: rel L2 %.2e, worst row %.2e of the scale" % (what, rel, row))
    assert rel <= 1e-12, (what, rel)
    assert row <= 1e-11, (what, int(np.argmax(np.abs(q - ref) * s)), row)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in Q.CASES if n != "awkward"])
def test_every_order_equals_composed_reference(fb, name):
    F = get(fb, name)
    scale = F.R.scale()
    for p in range(1, P_MAX[name] + 1):
        check(F.run(p), F.R.pressure(p), scale, (name, p))
    if name == "big_leaves":
        tb = F.plan.target_boxes()
        assert (tb["be"] - tb["bb"])[tb["leaf"] != 0].max() > 64
    if name == "no_far":
        assert F.plan.stats()["m2l_pairs"] == 0
        q8 = F.run(8)
        for p2 in (3, 13):                                  # no far field: the near sum, the same bits at every order
            assert np.array_equal(F.run(p2), q8), p2
    if name == "far_only":
        st = F.plan.stats()
        assert st["p2p_pairs"] == 0 and st["m2l_pairs"] >= 1
        # the near kernel stores exact zeros in every row before L2P subtracts: after the executes above, x = 0 leaves nothing but
        # them (a row the near kernel skipped would keep the previous execute's value), and a repeat has the same bits
        assert np.all(F.R.near_half("x") == 0)
        q8 = F.run(8)
        assert np.array_equal(F.run(8), q8)
        F.K.set_p(8)
        assert np.all(F.plan.execute_pressure(np.zeros_like(F.R.x)) == 0)
        assert np.array_equal(F.run(8), q8)


@pytest.mark.parametrize("p", [12, 13])
def test_targets_on_the_axis_of_their_leaf(fb, p):
    """The 16 added rows (a leaf's centre and 0.3 side above it): finite, within 1e-9 of the scale -- what a double-precision
    spherical chain loses there against the singularity-free reference.  Every other row keeps the bounds."""
    F = get(fb, "awkward")
    ref = F.R
    q, want = F.run(p), ref.pressure(p)
    exempt = np.zeros(len(ref.pts), bool)
    exempt[-Q.N_AWKWARD:] = True
    check(q, want, ref.scale(), ("awkward, the other rows", p), exempt=exempt)
    err = float(np.abs(q[exempt] - want[exempt]).max() / ref.scale())
    WORST["axis"] = max(WORST["axis"], err)
    print("awkward rows p = %d: %.3e of the scale" % (p, err))
    assert err <= ON_AXIS, (p, err)


def test_awkward_every_order(fb):
    F = get(fb, "awkward")
    ref = F.R
    exempt = np.zeros(len(ref.pts), bool)
    exempt[-Q.N_AWKWARD:] = True
    for p in range(1, P_MAX["awkward"] + 1):
        q, want = F.run(p), ref.pressure(p)
        check(q, want, ref.scale(), ("awkward", p), exempt=exempt)
        assert np.abs(q[exempt] - want[exempt]).max() <= ON_AXIS * ref.scale(), p


def test_relaxed_sequence_and_second_vector(fb):
    F = get(fb, "two_r3")
    scale2 = F.R.scale("x2")
    for p in (10, 4, 13, 4, 10):
        check(F.run(p), F.R.pressure(p), F.R.scale(), ("relaxed", p))
        check(F.run(p, "x2"), F.R.pressure(p, "x2"), scale2, ("relaxed, second vector", p))


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
def test_bits(fb):
    import torch
    F = get(fb, "two_r3")
    ref, plan = F.R, F.plan
    p = 10
    F.K.set_p(p)
    y0 = plan.execute(ref.x)
    q0 = F.run(p)
    assert q0.shape == (len(ref.pts),)
    assert np.array_equal(F.run(p), q0)
    F.K.set_p(p)
    assert np.array_equal(plan.execute_pressure(ref.x.reshape(-1)), q0)       # (3N,) as (N, 3)
    assert np.array_equal(plan.execute(ref.x), y0)
    # coincident targets receive equal values (the ten copies), and not their neighbour's
    copies = np.arange(len(ref.pts) - 10, len(ref.pts))
    assert np.all(q0[copies] == q0[copies[0]]) and q0[copies[0]] != q0[copies[0] - 1]
    # graphs on: the pressure is launched plainly and the captured graphs of the velocity execute keep replaying its bits
    plan.set_graphs(True)
    try:
        for rep in range(3):
            F.K.set_p(p)
            assert np.array_equal(plan.execute(ref.x), y0), rep
            assert np.array_equal(F.run(p), q0), rep
            assert np.array_equal(F.run(7, "x2"), F.run(7, "x2")), rep       # another order and vector in between
        F.K.set_p(p)
        assert np.array_equal(plan.execute(ref.x), y0)
    finally:
        plan.set_graphs(False)
    F.K.set_p(p)
    assert np.array_equal(plan.execute(ref.x), y0)
    # the gradient's refusal on this plan is what it was
    with pytest.raises(fb.FmmBemError) as e:
        plan.execute_gradient(ref.x)
    assert e.value.status == 6 and "Laplace" in str(e.value)
    assert np.array_equal(F.run(p), q0)
    # the device form on the default stream and on a side stream
    F.K.set_p(p)
    xd = torch.from_numpy(ref.x).to("cuda:0")
    qd = plan.execute_pressure_torch(xd)
    torch.cuda.synchronize()
    assert tuple(qd.shape) == (len(ref.pts),) and np.array_equal(qd.cpu().numpy(), q0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        qs = plan.execute_pressure_torch(xd)
        out = torch.empty_like(qs)
        assert plan.execute_pressure_torch(xd, out=out) is out
    s.synchronize()
    assert np.array_equal(qs.cpu().numpy(), q0) and np.array_equal(out.cpu().numpy(), q0)
    with pytest.raises(ValueError):
        plan.execute_pressure_torch(xd[:-1].contiguous())
    with pytest.raises(ValueError):
        plan.execute_pressure(ref.x[:-1])


def test_plans_that_refuse_on_the_device(fb):
    ref = Q.reference("one_row")
    K, field = Q.host_plan(fb, ref.v, ref.pts, ref.c["ncrit"], host_only=False)
    opts = fb.FMMOptions()
    opts.set_mac_theta(G.THETA)
    single = fb.FMM_plan(K, ref.v, opts, p_max=16)
    flags = (np.arange(len(ref.pts)) % 2).astype(np.uint8)
    traction = single.field_plan(ref.pts, flags)
    laplace = fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), ref.v, opts, p_max=16).field_plan(ref.pts)
    for plan, x, word in ((single, ref.x, "separate targets"), (traction, ref.x, "VELOCITY"), (laplace, ref.x[:, 0].copy(), "Stokes")):
        y0 = plan.execute(x)
        with pytest.raises(fb.FmmBemError) as e:
            plan.execute_pressure(x)
        assert e.value.status == 6 and word in str(e.value), (word, str(e.value))
        assert np.array_equal(plan.execute(x), y0)             # the handle stays usable
    assert np.all(np.isfinite(field.execute_pressure(ref.x)))


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
def entry_pairs():
    """targets as degenerate triangles (all three vertices the point) against panels: far, near, self, and one target placed exactly
    on a fine-rule point of its panel"""
    ref = Q.reference("r4_ncrit8")
    rng = np.random.default_rng(11)
    n = len(ref.v)
    sj = rng.integers(0, n, 400)
    t = G._dirs(rng, 400) * (1.05 + 1.5 * rng.random(400))[:, None]
    near = np.arange(100, 250)                              # 0.1 .. 0.6 sqrt(2 A) above the panel: the near regime
    h = (0.1 + 0.5 * rng.random(len(near))) * np.sqrt(2 * ref.g["area"][sj[near]])
    nrm = ref.g["center"][sj[near]] / np.linalg.norm(ref.g["center"][sj[near]], axis=1)[:, None]
    t[near] = ref.g["center"][sj[near]] + nrm * h[:, None]
    self_ = np.arange(250, 290)
    bF = Q._rules()[1][0]
    on_point = 399                                          # a fine-rule point that is not the centroid: nearby, that point gives 0
    far_from_centre = int(np.argmax(np.abs(bF - 1.0 / 3).max(axis=1)))
    t[on_point] = bF[far_from_centre] @ ref.v[sj[on_point]]
    tv = np.repeat(t[:, None, :], 3, axis=1)
    tv[self_] = ref.v[sj[self_]]                            # the panel itself
    t = (tv[:, 0] + tv[:, 1] + tv[:, 2]) / 3                # the target point as the library forms it from the triangle
    return ref, t, tv, sj, near, self_, on_point


def test_pressure_entries(fb):
    ref, t, tv, sj, near, self_, on_point = entry_pairs()
    K = R.stokes_kernel(fb, 5)
    got = fb.kernel_pressure_entries(K, tv, ref.v[sj])
    assert got.shape == (len(t), 3)
    want = np.stack([Q.pi_entry(t[k], ref.v[sj[k]:sj[k] + 1], Q.sub(ref.g, sj[k:k + 1]))[0] for k in range(len(t))])
    scale = np.array([Q.pi_scale(t[k], ref.v[sj[k]:sj[k] + 1], Q.sub(ref.g, sj[k:k + 1]))[0] for k in range(len(t))])
    regime = np.array([Q.regimes(t[k], Q.sub(ref.g, sj[k:k + 1])) for k in range(len(t))])[:, :, 0]      # (pairs, [self, nearby])
    assert np.all(regime[self_, 0]) and np.all(regime[near, 1]) and regime[on_point, 1] and (~regime.any(axis=1)).sum() >= 100
    assert np.all(got[self_] == 0) and np.all(want[self_] == 0)
    rest = ~regime[:, 0]
    err = np.abs(got[rest] - want[rest]).max(axis=1) / scale[rest]
    print("pressure entries vs numpy: worst %.2e of the scale (near regime %.2e, on a fine-rule point %.2e)"
          % (err.max(), (np.abs(got[near] - want[near]).max(axis=1) / scale[near]).max(),
             np.abs(got[on_point] - want[on_point]).max() / scale[on_point]))
    assert np.all(np.isfinite(got)) and np.all(err <= 1e-13), float(err.max())
    # the point the target sits on was left out, by the library and by numpy: the full fine-rule sum without the r^2 cut is infinite
    d2 = ((t[on_point][None] - np.einsum("qk,kx->qx", Q._rules()[1][0], ref.v[sj[on_point]])) ** 2).sum(1)
    assert (d2 < 1e-8).sum() == 1


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
def test_timed_pressure_execute_reports_its_kernels(fb):
    F = get(fb, "r4_ncrit8")
    F.plan.set_timing(True)
    try:
        q = F.run(8)
        st = F.plan.stats()
    finally:
        F.plan.set_timing(False)
    assert st["timed_executes"] == 1 and st["last_p"] == 8
    assert st["ms_near"] > 0 and st["ms_l2p"] > 0 and st["ms_m2l"] > 0 and st["ms_total"] >= st["ms_near"]
    assert np.array_equal(q, F.run(8))


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
def sphere_points(m, radius):
    i = np.arange(m) + 0.5
    z = 1 - 2 * i / m
    r = np.sqrt(1 - z * z)
    phi = math.pi * (3 - math.sqrt(5)) * i
    return radius * np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


# The driver's first-kind solve converges on every unit sphere it accepts from 1 recursion on (8 panels: 2 iterations), so the
# smallest mesh is 1 recursion -- and its discretisation error leaves a bound that catches little more than a wrong sign.  Both
# are held: 1 recursion, the smallest, and 4 (512 panels), fine enough for the bound to hold the pressure to a percent.  Measured once on an MI355X, p = 8,
# K = 4, K_fine = 19: the largest deviation of q / (6 pi mu) from x / r^3 over 200 points at r = 3, relative to 1/9, beside the drag
# error the driver prints for the same mesh (recursions 2 and 3 give 7.443e-02 and 1.078e-02, drag 6.48e-02 and 8.64e-03):
#   recursions 1:  2.296e-01  (drag error 2.44323e-01)        recursions 4:  2.599e-03  (drag error 3.03171e-03)
# This is the discretisation's error, which cannot be derived; asserted: 4 x the measured figure.
MEASURED_DEVIATION = {1: 2.296e-01, 4: 2.599e-03}


@pytest.mark.parametrize("recursions", [1, 4])
def test_translating_sphere_end_to_end(fb, recursions):
    import torch
    mu, p = 1e-3, 8
    v = fb.unit_sphere(recursions)
    n = len(v)
    K = fb.StokesSphericalBEM(p, 4, mu)
    K.set_Kfine(19)
    opts = fb.FMMOptions()
    plan = fb.FMM_plan(K, v, opts, p_max=p)
    so = fb.SolverOptions()
    so.max_p, so.p_min, so.max_iters, so.restart = p, 5, 100, 100
    b = torch.zeros((n, 3), dtype=torch.float64, device="cuda:0")
    b[:, 0] = 4 * math.pi                                  # the driver's right-hand side: u = e_x on every panel
    x, it, res = fb.gmres(plan, torch.zeros(3 * n, dtype=torch.float64, device="cuda:0"), b.reshape(-1), so, stokes=True)
    assert res <= so.residual, (it, res)
    pts = sphere_points(200, 3.0)
    K.set_p(p)
    q = plan.field_plan(pts).execute_pressure(x.cpu().numpy())
    dev = float(np.abs(q / (6 * math.pi * mu) - pts[:, 0] / 27.0).max() * 9.0)
    print("translating sphere, %d panels, %d iterations: largest deviation of q / (6 pi mu) from x / r^3: %.3e of 1/9" % (n, it, dev))
    assert dev <= 4 * MEASURED_DEVIATION[recursions], dev


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
def driver(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "examples", "StokesBEM.py")] + list(args), capture_output=True, text=True, timeout=600)


def test_driver_field_pressure():
    r = driver("-recursions", "4", "-p", "8", "-field_fmm", "200", "-field_pressure")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    line = [ln for ln in lines if ln.startswith("field pressure (FMM):")]
    assert len(line) == 1 and "200 points at r = 3" in line[0], lines[-12:]
    assert sum(ln.startswith("field (FMM):") for ln in lines) == 1
    sphere = [ln for ln in lines if ln.startswith("field pressure against the translating sphere's:")]
    assert len(sphere) == 1
    print("\n".join([ln for ln in lines if ln.startswith("error on a sphere:")] + [line[0], sphere[0]]))
    assert float(sphere[0].split("deviation")[1].split("of")[0]) <= 4 * MEASURED_DEVIATION[4]
    r = driver("-recursions", "4", "-p", "8", "-field_pressure")
    assert r.returncode != 0 and "-field_fmm" in r.stderr


def test_report_worst_errors():
    print("\nfield pressure vs composed reference: worst relative L2 %.2e, worst row %.2e of the scale, rows on the axis %.2e"
          % (WORST["rel"], WORST["row"], WORST["axis"]))
