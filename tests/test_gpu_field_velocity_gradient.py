"""The field velocity gradient on the GPU (fmmbem_plan_execute_velocity_gradient) against the composed CPU reference of
tests/field_velocity_gradient_reference.py: the near pairs by gamma_entry in numpy over the plan's own p2p list, the far half by the
oracle's P2M and translations and the long-double gradients and Hessians of the local expansions.

1 composed reference: orders 1 .. 16 on two_r3 and 1, 2, 3, 8, 12, 13, 16 on the other cases (the empty Hessian, the antisymmetric-only
  order, the unrolled / generic boundary), relative L2 <= 1e-12 and every row within 1e-11 of the case's scale max_i sum_j sum |Gamma_ij|
  |x_j| (the bounds of the gradient and pressure tests for the same recurrence); the 16 rows on the axis or at the centre of their leaf
  (awkward) within ON_AXIS_DEVIATION of the scale; the trace of every row of every case within 1e-11 of the scale; G far from its
  transpose; a relaxed sequence of orders and a second vector on one plan
2 bits: repeats, host and device forms, coincident copies, execute / execute_batch / execute_pressure around a gradient execute with
  graphs on and off
3 kernel_velocity_gradient_entries against gamma_entry in numpy in all three regimes and on a fine-rule point
4 execute_stress    5 stage times of a timed execute    6 the translating sphere, end to end    7 the driver's -field_stress line"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import field_gradient_reference as G
import field_plan_reference as R
import field_pressure_reference as Q
import field_velocity_gradient_reference as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = {name: (tuple(range(1, 17)) if name == "two_r3" else (1, 2, 3, 8, 12, 13, 16)) for name in V.CASES}
WORST = {"rel": 0.0, "row": 0.0, "axis": 0.0, "trace": 0.0}


class Fixture:
    def __init__(self, fb, name):
        self.R = ref = V.reference(name)
        self.K, self.plan = Q.host_plan(fb, ref.v, ref.pts, ref.c["ncrit"], p_max=16, host_only=False)
        # the reference sums over the host-only plan's lists: they are this plan's
        for which in ("p2p", "m2l", "m2m", "l2l"):
            assert np.array_equal(self.plan.pairs(which), ref.lists[which]), which
        assert np.array_equal(self.plan.target_perm()[0], ref.tree) and np.array_equal(self.plan.perm(), ref.perm)

    def run(self, p, key="x"):
        self.K.set_p(p)
        return self.plan.execute_velocity_gradient(self.R.vector(key))


_FIX = {}


def get(fb, name):
    if name not in _FIX:
        _FIX[name] = Fixture(fb, name)
    return _FIX[name]


def check(g, ref, scale, what, exempt=None):
    assert g.shape == ref.shape and g.shape[1:] == (3, 3) and np.all(np.isfinite(g)), what
    s = np.ones(len(g), bool) if exempt is None else ~exempt
    top = float(np.linalg.norm(ref[s]))
    rel = float(np.linalg.norm(g[s] - ref[s]) / top) if top > 0 else float(np.any(g[s] != 0))
    row = float(np.abs(g[s] - ref[s]).max() / scale)
    trace = float(np.abs(g[:, 0, 0] + g[:, 1, 1] + g[:, 2, 2]).max() / scale)           # every row, the exempt ones too
    WORST["rel"], WORST["row"], WORST["trace"] = max(WORST["rel"], rel), max(WORST["row"], row), max(WORST["trace"], trace)
    print("%s: rel L2 %.2e, worst row %.2e of the scale, trace %.2e of the scale" % (what, rel, row, trace))
    assert rel <= 1e-12, (what, rel)
    assert row <= 1e-11, (what, row)
    assert trace <= 1e-11, (what, trace)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in V.CASES if n != "awkward"])
def test_every_order_equals_composed_reference(fb, name):
    F = get(fb, name)
    scale = F.R.scale()
    for p in ORDERS[name]:
        check(F.run(p), F.R.gradient(p), scale, (name, p))
    if name == "two_r3":
        # the far half at p = 1 is nothing, at p = 2 antisymmetric: the symmetric parts of the three results are the near half's
        g1, g2, near = F.run(1), F.run(2), F.R.near_half()[F.R.given]
        assert np.abs(g1 - near).max() <= 1e-11 * scale
        assert np.abs((g2 + g2.transpose(0, 2, 1)) - (g1 + g1.transpose(0, 2, 1))).max() <= 1e-11 * scale
        assert np.abs(g2 - g1).max() > 1e-6 * scale
    if name == "big_leaves":
        tb = F.plan.target_boxes()
        assert (tb["be"] - tb["bb"])[tb["leaf"] != 0].max() > 64
    if name == "no_far":
        assert F.plan.stats()["m2l_pairs"] == 0
        g8 = F.run(8)
        for p2 in (3, 13):                                  # no far field: the near sums, the same bits at every order
            assert np.array_equal(F.run(p2), g8), p2
    if name == "far_only":
        st = F.plan.stats()
        assert st["p2p_pairs"] == 0 and st["m2l_pairs"] >= 1
        # the near kernel stores zeros in every row before the far kernel adds: x = 0 leaves nothing but them (a row the near
        # kernel skipped would keep the previous execute's value), and a repeat has the same bits
        assert np.all(F.R.near_half("x") == 0)
        g8 = F.run(8)
        assert np.array_equal(F.run(8), g8)
        F.K.set_p(8)
        assert np.all(F.plan.execute_velocity_gradient(np.zeros_like(F.R.x)) == 0)
        assert np.array_equal(F.run(8), g8)
        assert np.all(F.run(1) == 0)                        # order 1: no far kernel at all, the stored zeros


def test_awkward_orders(fb):
    """The 16 added rows (a leaf's centre and points on its axis): finite, within ON_AXIS_DEVIATION of the scale -- what a
    double-precision spherical chain loses there against the singularity-free reference (tests/test_field_velocity_gradient_host.py
    (e)).  Every other row keeps the bounds, and every row the trace's."""
    F = get(fb, "awkward")
    ref = F.R
    exempt = np.zeros(len(ref.pts), bool)
    exempt[-V.N_AWKWARD:] = True
    for p in ORDERS["awkward"]:
        g, want = F.run(p), ref.gradient(p)
        check(g, want, ref.scale(), ("awkward, the other rows", p), exempt=exempt)
        err = float(np.abs(g[exempt] - want[exempt]).max() / ref.scale())
        WORST["axis"] = max(WORST["axis"], err)
        print("awkward rows p = %d: %.3e of the scale" % (p, err))
        assert err <= V.ON_AXIS_DEVIATION, (p, err)


def test_index_order(fb):
    """G differs from its transpose by far more than any bound: a transposed store cannot pass the comparisons above unnoticed"""
    F = get(fb, "two_r3")
    g = F.run(8)
    assert np.linalg.norm(g - g.transpose(0, 2, 1)) > 1e-3 * np.linalg.norm(g)
    want = F.R.gradient(8)
    assert np.linalg.norm(g.transpose(0, 2, 1) - want) > 1e-3 * np.linalg.norm(want)


def test_relaxed_sequence_and_second_vector(fb):
    F = get(fb, "two_r3")
    scale2 = F.R.scale("x2")
    for p in (10, 4, 13, 4, 10):
        check(F.run(p), F.R.gradient(p), F.R.scale(), ("relaxed", p))
        check(F.run(p, "x2"), F.R.gradient(p, "x2"), scale2, ("relaxed, second vector", p))


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
def test_bits(fb):
    import torch
    F = get(fb, "two_r3")
    ref, plan = F.R, F.plan
    p = 10
    xb = np.stack([ref.x, ref.x2])
    F.K.set_p(p)
    y0, yb0, q0 = plan.execute(ref.x), plan.execute_batch(xb), plan.execute_pressure(ref.x)
    g0 = F.run(p)
    assert g0.shape == (len(ref.pts), 3, 3)
    assert np.array_equal(F.run(p), g0)
    F.K.set_p(p)
    assert np.array_equal(plan.execute_velocity_gradient(ref.x.reshape(-1)), g0)       # (3N,) as (N, 3)

    def others_unchanged(what):
        F.K.set_p(p)
        assert np.array_equal(plan.execute(ref.x), y0), what
        assert np.array_equal(plan.execute_batch(xb), yb0), what
        assert np.array_equal(plan.execute_pressure(ref.x), q0), what

    others_unchanged("graphs off")
    # coincident targets receive equal values (the ten copies), and not their neighbour's
    copies = np.arange(len(ref.pts) - 10, len(ref.pts))
    assert np.all(g0[copies] == g0[copies[0]]) and np.all(g0[copies[0]] != g0[copies[0] - 1])
    # graphs on: the gradient is launched plainly and the captured graphs of the velocity execute keep replaying its bits
    plan.set_graphs(True)
    try:
        for rep in range(3):
            others_unchanged(("graphs on", rep))
            assert np.array_equal(F.run(p), g0), rep
            assert np.array_equal(F.run(7, "x2"), F.run(7, "x2")), rep       # another order and vector in between
        others_unchanged("graphs on, after")
    finally:
        plan.set_graphs(False)
    others_unchanged("graphs off again")
    # the Laplace gradient's refusal on this plan is what it was
    with pytest.raises(fb.FmmBemError) as e:
        plan.execute_gradient(ref.x)
    assert e.value.status == 6 and "Laplace" in str(e.value)
    assert np.array_equal(F.run(p), g0)
    # the device form on the default stream and on a side stream
    F.K.set_p(p)
    xd = torch.from_numpy(ref.x).to("cuda:0")
    gd = plan.execute_velocity_gradient_torch(xd)
    torch.cuda.synchronize()
    assert tuple(gd.shape) == (len(ref.pts), 3, 3) and np.array_equal(gd.cpu().numpy(), g0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gs = plan.execute_velocity_gradient_torch(xd)
        out = torch.empty_like(gs)
        assert plan.execute_velocity_gradient_torch(xd, out=out) is out
    s.synchronize()
    assert np.array_equal(gs.cpu().numpy(), g0) and np.array_equal(out.cpu().numpy(), g0)
    with pytest.raises(ValueError):
        plan.execute_velocity_gradient_torch(xd[:-1].contiguous())
    with pytest.raises(ValueError):
        plan.execute_velocity_gradient(ref.x[:-1])


def test_plans_that_refuse_on_the_device(fb):
    ref = V.reference("one_row")
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
            plan.execute_velocity_gradient(x)
        assert e.value.status == 6 and word in str(e.value), (word, str(e.value))
        assert np.array_equal(plan.execute(x), y0)             # the handle stays usable
    assert np.all(np.isfinite(field.execute_velocity_gradient(ref.x)))


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
def entry_pairs():
    """targets as degenerate triangles (all three vertices the point) against panels: far, near, self, and one target placed exactly
    on a fine-rule point of its panel (the pairs of the pressure's entries test)"""
    ref = V.reference("r4_ncrit8")
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


def gamma_scale(t, v, g):
    """sum_q |w_q A| (3 / r^2 + 3 / r^2) / (2 mu) of the rule the pair takes: the size of the terms an entry is the sum of"""
    wK, (bF, wF) = Q._rules()
    self_, near = Q.regimes(t, g)
    out = np.zeros(len(v))
    for mask, y, w in ((~near & ~self_, g["quad"], wK), (near, np.einsum("qk,pkx->pqx", bF, v), wF)):
        if not mask.any():
            continue
        d = t[None, None] - y[mask]
        r2 = (d * d).sum(-1)
        ok = r2 >= 1e-8
        out[mask] = np.where(ok, 6 * w[None] * g["area"][mask][:, None] / np.where(ok, r2, 1.0), 0.0).sum(1) / (2 * R.MU)
    return out


def test_velocity_gradient_entries(fb):
    """to 1e-13 of the terms' size: a few roundings of ~ 20 operations per point, as the pressure's entries"""
    ref, t, tv, sj, near, self_, on_point = entry_pairs()
    K = R.stokes_kernel(fb, 5)
    got = fb.kernel_velocity_gradient_entries(K, tv, ref.v[sj])
    assert got.shape == (len(t), 3, 3, 3)
    want = np.stack([V.gamma_entry(t[k], ref.v[sj[k]:sj[k] + 1], Q.sub(ref.g, sj[k:k + 1]))[0] for k in range(len(t))])
    scale = np.array([gamma_scale(t[k], ref.v[sj[k]:sj[k] + 1], Q.sub(ref.g, sj[k:k + 1]))[0] for k in range(len(t))])
    regime = np.array([Q.regimes(t[k], Q.sub(ref.g, sj[k:k + 1])) for k in range(len(t))])[:, :, 0]      # (pairs, [self, nearby])
    assert np.all(regime[self_, 0]) and np.all(regime[near, 1]) and regime[on_point, 1] and (~regime.any(axis=1)).sum() >= 100
    assert np.all(got[self_] == 0) and np.all(want[self_] == 0)
    rest = ~regime[:, 0]
    err = np.abs(got[rest] - want[rest]).reshape(rest.sum(), -1).max(axis=1) / scale[rest]
    print("velocity gradient entries vs numpy: worst %.2e of the scale (near regime %.2e, on a fine-rule point %.2e)"
          % (err.max(), (np.abs(got[near] - want[near]).reshape(len(near), -1).max(axis=1) / scale[near]).max(),
             np.abs(got[on_point] - want[on_point]).max() / scale[on_point]))
    assert np.all(np.isfinite(got)) and np.all(err <= 1e-13), float(err.max())
    assert np.abs(np.einsum("pkke->pe", got)).max() <= 1e-13 * scale.max()
    d2 = ((t[on_point][None] - np.einsum("qk,kx->qx", Q._rules()[1][0], ref.v[sj[on_point]])) ** 2).sum(1)
    assert (d2 < 1e-8).sum() == 1


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
def test_stress_is_the_two_executes(fb):
    F = get(fb, "two_r3")
    F.K.set_p(9)
    x = F.R.x
    q, g = F.plan.execute_pressure(x), F.plan.execute_velocity_gradient(x)
    s = F.plan.execute_stress(x)
    want = -q[:, None, None] * np.eye(3)[None] + R.MU * (g + g.transpose(0, 2, 1))
    assert s.shape == (len(F.R.pts), 3, 3) and np.array_equal(s, want)
    assert np.array_equal(s, s.transpose(0, 2, 1))
    # -q I + mu (G + G^T): the trace is -3 q, G being trace-free
    assert np.abs(np.trace(s, axis1=1, axis2=2) + 3 * q).max() <= 1e-11 * (R.MU * F.R.scale() + np.abs(q).max())


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
def test_timed_execute_reports_its_kernels(fb):
    F = get(fb, "r4_ncrit8")
    F.plan.set_timing(True)
    try:
        g = F.run(8)
        st = F.plan.stats()
    finally:
        F.plan.set_timing(False)
    assert st["timed_executes"] == 1 and st["last_p"] == 8
    assert st["ms_near"] > 0 and st["ms_l2p"] > 0 and st["ms_m2l"] > 0 and st["ms_total"] >= st["ms_near"]
    assert np.array_equal(g, F.run(8))


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
def sphere_points(m, radius):
    i = np.arange(m) + 0.5
    z = 1 - 2 * i / m
    r = np.sqrt(1 - z * z)
    phi = math.pi * (3 - math.sqrt(5)) * i
    return radius * np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def exact_velocity(x):
    """a unit sphere translating with e_x: u = 3/4 (e_x / r + x x_1 / r^3) + 1/4 (e_x / r^3 - 3 x x_1 / r^5)"""
    r = np.linalg.norm(x, axis=-1)[..., None]
    ex = np.zeros_like(x)
    ex[..., 0] = 1
    x1 = x[..., 0:1]
    return 0.75 * (ex / r + x * x1 / r ** 3) + 0.25 * (ex / r ** 3 - 3 * x * x1 / r ** 5)


def exact_gradient(pts, h=1e-4):
    """(M, 3, 3) [k][m] by central differences of the closed form: truncation h^2 / 6 |d^3 u| ~ 1e-9 . 1e-2 at r = 3, rounding
    2^-53 |u| / h ~ 1e-12: far below the discretisation's error"""
    out = np.empty((len(pts), 3, 3))
    for m in range(3):
        e = np.zeros(3)
        e[m] = h
        out[:, :, m] = (exact_velocity(pts + e) - exact_velocity(pts - e)) / (2 * h)
    return out


# The driver's first-kind solve at 1 recursion (8 panels) and 4 (512), as the pressure's end-to-end test holds them.  Measured once on
# an MI355X, p = 8, K = 4, K_fine = 19: the largest deviation of G / 4 pi from the exact gradient over 200 points at r = 3, relative
# to the largest entry of the exact gradient there, beside the drag error the driver prints for the same mesh:
#   recursions 1:  2.080e-01  (drag error 2.44323e-01)        recursions 4:  2.734e-03  (drag error 3.03171e-03)
# This is the discretisation's error, which cannot be derived; asserted: 4 x the measured figure.
MEASURED_DEVIATION = {1: 2.080e-01, 4: 2.734e-03}


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
    g = plan.field_plan(pts).execute_velocity_gradient(x.cpu().numpy())
    want = exact_gradient(pts)
    dev = float(np.abs(g / (4 * math.pi) - want).max() / np.abs(want).max())
    print("translating sphere, %d panels, %d iterations: largest deviation of G / 4 pi from the exact gradient: %.3e of its largest entry"
          % (n, it, dev))
    assert dev <= 4 * MEASURED_DEVIATION[recursions], dev


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
def driver(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "examples", "StokesBEM.py")] + list(args), capture_output=True, text=True, timeout=600)


def test_driver_field_stress():
    r = driver("-recursions", "4", "-p", "8", "-field_fmm", "200", "-field_stress")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    line = [ln for ln in lines if ln.startswith("field velocity gradient (FMM):")]
    assert len(line) == 1 and "200 points at r = 3" in line[0], lines[-12:]
    assert sum(ln.startswith("field (FMM):") for ln in lines) == 1
    sphere = [ln for ln in lines if ln.startswith("field velocity gradient against the translating sphere's:")]
    assert len(sphere) == 1
    print("\n".join([ln for ln in lines if ln.startswith("error on a sphere:")] + [line[0], sphere[0]]))
    assert float(sphere[0].split("deviation")[1].split("of")[0]) <= 4 * MEASURED_DEVIATION[4]
    r = driver("-recursions", "4", "-p", "8", "-field_stress")
    assert r.returncode != 0 and "-field_fmm" in r.stderr


def test_report_worst_errors():
    print("\nfield velocity gradient vs composed reference: worst relative L2 %.2e, worst row %.2e of the scale, rows on the axis %.2e, "
          "trace %.2e" % (WORST["rel"], WORST["row"], WORST["axis"], WORST["trace"]))
