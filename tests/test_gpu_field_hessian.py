"""The field Hessian on the GPU (fmmbem_plan_execute_hessian) against the composed CPU reference of tests/field_hessian_reference.py:
the near pairs by eta in numpy over the plan's own p2p list, the far half by the oracle's P2M and translations and the long-double
Hessian of the local expansions.

1 composed reference, per flag class relative L2 <= 1e-12, every row within 1e-11 of the class scale (max_i sum_j sum |eta_ij| |x_j|),
  the trace within 1e-11 of it, H == H^T bit for bit: two_r3 at every order 1..16, the other cases at 1, 2, 3, 8, 12, 13, 16; p = 1 and
  p = 2 are the near half; no_far and far_only's special results; the rows on the axis of their leaf within ON_AXIS_DEVIATION; a
  relaxed sequence and a second vector; a rule of 13 points (23 panels per staged batch)
2 the limit sum (no expansions): the execute's error is the composed reference's error
3 the index order: a rotated case against the rotated reference, no permutation of axes fits
4 kernel_hessian_entries against eta in numpy in all three regimes
5 bits: repeats, host and device forms, coincident targets, a field plan, the other executes around a Hessian execute, graphs on and off
6 stage times of a timed Hessian execute    7 the driver's -field_hess line"""
import os
import subprocess
import sys

import numpy as np
import pytest

import field_gradient_reference as G
import field_hessian_reference as H
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = (1, 2, 3, 8, 12, 13, 16)
WORST = {}


class Fixture:
    def __init__(self, fb, name, k=H.K):
        self.R = R = H.reference(name, k)
        opts = fb.FMMOptions()
        opts.set_mac_theta(H.THETA)
        opts.set_max_per_box(R.c["ncrit"])
        self.K = fb.LaplaceSphericalBEM(8, k)
        self.plan = fb.FMM_plan(self.K, R.v, opts, p_max=16, targets=R.pts, target_bc=R.flags)
        # the reference sums over the oracle's lists: they are the plan's (tests/test_target_plan_oracle_host.py pins the trees)
        for which in ("p2p", "m2l", "l2l"):
            assert np.array_equal(self.plan.pairs(which), R.T.pairs(which)), which

    def run(self, p, key="x"):
        self.K.set_p(p)
        return self.plan.execute_hessian(self.R.vector(key))


_FIX = {}


def get(fb, name, k=H.K):
    if (name, k) not in _FIX:
        _FIX[(name, k)] = Fixture(fb, name, k)
    return _FIX[(name, k)]


def check(h, ref, R, what, key="x", exempt=None):
    flags = R.flags
    assert h.shape == ref.shape == (len(flags), 3, 3) and np.all(np.isfinite(h)), what
    assert np.array_equal(h, h.transpose(0, 2, 1)), what
    for f in (0, 1):
        s = flags == f
        if exempt is not None:
            s = s & ~exempt
        if not s.any():
            continue
        scale = R.scale(f, key)
        if not np.any(ref[s]):                              # no near pair and no term in the expansion: zeros, exactly
            assert np.all(h[s] == 0), (what, f)
            continue
        rel = float(np.linalg.norm(h[s] - ref[s]) / np.linalg.norm(ref[s]))
        err = float(np.abs(h[s] - ref[s]).max() / scale)
        tr = float(np.abs(np.trace(h[s], axis1=1, axis2=2)).max() / scale)
        WORST[f] = max(WORST.get(f, 0.0), rel)
        print("%s flag %d: rel L2 %.2e, worst row %.2e and trace %.2e of the scale" % (what, f, rel, err, tr))
        assert rel <= 1e-12, (what, f, rel)
        assert err <= 1e-11, (what, f, err)
        assert tr <= 1e-11, (what, f, tr)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
def test_every_order_on_one_plan(fb):
    F = get(fb, "two_r3")
    got = {}
    for p in range(1, 17):
        got[p] = F.run(p)
        check(got[p], F.R.hessian(p), F.R, ("two_r3", p))
    near = F.R.near_half("x")[F.R.given]
    assert np.array_equal(got[1], got[2])                   # no second derivative in an expansion of order 1 or 2: the near half
    check(got[1], near, F.R, ("two_r3", "the near half"))
    assert not np.array_equal(got[3], got[2])


@pytest.mark.parametrize("name", ["r4_ncrit8", "big_leaves", "one_row", "far_only", "no_far"])
def test_case_equals_composed_reference(fb, name):
    F = get(fb, name)
    got = {}
    for p in ORDERS:
        got[p] = F.run(p)
        check(got[p], F.R.hessian(p), F.R, (name, p))
    assert np.array_equal(got[1], got[2])
    if name == "r4_ncrit8":                                 # four targets on centroids: the zero self rule, and finite
        on = np.arange(len(F.R.pts) - 4, len(F.R.pts))
        assert np.all(np.isfinite(got[8][on])) and np.abs(got[8][on]).max() > 0
    if name == "big_leaves":
        tb = F.plan.target_boxes()
        assert (tb["be"] - tb["bb"])[tb["leaf"] != 0].max() > 64
    if name == "far_only":
        st = F.plan.stats()
        assert st["p2p_pairs"] == 0 and st["m2l_pairs"] >= 1
        assert np.all(got[1] == 0) and np.abs(got[8]).max() > 0
        F.K.set_p(8)
        zero = F.plan.execute_hessian(np.zeros(len(F.R.v)))
        assert np.all(zero == 0)
        assert np.array_equal(F.run(8), got[8])
    if name == "no_far":
        assert F.plan.stats()["m2l_pairs"] == 0
        for p in (3, 13):                                   # no far field: the near sum, the same bits at every order
            assert np.array_equal(got[p], got[8]), p


@pytest.mark.parametrize("p", [12, 13])
def test_targets_on_the_axis_of_their_leaf(fb, p):
    """The 16 added rows (a leaf's centre and 0.3 side above it): finite, within ON_AXIS_DEVIATION of the class scale -- what a
    double-precision spherical chain loses there against the singularity-free reference.  Every other row keeps the bounds."""
    F = get(fb, "awkward")
    R = F.R
    h, ref = F.run(p), R.hessian(p)
    exempt = np.zeros(len(R.pts), bool)
    exempt[-H.N_AWKWARD:] = True
    check(h, ref, R, ("awkward, the other rows", p), exempt=exempt)
    added = np.nonzero(exempt)[0]
    assert np.all(np.isfinite(h[added])) and np.array_equal(h[added], h[added].transpose(0, 2, 1))
    for f in (0, 1):
        rows = added[R.flags[added] == f]
        assert len(rows) == 8
        err = float(np.abs(h[rows] - ref[rows]).max() / R.scale(f))
        print("awkward rows p = %d, flag %d: %.3e of the scale" % (p, f, err))
        assert err <= H.ON_AXIS_DEVIATION, (p, f, err)


def test_relaxed_sequence_and_a_second_vector(fb):
    F = get(fb, "two_r3")
    seen = {}
    for p in (10, 4, 13, 4, 10):
        h = F.run(p)
        check(h, F.R.hessian(p), F.R, ("relaxed", p))
        assert np.array_equal(seen.setdefault(p, h), h), p
    for p in (4, 13):
        check(F.run(p, "x2"), F.R.hessian(p, "x2"), F.R, ("second vector", p), key="x2")
    assert np.array_equal(F.run(10), seen[10])


def test_rule_of_thirteen_points(fb):
    """K = 13: 8 + 39 doubles per staged panel, 23 panels per batch, so a leaf's run of near panels spans several batches.  The same
    bounds, against the reference built at that rule."""
    F = get(fb, "two_r3", 13)
    assert max(sum(len(F.R.base.leaf_panels(s)) for s in lists) for lists in F.R.near.values()) > 3 * 23
    for p in (2, 9, 13):
        check(F.run(p), F.R.hessian(p), F.R, ("K = 13", p))


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
def class_errors(h, lim, flags):
    return [float(np.linalg.norm(h[flags == f] - lim[flags == f]) / np.linalg.norm(lim[flags == f])) for f in (0, 1)]


def test_error_against_the_limit_sum_is_the_references(fb):
    F = get(fb, "two_r3")
    lim = F.R.limit()
    for p in (4, 8, 12, 16):
        got, want = class_errors(F.run(p), lim, F.R.flags), class_errors(F.R.hessian(p), lim, F.R.flags)
        print("two_r3 vs limit sum at p = %d (flag 0, flag 1): execute %s, composed reference %s" % (p, got, want))
        for f in (0, 1):
            assert abs(got[f] - want[f]) <= 1e-12, (p, f, got, want)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
def test_index_order_under_a_rotation(fb):
    """no_far -- every pair a near pair, so the result does not depend on how a tree cuts the rotated points -- turned by a fixed
    rotation Q without symmetry: H' = Q H Q^T of the reference.  The rotated vertices carry roundings of 2e-16 against distances
    >= 0.05, which eta amplifies by 7 / r, and a row's sum cancels by up to 30: held to 1e-11 of the class scale.  No permutation of
    the axes of the result fits the rotated reference (H is symmetric: the transposition is no permutation to find)."""
    R = H.reference("no_far")
    ax = np.array([0.3, -0.5, 0.81])
    ax /= np.linalg.norm(ax)
    a = 0.7
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    Qr = np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx
    assert np.abs(Qr @ Qr.T - np.eye(3)).max() < 1e-15
    opts = fb.FMMOptions()
    opts.set_mac_theta(H.THETA)
    opts.set_max_per_box(R.c["ncrit"])
    K = fb.LaplaceSphericalBEM(8, H.K)
    plan = fb.FMM_plan(K, R.v @ Qr.T, opts, p_max=8, targets=R.pts @ Qr.T, target_bc=R.flags)
    assert plan.stats()["m2l_pairs"] == 0
    got = plan.execute_hessian(R.x)
    plan.close()
    ref = R.hessian(8)
    want = np.einsum("ia,nab,jb->nij", Qr, ref, Qr)
    for f in (0, 1):
        s = R.flags == f
        err = float(np.abs(got[s] - want[s]).max() / R.scale(f))
        print("rotated no_far, flag %d: %.2e of the scale" % (f, err))
        assert err <= 1e-11, (f, err)
    k = int(np.argmax(np.abs(want).max(axis=(1, 2))))       # the row with the largest entries: next to one panel, nothing symmetric
    for perm in ((0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        moved = got[k][np.ix_(perm, perm)]
        assert np.linalg.norm(moved - want[k]) > 1e-3 * np.linalg.norm(want[k]), perm
    assert np.linalg.norm(got[k] - ref[k]) > 1e-3 * np.linalg.norm(ref[k])       # and the rotation did turn it


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
def test_hessian_entries(fb):
    """Targets as degenerate triangles against the panels of unit_sphere(2): far (1.05 .. 2.55 from the centre), near (0.1 .. 0.6
    sqrt(2 A) above the panel), self (the panel itself), both flags; <= 1e-13 of the entry's largest component.  The mesh is the
    coarse one on purpose: a quadrature point is a sum of three products of coordinates ~ 1, so library and numpy may place it 2e-16
    apart, which 1 / r^7 turns into 7 . 2e-16 / r of a term -- 3e-14 at r >= 0.044 here, and past the bound on the finer meshes of
    the other tests."""
    v = O.unit_sphere(2)
    g = G.geometry(v)
    rng = np.random.default_rng(11)
    n = len(v)
    sj = rng.integers(0, n, 400)
    t = G._dirs(rng, 400) * (1.05 + 1.5 * rng.random(400))[:, None]
    near = np.arange(100, 250)
    h = (0.1 + 0.5 * rng.random(len(near))) * np.sqrt(2 * g["area"][sj[near]])
    t[near] = g["center"][sj[near]] + g["normal"][sj[near]] * h[:, None]
    self_ = np.arange(250, 290)
    flags = (np.arange(400) % 2).astype(np.uint8)
    tv = np.repeat(t[:, None, :], 3, axis=1)
    tv[self_] = v[sj[self_]]
    t = (tv[:, 0] + tv[:, 1] + tv[:, 2]) / 3                # the target point as the library forms it from the triangle
    K = fb.LaplaceSphericalBEM(5, H.K)
    got = fb.kernel_hessian_entries(K, tv, v[sj], target_bc=flags)
    assert got.shape == (400, 3, 3) and np.array_equal(got, got.transpose(0, 2, 1))
    want = np.stack([H.eta(t[k], int(flags[k]), v[sj[k]:sj[k] + 1], G.sub(g, sj[k:k + 1]))[0] for k in range(len(t))])
    d = np.linalg.norm(t - g["center"][sj], axis=1)
    ratio = np.sqrt(2 * g["area"][sj]) / np.maximum(d, 1e-300)
    regime = np.where(d < 1e-8, 2, np.where(ratio >= 0.5, 1, 0))
    assert (regime == 2).sum() == 40 and (regime == 1).sum() >= 150 and (regime == 0).sum() >= 100
    assert np.all(got[regime == 2] == 0) and np.all(want[regime == 2] == 0)
    scale = np.abs(want).max(axis=(1, 2))
    live = regime != 2
    err = np.abs(got - want).max(axis=(1, 2))[live] / scale[live]
    print("Hessian entries vs numpy: worst %.2e (16-point regime %.2e, K-point regime %.2e)"
          % (err.max(), err[regime[live] == 1].max(), err[regime[live] == 0].max()))
    assert np.all(err <= 1e-13), float(err.max())
    tr = np.abs(np.trace(got, axis1=1, axis2=2))[live] / scale[live]
    assert tr.max() <= 1e-13, float(tr.max())


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
def test_bits(fb):
    import torch
    F = get(fb, "two_r3")
    R, plan = F.R, F.plan
    p = 10
    X = np.stack([R.x, R.x2, -R.x])

    def others():
        F.K.set_p(p)
        phi, grad = plan.execute_representation(R.x, R.x2)
        return plan.execute(R.x), plan.execute_batch(X), plan.execute_gradient(R.x), phi, grad

    before = others()
    h0 = F.run(p)
    assert np.array_equal(F.run(p), h0)
    for a, b in zip(before, others()):
        assert np.array_equal(a, b)
    # coincident targets receive equal rows (the ten copies: five per flag)
    copies = np.arange(len(R.pts) - 10, len(R.pts))
    for f in (0, 1):
        rows = copies[R.flags[copies] == f]
        assert len(rows) == 5 and np.all(h0[rows] == h0[rows[0]])
    assert not np.array_equal(h0[copies[0]], h0[copies[1]])
    # graphs on: the Hessian is launched plainly and the captured graphs of the other executes keep replaying their bits
    plan.set_graphs(True)
    try:
        for rep in range(2):
            for a, b in zip(before, others()):
                assert np.array_equal(a, b), rep
            assert np.array_equal(F.run(p), h0), rep
            assert np.array_equal(F.run(7, "x2"), F.run(7, "x2")), rep       # another order and vector in between
        for a, b in zip(before, others()):
            assert np.array_equal(a, b)
    finally:
        plan.set_graphs(False)
    for a, b in zip(before, others()):
        assert np.array_equal(a, b)
    # a side stream, device pointers: the host form's bits
    F.K.set_p(p)
    xd = torch.from_numpy(R.x).to("cuda:0")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        hd = plan.execute_hessian_torch(xd)
        out = torch.empty_like(hd)
        assert plan.execute_hessian_torch(xd, out=out) is out
    s.synchronize()
    assert tuple(hd.shape) == (len(R.pts), 3, 3)
    assert np.array_equal(hd.cpu().numpy(), h0) and np.array_equal(out.cpu().numpy(), h0)
    with pytest.raises(ValueError):
        plan.execute_hessian_torch(xd, out=out[:-1])


def test_field_plan_has_the_target_plans_bits(fb):
    F = get(fb, "two_r3")
    R = F.R
    opts = fb.FMMOptions()
    opts.set_mac_theta(H.THETA)
    opts.set_max_per_box(R.c["ncrit"])
    K = fb.LaplaceSphericalBEM(9, H.K)
    field = fb.FMM_plan(K, R.v, opts, p_max=16).field_plan(R.pts, R.flags)
    assert np.array_equal(field.execute_hessian(R.x), F.run(9))
    with pytest.raises(fb.FmmBemError) as e:                 # and the plan it came from is no plan over separate targets
        fb.FMM_plan(K, R.v, opts, p_max=16).execute_hessian(R.x)
    assert e.value.status == 6 and "the field Hessian" in str(e.value)
    stokes = fb.FMM_plan(fb.StokesSphericalBEM(5, 3), R.v, opts).field_plan(R.pts)
    with pytest.raises(fb.FmmBemError) as e:
        stokes.execute_hessian(np.ones((len(R.v), 3)))
    assert e.value.status == 6 and "Laplace" in str(e.value)


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
def test_timed_hessian_execute_reports_its_kernels(fb):
    F = get(fb, "r4_ncrit8")
    st = {}
    for p in (8, 1):                                        # (the stage times are means over the executes since timing was set)
        F.plan.set_timing(True)
        try:
            h = F.run(p)
            st[p] = F.plan.stats()
        finally:
            F.plan.set_timing(False)
        assert st[p]["timed_executes"] == 1 and st[p]["last_p"] == p
    assert st[8]["ms_near"] > 0 and st[8]["ms_l2p"] > 0 and st[8]["ms_m2l"] > 0 and st[8]["ms_total"] >= st[8]["ms_near"]
    assert st[1]["ms_near"] > 0 and st[1]["ms_l2p"] == 0    # order 1: the L2P is not launched
    h = F.run(8)
    assert np.array_equal(h, F.run(8))


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
def driver(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "LaplaceBEM.py")] + list(args), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.splitlines()


def figure(lines, start):
    line = [ln for ln in lines if ln.startswith(start)]
    assert len(line) == 1, lines
    print(line[0])
    assert "200 points at r = 3" in line[0]
    return float(line[0].split("max error:")[1].split(",")[0])


def test_driver_field_hessian():
    """Both figures are the discretisation's on the same mesh: the Hessian's max error stays below 3 x the gradient's"""
    args = ["-recursions", "4", "-p", "12", "-fixed_p", "-field", "200", "-field_grad"]
    lines = driver(*args, "-field_hess")
    gerr, herr = figure(lines, "field gradient:"), figure(lines, "field Hessian:")
    print("field Hessian / field gradient, max error: %.3f" % (herr / gerr))
    assert herr <= 3 * gerr, (herr, gerr)
    one_pass = driver(*args, "-field_hess", "-field_one_pass")
    assert figure(one_pass, "field Hessian:") == herr       # the two plans' Hessian executes, also with -field_one_pass


def test_report_worst_errors():
    print("\nfield Hessian vs composed reference, worst relative L2: flag 0 %.2e, flag 1 %.2e" % (WORST.get(0, 0.0), WORST.get(1, 0.0)))
