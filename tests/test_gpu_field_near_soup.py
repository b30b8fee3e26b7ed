"""The matrix-free near kernels of the field quantities on ragged triangle soups, row by row against the long-double sum of
tests/field_near_cases.py -- never against another device result:

    |got_ic - ref_ic| <= (C_Q + T_i) 2^-53 S_i        (derived there; C_Q from the reference's own float64 error, not from the device)

on every row of every vector (normal, one entry x 1e8, three unit vectors: a row is then ONE pair, and a wrong panel, regime or
stale record cannot hide in a sum) of every case.  The plans take theta = THETA: no M2L pair, so an execute is its near kernel alone
over every (target leaf, source leaf) pair on a deep tree -- each test reads m2l_pairs == 0 from stats(), a positive ms_near from a
timed execute, and the same bits at p = 3 and p = 13.

  near_field_kernel<GradientQ>            execute_gradient, flags all 0 / all 1 / mixed, quad_k 1, 3, 4, 13 (13: 23 panels per batch)
  near_field_kernel<PressureQ>            execute_pressure
  near_field_kernel<VelocityGradientQ>    execute_velocity_gradient, and |G00 + G11 + G22| of every row within the row's own bound
  near_flow_kernel                        execute_flow(pressure, velocity gradient): the bound, and in every subset of outputs the
                                          bits of the single executes; last_near_f32 2 / 3 / 0
  near_representation_kernel<V, G>        execute_representation: value, gradient, both x sigma, mu, both; quad_k 3 and 13
  direct_field_partial_kernel             Direct.gradient / pressure / velocity_gradient: with no far field the all-pairs sum is the
                                          same sum
  state                                   every execute (each representation instantiation too) repeated with equal bits, an
                                          execute of another quantity in between

Every test prints its worst ratio to the bound (pytest -s); DESIGN.md section 8 tabulates them."""
import itertools

import numpy as np
import pytest

import field_near_cases as F

pytestmark = pytest.mark.gpu

P_RUN = 13
WORST = {}
_PLANS, _VECTORS, _ROWS = {}, {}, {}


def vectors(case):
    if case not in _VECTORS:
        X, names = F.vectors(case)
        X2, _ = F.vectors(case, seed_shift=50)                    # the second layer of the representation: independent seeds
        _VECTORS[case] = (X, X2, names)
    return _VECTORS[case]


def plan_of(fb, case, K=None, flagname=None):
    """the device plan, checked once: no M2L pair, every panel in every row's near list, the near kernel timed"""
    key = (case, K, flagname)
    if key not in _PLANS:
        flags = None if flagname is None else F.flag_sets(case)[flagname]
        plan = F.make_plan(fb, case, K=K, flags=flags)
        st = plan.stats()
        assert st["m2l_pairs"] == 0 and st["p2p_pairs"] > 0, key
        assert np.all(F.plan_layout(plan)["mask"] == 1), key
        _PLANS[key] = plan
    return _PLANS[key]


def timed(plan, call):
    """one timed execute: the near kernel ran, and at the order asked"""
    plan.set_timing(True)
    try:
        out = call()
        st = plan.stats()
    finally:
        plan.set_timing(False)
    assert st["timed_executes"] >= 1 and st["last_p"] == plan.kernel().P and st["ms_near"] > 0 and st["m2l_pairs"] == 0
    return out


def reference(case, K, quantity, flagname, tag, x):
    """(ref, bound) of one input, computed once per process and shared"""
    key = (case, K, quantity, flagname, tag)
    if key not in _ROWS:
        E = F.pairs(case, K)
        t = F.targets(case)[0]
        flags = None if flagname is None else F.flag_sets(case)[flagname]
        mask = np.ones((len(t), len(F.sources(case))))
        ref, S, T = F.row(E, quantity, x, mask, flags)
        bnd = F.bound(quantity, S, T, flags)
        ref.setflags(write=False)
        bnd.setflags(write=False)
        _ROWS[key] = (ref, bnd)
    return _ROWS[key]


FLAGS = {"all0": "0", "all1": "1", "mixed": "mixed"}
KIND = {"normal": "normal", "one entry x 1e8": "one entry x 1e8"}      # every other name is a unit vector


def hold(kernel, got, ref, bnd, what):
    """every row of one result within its bound; the worst ratio, recorded per kernel and kind of input"""
    got = np.asarray(got)
    assert got.shape == ref.shape and np.all(np.isfinite(got)), what
    r = F.ratios(got, ref, bnd)
    i = int(np.argmax(r))
    kind = next(KIND.get(w, "unit") for w in what if isinstance(w, str) and (w in KIND or w.startswith("e_")))
    if r[i] >= WORST.get((kernel, kind), (-1.0, None))[0]:
        WORST[(kernel, kind)] = (float(r[i]), what + (i,))
    assert r[i] <= 1.0, (kernel, what, "row", i, float(r[i]))
    return float(r[i])


def same(a, b, what):
    assert np.array_equal(np.asarray(a), np.asarray(b)), what


def report(kernel, worst):
    print("%s: worst row / bound %.3g" % (kernel, worst))


# ------------------------------------------------------------------ execute_gradient
@pytest.mark.parametrize("K", F.LAPLACE_K)
@pytest.mark.parametrize("case", F.LAPLACE_CASES)
def test_gradient(fb, case, K):
    X, _, names = vectors(case)
    worst = 0.0
    for flagname in ("all0", "all1", "mixed"):
        plan = plan_of(fb, case, K, flagname)
        kern = plan.kernel()
        kern.set_p(P_RUN)
        g0 = timed(plan, lambda: plan.execute_gradient(X[0]))
        for k, name in enumerate(names):
            g = plan.execute_gradient(X[k])
            ref, bnd = reference(case, K, "gradient", flagname, name, X[k])
            worst = max(worst, hold("near_field_kernel<GradientQ>, flags " + FLAGS[flagname], g, ref, bnd, (case, K, flagname, name)))
            if k == 0:
                same(g, g0, "timed")
                plan.execute(X[1])                                # another quantity in between
                same(plan.execute_gradient(X[0]), g0, "repeat")
                kern.set_p(3)                                     # no far field: the same bits at every order
                same(plan.execute_gradient(X[0]), g0, "p = 3")
                kern.set_p(P_RUN)
    report("gradient (%d) K=%d" % (case, K), worst)


# ------------------------------------------------------------------ execute_pressure, execute_velocity_gradient, execute_flow
def _hold_trace(kernel, G, bnd, what):
    """The trace of a row within the row's own bound.  Every quadrature point's tensor is trace-free, so the exact trace is 0; the
    three diagonal sums hold, per point, the terms |s| / r^3 and 3 |s| d_k^2 / r^5 (the f_k d_k terms of the diagonal cancel exactly),
    together 6 |s| / r^3 <= 6 |f|_1 / r^2 -- mu_VG, once for all three: |G00 + G11 + G22| <= (C_VG + T_i) 2^-53 S_i."""
    G = np.asarray(G)
    tr = np.abs(G[:, 0, 0].astype(np.longdouble) + G[:, 1, 1] + G[:, 2, 2]).astype(np.float64)
    r = np.where(bnd > 0, tr / np.where(bnd > 0, bnd, 1.0), np.where(tr > 0, np.inf, 0.0))
    i = int(np.argmax(r))
    kernel = kernel + ", trace"
    kind = next(KIND.get(w, "unit") for w in what if isinstance(w, str) and (w in KIND or w.startswith("e_")))
    if r[i] >= WORST.get((kernel, kind), (-1.0, None))[0]:
        WORST[(kernel, kind)] = (float(r[i]), what + (i,))
    assert r[i] <= 1.0, (kernel, what, "row", i, float(r[i]))
    return float(r[i])


@pytest.mark.parametrize("case", F.STOKES_CASES)
def test_pressure_and_velocity_gradient(fb, case):
    X, _, names = vectors(case)
    plan = plan_of(fb, case)
    kern = plan.kernel()
    kern.set_p(P_RUN)
    q0 = timed(plan, lambda: plan.execute_pressure(X[0]))
    G0 = timed(plan, lambda: plan.execute_velocity_gradient(X[0]))
    wq = wg = wt = 0.0
    for k, name in enumerate(names):
        q, G = plan.execute_pressure(X[k]), plan.execute_velocity_gradient(X[k])
        ref, bnd = reference(case, None, "pressure", None, name, X[k])
        wq = max(wq, hold("near_field_kernel<PressureQ>", q, ref, bnd, (case, name)))
        ref, bnd = reference(case, None, "velocity_gradient", None, name, X[k])
        wg = max(wg, hold("near_field_kernel<VelocityGradientQ>", G, ref, bnd, (case, name)))
        wt = max(wt, _hold_trace("near_field_kernel<VelocityGradientQ>", G, bnd, (case, name)))
    same(plan.execute_pressure(X[0]), q0, "pressure after the gradient")
    plan.execute(X[1].reshape(-1, 3))
    same(plan.execute_velocity_gradient(X[0]), G0, "gradient after the velocity")
    kern.set_p(3)
    same(plan.execute_pressure(X[0]), q0, "p = 3")
    same(plan.execute_velocity_gradient(X[0]), G0, "p = 3")
    kern.set_p(P_RUN)
    report("pressure (%d)" % case, wq)
    report("velocity gradient (%d)" % case, wg)
    report("velocity gradient (%d), trace" % case, wt)


@pytest.mark.parametrize("case", F.STOKES_CASES)
def test_flow(fb, case):
    X, _, names = vectors(case)
    plan = plan_of(fb, case)
    kern = plan.kernel()
    kern.set_p(P_RUN)
    wq = wg = wt = 0.0
    for k, name in enumerate(names):
        x = X[k]
        single = (plan.execute(x.reshape(-1, 3)), plan.execute_pressure(x), plan.execute_velocity_gradient(x))
        for sub in itertools.product((False, True), repeat=3):
            if not any(sub):
                continue
            out = timed(plan, lambda: plan.execute_flow(x, *sub)) if k == 0 else plan.execute_flow(x, *sub)
            assert plan.stats()["last_near_f32"] == (2 if sub[1] and sub[2] else 3 if sub[1] or sub[2] else 0), sub
            for o, s, asked in zip(out, single, sub):
                assert (o is not None) == asked
                if asked:
                    same(o, s, (case, name, sub))
            if sub[1] and sub[2]:                                  # near_flow_kernel: to the bound, not only to the singles
                ref, bnd = reference(case, None, "pressure", None, name, x)
                wq = max(wq, hold("near_flow_kernel (pressure)", out[1], ref, bnd, (case, name, sub)))
                ref, bnd = reference(case, None, "velocity_gradient", None, name, x)
                wg = max(wg, hold("near_flow_kernel (velocity gradient)", out[2], ref, bnd, (case, name, sub)))
                wt = max(wt, _hold_trace("near_flow_kernel (velocity gradient)", out[2], bnd, (case, name, sub)))
        if k == 0:
            kern.set_p(3)
            same(plan.execute_flow(x, False, True, True)[1], single[1], "p = 3")
            same(plan.execute_flow(x, False, True, True)[2], single[2], "p = 3")
            kern.set_p(P_RUN)
    report("flow (%d) pressure" % case, wq)
    report("flow (%d) velocity gradient" % case, wg)
    report("flow (%d) velocity gradient, trace" % case, wt)


# ------------------------------------------------------------------ execute_representation
@pytest.mark.parametrize("K", (3, 13))
@pytest.mark.parametrize("case", F.LAPLACE_CASES)
def test_representation(fb, case, K):
    X, X2, names = vectors(case)
    plan = plan_of(fb, case, K, "mixed")                          # the targets' own flags do not enter
    kern = plan.kernel()
    kern.set_p(P_RUN)
    worst = {}
    first = {}
    ran_timed = False
    for k, name in enumerate(names):
        for layers, (sigma, mu) in (("sigma", (X[k], None)), ("mu", (None, X[k])), ("both", (X[k], X2[k]))):
            refs = {part: reference(case, K, ("representation", part), None, (name, layers), (sigma, mu)) for part in ("value", "gradient")}
            for value, gradient in ((True, False), (False, True), (True, True)):
                kernel = "near_representation_kernel<%s, %s>" % (str(value).lower(), str(gradient).lower())
                call = lambda: plan.execute_representation(sigma, mu, value=value, gradient=gradient)
                phi, grad = call() if ran_timed else timed(plan, call)
                ran_timed = True
                assert (phi is not None) == value and (grad is not None) == gradient
                what = (case, K, name, layers)
                if value:
                    worst[kernel] = max(worst.get(kernel, 0.0), hold(kernel, phi, *refs["value"], what + ("value",)))
                if gradient:
                    worst[kernel] = max(worst.get(kernel, 0.0), hold(kernel, grad, *refs["gradient"], what + ("gradient",)))
                if k == 0 and layers == "both":
                    first[(value, gradient)] = (phi, grad)
    # state, for each of the three instantiations: repeated after an execute of another quantity, and at another order
    sigma, mu = X[0], X2[0]
    for (value, gradient), want in first.items():
        plan.execute_gradient(X[1])
        for p in (P_RUN, 3):
            kern.set_p(p)
            got = plan.execute_representation(sigma, mu, value=value, gradient=gradient)
            for a, b in zip(got, want):
                assert (a is None) == (b is None)
                if a is not None:
                    same(a, b, (value, gradient, p))
    kern.set_p(P_RUN)
    for kernel, w in sorted(worst.items()):
        report("%s (%d) K=%d" % (kernel, case, K), w)


# ------------------------------------------------------------------ the Direct sum's field template
@pytest.mark.parametrize("K", (3, 13))
@pytest.mark.parametrize("case", F.LAPLACE_CASES)
def test_direct_gradient(fb, case, K):
    X, _, names = vectors(case)
    t = F.targets(case)[0]
    D = fb.Direct(fb.LaplaceSphericalBEM(P_RUN, K), F.sources(case))
    worst = 0.0
    for flagname, flags in F.flag_sets(case).items():
        for k, name in enumerate(names):
            g = D.gradient(X[k], t, flags)
            ref, bnd = reference(case, K, "gradient", flagname, name, X[k])
            worst = max(worst, hold("direct_field_partial_kernel (gradient), flags " + FLAGS[flagname], g, ref, bnd, (case, K, flagname, name)))
            if k == 0:
                same(D.gradient(X[k], t, flags), g, "repeat")
    D.close()
    report("Direct.gradient (%d) K=%d" % (case, K), worst)


@pytest.mark.parametrize("case", F.STOKES_CASES)
def test_direct_pressure_and_velocity_gradient(fb, case):
    X, _, names = vectors(case)
    t = F.targets(case)[0]
    kern = fb.StokesSphericalBEM(P_RUN, F.N.STOKES_K, F.N.STOKES_MU)
    kern.set_Kfine(F.N.STOKES_KFINE)
    D = fb.Direct(kern, F.sources(case))
    wq = wg = wt = 0.0
    for k, name in enumerate(names):
        x = X[k].reshape(-1, 3)
        q, G = D.pressure(x, t), D.velocity_gradient(x, t)
        ref, bnd = reference(case, None, "pressure", None, name, X[k])
        wq = max(wq, hold("direct_field_partial_kernel (pressure)", q, ref, bnd, (case, name)))
        ref, bnd = reference(case, None, "velocity_gradient", None, name, X[k])
        wg = max(wg, hold("direct_field_partial_kernel (velocity gradient)", G, ref, bnd, (case, name)))
        wt = max(wt, _hold_trace("direct_field_partial_kernel (velocity gradient)", G, bnd, (case, name)))
        if k == 0:
            same(D.pressure(x, t), q, "repeat")
            same(D.velocity_gradient(x, t), G, "repeat")
    D.close()
    report("Direct.pressure (%d)" % case, wq)
    report("Direct.velocity_gradient (%d)" % case, wg)
    report("Direct.velocity_gradient (%d), trace" % case, wt)


def test_zz_worst_ratio_per_kernel():
    """the table of DESIGN.md section 8 (pytest -s); the tests above have asserted every figure"""
    for (kernel, kind), (w, where) in sorted(WORST.items()):
        print("%-52s %-16s %.3g  %s" % (kernel, kind, w, where))
        assert w <= 1.0
