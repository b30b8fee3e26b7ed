"""The field velocity gradient (fmmbem_plan_execute_velocity_gradient), host side: the long-double Hessian of the solid harmonics, the
lowering identities the device's far half rests on, the near tensor against differences of the oracle's velocity entries, the composed
reference's convergence, what a double-precision evaluation by the device's route loses on the axis of a leaf, and the refusals of
the C ABI.  No device needed."""
import ctypes
import math

import numpy as np
import pytest

import double_layer_reference as D
import field_gradient_reference as G
import field_plan_reference as R
import field_pressure_reference as Q
import field_velocity_gradient_reference as V
from oracle import oracle as O

LD, CLD = D.LD, D.CLD


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def idx(n, m):
    return n * (n + 1) // 2 + m


def s_factor(n, m):
    """s(n, m) = sqrt((n - |m|)! (n + |m|)!) in long double"""
    return np.sqrt(LD(math.factorial(n - abs(m))) * LD(math.factorial(n + abs(m))))


def derived_coefficients(p, L):
    """(3, S(p - 1)): the coefficients of d_x phi, d_y phi, d_z phi, local expansions of order p - 1, from L (S(p),) of phi, by the
    lowering identities; in L's precision.  The factors are s(n + 1, m') / s(n, m) written out."""
    out = np.zeros((3, (p - 1) * p // 2), dtype=L.dtype)
    real = L.real.dtype.type
    for n in range(p - 1):
        for m in range(n + 1):
            fz = np.sqrt(real((n + 1 - m) * (n + 1 + m)))
            hp = np.sqrt(real((n - m + 1) * (n - m + 2))) / 2
            hm = np.sqrt(real((n + m + 1) * (n + m + 2))) / 2
            Lp = L[idx(n + 1, m + 1)]
            Ll = L[idx(n + 1, m - 1)] if m else -np.conj(Lp)       # L_{n,-1} = -conj L_{n,1}
            dp, dm = hp * Ll, -hm * Lp                             # D+ / 2, D- / 2
            out[0, idx(n, m)] = dp + dm
            out[1, idx(n, m)] = (dp - dm) / 1j
            out[2, idx(n, m)] = fz * L[idx(n + 1, m)]
    return out


# ---- (a) the Hessian ----------------------------------------------------------------------------------------------------------
def test_hessian_against_central_differences_and_traceless():
    """grad grad R of solid_harmonics_hessian against central differences of solid_harmonics' gradient in long double, p = 8,
    |d| <= 0.9, h = 1e-5: truncation h^2 / 6 |d^4 R| <= 1.7e-11 . 840 (n (n-1)(n-2)(n-3) at n = 7) = 1.4e-8, rounding 1e-19 |grad R| /
    h ~ 1e-13; asserted 1e-7 absolute, where the entries reach 8.  The trace: every R_nm is harmonic, to long-double rounding."""
    p, h = 8, LD(1e-5)
    rng = np.random.default_rng(3)
    d = (G._dirs(rng, 12) * (0.1 + 0.8 * rng.random(12))[:, None]).astype(LD)
    Rn, dR, hR = V.solid_harmonics_hessian(p, d)
    R0, dR0 = D.solid_harmonics(p, d)
    assert np.array_equal(Rn, R0) and np.array_equal(dR, dR0)
    worst = 0.0
    for b in range(3):
        e = np.zeros(3, dtype=LD)
        e[b] = h
        fd = (D.solid_harmonics(p, d + e)[1] - D.solid_harmonics(p, d - e)[1]) / (2 * h)      # (S, N, 3): d_b d_a R
        worst = max(worst, float(np.abs(fd - hR[:, :, :, b]).max()))
    top = float(np.abs(hR).max())
    tr = float(np.abs(hR[:, :, 0, 0] + hR[:, :, 1, 1] + hR[:, :, 2, 2]).max())
    print("Hessian vs differences: %.2e absolute (largest entry %.1f); trace %.2e; asymmetry %.2e"
          % (worst, top, tr, float(np.abs(hR - hR.transpose(0, 1, 3, 2)).max())))
    assert top > 1 and worst <= 1e-7
    assert tr <= 1e-16 * top
    assert np.array_equal(hR, hR.transpose(0, 1, 3, 2))


# ---- (b) the lowering identities ---------------------------------------------------------------------------------------------
def test_lowering_identities_of_the_basis():
    """With Q_nm = R_nm / s(n, m), Q_{n,-m} = (-1)^m conj Q_nm:  d_z Q_n^m = Q_{n-1}^m,  (d_x + i d_y) Q_n^m = Q_{n-1}^{m+1},
    (d_x - i d_y) Q_n^m = -Q_{n-1}^{m-1}; in long double to 1e-17 of the largest term"""
    p = 12
    rng = np.random.default_rng(5)
    d = (G._dirs(rng, 8) * (0.2 + 0.7 * rng.random(8))[:, None]).astype(LD)
    Rn, dR = D.solid_harmonics(p, d)

    def Qf(n, m):
        if n < 0 or abs(m) > n:
            return np.zeros(len(d), dtype=CLD)
        q = Rn[idx(n, abs(m))] / s_factor(n, m)
        return q if m >= 0 else (-1) ** m * np.conj(q)

    def dQ(n, m):
        g = dR[idx(n, abs(m))] / s_factor(n, m)
        return g if m >= 0 else (-1) ** m * np.conj(g)

    worst = 0.0
    for n in range(1, p):
        for m in range(-n, n + 1):
            g = dQ(n, m)
            top = float(np.abs(g).max()) + 1e-300
            worst = max(worst, float(np.abs(g[:, 2] - Qf(n - 1, m)).max()) / top,
                        float(np.abs(g[:, 0] + CLD(1j) * g[:, 1] - Qf(n - 1, m + 1)).max()) / top,
                        float(np.abs(g[:, 0] - CLD(1j) * g[:, 1] + Qf(n - 1, m - 1)).max()) / top)
    print("lowering identities, n < %d: %.2e of the gradient" % (p, worst))
    assert worst <= 1e-17


@pytest.mark.parametrize("p", [1, 2, 6, 12, 16])
def test_coefficient_space_gradient(p):
    """the value of the three derived expansions of order p - 1 is the gradient of the expansion of order p
    (double_layer_reference.local_value_and_gradient), in long double to 1e-17 of sum |L| |grad R|; at p = 1 there is no term"""
    rng = np.random.default_rng(p)
    S = p * (p + 1) // 2
    L = (rng.standard_normal(S) + 1j * rng.standard_normal(S)).astype(CLD)
    for n in range(p):
        L[idx(n, 0)] = L[idx(n, 0)].real                   # the project's L_n0 is real in effect: only Re(L_n0 R_n0) enters
    x = G._dirs(rng, 9) * (0.05 + 0.5 * rng.random(9))[:, None]
    c = np.zeros(3)
    _, gr = D.local_value_and_gradient(p, L[None], c, x)
    dc = derived_coefficients(p, L)
    assert dc.shape == (3, (p - 1) * p // 2)
    if p == 1:
        assert np.all(gr == 0)
        return
    val, _ = D.local_value_and_gradient(p - 1, dc, c, x)
    _, dR = D.solid_harmonics(p, D.placed(x))
    top = float(np.einsum("s,sn->n", np.abs(L), np.linalg.norm(np.abs(dR), axis=2)).max())
    err = float(np.abs(val.T - gr[0]).max()) / top
    print("p = %d: derived coefficients vs the gradient: %.2e" % (p, err))
    assert err <= 1e-17
    # once more: the gradient of the derived expansions is the Hessian
    _, g2 = D.local_value_and_gradient(p - 1, dc, c, x)
    _, he = V.local_gradient_and_hessian(p, L[None], c, x)
    assert float(np.abs(g2.transpose(1, 0, 2) - he[0]).max()) <= 1e-16 * float(np.abs(he).max() + top)


# ---- (c) the near tensor ------------------------------------------------------------------------------------------------------
def test_gamma_entry_is_the_gradient_of_the_oracles_velocity_entries():
    """Gamma[k][m][e] = d_m U[k][e] for single pairs: U the oracle's velocity entries (Probes.entries, with their 1/(2 mu)), by
    central differences with step h at targets that keep their regime within h -- far-regime pairs at 1.6 .. 2.6 from the centre of
    unit_sphere(3) with h = 1e-3, near-regime pairs 0.5 .. 1.2 sqrt(2 A) above their panel (sqrt(2 A) / dist between 0.8 and 2) with
    h = 1e-4.  The differences' own accuracy: truncation h^2 / 6 times the ratio of the third to the first derivatives (~ 15 / r^2):
    ~ 1e-6 in the far regime (r >= 0.6) and ~ 1e-9 . 15 / 0.1^2 ~ 1e-7 in the near regime against the nearest fine-rule points.
    Measured disagreement: 1.21e-06 (far) and 7.24e-08 (near) of the largest |Gamma| of the pairs; asserted: 10 x that.  This pins
    the sign, the index order [k][m] and the 1/(2 mu) against the velocity the library returns, with none of the library's code."""
    v = O.unit_sphere(3)
    g = Q.geometry(v)
    rng = np.random.default_rng(12)
    T = 6
    steps0 = np.concatenate([np.zeros((1, 3)), np.eye(3), -np.eye(3)])                  # centre, +x +y +z, -x -y -z
    measured = {"far": 1.21e-06, "near": 7.24e-08}
    for regime, h in (("far", 1e-3), ("near", 1e-4)):
        if regime == "far":
            t0 = G._dirs(rng, T) * (1.6 + rng.random(T))[:, None]
            chosen = None
        else:
            chosen = rng.integers(0, len(v), T)
            nrm = g["center"][chosen] / np.linalg.norm(g["center"][chosen], axis=1)[:, None]
            t0 = g["center"][chosen] + nrm * ((0.5 + 0.7 * rng.random(T)) * np.sqrt(2 * g["area"][chosen]))[:, None]
        pts = (t0[:, None, :] + h * steps0[None, :, :]).reshape(-1, 3)
        probes = R.Probes(v, pts, np.zeros(len(pts), np.uint8))
        placed = probes.centres.reshape(T, 7, 3)
        worst, top, pairs = 0.0, 0.0, 0
        for a in range(T):
            masks = np.array([Q.regimes(placed[a, k], g)[1] for k in range(7)])        # (7, panels): the near regime
            same = np.all(masks == masks[0], axis=0)                                   # the regime does not change within h
            src = np.nonzero(same & (masks[0] if regime == "near" else ~masks[0]))[0][:40]
            if regime == "near":
                assert chosen[a] in src
            else:
                assert len(src) == 40
            E = probes.entries(np.arange(7 * a, 7 * a + 7), src)                       # (7, src, 3, 3) [k][e]
            fd = np.stack([(E[1 + m] - E[4 + m]) / (2 * h) for m in range(3)], axis=2)  # (src, 3, 3, 3) [k][m][e]
            want = V.gamma_entry(placed[a, 0], v[src], Q.sub(g, src))
            worst = max(worst, float(np.abs(fd - want).max()))
            top = max(top, float(np.abs(want).max()))
            pairs += len(src)
        probes.close()
        print("gamma_entry vs differences of the oracle's velocity entries, %d %s-regime pairs, h = %g: %.2e of the largest |Gamma|"
              % (pairs, regime, h, worst / top))
        assert worst <= 10 * measured[regime] * top, (regime, worst / top)


def test_gamma_entry_is_trace_free_and_not_symmetric():
    v = O.unit_sphere(2)
    g = Q.geometry(v)
    t = np.array([0.3, -1.4, 0.9])
    e = V.gamma_entry(t, v, g)
    assert np.abs(np.einsum("pkke->pe", e)).max() <= 1e-15 * np.abs(e).max()
    assert np.abs(e - e.transpose(0, 2, 1, 3)).max() > 0.1 * np.abs(e).max()


# ---- (d) convergence ----------------------------------------------------------------------------------------------------------
def test_reference_converges_to_the_limit_sum():
    """|reference(p) - limit| / |limit| falls monotonically over p = 4, 8, 12, 16 (a wrong sign of a far term does not converge)"""
    for name in ("two_r3", "far_only"):
        ref = V.reference(name)
        lim = ref.limit()
        errs = [rel(ref.gradient(p), lim) for p in (4, 8, 12, 16)]
        print("%s vs limit sum at p = 4, 8, 12, 16: %s" % (name, " ".join("%.1e" % e for e in errs)))
        assert errs[0] > errs[1] > errs[2] > errs[3], (name, errs)
        assert errs[0] < 0.3, (name, errs)
        tr = np.abs(np.trace(ref.gradient(8), axis1=1, axis2=2)).max()
        assert tr <= 1e-13 * ref.scale(), tr / ref.scale()


# ---- (e) the device's route in double precision ------------------------------------------------------------------------------
def device_route(p, L4, center, x, mu=R.MU):
    """(N, 3, 3) float64: l2p_velgrad_kernel's route restated in numpy -- the derived coefficients, ONE spherical chain along the
    recurrence of Ynm and YnmTheta with the project's cart2sph (rho = |d| + EPS), sph2cart"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    N = len(x)
    out = np.zeros((N, 3, 3))
    if p < 2:
        return out
    c = np.stack([derived_coefficients(p, np.asarray(L4[e], dtype=np.complex128)) for e in range(4)])     # (4, 3, S1) [slot][x y z]
    d = x - np.asarray(center, dtype=np.float64)
    rho = np.sqrt((d * d).sum(1)) + D.EPS
    ca = d[:, 2] / rho
    sa = np.sqrt((1.0 - ca) * (1.0 + ca))
    ax, ay = np.abs(d[:, 0]), np.abs(d[:, 1])
    axis, on_y = ax + ay < D.EPS, ax < D.EPS
    with np.errstate(divide="ignore", invalid="ignore"):
        h = 1.0 / np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2)
        cb = np.where(axis, 1.0, np.where(on_y, 0.0, d[:, 0] * h))
        sb = np.where(axis, 0.0, np.where(on_y, np.where(d[:, 1] > 0, 1.0, -1.0), d[:, 1] * h))
    W = c[3][:, :, None] - np.einsum("ne,eks->ksn", x, c[0:3])                       # (3, S1, N)
    A = np.stack([c[0, 1] - c[1, 0], c[0, 2] - c[2, 0], c[1, 2] - c[2, 1]])          # (3, S1): A_01, A_02, A_12
    gs, av = np.zeros((3, 3, N)), np.zeros((3, N))
    pn, rhom, er, ei, fact = np.ones(N), np.ones(N), np.ones(N), np.zeros(N), 1.0
    for m in range(p - 1):
        pc, p1, rhon = pn.copy(), pn.copy(), rhom.copy()
        w = 1.0 if m == 0 else 2.0
        for n in range(m, p - 1):
            pref = math.sqrt(math.factorial(n - m) / math.factorial(n + m))
            rk = 1.0 / (n - m + 1)
            c1, c2 = (2 * m + 1.0, 0.0) if n == m else ((2 * n + 1) * rk, (n + m) * rk)
            mag = rhon * pc * pref
            yr, yi = mag * er, mag * ei
            pnext = c1 * ca * pc - c2 * p1
            tmag = rhon * ((n - m + 1) * pnext - (n + 1) * ca * pc) / sa * pref
            tr, ti = tmag * er, tmag * ei
            Wn = W[:, idx(n, m)]
            gs[:, 0] += w * (Wn.real * yr - Wn.imag * yi) * (n / rho)
            gs[:, 1] += w * (Wn.real * tr - Wn.imag * ti)
            if m:
                gs[:, 2] += 2 * (-(Wn.real * yi + Wn.imag * yr)) * m
            An = A[:, idx(n, m)]
            av += w * (An.real[:, None] * yr[None] - An.imag[:, None] * yi[None])
            p1, pc = pc, pnext
            rhon = rhon * rho
        pn = -pn * fact * sa
        fact += 2
        rhom = rhom * rho
        er, ei = er * cb - ei * sb, er * sb + ei * cb
    H = np.stack([sa * cb * gs[:, 0] + ca * cb / rho * gs[:, 1] - sb / rho / sa * gs[:, 2],
                  sa * sb * gs[:, 0] + ca * sb / rho * gs[:, 1] + cb / rho / sa * gs[:, 2],
                  ca * gs[:, 0] - sa / rho * gs[:, 1]], axis=1)                        # (3 k, 3 m, N)
    out = H.transpose(2, 0, 1).copy()
    out[:, 0, 1] += av[0]; out[:, 1, 0] -= av[0]
    out[:, 0, 2] += av[1]; out[:, 2, 0] -= av[1]
    out[:, 1, 2] += av[2]; out[:, 2, 1] -= av[2]
    return out / (2 * mu)


def leaf_of(ref, k):
    """the target leaf that holds given target k"""
    leaves = np.nonzero(ref.tb["leaf"])[0]
    pos = np.empty(len(ref.tree), dtype=np.int64)
    pos[ref.tree] = np.arange(len(ref.tree))
    at = pos[ref.given[k]]
    b = leaves[(ref.tb["bb"][leaves] <= at) & (at < ref.tb["be"][leaves])]
    assert len(b) == 1
    return int(b[0])


def test_device_route_in_double_on_the_awkward_rows():
    """The 16 awkward rows (on the axis or at the centre of their leaf) at p = 1, 6, 12, 16: device_route in float64 against the
    long-double far half, relative to the case's scale.  Measured worst: see ON_AXIS_DEVIATION, set at 10 x it.  On the rows of
    random position the same comparison gives rounding level, which pins the restatement itself."""
    ref = V.reference("awkward")
    scale = ref.scale()
    rows = np.arange(len(ref.pts) - V.N_AWKWARD, len(ref.pts))
    others = np.arange(0, len(ref.pts) - V.N_AWKWARD, 7)
    worst, trace = {"awkward": 0.0, "others": 0.0}, 0.0
    for p in (1, 6, 12, 16):
        L = ref.base.far_half("x", p)[2]
        for what, sel in (("awkward", rows), ("others", others)):
            for k in sel:
                b = leaf_of(ref, k)
                got = device_route(p, L[b], ref.tb["center"][b], ref.pts[k:k + 1])[0]
                want = V.far_rows_long(p, L[b], ref.tb["center"][b], ref.pts[k:k + 1])[0].astype(np.float64)
                assert np.all(np.isfinite(got))
                worst[what] = max(worst[what], float(np.abs(got - want).max() / scale))
                trace = max(trace, float(abs(np.trace(got)) / scale))
        if p == 1:
            assert worst["awkward"] == 0 and worst["others"] == 0
    print("device route in double vs long double, of the scale: awkward rows %.2e, other rows %.2e; largest |trace| %.2e"
          % (worst["awkward"], worst["others"], trace))
    assert worst["others"] <= 1e-13
    assert worst["awkward"] <= V.ON_AXIS_DEVIATION


# ---- (f) the C ABI ------------------------------------------------------------------------------------------------------------
def test_symbols_present(fb):
    L = fb.lib()
    for name in ("fmmbem_plan_execute_velocity_gradient", "fmmbem_plan_execute_velocity_gradient_device",
                 "fmmbem_kernel_velocity_gradient_entries"):
        assert name in fb.SYMBOLS
        getattr(L, name)
    assert L.fmmbem_version() == 1
    assert callable(fb.kernel_velocity_gradient_entries)
    for name in ("execute_velocity_gradient", "execute_velocity_gradient_torch", "execute_velocity_gradient_device", "execute_stress"):
        assert hasattr(fb.FMM_plan, name)


def test_refusals_in_order_and_the_handle_stays_usable(fb):
    L = fb.lib()
    v = fb.unit_sphere(3)
    pts = np.random.default_rng(1).normal(size=(50, 3)) * 2
    KS, KL = fb.StokesSphericalBEM(5, 3), fb.LaplaceSphericalBEM(5, 3)
    tp = fb.FMM_plan(KS, v, host_only=True).field_plan(pts)
    single = fb.FMM_plan(KS, v, host_only=True)
    laplace = fb.FMM_plan(KL, v, host_only=True).field_plan(pts)
    flags = np.zeros(50, np.uint8)
    flags[7] = 1
    traction = fb.FMM_plan(KS, v, host_only=True).field_plan(pts, flags)
    buf = np.zeros(3 * len(v) + 9 * len(pts))
    bp, null = buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p()
    before = tp.pairs("m2l").copy()
    forms = (lambda h, p, x, q: L.fmmbem_plan_execute_velocity_gradient(h, p, x, q),
             lambda h, p, x, q: L.fmmbem_plan_execute_velocity_gradient_device(h, p, x, q, null))
    for call in forms:
        assert call(None, 5, bp, bp) == 1                               # 1 null plan
        assert call(tp._h, 5, None, bp) == 1 and call(tp._h, 5, bp, None) == 1
        assert call(single._h, 5, None, bp) == 1                        #   null before everything else
        assert call(tp._h, 0, bp, bp) == 1 and call(tp._h, 6, bp, bp) == 1       # 2 p outside 1..p_max
        assert "p_max" in L.fmmbem_last_error().decode()
        assert call(single._h, 0, bp, bp) == 1 and call(laplace._h, 17, bp, bp) == 1 and call(traction._h, 0, bp, bp) == 1   #   before the kind of plan
        assert call(single._h, 5, bp, bp) == 6                          # 3 not over separate targets
        assert "separate targets" in L.fmmbem_last_error().decode()
        assert call(laplace._h, 5, bp, bp) == 6                         # 4 a Laplace plan
        assert "Stokes" in L.fmmbem_last_error().decode()
        assert call(traction._h, 5, bp, bp) == 6                        # 5 a TRACTION target (before host-only)
        assert "VELOCITY" in L.fmmbem_last_error().decode()
        assert call(tp._h, 5, bp, bp) == 6                              # 6 host-only, as execute
        assert "host-only" in L.fmmbem_last_error().decode()
    assert np.all(buf == 0)
    for plan, x in ((tp, np.ones((len(v), 3))), (single, np.ones(3 * len(v))), (laplace, np.ones(len(v))), (traction, np.ones((len(v), 3)))):
        for method in (plan.execute_velocity_gradient, plan.execute_stress):
            with pytest.raises(fb.FmmBemError) as e:
                method(x)
            assert e.value.status == 6
    for bad in (np.ones(len(v)), np.ones(3 * len(v) + 1), np.ones((len(v), 2)), np.ones((3, len(v)))):
        with pytest.raises(ValueError):
            tp.execute_velocity_gradient(bad)
    # the gradient of the Laplace field goes on refusing Stokes plans
    with pytest.raises(fb.FmmBemError) as e:
        tp.execute_gradient(np.ones((len(v), 3)))
    assert e.value.status == 6
    # the handles are still usable
    assert np.array_equal(tp.pairs("m2l"), before)
    assert tp.stats()["n_panels"] == len(v) and tp.target_info()["n_targets"] == 50
    assert single.stats()["n_panels"] == len(v)
    assert laplace.target_info()["n_targets"] == 50 and traction.target_info()["n_targets"] == 50


def test_velocity_gradient_entries_arguments(fb):
    L = fb.lib()
    o = fb.Options()
    L.fmmbem_options_default(ctypes.byref(o))
    o.kernel = 1
    out = np.zeros(27)
    op = out.ctypes.data_as(ctypes.c_void_p)
    f = L.fmmbem_kernel_velocity_gradient_entries
    assert f(ctypes.byref(o), 1, None, None, None) == 1
    assert f(ctypes.byref(o), 1, op, op, None) == 1
    assert f(None, 1, op, op, op) == 1
    assert f(ctypes.byref(o), 0, op, op, op) == 0
    o.kernel = 0
    assert f(ctypes.byref(o), 1, op, op, op) == 6             # Laplace
    o.kernel, o.quad_k = 1, 5
    assert f(ctypes.byref(o), 1, op, op, op) == 1             # no such rule
    o.quad_k, o.quad_k_fine = 4, 5
    assert f(ctypes.byref(o), 1, op, op, op) == 1             # no such fine rule
    assert np.all(out == 0)
    with pytest.raises(ValueError):
        fb.kernel_velocity_gradient_entries(fb.StokesSphericalBEM(5, 3), np.zeros((2, 3, 3)), np.zeros((3, 3, 3)))
