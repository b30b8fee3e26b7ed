"""The field Hessian (fmmbem_plan_execute_hessian), host side: the entry formula against central differences of the gradient's entry,
the long-double Hessian of a local expansion against differences of its gradient, the composed reference's convergence, what a
double-precision evaluation by the device's route loses on the axis of a leaf, and the refusals of the C ABI.  No device needed."""
import ctypes
import inspect
import math

import numpy as np
import pytest

import double_layer_reference as D
import field_gradient_reference as G
import field_hessian_reference as H
import field_velocity_gradient_reference as V
from oracle import oracle as O
from test_field_velocity_gradient_host import derived_coefficients, idx, leaf_of

LD, CLD = D.LD, D.CLD


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# ---- (a) eta ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["k_point", "sixteen_point"])
def test_eta_is_the_derivative_of_gamma(regime):
    """Central differences, h = 1e-5, of field_gradient_reference.gamma -- the step and the bound, 1e-8 of the largest entry, are
    those of test_field_gradient_host.py for gamma against the potentials -- on pairs whose regime is the same at t and at t +- h e.
    K-point regime: unit_sphere(3), targets at 1.6 .. 2.6 from the centre.  16-point regime: unit_sphere(2), targets 1.0 .. 1.8
    sqrt(2 A) above a panel's centroid (sqrt(2 A) / dist between 0.55 and 1), the pairs of that target in the near regime.  The
    differences' own accuracy: truncation h^2 / 6 times the ratio of the third derivative of gamma to its first, ~ 20 / r^2: 2e-10 at
    r >= 0.6 and 1.5e-9 at r >= 0.45, the nearest 16-point node of the near pairs; rounding 1e-16 |gamma| / h ~ 1e-11 r |eta|.
    Also: eta is symmetric and trace-free to rounding."""
    h = 1e-5
    rng = np.random.default_rng(2)
    if regime == "k_point":
        v = O.unit_sphere(3)
        g = G.geometry(v)
        ts = G._dirs(rng, 8) * (1.6 + rng.random(8))[:, None]
    else:
        v = O.unit_sphere(2)
        g = G.geometry(v)
        pick = rng.choice(len(v), 8, replace=False)
        ts = g["center"][pick] + g["normal"][pick] * ((1.0 + 0.8 * rng.random(8)) * np.sqrt(2 * g["area"][pick]))[:, None]
    for flag in (0, 1):
        worst, top, pairs, sym, trace = 0.0, 0.0, 0, 0.0, 0.0
        for t in ts:
            def near_of(u):
                return np.sqrt(2 * g["area"]) / np.linalg.norm(u[None] - g["center"], axis=1) >= 0.5
            masks = np.array([near_of(t)] + [near_of(t + s * h * e) for e in np.eye(3) for s in (1, -1)])
            same = np.all(masks == masks[0], axis=0)
            sel = same & (masks[0] if regime == "sixteen_point" else ~masks[0])
            assert sel.sum() >= (1 if regime == "sixteen_point" else 30)
            got = H.eta(t, flag, v, g)
            fd = np.stack([(G.gamma(t + h * e, flag, v, g) - G.gamma(t - h * e, flag, v, g)) / (2 * h) for e in np.eye(3)], axis=2)
            worst, top = max(worst, float(np.abs(got - fd)[sel].max())), max(top, float(np.abs(fd[sel]).max()))
            pairs += int(sel.sum())
            big = np.abs(got).max()
            sym = max(sym, float(np.abs(got - got.transpose(0, 2, 1)).max() / big))
            trace = max(trace, float(np.abs(np.trace(got, axis1=1, axis2=2)).max() / big))
        print("eta vs central differences of gamma, %s regime, flag %d, %d pairs: %.2e of the largest entry; asymmetry %.1e, trace %.1e"
              % (regime, flag, pairs, worst / top, sym, trace))
        assert worst <= 1e-8 * top, (regime, flag, worst / top)
        assert sym == 0 and trace <= 1e-15


def test_eta_on_the_panel_is_zero():
    v = O.unit_sphere(2)
    g = G.geometry(v)
    for flag in (0, 1):
        e = H.eta(g["center"][5], flag, v, g)
        assert np.all(e[5] == 0) and np.all(np.isfinite(e)) and np.abs(e).max() > 0


# ---- (b) the Hessian of a local expansion -------------------------------------------------------------------------------------
def test_hessian_of_L_against_central_differences_of_its_gradient():
    """field_velocity_gradient_reference.local_gradient_and_hessian against central differences, h = 1e-5 in long double, of
    double_layer_reference.local_value_and_gradient's gradient, p = 8, |x - c| <= 0.45: truncation h^2 / 6 |d^4| ~ 1.7e-11 . 840 /
    0.45^3 of the top degree's size, rounding 1e-19 / h; asserted 1e-7 of sum |L| max |grad grad R|.  Symmetric and trace-free."""
    p, h = 8, LD(1e-5)
    rng = np.random.default_rng(7)
    S = p * (p + 1) // 2
    L = (rng.standard_normal((2, S)) + 1j * rng.standard_normal((2, S))).astype(CLD)
    c = np.array([0.3, -0.2, 0.1])
    x = c[None] + G._dirs(rng, 10) * (0.05 + 0.4 * rng.random(10))[:, None]
    gr, he = V.local_gradient_and_hessian(p, L, c, x)
    assert np.array_equal(gr, D.local_value_and_gradient(p, L, c, x)[1])
    worst = 0.0
    for b in range(3):
        e = np.zeros(3, dtype=LD)
        e[b] = h
        fd = (D.local_value_and_gradient(p, L, c, x.astype(LD) + e)[1] - D.local_value_and_gradient(p, L, c, x.astype(LD) - e)[1]) / (2 * h)
        worst = max(worst, float(np.abs(fd - he[:, :, :, b]).max()))
    top = float(np.abs(he).max())
    print("Hessian of L vs differences of its gradient: %.2e of the largest entry" % (worst / top))
    assert worst <= 1e-7 * top
    assert np.array_equal(he, he.transpose(0, 1, 3, 2))
    assert float(np.abs(np.trace(he, axis1=2, axis2=3)).max()) <= 1e-16 * top


# ---- (c) convergence ----------------------------------------------------------------------------------------------------------
def test_reference_converges_to_the_limit_sum():
    """|reference(p) - limit| / |limit| per flag class falls monotonically over p = 4, 8, 12, 16 on two_r3 (a wrong sign or index of a
    far term does not converge); at p = 1 and p = 2 the far half is nothing"""
    ref = H.reference("two_r3")
    lim = ref.limit()
    for f in (0, 1):
        s = ref.flags == f
        errs = [rel(ref.hessian(p)[s], lim[s]) for p in (4, 8, 12, 16)]
        print("two_r3 flag %d vs limit sum at p = 4, 8, 12, 16: %s" % (f, " ".join("%.1e" % e for e in errs)))
        assert errs[0] > errs[1] > errs[2] > errs[3], (f, errs)
        assert errs[0] < 0.3 and errs[3] < 1e-3, (f, errs)
    for p in (1, 2):
        assert np.all(ref.far_half("x", p) == 0)
    h8 = ref.hessian(8)
    assert np.array_equal(h8, h8.transpose(0, 2, 1))
    assert np.abs(np.trace(h8, axis1=1, axis2=2)).max() <= 1e-13 * max(ref.scale(0), ref.scale(1))


# ---- (d) the device's route in double precision -------------------------------------------------------------------------------
def device_route(p, L, center, x):
    """(N, 3, 3) float64: l2p_hessian_kernel's route restated in numpy -- the derived coefficients of one slot, ONE spherical chain
    along the recurrence of Ynm and YnmTheta with the project's cart2sph (rho = |d| + EPS), sph2cart, the upper triangle mirrored"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    N = len(x)
    out = np.zeros((N, 3, 3))
    if p < 2:
        return out
    W = derived_coefficients(p, np.asarray(L, dtype=np.complex128))                  # (3, S1)
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
    gs = np.zeros((3, 3, N))
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
            Wn = W[:, idx(n, m)][:, None]
            gs[:, 0] += w * (Wn.real * yr - Wn.imag * yi) * (n / rho)
            gs[:, 1] += w * (Wn.real * tr - Wn.imag * ti)
            if m:
                gs[:, 2] += 2 * (-(Wn.real * yi + Wn.imag * yr)) * m
            p1, pc = pc, pnext
            rhon = rhon * rho
        pn = -pn * fact * sa
        fact += 2
        rhom = rhom * rho
        er, ei = er * cb - ei * sb, er * sb + ei * cb
    Hc = np.stack([sa * cb * gs[:, 0] + ca * cb / rho * gs[:, 1] - sb / rho / sa * gs[:, 2],
                   sa * sb * gs[:, 0] + ca * sb / rho * gs[:, 1] + cb / rho / sa * gs[:, 2],
                   ca * gs[:, 0] - sa / rho * gs[:, 1]], axis=1).transpose(2, 0, 1)     # (N, 3 k, 3 m): component m of grad d_k phi
    for a in range(3):
        for b in range(a, 3):
            out[:, a, b] = out[:, b, a] = Hc[:, a, b]
    return out


def test_device_route_in_double():
    """device_route in float64 against the long-double far half, relative to the class scale, on the 16 awkward rows (on the axis or at
    the centre of their leaf) and on every seventh other row at p = 1, 2, 6, 12, 16.  The other rows <= 1e-13, which pins the
    restatement; the awkward rows give the measured on-axis loss, of which field_hessian_reference.ON_AXIS_DEVIATION is 10 x."""
    ref = H.reference("awkward")
    scale = [ref.scale(0), ref.scale(1)]
    rows = np.arange(len(ref.pts) - H.N_AWKWARD, len(ref.pts))
    others = np.arange(0, len(ref.pts) - H.N_AWKWARD, 7)
    worst, trace = {"awkward": 0.0, "others": 0.0}, 0.0
    for p in (1, 2, 6, 12, 16):
        L = ref.base.expansions(ref.x, p)
        for what, sel in (("awkward", rows), ("others", others)):
            for k in sel:
                b, f = leaf_of(ref, k), int(ref.flags[k])
                got = device_route(p, L[b, f], ref.tb["center"][b], ref.pts[k:k + 1])[0]
                want = V.local_gradient_and_hessian(p, L[b, f], ref.tb["center"][b], ref.pts[k:k + 1])[1][0, 0].astype(np.float64)
                assert np.all(np.isfinite(got))
                worst[what] = max(worst[what], float(np.abs(got - want).max() / scale[f]))
                trace = max(trace, float(abs(np.trace(got)) / scale[f]))
        if p <= 2:
            assert worst["awkward"] == 0 and worst["others"] == 0
    print("device route in double vs long double, of the scale: awkward rows %.2e, other rows %.2e; largest |trace| %.2e"
          % (worst["awkward"], worst["others"], trace))
    assert worst["others"] <= 1e-13
    assert worst["awkward"] <= H.ON_AXIS_DEVIATION


# ---- (e) the C ABI ------------------------------------------------------------------------------------------------------------
PLAN_SYMBOLS = ("fmmbem_plan_execute_hessian", "fmmbem_plan_execute_hessian_device", "fmmbem_kernel_hessian_entries")
DIRECT_SYMBOLS = ("fmmbem_direct_hessian", "fmmbem_direct_hessian_device")


def test_symbols_present(fb):
    L = fb.lib()
    for name in PLAN_SYMBOLS + DIRECT_SYMBOLS:
        assert name in fb.SYMBOLS
        assert getattr(L, name).argtypes is not None, name
    assert L.fmmbem_version() == 1
    assert callable(fb.kernel_hessian_entries)
    for name in ("execute_hessian", "execute_hessian_torch", "execute_hessian_device"):
        assert hasattr(fb.FMM_plan, name)
    assert list(inspect.signature(fb.Direct.hessian).parameters)[1:] == ["x", "targets", "target_bc"]
    assert list(inspect.signature(fb.Direct.hessian_torch).parameters)[1:] == ["x", "targets", "target_bc", "out"]


def test_refusals_in_order_and_the_handle_stays_usable(fb):
    L = fb.lib()
    v = fb.unit_sphere(3)
    pts = np.random.default_rng(1).normal(size=(50, 3)) * 2
    K = fb.LaplaceSphericalBEM(5, 3)
    tp = fb.FMM_plan(K, v, host_only=True, targets=pts)
    single = fb.FMM_plan(K, v, host_only=True)
    stokes = fb.FMM_plan(fb.StokesSphericalBEM(5, 3), v, host_only=True).field_plan(pts)
    buf = np.zeros(3 * len(v) + 9 * len(pts))
    bp, null = buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p()
    before = tp.pairs("m2l").copy()
    forms = (lambda h, p, x, g: L.fmmbem_plan_execute_hessian(h, p, x, g),
             lambda h, p, x, g: L.fmmbem_plan_execute_hessian_device(h, p, x, g, null))
    for call in forms:
        assert call(None, 5, bp, bp) == 1                               # 1 null plan
        assert call(tp._h, 5, None, bp) == 1 and call(tp._h, 5, bp, None) == 1
        assert call(single._h, 5, None, bp) == 1                        #   null before everything else
        assert call(tp._h, 0, bp, bp) == 1 and call(tp._h, 6, bp, bp) == 1       # 2 p outside 1..p_max
        assert "p_max" in L.fmmbem_last_error().decode()
        assert call(single._h, 0, bp, bp) == 1 and call(stokes._h, 17, bp, bp) == 1   #   before the kind of plan
        assert call(single._h, 5, bp, bp) == 6                          # 3 not over separate targets
        assert "the field Hessian" in L.fmmbem_last_error().decode() and "separate targets" in L.fmmbem_last_error().decode()
        assert call(stokes._h, 5, bp, bp) == 6                          # 4 a Stokes plan (before host-only)
        assert "the field Hessian" in L.fmmbem_last_error().decode() and "Laplace" in L.fmmbem_last_error().decode()
        assert call(tp._h, 5, bp, bp) == 6                              # 5 host-only, as execute
        assert "host-only" in L.fmmbem_last_error().decode()
    assert np.all(buf == 0)
    for plan, x in ((tp, np.ones(len(v))), (single, np.ones(len(v))), (stokes, np.ones((len(v), 3)))):
        with pytest.raises(fb.FmmBemError) as e:
            plan.execute_hessian(x)
        assert e.value.status == 6
    with pytest.raises(ValueError):
        tp.execute_hessian(np.ones(len(v) + 1))
    # the gradient and the velocity gradient keep their refusals
    with pytest.raises(fb.FmmBemError) as e:
        stokes.execute_gradient(np.ones((len(v), 3)))
    assert e.value.status == 6 and "the field gradient" in str(e.value)
    with pytest.raises(fb.FmmBemError) as e:
        tp.execute_velocity_gradient(np.ones(len(v)))
    assert e.value.status == 6 and "the field velocity gradient" in str(e.value)
    # the handles are still usable
    assert np.array_equal(tp.pairs("m2l"), before)
    assert tp.stats()["n_panels"] == len(v) and tp.target_info()["n_targets"] == 50
    assert single.stats()["n_panels"] == len(v)
    assert stokes.target_info()["n_targets"] == 50


def test_hessian_entries_arguments(fb):
    L = fb.lib()
    o = fb.Options()
    L.fmmbem_options_default(ctypes.byref(o))
    out = np.zeros(9)
    op = out.ctypes.data_as(ctypes.c_void_p)
    f = L.fmmbem_kernel_hessian_entries
    assert f(ctypes.byref(o), 1, None, None, None, None) == 1
    assert f(ctypes.byref(o), 1, op, None, op, None) == 1
    assert f(None, 1, op, None, op, op) == 1
    assert f(ctypes.byref(o), 0, op, None, op, op) == 0
    o.kernel = 1
    assert f(ctypes.byref(o), 1, op, None, op, op) == 6                 # Stokes
    assert "the field Hessian" in L.fmmbem_last_error().decode()
    o.kernel, o.quad_k = 0, 5
    assert f(ctypes.byref(o), 1, op, None, op, op) == 1                 # no such rule
    assert np.all(out == 0)
    with pytest.raises(ValueError):
        fb.kernel_hessian_entries(fb.LaplaceSphericalBEM(5, 3), np.zeros((2, 3, 3)), np.zeros((3, 3, 3)))
    with pytest.raises(ValueError):
        fb.kernel_hessian_entries(fb.LaplaceSphericalBEM(5, 3), np.zeros((2, 3, 3)), np.zeros((2, 3, 3)), target_bc=np.zeros(3, np.uint8))


def test_direct_hessian_arguments(fb, gpu_available):
    """the null checks come first, before any device is touched; without a device a handle cannot be made, and says so"""
    L = fb.lib()
    buf = np.zeros(64)
    bp = buf.ctypes.data_as(ctypes.c_void_p)
    assert L.fmmbem_direct_hessian(None, 4, bp, None, bp, bp) == 1
    assert "null" in L.fmmbem_last_error().decode()
    assert L.fmmbem_direct_hessian_device(None, 4, bp, None, bp, bp, None) == 1
    assert np.all(buf == 0)
    if gpu_available:
        v = fb.unit_sphere(2)
        Dl = fb.Direct(fb.LaplaceSphericalBEM(5, 3), v)
        with pytest.raises(ValueError):
            Dl.hessian(np.ones(len(v) - 1), np.zeros((3, 3)))           # shape errors are ValueError, as in matvec
        with pytest.raises(ValueError):
            Dl.hessian(np.ones(len(v)), None)                           # no symmetric form
        Dl.close()
    else:
        with pytest.raises(fb.FmmBemError) as e:
            fb.Direct(fb.LaplaceSphericalBEM(5, 3), fb.unit_sphere(2))
        assert e.value.status == 2
