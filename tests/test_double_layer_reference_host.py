"""CPU pins of tests/double_layer_reference.py, the reference the GPU tests hold the Stokes double layer's far field to
(tests/test_gpu_stokes_double_layer.py).  They tell a wrong reference from a wrong kernel before any device run:

(a) the gradient moments against the oracle's Laplace P2M (NORMAL_DERIV panels: n.G; POTENTIAL panels: the values);
(b) the local value and gradient against the oracle's L2P;
(c) the whole chain P2M -> M2M -> M2L -> L2L -> rows against the stresslet sum over the same quadrature points, tight;
(d) the composition on a real plan's lists: its VELOCITY rows are field_plan_reference.composed_reference's;
(e) what the oracle's own double-precision spherical chain loses on the axis of a box, measured.

No device needed: host-only plans supply the lists."""
import numpy as np
import pytest

import double_layer_reference as D
import field_plan_reference as R
from test_field_plan_host import host_opts

ORDERS = (1, 6, 12, 16)
ABOUT = np.array([0.3, -0.2, 0.1])


def m0_real(L, p):
    """a local expansion's m = 0 coefficients are real"""
    k = [n * (n + 1) // 2 for n in range(p)]
    L[..., k] = L[..., k].real
    return L


def degree_of(p):
    return np.array([n for n in range(p) for m in range(n + 1)])


# ---- (a) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 4, 7])
def test_gradient_moments_are_the_oracles_normal_derivative_moments(oracle_mod, k):
    """n.G summed with unit charge is the oracle's P2M of NORMAL_DERIV panels, and the basis itself the P2M of POTENTIAL panels, to
    1e-13 of the largest coefficient; and degree by degree to 1e-12 of the degree's largest coefficient (the oracle's recurrences
    take at most 16 steps of a few roundings each in double: 16 * 16 * 2^-53 = 3e-14), so a slip at high degree cannot hide behind
    the low degrees.  Random triangles: the normals cover all directions, every Cartesian component of G enters."""
    rng = np.random.default_rng(3 + k)
    v = ABOUT + 0.3 * (rng.random((20, 1, 3)) - 0.5) + 0.08 * rng.normal(size=(20, 3, 3))
    o = oracle_mod.Oracle(v, K=k)
    pan = o.panels()
    o.close()
    assert np.all(np.abs(pan["normal"]).min(axis=0) < 0.5) and np.all(np.abs(pan["normal"]).max(axis=0) > 0.8)
    for axis in range(3):
        assert (pan["normal"][:, axis] > 0.3).any() and (pan["normal"][:, axis] < -0.3).any()
    w = oracle_mod.quadrature(k)[1]
    wA = (w[None, :] * pan["area"][:, None]).reshape(-1).astype(D.LD)
    nq = np.repeat(pan["normal"], len(w), axis=0).astype(D.LD)
    for p in ORDERS:
        b, G = D.basis_and_gradient(p, pan["quad"].reshape(-1, 3), ABOUT)
        assert G.shape == (20 * len(w), 3, p * (p + 1) // 2)
        assert np.array_equal(G, D.grad_moments(p, pan["quad"].reshape(-1, 3), ABOUT))
        val = np.einsum("q,qs->s", wA, b).astype(np.complex128)
        der = np.einsum("q,qk,qks->s", wA, nq, G).astype(np.complex128)
        M0 = oracle_mod.single_p2m(0, p, k, v, None, np.ones(20), ABOUT)[0]
        M1 = oracle_mod.single_p2m(0, p, k, v, np.ones(20, np.uint8), np.ones(20), ABOUT)[1]
        assert np.abs(val - M0).max() <= 1e-13 * np.abs(M0).max(), (k, p)
        assert np.abs(der - M1).max() <= 1e-13 * np.abs(M1).max(), (k, p)
        deg = degree_of(p)
        for n in range(p):
            s = deg == n
            assert np.abs(val[s] - M0[s]).max() <= 1e-12 * np.abs(M0[s]).max(), (k, p, n)
            assert np.abs(der[s] - M1[s]).max() <= 1e-12 * np.abs(M1[s]).max(), (k, p, n)
        if p > 1:
            assert np.abs(M1).max() > 0
        else:
            assert np.all(der == 0) and np.all(M1 == 0)        # the gradient of a constant


# ---- (b) -------------------------------------------------------------------------------------------------------------------------
def plane_probes(rng, m):
    """one-point-rule triangles of size about 0.1 in the three coordinate planes: their normals are exactly +-e_x, +-e_y, +-e_z"""
    tri = []
    for k in range(m):
        axis = k % 3
        t = 0.1 * (rng.random((3, 3)) - 0.5)
        t[:, axis] = 0.0
        tri.append(ABOUT + 0.3 * (rng.random(3) - 0.5) + t)
    return np.array(tri)


@pytest.mark.parametrize("p", ORDERS)
def test_local_value_and_gradient_are_the_oracles_l2p(oracle_mod, p):
    """The oracle's Laplace L2P gives VALUES only -- a POTENTIAL probe reads +(first expansion), a NORMAL_DERIV probe -(second
    expansion), the sign orc_l2p_panel documents; the normal derivative of that operator sits in the source's moments -- so the
    values are pinned to it with both flags, and the gradient to the one oracle operator that differentiates a local expansion,
    the Stokes L2P: u = (phi_k - x_e d_k phi_e + d_k phi_3) / (2 mu) with one potential live at a time is d phi_3 (every Cartesian
    component) and phi e_e - x_e d phi.  n.grad at the probes is the component along the plane's axis.  1e-13 of max."""
    rng = np.random.default_rng(11 + p)
    S = p * (p + 1) // 2
    tri = plane_probes(rng, 12)
    o = oracle_mod.Oracle(tri, K=1)
    pan = o.panels()
    o.close()
    ctr, nrm = pan["center"], pan["normal"]
    assert np.all(np.sort(np.abs(nrm), axis=1) == np.array([0.0, 0.0, 1.0]))
    L = m0_real(rng.normal(size=(4, S)) + 1j * rng.normal(size=(4, S)), p)
    val, grad = D.local_value_and_gradient(p, L, ABOUT, ctr)
    assert val.shape == (4, 12) and grad.shape == (4, 12, 3)
    pot = oracle_mod.single_l2p(0, p, 1, L[:2], ABOUT, tri, None)
    dn = oracle_mod.single_l2p(0, p, 1, L[:2], ABOUT, tri, np.ones(12, np.uint8))
    scale = np.abs(val[:2]).max()
    assert np.abs(pot - val[0]).max() <= 1e-13 * scale and np.abs(dn + val[1]).max() <= 1e-13 * scale
    mu = 0.5
    for e in range(4):
        Le = np.zeros_like(L)
        Le[e] = L[e]
        u = oracle_mod.single_l2p(1, p, 1, Le, ABOUT, tri, None, mu=mu).reshape(-1, 3)
        if e == 3:
            want = grad[3]
        else:
            want = -ctr[:, e:e + 1] * grad[e]
            want[:, e] += val[e]
        want = (want / (2 * mu)).astype(np.float64)
        assert np.abs(u - want).max() <= 1e-13 * max(np.abs(want).max(), 1e-300), (p, e)
        if e == 3 and p > 1:
            ndn = np.einsum("ni,ni->n", nrm, u)
            assert np.abs(ndn - np.einsum("ni,ni->n", nrm, want)).max() <= 1e-13 * np.abs(want).max()
            assert np.abs(ndn).max() > 0.01 * np.abs(want).max()
    allu = oracle_mod.single_l2p(1, p, 1, L, ABOUT, tri, None, mu=mu).reshape(-1, 3)
    mine = D.velocity_rows_long(p, L, ABOUT, ctr, mu=mu).astype(np.float64)
    assert np.abs(allu - mine).max() <= 1e-13 * np.abs(mine).max()


# ---- (c) -------------------------------------------------------------------------------------------------------------------------
def two_clusters(rng):
    """12 source panels within 0.05 of a child centre whose parent centre is 0.03 away; 10 targets within 0.05 of a target child
    centre, 0.03 from its parent; the parents (2.0, 0.7, -0.4) apart; the whole about (0.3, -0.2, 0.1)"""
    def offset(r):
        d = rng.normal(size=3)
        return r * d / np.linalg.norm(d)
    s_par = ABOUT.copy()
    s_child = s_par + offset(0.03)
    t_par = s_par + np.array([2.0, 0.7, -0.4])
    t_child = t_par + offset(0.03)
    v = s_child + np.array([offset(0.03 * rng.random()) for _ in range(12)])[:, None, :] + np.array(
        [[offset(0.02 * rng.random()) for _ in range(3)] for _ in range(12)])
    pts = t_child + np.array([offset(0.05 * rng.random() ** (1 / 3)) for _ in range(10)])
    assert np.linalg.norm(v - s_child, axis=2).max() < 0.05 and np.linalg.norm(pts - t_child, axis=1).max() < 0.05
    return s_par, s_child, t_par, t_child, np.ascontiguousarray(v), pts


def chain_rows(oracle_mod, p, geometry, probes, pan, g, direct):
    s_par, s_child, t_par, t_child, v, pts = geometry
    T = oracle_mod.Tables(p)
    M = D.dipole_slots(p, pan["quad"][:12], D.weights(), pan["area"][:12], pan["normal"][:12], g, s_child)
    if direct:
        L = np.array([T.m2l(M[s], t_child - s_child) for s in range(7)])
    else:
        Mp = np.array([T.m2m(M[s], s_par - s_child) for s in range(7)])
        Lp = np.array([T.m2l(Mp[s], t_par - s_par) for s in range(7)])
        L = np.array([T.l2l(Lp[s], t_child - t_par) for s in range(7)])
    return D.traction_rows(p, L, t_child, probes.centres)


def test_the_chain_is_the_stresslet_sum(oracle_mod):
    """P2M(child) -> M2M -> M2L -> L2L -> rows at p = 12, and the direct M2L child to child, against
    sum_q -3 w A (d.n) d_i (d.g) / r^5 over the same quadrature points: the oracle's TRACTION entries in their far branch
    (asserted by distance).  1e-10 of the largest row: truncation is (0.08 / 2.16)^12 p^2 = 4e-12, the rest the cancellation of
    x_k d_i Psi_k against d_i Psi_0.  The same chain at p = 6 misses by more than 1e-8: the check is sensitive."""
    rng = np.random.default_rng(17)
    geometry = two_clusters(rng)
    v, pts = geometry[4], geometry[5]
    probes = R.Probes(v, pts, np.ones(10, np.uint8))
    pan = probes.ctx.panels()
    dist = np.linalg.norm(probes.centres[:, None, :] - probes.panel_centres[None, :, :], axis=2)
    assert np.all(np.sqrt(2 * pan["area"][:12])[None, :] / dist < 0.5)          # stokes_traction_entry's far branch: the K stored points
    g = rng.normal(size=(12, 3))
    E = probes.entries(np.arange(10), np.arange(12))
    ref = np.einsum("ijab,jb->ia", E, g)
    scale = np.abs(ref).max()
    for direct in (False, True):
        t, T = chain_rows(oracle_mod, 12, geometry, probes, pan, g, direct)
        err = np.abs(t - ref).max() / scale
        print("chain p = 12, direct %d: %.3e of the largest row; T / |t| up to %.1f" % (direct, err, (T / np.linalg.norm(ref, axis=1)).max()))
        assert err <= 1e-10, (direct, err)
        assert np.all(T >= np.linalg.norm(t, axis=1) * (1 - 1e-12))
    t6, _ = chain_rows(oracle_mod, 6, geometry, probes, pan, g, False)
    err6 = np.abs(t6 - ref).max() / scale
    print("chain p = 6: %.3e" % err6)
    assert err6 > 1e-8, err6
    probes.close()


# ---- (d) -------------------------------------------------------------------------------------------------------------------------
DENSITY_SEED = 1


def two_spheres(fb):
    return np.ascontiguousarray(np.concatenate([fb.unit_sphere(4), fb.unit_sphere(3, center=(2.6, 0.2, -0.3))]))


def test_the_composition_on_real_lists(fb, oracle_mod):
    """unit_sphere(4) + unit_sphere(3) at (2.6, 0.2, -0.3), 640 panels, ncrit 16, flags i % 2: the VELOCITY rows of compose are
    composed_reference's to 1e-14, on the single plan and on the field plan at its centroids (the same lists); the lists are all
    live and the tree has 3 levels or more; no dipole slot hides behind a shared scale."""
    v = two_spheres(fb)
    n = len(v)
    assert n == 640
    flags = (np.arange(n) % 2).astype(np.uint8)
    x = np.random.default_rng(DENSITY_SEED).normal(size=(n, 3))
    probes = R.Probes(v, R.centroids(v), flags)
    single = fb.FMM_plan(R.stokes_kernel(fb, 6), v, host_opts(fb, ncrit=16), bc=flags, host_only=True)
    field = single.field_plan(probes.centres, flags)
    for which in ("m2m", "m2l", "l2l", "p2p"):
        assert len(single.pairs(which)) > 0, which
        assert np.array_equal(single.pairs(which), field.pairs(which)), which
    assert single.boxes()["level"].max() + 1 >= 3
    ref = R.composed_reference(field, probes, v, x, 6)
    vel = flags == 0
    for plan in (single, field):
        c = D.compose(plan, v, x, 6, probes)
        assert c["M"].shape == (len(single.boxes()["leaf"]), 11, 21) and c["rows"].shape == (n, 3) and c["T"].shape == (n,)
        assert np.linalg.norm(c["rows"][vel] - ref[vel]) <= 1e-14 * np.linalg.norm(ref[vel])
        assert np.abs(c["rows"][vel] - ref[vel]).max() <= 1e-14 * np.abs(ref[vel]).max()
        assert np.all(np.isfinite(c["rows"])) and np.all(c["T"][~vel] > 0) and np.all(c["T"][vel] == 0)
        assert np.all(c["T"][~vel] >= np.linalg.norm(c["rows"][~vel], axis=1) * (1 - 1e-12))
        for E in (c["M"], c["L"]):
            norms = np.linalg.norm(E[:, D.DIPOLE], axis=(0, 2))
            print("dipole slot norms", norms)
            assert norms.min() > 0 and norms.max() <= 10 * norms.min(), norms
    probes.close()


# ---- (e) -------------------------------------------------------------------------------------------------------------------------
def test_the_oracles_spherical_chain_on_the_axis(oracle_mod):
    """The oracle's Stokes VELOCITY L2P (double, spherical chain: divisions by sin a) at targets exactly above and below a box
    centre and at the centre itself, against the same rows from local_value_and_gradient (long double, no division).  On the axis
    cart2sph gives sin a = sqrt(2 EPS / rho), whose double-precision value carries the rounding of cos a = z / rho amplified by
    1 / (1 - cos a): 2^-53 rho / (2 EPS) relative, so the m = 1 terms (proportional to sin a) move by about 1e-10 sqrt(rho) of
    their coefficients' size.  The worst deviation over the orders, relative to the largest row, stays below
    D.ON_AXIS_DEVIATION and within a factor 30 of it: it is this effect, not rounding (1e-16) and not a convention gap (1e-6)."""
    worst = 0.0
    for p in ORDERS:
        rng = np.random.default_rng(23 + p)
        S = p * (p + 1) // 2
        L = m0_real(rng.normal(size=(4, S)) + 1j * rng.normal(size=(4, S)), p)
        z = np.array([0.0, 0.02, 0.05, 0.075, 0.11, -0.03, -0.075, -0.2, 0.2])
        pts = ABOUT + np.stack([0 * z, 0 * z, z], axis=1)
        u = oracle_mod.single_l2p(1, p, 1, L, ABOUT, R.point_panels(pts), None, mu=0.5).reshape(-1, 3)
        mine = D.velocity_rows_long(p, L, ABOUT, pts, mu=0.5).astype(np.float64)
        assert np.all(np.isfinite(u)) and np.all(np.isfinite(mine))
        dev = float(np.abs(u - mine).max() / np.abs(mine).max())
        print("on the axis, p = %2d: %.3e of the largest row" % (p, dev))
        worst = max(worst, dev)
    assert D.ON_AXIS_DEVIATION / 30 <= worst <= D.ON_AXIS_DEVIATION, worst
