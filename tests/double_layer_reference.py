"""The reference of the Stokes double layer's far field (the rows of TRACTION targets), composed on the CPU.

With phi = 1/|x - y|, the source's density g and normal n, and d = x - y,
    -3 (d.n) d_i (d.g) / r^5  =  x_k d_i Psi_k - d_i Psi_0 - Theta_i,
    Psi_k = sum w A n_k (g.grad_y) phi,   Psi_0 = sum w A (y.n) (g.grad_y) phi,   Theta_i = sum w A g_i (n.grad_y) phi:
seven harmonic dipole potentials, expansion slots 4..10 beside the single layer's 0..3.  The oracle has no far field for this
operator, so its pieces are written here from that mathematics, in numpy long double:

  solid_harmonics   R_nm(d) = rho^n P_n^m(cos a) sqrt((n-m)!/(n+m)!) e^{+i m b} and its CARTESIAN gradient, both from the
                    recurrences of the harmonics as polynomials in (x, y, z) and their term-by-term derivatives: no spherical
                    chain rule, no division by sin a, nothing singular on the axis or at the centre.
  grad_moments      the gradient of the P2M basis b_nm = conj(R_nm) at source points; dipole_slots sums them into slots 4..10.
  local_value_and_gradient   value and Cartesian gradient of a local expansion sum_n (Re L_n0 R_n0 + 2 sum_m Re L_nm R_nm).
  compose           P2M per source leaf, M2M / M2L / L2L per listed pair and slot by oracle.Tables (every slot is a harmonic
                    potential, so the oracle's Laplace operators are the reference), the rows, the near part from the oracle's
                    kernel entries, and per TRACTION row the magnitude T of the terms the row is the sum of.

One convention of the project enters, and it is a convention of where a point is, not of a formula: cart2sph gives rho = |d| + EPS
(EPS = 1e-12) and a = acos(z / rho), so every harmonic is evaluated at placed(d) -- the point with d's z and azimuth at distance
|d| + EPS.  The spherical chain rule is an identity in (rho, a, b), so the oracle's and the kernels' gradients are the exact
Cartesian gradients AT THAT POINT, which is what the recurrences here give (tests/test_double_layer_reference_host.py pins both
to the oracle at 1e-13).  On the axis placed(d) is sqrt(2 EPS |d|) beside it, at the centre it is (EPS, 0, 0).

Why T: x_k d_i Psi_k - d_i Psi_0 = sum w A (x.n - y.n) d_i (g.grad_y) phi, the two terms cancel to |x - y| / |x| of their size, so a
row's rounding error is that of its terms.  Row errors are measured against T, not against |t|."""
import numpy as np

import field_plan_reference as R
from oracle import oracle as O

EPS = 1e-12                      # the project's cart2sph: rho = |d| + EPS
LD, CLD = np.longdouble, np.clongdouble
DIPOLE = slice(4, 11)
N_SLOTS = 11
# What the oracle's double-precision spherical chain (and any other double-precision evaluation of the same formulae) may lose
# on the axis of a box against the singularity-free evaluation here, relative to the largest row: there sin a = sqrt(2 EPS / rho)
# carries the rounding of cos a = z / rho amplified by 1 / (1 - cos a), i.e. 2^-53 rho / (2 EPS) relative, and the m = 1 terms are
# proportional to it: 2^-53 sqrt(rho / (2 EPS)) = 3.5e-11 of their coefficients' size at rho = 0.2, a few such terms per row.
# Measured by tests/test_double_layer_reference_host.py (e): 4.4e-11 at worst over p = 1, 6, 12, 16.
ON_AXIS_DEVIATION = 1e-10


def placed(d):
    """(N, 3) long double: where the project's cart2sph places d -- z and the azimuth of d, |.| = |d| + EPS; the azimuth's
    degenerate branches as there (|x| + |y| < EPS: b = 0; |x| < EPS: b = +-pi/2)"""
    d = np.asarray(d, dtype=LD).reshape(-1, 3)
    rho = np.sqrt(np.sum(d * d, axis=1)) + LD(EPS)
    z = d[:, 2]
    hp = np.sqrt((rho - z) * (rho + z))
    ax, ay = np.abs(d[:, 0]), np.abs(d[:, 1])
    h = np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2)
    axis, on_y = ax + ay < EPS, ax < EPS
    hs = np.where(h > 0, h, LD(1))
    cb = np.where(axis, LD(1), np.where(on_y, LD(0), d[:, 0] / hs))
    sb = np.where(axis, LD(0), np.where(on_y, np.sign(d[:, 1]), d[:, 1] / hs))
    return np.stack([hp * cb, hp * sb, z], axis=1)


def solid_harmonics(p, d):
    """R (S, N) and grad R (S, N, 3), complex long double, S = p (p + 1) / 2 at index n (n + 1) / 2 + m, at the points d (N, 3) as
    given (no placement here).  With Q_nm = R_nm / sqrt((n - m)! (n + m)!):
        Q_00 = 1,   Q_mm = -(x + i y) Q_{m-1,m-1} / (2 m),   (n + m)(n - m) Q_nm = (2 n - 1) z Q_{n-1,m} - r^2 Q_{n-2,m}
    (the Legendre recurrences with the Condon-Shortley sign the project's P_m^m = (-1)^m (2m - 1)!! sin^m a carries), and the
    gradients by differentiating each line."""
    d = np.asarray(d, dtype=LD).reshape(-1, 3)
    N = len(d)
    S = p * (p + 1) // 2
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    r2 = x * x + y * y + z * z
    xy = x + CLD(1j) * y
    e_xy = np.array([1, 1j, 0], dtype=CLD)
    e_z = np.array([0, 0, 1], dtype=CLD)
    Q = np.zeros((S, N), dtype=CLD)
    dQ = np.zeros((S, N, 3), dtype=CLD)
    fact = [LD(1)]
    for k in range(1, 2 * p + 1):
        fact.append(fact[-1] * k)
    for m in range(p):
        mm = m * (m + 1) // 2 + m
        if m == 0:
            Q[0] = 1
        else:
            pm = (m - 1) * m // 2 + m - 1
            Q[mm] = -xy * Q[pm] / LD(2 * m)
            dQ[mm] = -(e_xy[None, :] * Q[pm][:, None] + xy[:, None] * dQ[pm]) / LD(2 * m)
        for n in range(m + 1, p):
            i0, i1 = n * (n + 1) // 2 + m, (n - 1) * n // 2 + m
            den = LD((n + m) * (n - m))
            Q[i0] = LD(2 * n - 1) * z * Q[i1]
            dQ[i0] = LD(2 * n - 1) * (e_z[None, :] * Q[i1][:, None] + z[:, None] * dQ[i1])
            if n - 2 >= m:
                i2 = (n - 2) * (n - 1) // 2 + m
                Q[i0] -= r2 * Q[i2]
                dQ[i0] -= 2 * d * Q[i2][:, None] + r2[:, None] * dQ[i2]
            Q[i0] /= den
            dQ[i0] /= den
    for n in range(p):
        for m in range(n + 1):
            s = np.sqrt(fact[n - m] * fact[n + m])
            Q[n * (n + 1) // 2 + m] *= s
            dQ[n * (n + 1) // 2 + m] *= s
    return Q, dQ


def basis_and_gradient(p, points, center):
    """b (q, S) and grad_y b (q, 3, S) of the P2M basis b_nm(y - c) = conj(R_nm) at the placed points"""
    d = placed(np.asarray(points, dtype=LD).reshape(-1, 3) - np.asarray(center, dtype=LD))
    Rn, dR = solid_harmonics(p, d)
    return np.conj(Rn).T, np.conj(dR).transpose(1, 2, 0)


def grad_moments(p, points, center):
    """G[q, 3, S]: the Cartesian gradient, with respect to the source point, of the project's P2M basis function"""
    return basis_and_gradient(p, points, center)[1]


def weights():
    return O.quadrature(R.QUAD_K)[1]


def dipole_slots(p, quad, w, area, normal, g, center):
    """(7, S) complex128: slots 4..10 of one leaf.  quad (P, nq, 3), w (nq), area (P), normal (P, 3), density g (P, 3)."""
    quad = np.asarray(quad, dtype=LD)
    P, nq = quad.shape[:2]
    G = grad_moments(p, quad.reshape(-1, 3), center).reshape(P, nq, 3, -1)
    wA = (np.asarray(w, dtype=LD)[None, :] * np.asarray(area, dtype=LD)[:, None]).astype(CLD)
    n, g = np.asarray(normal, dtype=LD).astype(CLD), np.asarray(g, dtype=LD).astype(CLD)
    gG = np.einsum("pk,pqks->pqs", g, G)
    nG = np.einsum("pk,pqks->pqs", n, G)
    yn = np.einsum("pqk,pk->pq", quad, np.asarray(normal, dtype=LD)).astype(CLD)
    out = np.zeros((7, G.shape[-1]), dtype=CLD)
    for k in range(3):
        out[k] = np.einsum("pq,p,pqs->s", wA, n[:, k], gG)
        out[4 + k] = np.einsum("pq,p,pqs->s", wA, g[:, k], nG)
    out[3] = np.einsum("pq,pq,pqs->s", wA, yn, gG)
    return out.astype(np.complex128)


def local_value_and_gradient(p, L, center, x):
    """value (k, N) and Cartesian gradient (k, N, 3), long double, at the points x of the k local expansions L (k, S) about
    center in the project's convention: sum_n (Re L_n0 R_n0 + 2 sum_{m >= 1} Re L_nm R_nm) at placed(x - center)"""
    L = np.atleast_2d(np.asarray(L)).astype(CLD)
    d = placed(np.asarray(x, dtype=LD).reshape(-1, 3) - np.asarray(center, dtype=LD))
    Rn, dR = solid_harmonics(p, d)
    wm = np.array([1 if m == 0 else 2 for n in range(p) for m in range(n + 1)], dtype=LD)
    Lw = L * wm[None, :]
    val = np.real(np.einsum("ks,sn->kn", Lw, Rn))
    grad = np.real(np.einsum("ks,sni->kni", Lw, dR))
    return val, grad


def traction_rows(p, L7, center, x):
    """t (N, 3) and the far part of T (N): t_i = x_k d_i Psi_k - d_i Psi_0 - Theta_i from slots 4..10 of one box, no 1/(2 mu);
    x are the targets' own coordinates (the factor x_k is not placed)"""
    x = np.asarray(x, dtype=LD).reshape(-1, 3)
    val, grad = local_value_and_gradient(p, L7, center, x)
    t = np.einsum("nk,kni->ni", x, grad[0:3]) - grad[3] - val[4:7].T
    T = (np.einsum("nk,kn->n", np.abs(x), np.linalg.norm(grad[0:3], axis=2)) + np.linalg.norm(grad[3], axis=1)
         + np.linalg.norm(val[4:7], axis=0))
    return t.astype(np.float64), T.astype(np.float64)


def velocity_rows_long(p, L4, center, x, mu=R.MU):
    """(N, 3) long double: the single layer's rows u_k = (phi_k - x_e d_k phi_e + d_k phi_3) / (2 mu) from slots 0..3"""
    x = np.asarray(x, dtype=LD).reshape(-1, 3)
    val, grad = local_value_and_gradient(p, L4, center, x)
    return (val[0:3].T - np.einsum("ne,eni->ni", x, grad[0:3]) + grad[3]) / (2 * LD(mu))


def plan_lists(plan):
    """source boxes, target boxes, source perm, (target-tree position -> distinct target), (given -> distinct): a plan over the
    panels' own centres (a single plan) is its source tree on both sides"""
    sb = plan.boxes()
    perm = plan.perm().astype(np.int64)
    if plan.n_targets is None:
        return sb, sb, perm, perm, np.arange(len(perm))
    tree, given = plan.target_perm()
    return sb, plan.target_boxes(), perm, tree.astype(np.int64), given.astype(np.int64)


def compose_expansions(plan, v, x, p):
    """M (source boxes, 11, S) and L (target boxes, 11, S) over the plan's own lists.  P2M at the leaves some listed pair reads
    (an M2L source or an M2M child): a box nothing reads has no multipole on either side."""
    sb, tb, perm, _, _ = plan_lists(plan)
    S = p * (p + 1) // 2
    T = O.Tables(p)
    so = O.StokesOracle(v, K=R.QUAD_K, K_fine=R.QUAD_K_FINE, mu=R.MU, ncrit=1 << 30)
    pan = so.panels()
    so.close()
    w = weights()
    m2m, m2l, l2l = plan.pairs("m2m"), plan.pairs("m2l"), plan.pairs("l2l")
    read = np.zeros(len(sb["leaf"]), dtype=bool)
    read[m2l[:, 0]] = True
    read[m2m[:, 0]] = True
    M = np.zeros((len(sb["leaf"]), N_SLOTS, S), dtype=np.complex128)
    for b in np.nonzero(sb["leaf"] & read)[0]:
        idx = perm[sb["bb"][b]:sb["be"][b]]
        M[b, :4] = O.single_p2m(1, p, R.QUAD_K, v[idx], None, x[idx], sb["center"][b], mu=R.MU)
        M[b, DIPOLE] = dipole_slots(p, pan["quad"][idx], w, pan["area"][idx], pan["normal"][idx], x[idx], sb["center"][b])
    for c, par in m2m:                                     # deepest level first
        tr = sb["center"][par] - sb["center"][c]
        for s in range(N_SLOTS):
            M[par, s] += T.m2m(M[c, s], tr)
    L = np.zeros((len(tb["leaf"]), N_SLOTS, S), dtype=np.complex128)
    for s_box, t_box in m2l:
        tr = tb["center"][t_box] - sb["center"][s_box]
        for s in range(N_SLOTS):
            L[t_box, s] += T.m2l(M[s_box, s], tr)
    for par, c in l2l:                                     # top level first
        tr = tb["center"][c] - tb["center"][par]
        for s in range(N_SLOTS):
            L[c, s] += T.l2l(L[par, s], tr)
    return M, L


def compose_rows(plan, x, p, probes, L, singularity_free=False):
    """rows (given targets, 3) and T (given targets; 0 on VELOCITY rows) from the local expansions L of compose_expansions.
    The far part of VELOCITY rows is the oracle's Stokes L2P, as in field_plan_reference.composed_reference; singularity_free:
    velocity_rows_long instead (targets on the axis of their leaf, where the oracle's chain divides by sin a)."""
    sb, tb, perm, tree, given = plan_lists(plan)
    first = np.full(len(tree), -1, dtype=np.int64)         # distinct point -> the first given target at it
    for k in range(len(given) - 1, -1, -1):
        first[given[k]] = k
    rows, Tm = np.zeros((len(tree), 3)), np.zeros(len(tree))
    near = {}
    for s_box, t_box in plan.pairs("p2p"):
        near.setdefault(int(t_box), []).append(int(s_box))
    for b in np.nonzero(tb["leaf"])[0]:
        here = tree[tb["bb"][b]:tb["be"][b]]
        tg = first[here]
        trac = probes.flags[tg] != 0
        y, Ty = np.zeros((len(tg), 3)), np.zeros(len(tg))
        if np.any(~trac) and singularity_free:
            y[~trac] = velocity_rows_long(p, L[b, :4], tb["center"][b], probes.centres[tg[~trac]]).astype(np.float64)
        elif np.any(~trac):
            y[~trac] = O.single_l2p(1, p, R.QUAD_K, L[b, :4], tb["center"][b], probes.tri[tg[~trac]], None, mu=R.MU).reshape(-1, 3)
        if np.any(trac):
            y[trac], Ty[trac] = traction_rows(p, L[b, DIPOLE], tb["center"][b], probes.centres[tg[trac]])
        for s_box in near.get(int(b), []):
            idx = perm[sb["bb"][s_box]:sb["be"][s_box]]
            E = probes.entries(tg, idx)
            y += np.einsum("ijab,jb->ia", E, x[idx])
            Ty += np.linalg.norm(np.einsum("ijab,jb->ia", np.abs(E), np.abs(x[idx])), axis=1) * trac
        rows[here], Tm[here] = y, Ty
    return rows[given], Tm[given]


def compose(plan, v, x, p, probes, singularity_free=False):
    """dict(M, L, rows, T) of a single plan or a field plan; probes: field_plan_reference.Probes of the plan's targets (a single
    plan: the panels' centroids with the panels' flags)"""
    M, L = compose_expansions(plan, v, x, p)
    rows, T = compose_rows(plan, x, p, probes, L, singularity_free)
    return dict(M=M, L=L, rows=rows, T=T)
