"""The reference of the field velocity gradient (fmmbem_plan_execute_velocity_gradient), composed on the CPU with no product
arithmetic in it.  It stands on field_pressure_reference.Reference -- the field plan's trees and lists, the near lists per leaf and
expansions(x, p), the oracle's P2M / M2M / M2L / L2L for slots 0..3 -- and adds

  gamma_entry       the entry of include/fmmbem.h "Field velocity gradient" in numpy, (P, 3, 3, 3) [k][m][e] per (target, panel):
                    G[k][m] += sum_e Gamma[k][m][e] f_e, the regimes those of pi_entry.
  solid_harmonics_hessian   R, grad R and grad grad R in long double by differentiating the recurrences of
                    double_layer_reference.solid_harmonics once more: no chain rule, nothing singular.
  Reference         NEAR half = gamma_entry . x over the listed p2p pairs; FAR half, at placed(x - centre) with the unplaced x_e as
                    the factor,  (1 / 2 mu) [ d_m phi_k - d_k phi_m - x_e d_k d_m phi_e + d_k d_m phi_3 ]  of the leaf's L.
  limit             the near half plus the K-point tensor of every panel outside the leaf's near list.
  scale             max_i sum_j sum |Gamma_ij| |x_j|.

ON_AXIS_DEVIATION is what a double-precision evaluation by the device's route -- derived coefficients, ONE spherical chain, sph2cart
-- may lose on the axis or at the centre of a leaf against the evaluation here, relative to scale."""
import numpy as np

import double_layer_reference as D
import field_plan_reference as R
import field_pressure_reference as Q

CASES = Q.CASES
N_AWKWARD = Q.N_AWKWARD
LD, CLD = D.LD, D.CLD
# The reasoning is double_layer_reference.ON_AXIS_DEVIATION's: on the axis sin a = sqrt(2 EPS / rho) carries the rounding of
# cos a = z / rho amplified by 1 / (1 - cos a), and the m = 1 terms of the ONE chain are proportional to it: 2^-53 sqrt(rho / 2 EPS)
# = 3.5e-11 of their coefficients' size at rho = 0.2.  Here those coefficients are the DERIVED ones, and a row's scale holds every
# pair's tensor -- the far panels' too, which the expansions sum with cancellation -- so relative to scale the figure is far smaller
# and is what is measured, not derived: tests/test_field_velocity_gradient_host.py (e) measures, over the 16 awkward rows at
# p = 1, 6, 12, 16, 1.68e-13 at worst (5.0e-18 on rows of general position; the trace of an awkward row 8.7e-14).  Set at 10 x that.
ON_AXIS_DEVIATION = 1.7e-12


def gamma_entry(t, v, g, far_only=False, rules=None, mu=R.MU):
    """(P, 3, 3, 3) [k][m][e]: Gamma(t, panel j) for the P panels of v (P, 3, 3) with geometry g; far_only and rules as pi_entry"""
    wK, (bF, wF) = rules if rules is not None else Q._rules()
    A = g["area"]
    self_, near = Q.regimes(t, g)
    if far_only:
        self_[:], near[:] = False, False
    I = np.eye(3)
    out = np.zeros((len(v), 3, 3, 3))
    for mask, y, w in ((~near & ~self_, g["quad"], wK), (near, np.einsum("qk,pkx->pqx", bF, v), wF)):
        if not mask.any():
            continue
        d = t[None, None] - y[mask]                          # (P, q, 3)
        r2 = (d * d).sum(-1)
        ok = r2 >= 1e-8                                     # a quadrature point with |d|^2 < 1e-8 contributes 0
        r = np.sqrt(np.where(ok, r2, 1.0))
        f3 = np.where(ok, w[None] * A[mask][:, None] / r ** 3, 0.0)
        f5 = np.where(ok, w[None] * A[mask][:, None] / r ** 5, 0.0)
        T3 = (-np.einsum("ke,pqm->pqkme", I, d) + np.einsum("km,pqe->pqkme", I, d) + np.einsum("me,pqk->pqkme", I, d))
        T5 = np.einsum("pqk,pqm,pqe->pqkme", d, d, d)
        out[mask] = (f3[..., None, None, None] * T3 - 3 * f5[..., None, None, None] * T5).sum(1) / (2 * mu)
    return out


def solid_harmonics_hessian(p, d):
    """R (S, N), grad R (S, N, 3) and grad grad R (S, N, 3, 3), complex long double, at the points d as given: the recurrences of
    double_layer_reference.solid_harmonics and their first and second term-by-term derivatives"""
    d = np.asarray(d, dtype=LD).reshape(-1, 3)
    N = len(d)
    S = p * (p + 1) // 2
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    r2 = x * x + y * y + z * z
    xy = x + CLD(1j) * y
    e_xy = np.array([1, 1j, 0], dtype=CLD)
    e_z = np.array([0, 0, 1], dtype=CLD)
    eye = np.eye(3, dtype=LD)
    Qn = np.zeros((S, N), dtype=CLD)
    dQ = np.zeros((S, N, 3), dtype=CLD)
    hQ = np.zeros((S, N, 3, 3), dtype=CLD)

    def sym(e, g):                                           # e_a g_b + e_b g_a, e (3,), g (N, 3)
        o = e[None, :, None] * g[:, None, :]
        return o + o.transpose(0, 2, 1)

    def symd(g):                                             # d_a g_b + d_b g_a
        o = d[:, :, None] * g[:, None, :]
        return o + o.transpose(0, 2, 1)

    fact = [LD(1)]
    for k in range(1, 2 * p + 1):
        fact.append(fact[-1] * k)
    for m in range(p):
        mm = m * (m + 1) // 2 + m
        if m == 0:
            Qn[0] = 1
        else:
            pm = (m - 1) * m // 2 + m - 1
            Qn[mm] = -xy * Qn[pm] / LD(2 * m)
            dQ[mm] = -(e_xy[None, :] * Qn[pm][:, None] + xy[:, None] * dQ[pm]) / LD(2 * m)
            hQ[mm] = -(sym(e_xy, dQ[pm]) + xy[:, None, None] * hQ[pm]) / LD(2 * m)
        for n in range(m + 1, p):
            i0, i1 = n * (n + 1) // 2 + m, (n - 1) * n // 2 + m
            den = LD((n + m) * (n - m))
            Qn[i0] = LD(2 * n - 1) * z * Qn[i1]
            dQ[i0] = LD(2 * n - 1) * (e_z[None, :] * Qn[i1][:, None] + z[:, None] * dQ[i1])
            hQ[i0] = LD(2 * n - 1) * (sym(e_z, dQ[i1]) + z[:, None, None] * hQ[i1])
            if n - 2 >= m:
                i2 = (n - 2) * (n - 1) // 2 + m
                Qn[i0] -= r2 * Qn[i2]
                dQ[i0] -= 2 * d * Qn[i2][:, None] + r2[:, None] * dQ[i2]
                hQ[i0] -= 2 * eye[None] * Qn[i2][:, None, None] + 2 * symd(dQ[i2]) + r2[:, None, None] * hQ[i2]
            Qn[i0] /= den
            dQ[i0] /= den
            hQ[i0] /= den
    for n in range(p):
        for m in range(n + 1):
            s = np.sqrt(fact[n - m] * fact[n + m])
            i = n * (n + 1) // 2 + m
            Qn[i] *= s
            dQ[i] *= s
            hQ[i] *= s
    return Qn, dQ, hQ


def local_gradient_and_hessian(p, L, center, x):
    """gradient (k, N, 3) and Hessian (k, N, 3, 3), long double, of the k local expansions L (k, S) about center at placed(x - center),
    in the convention of double_layer_reference.local_value_and_gradient"""
    L = np.atleast_2d(np.asarray(L)).astype(CLD)
    d = D.placed(np.asarray(x, dtype=LD).reshape(-1, 3) - np.asarray(center, dtype=LD))
    _, dR, hR = solid_harmonics_hessian(p, d)
    wm = np.array([1 if m == 0 else 2 for n in range(p) for m in range(n + 1)], dtype=LD)
    Lw = L * wm[None, :]
    return np.real(np.einsum("ks,sni->kni", Lw, dR)), np.real(np.einsum("ks,snij->knij", Lw, hR))


def far_rows_long(p, L4, center, x, mu=R.MU):
    """(N, 3, 3) long double [k][m]: (1 / 2 mu) [ d_m phi_k - d_k phi_m - x_e d_k d_m phi_e + d_k d_m phi_3 ] from slots 0..3 of one
    box; x are the targets' own coordinates (the factor x_e is not placed)"""
    x = np.asarray(x, dtype=LD).reshape(-1, 3)
    gr, he = local_gradient_and_hessian(p, L4, center, x)
    a = gr[0:3].transpose(1, 0, 2)                           # [n][k][m] = d_m phi_k
    return (a - a.transpose(0, 2, 1) - np.einsum("ne,enkm->nkm", x, he[0:3]) + he[3]) / (2 * LD(mu))


class Reference:
    """One case: field_pressure_reference.Reference's trees, lists and L, and the composed halves of the velocity gradient (cached
    per vector and order)"""

    def __init__(self, name):
        self.base = b = Q.reference(name)
        self.name, self.c, self.v, self.pts, self.g, self.P, self.given = name, b.c, b.v, b.pts, b.g, b.P, b.given
        self.tb, self.lists, self.tree, self.perm, self.x, self.x2 = b.tb, b.lists, b.tree, b.perm, b.x, b.x2
        self._near, self._far, self._limit, self._scale = {}, {}, {}, {}

    def vector(self, key):
        return self.base.vector(key)

    def near_half(self, key="x"):
        """(distinct points, 3, 3)"""
        if key not in self._near:
            b, x = self.base, self.vector(key)
            out = np.zeros((len(self.P), 3, 3))
            for leaf in np.nonzero(self.tb["leaf"])[0]:
                lists = [b.leaf_panels(s) for s in b.near.get(int(leaf), [])]
                if not lists:
                    continue
                idx = np.concatenate(lists)
                vi, gi = self.v[idx], Q.sub(self.g, idx)
                for k in b.leaf_points(leaf):
                    out[k] = np.einsum("pkme,pe->km", gamma_entry(self.P[k], vi, gi), x[idx])
            self._near[key] = out
        return self._near[key]

    def far_half(self, key, p):
        """(distinct points, 3, 3)"""
        if (key, p) not in self._far:
            b = self.base
            L = b.far_half(key, p)[2]
            out = np.zeros((len(self.P), 3, 3))
            for leaf in np.nonzero(self.tb["leaf"])[0]:
                here = b.leaf_points(leaf)
                if len(here) == 0 or not np.any(L[leaf]):
                    continue
                out[here] = far_rows_long(p, L[leaf], self.tb["center"][leaf], self.P[here]).astype(np.float64)
            self._far[(key, p)] = out
        return self._far[(key, p)]

    def gradient(self, p, key="x"):
        """(given targets, 3, 3): the composed reference of an execute at order p"""
        return (self.near_half(key) + self.far_half(key, p))[self.given]

    def _rest(self, key):
        if key not in self._limit:
            b, x = self.base, self.vector(key)
            out = self.near_half(key).copy()
            scale = np.zeros(len(self.P))
            for leaf in np.nonzero(self.tb["leaf"])[0]:
                rest = np.ones(len(self.v), dtype=bool)
                lists = [b.leaf_panels(s) for s in b.near.get(int(leaf), [])]
                for idx in lists:
                    rest[idx] = False
                far = np.nonzero(rest)[0]
                nr = np.concatenate(lists) if lists else np.zeros(0, dtype=np.int64)
                vf, gf, vn, gn = self.v[far], Q.sub(self.g, far), self.v[nr], Q.sub(self.g, nr)
                for k in b.leaf_points(leaf):
                    e = gamma_entry(self.P[k], vf, gf, far_only=True)
                    out[k] += np.einsum("pkme,pe->km", e, x[far])
                    scale[k] = np.einsum("pkme,pe->", np.abs(e), np.abs(x[far]))
                    if len(nr):
                        scale[k] += np.einsum("pkme,pe->", np.abs(gamma_entry(self.P[k], vn, gn)), np.abs(x[nr]))
            self._limit[key], self._scale[key] = out, float(scale.max())
        return self._limit[key]

    def limit(self, key="x"):
        """(given targets, 3, 3): the near half plus the K-point tensor of every panel not in the leaf's near list"""
        return self._rest(key)[self.given]

    def scale(self, key="x"):
        """max_i sum_j sum |Gamma_ij| |x_j|"""
        self._rest(key)
        return self._scale[key]


_REFS = {}


def reference(name):
    if name not in _REFS:
        _REFS[name] = Reference(name)
    return _REFS[name]
