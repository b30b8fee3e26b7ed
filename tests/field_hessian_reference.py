"""The reference of the field Hessian (fmmbem_plan_execute_hessian), composed on the CPU with no product arithmetic in it.  It stands
on field_gradient_reference.Reference -- the cases, the oracle's target plan and lists, the near lists per leaf and expansions(x, p) --
and adds

  eta               the entry of include/fmmbem.h "Field Hessian" in numpy, (P, 3, 3) per (target, panel): the derivative with respect
                    to the target point of field_gradient_reference.gamma, in gamma's regimes; 0 on the panel itself.
  Reference         NEAR half = eta . x over the listed p2p pairs; FAR half = + (flag 0) or - (flag 1) the long-double Hessian of the
                    leaf's L of the row's slot (field_velocity_gradient_reference.local_gradient_and_hessian: no chain rule, nothing
                    singular on the axis).
  limit             the near half plus the K-point eta of every panel outside the leaf's near list.
  scale(flag)       max_i sum_j sum |eta_ij| |x_j| over the rows of the flag class.

ON_AXIS_DEVIATION is what a double-precision evaluation by the device's route -- derived coefficients, ONE spherical chain, sph2cart
-- may lose on the axis or at the centre of a leaf against the evaluation here, relative to scale."""
import numpy as np

import field_gradient_reference as G
import field_velocity_gradient_reference as V
from oracle import oracle as O

CASES = G.CASES
N_AWKWARD = G.N_AWKWARD
K, THETA = G.K, G.THETA
# The reasoning is field_velocity_gradient_reference.ON_AXIS_DEVIATION's, for the same chain over the derived coefficients of ONE slot:
# on the axis sin a = sqrt(2 EPS / rho) carries the rounding of cos a = z / rho, and the m = 1 terms are proportional to it.  Relative
# to a row's scale -- which holds every pair's eta, the far panels' too -- the figure is what is measured, not derived:
# tests/test_field_hessian_host.py::test_device_route_in_double measures, over the 16 awkward rows at p = 1, 2, 6, 12, 16, 1.58e-14 at
# worst (3.0e-19 on rows of general position; the trace of an awkward row 1.5e-14).  Set at 10 x that, the margin the velocity
# gradient's constant takes.
ON_AXIS_DEVIATION = 1.6e-13


def eta(t, flag, v, g, far_only=False, rules=None):
    """(P, 3, 3): eta(t, panel j) for the P panels of v (P, 3, 3) with geometry g (center, area, normal, quad restricted to them);
    far_only: the K stored points whatever the distance (the limit sum's far part); rules: (wK, (bF, wF)) of another K"""
    wK, (bF, wF) = rules if rules is not None else G._rules()
    c, A, n = g["center"], g["area"], g["normal"]
    d = np.linalg.norm(t[None] - c, axis=1)
    with np.errstate(divide="ignore"):
        near = (np.sqrt(2 * A) / d >= 0.5) & (not far_only)
    self_ = (d < 1e-8) & (not far_only)
    near = near & ~self_
    I = np.eye(3)
    out = np.zeros((len(v), 3, 3))
    for mask, y, w in ((~near & ~self_, g["quad"], wK), (near, np.einsum("qk,pkx->pqx", bF, v), wF)):
        if not mask.any():
            continue
        dx = y[mask] - t[None, None]                          # (P, q, 3)
        r2 = (dx * dx).sum(-1)
        r = np.sqrt(r2)
        wA = w[None] * A[mask][:, None]
        dd = dx[..., :, None] * dx[..., None, :]
        if flag == 0:
            e = 3 * dd / (r ** 5)[..., None, None] - I / (r ** 3)[..., None, None]
        else:
            nm = np.broadcast_to(n[mask][:, None, :], dx.shape)
            dn = (dx * nm).sum(-1)
            nd = nm[..., :, None] * dx[..., None, :]
            e = (15 * (dn / r ** 7)[..., None, None] * dd
                 - 3 * (nd + nd.swapaxes(-1, -2) + dn[..., None, None] * I) / (r ** 5)[..., None, None])
        out[mask] = (wA[..., None, None] * e).sum(1)
    return out


class Reference:
    """One case: field_gradient_reference.Reference's trees, lists and L, and the composed halves of the Hessian (cached per vector
    and order)"""

    def __init__(self, name, base=None):
        self.base = b = base if base is not None else G.reference(name)
        self.name, self.c, self.v, self.pts, self.flags, self.g = name, b.c, b.v, b.pts, b.flags, b.g
        self.P, self.F, self.given, self.tb, self.tree, self.perm, self.x, self.x2 = b.P, b.F, b.given, b.tb, b.tree, b.perm, b.x, b.x2
        self.T, self.info, self.near = b.T, b.info, b.near
        self.rules = None
        self._near, self._far, self._limit, self._scale = {}, {}, {}, {}

    def vector(self, key):
        return self.base.vector(key)

    def _lists(self, leaf):
        return [self.base.leaf_panels(s) for s in self.near.get(int(leaf), [])]

    def near_half(self, key="x"):
        """(distinct points, 3, 3)"""
        if key not in self._near:
            b, x = self.base, self.vector(key)
            out = np.zeros((len(self.P), 3, 3))
            for leaf in np.nonzero(self.tb["leaf"])[0]:
                lists = self._lists(leaf)
                if not lists:
                    continue
                idx = np.concatenate(lists)
                vi, gi = self.v[idx], G.sub(self.g, idx)
                for k in b.leaf_points(leaf):
                    out[k] = np.einsum("pab,p->ab", eta(self.P[k], int(self.F[k]), vi, gi, rules=self.rules), x[idx])
            self._near[key] = out
        return self._near[key]

    def far_half(self, key, p):
        """(distinct points, 3, 3), signed by flag"""
        if (key, p) not in self._far:
            b = self.base
            L = b.expansions(self.vector(key), p)
            out = np.zeros((len(self.P), 3, 3))
            for leaf in np.nonzero(self.tb["leaf"])[0]:
                here = b.leaf_points(leaf)
                for f in (0, 1):
                    sel = here[self.F[here] == f]
                    if len(sel) == 0 or not np.any(L[leaf, f]):
                        continue
                    he = V.local_gradient_and_hessian(p, L[leaf, f], self.tb["center"][leaf], self.P[sel])[1]
                    out[sel] = (-1.0 if f else 1.0) * he[0].astype(np.float64)
            self._far[(key, p)] = out
        return self._far[(key, p)]

    def hessian(self, p, key="x"):
        """(given targets, 3, 3): the composed reference of an execute at order p"""
        return (self.near_half(key) + self.far_half(key, p))[self.given]

    def _rest(self, key):
        if key not in self._limit:
            b, x = self.base, self.vector(key)
            out = self.near_half(key).copy()
            scale = np.zeros(len(self.P))
            for leaf in np.nonzero(self.tb["leaf"])[0]:
                rest = np.ones(len(self.v), dtype=bool)
                lists = self._lists(leaf)
                for idx in lists:
                    rest[idx] = False
                far = np.nonzero(rest)[0]
                nr = np.concatenate(lists) if lists else np.zeros(0, dtype=np.int64)
                vf, gf, vn, gn = self.v[far], G.sub(self.g, far), self.v[nr], G.sub(self.g, nr)
                for k in b.leaf_points(leaf):
                    f = int(self.F[k])
                    e = eta(self.P[k], f, vf, gf, far_only=True, rules=self.rules)
                    out[k] += np.einsum("pab,p->ab", e, x[far])
                    scale[k] = np.einsum("pab,p->", np.abs(e), np.abs(x[far]))
                    if len(nr):
                        scale[k] += np.einsum("pab,p->", np.abs(eta(self.P[k], f, vn, gn, rules=self.rules)), np.abs(x[nr]))
            self._limit[key] = out
            self._scale[key] = [float(scale[self.F == f].max()) if np.any(self.F == f) else 0.0 for f in (0, 1)]
        return self._limit[key]

    def limit(self, key="x"):
        """(given targets, 3, 3): the near half plus the K-point eta of every panel not in the leaf's near list"""
        return self._rest(key)[self.given]

    def scale(self, flag, key="x"):
        """max_i sum_j sum |eta_ij| |x_j| over the rows of the flag class"""
        self._rest(key)
        return self._scale[key][flag]


class _BaseAtRule:
    """field_gradient_reference.Reference's case at another quadrature rule: the trees and lists do not depend on the rule (they are
    built on centroids) and are the base's; the panels' stored points and the multipoles do, and are made here at rule `k`"""

    def __init__(self, base, k):
        self._b, self.k = base, k
        pan = O.Oracle(base.v, K=k, ncrit=1 << 30)
        self.g = pan.panels()
        pan.close()

    def __getattr__(self, name):
        return getattr(self._b, name)

    def expansions(self, x, p):
        """L (target boxes, 2, S): field_gradient_reference.Reference.expansions with P2M at rule k"""
        b = self._b
        sb, tb = b.sb, b.tb
        S = p * (p + 1) // 2
        Tb = O.Tables(p)
        m2m, m2l, l2l = b.T.pairs("m2m"), b.T.pairs("m2l"), b.T.pairs("l2l")
        M = np.zeros((len(sb["leaf"]), 2, S), dtype=np.complex128)
        read = np.zeros(len(sb["leaf"]), dtype=bool)
        read[m2l[:, 0]] = True
        read[m2m[:, 0]] = True
        for box in np.nonzero((sb["leaf"] != 0) & read)[0]:
            idx = b.leaf_panels(box)
            M[box, 0] = O.single_p2m(0, p, self.k, b.v[idx], np.zeros(len(idx), np.uint8), x[idx], sb["center"][box])[0]
            M[box, 1] = O.single_p2m(0, p, self.k, b.v[idx], np.ones(len(idx), np.uint8), x[idx], sb["center"][box])[1]
        for c_, par in m2m:
            M[par] += np.stack([Tb.m2m(M[c_, s], sb["center"][par] - sb["center"][c_]) for s in range(2)])
        L = np.zeros((len(tb["leaf"]), 2, S), dtype=np.complex128)
        for s_, t_ in m2l:
            L[t_] += np.stack([Tb.m2l(M[s_, s], tb["center"][t_] - sb["center"][s_]) for s in range(2)])
        for par, c_ in l2l:
            L[c_] += np.stack([Tb.l2l(L[par, s], tb["center"][c_] - tb["center"][par]) for s in range(2)])
        return L


_REFS = {}


def reference(name, k=K):
    """the case at the quadrature rule k (the cases' own: K)"""
    if (name, k) not in _REFS:
        if k == K:
            _REFS[(name, k)] = Reference(name)
        else:
            ref = Reference(name, base=_BaseAtRule(G.reference(name), k))
            ref.rules = (O.quadrature(k)[1], O.quadrature(17))
            _REFS[(name, k)] = ref
    return _REFS[(name, k)]
