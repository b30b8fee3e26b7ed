"""The reference of the field pressure (fmmbem_plan_execute_pressure), composed on the CPU with no product arithmetic in it.

  pi_entry          the entry of include/fmmbem.h "Field pressure" in numpy, from a StokesOracle's panel data (centre, area, the K
                    stored points), the vertices and the fine rule O.quadrature(QUAD_K_FINE): one (3,) row vector per (target, panel).
  Reference         per case of field_gradient_reference.make_case, every flag 0: a host-only Stokes field plan gives the trees and
                    the lists (as field_plan_reference.composed_reference reads them); the NEAR half = pi_entry . x summed over the
                    listed p2p pairs; the FAR half = slots 0..3 per source leaf by O.single_p2m(1, ...), O.Tables(p).m2m / m2l / l2l
                    over the listed pairs, then the value and the Cartesian gradient of every slot at the targets by
                    double_layer_reference.local_value_and_gradient (long double, nothing singular on the axis), and
                    q -= d_x phi_0 + d_y phi_1 + d_z phi_2.  velocity() recombines the VALUES and gradients of the same L as
                    l2p_stokes_kernel does (tests/test_field_pressure_host.py pins it to the oracle's operators).
  limit             the expansion-free number an execute converges to as p grows: the near half plus the K-point pi of every
                    panel NOT in the leaf's near list.
  scale             max_i sum_j |pi_ij| . |x_j|, the size of the terms a row is the sum of.

The targets are the points as the oracle places them (field_plan_reference.Probes.centres); kernel settings MU, QUAD_K, QUAD_K_FINE of
field_plan_reference, theta and the geometries of field_gradient_reference."""
import numpy as np

import double_layer_reference as D
import field_gradient_reference as G
import field_plan_reference as R
from oracle import oracle as O

CASES = G.CASES
N_AWKWARD = G.N_AWKWARD
_RULES = None


def _rules():
    global _RULES
    if _RULES is None:
        _RULES = (O.quadrature(R.QUAD_K)[1], O.quadrature(R.QUAD_K_FINE))
    return _RULES


def geometry(v):
    so = O.StokesOracle(v, K=R.QUAD_K, K_fine=R.QUAD_K_FINE, mu=R.MU, ncrit=1 << 30)
    out = so.panels()
    so.close()
    return out


def sub(g, idx):
    return {k: a[idx] for k, a in g.items()}


def regimes(t, g):
    """(self, nearby) masks over the panels of g for the target point t: the velocity entry's rule selection"""
    d = np.linalg.norm(t[None] - g["center"], axis=1)
    self_ = d < 1e-8
    with np.errstate(divide="ignore"):
        near = (np.sqrt(2 * g["area"]) / d >= 0.5) & ~self_
    return self_, near


def pi_entry(t, v, g, far_only=False, rules=None):
    """(P, 3): pi(t, panel j) for the P panels of v (P, 3, 3) with geometry g (center, area, quad restricted to them);
    far_only: the K stored points whatever the distance (the limit sum's far part, and the identity pi = -gamma);
    rules: (weights of the K rule g["quad"] was made with, (points, weights) of the fine rule) where they are not this module's"""
    wK, (bF, wF) = rules if rules is not None else _rules()
    A = g["area"]
    self_, near = regimes(t, g)
    if far_only:
        self_[:], near[:] = False, False
    out = np.zeros((len(v), 3))
    for mask, y, w in ((~near & ~self_, g["quad"], wK), (near, np.einsum("qk,pkx->pqx", bF, v), wF)):
        if not mask.any():
            continue
        d = t[None, None] - y[mask]
        r2 = (d * d).sum(-1)
        ok = r2 >= 1e-8                                     # a quadrature point with |d|^2 < 1e-8 contributes 0
        r3 = np.where(ok, r2 * np.sqrt(r2), 1.0)
        f = np.where(ok, w[None] * A[mask][:, None] / r3, 0.0)
        out[mask] = (f[..., None] * d).sum(1)
    return out


def pi_scale(t, v, g):
    """(P,): sum_q |w_q A d_q| / |d_q|^3 of the rule the pair takes (the tolerance scale of an entry)"""
    wK, (bF, wF) = _rules()
    self_, near = regimes(t, g)
    out = np.zeros(len(v))
    for mask, y, w in ((~near & ~self_, g["quad"], wK), (near, np.einsum("qk,pkx->pqx", bF, v), wF)):
        if not mask.any():
            continue
        d = t[None, None] - y[mask]
        r2 = (d * d).sum(-1)
        ok = r2 >= 1e-8
        out[mask] = np.where(ok, w[None] * g["area"][mask][:, None] / np.where(ok, r2, 1.0), 0.0).sum(1)
    return out


def host_plan(fb, v, pts, ncrit, p_max=16, host_only=True):
    opts = fb.FMMOptions()
    opts.set_mac_theta(G.THETA)
    opts.set_max_per_box(ncrit)
    K = R.stokes_kernel(fb, 5)
    return K, fb.FMM_plan(K, v, opts, p_max=p_max, host_only=host_only).field_plan(pts)


class Reference:
    """One case: the field plan's trees and lists, and the composed halves (cached per vector and order)"""

    def __init__(self, name):
        import fmm_bem_relaxed_amd as fb
        self.name = name
        self.c = c = G.make_case(name)
        self.v = np.ascontiguousarray(c["v"])
        probes = R.Probes(self.v, c["pts"], np.zeros(len(c["pts"]), np.uint8))
        self.pts, self.tri = probes.centres.copy(), probes.tri.copy()
        probes.close()
        self.g = geometry(self.v)
        _, plan = host_plan(fb, self.v, self.pts, c["ncrit"])
        self.info = dict(plan.target_info(), **{k: plan.stats()[k] for k in ("p2p_pairs", "m2l_pairs")})
        self.sb, self.tb = plan.boxes(), plan.target_boxes()
        self.perm = plan.perm().astype(np.int64)
        tree, given = plan.target_perm()
        self.tree, self.given = tree.astype(np.int64), given.astype(np.int64)
        self.lists = {w: plan.pairs(w).copy() for w in ("p2p", "m2l", "m2m", "l2l")}
        first = np.full(len(self.tree), -1, dtype=np.int64)    # distinct point -> the first given target at it
        for k in range(len(self.given) - 1, -1, -1):
            first[self.given[k]] = k
        self.first = first
        self.P = self.pts[first]
        self.near = {}
        for s_, t_ in self.lists["p2p"]:
            self.near.setdefault(int(t_), []).append(int(s_))
        self.x = np.random.default_rng(1).standard_normal((len(self.v), 3))
        self.x2 = np.random.default_rng(99).standard_normal((len(self.v), 3))
        self._near, self._far, self._limit, self._scale = {}, {}, {}, {}

    def leaf_points(self, b):
        return self.tree[self.tb["bb"][b]:self.tb["be"][b]]

    def leaf_panels(self, s):
        return self.perm[self.sb["bb"][s]:self.sb["be"][s]]

    def vector(self, key):
        return self.x if key == "x" else self.x2

    def near_half(self, key="x"):
        """(distinct points,)"""
        if key not in self._near:
            x = self.vector(key)
            out = np.zeros(len(self.P))
            for b in np.nonzero(self.tb["leaf"])[0]:
                lists = [self.leaf_panels(s) for s in self.near.get(int(b), [])]
                if not lists:
                    continue
                idx = np.concatenate(lists)
                vi, gi = self.v[idx], sub(self.g, idx)
                for k in self.leaf_points(b):
                    out[k] = np.sum(pi_entry(self.P[k], vi, gi) * x[idx])
            self._near[key] = out
        return self._near[key]

    def expansions(self, x, p):
        """L (target boxes, 4, S): slots 0..3 of the single layer"""
        sb, tb = self.sb, self.tb
        S = p * (p + 1) // 2
        Tb = O.Tables(p)
        m2m, m2l, l2l = self.lists["m2m"], self.lists["m2l"], self.lists["l2l"]
        M = np.zeros((len(sb["leaf"]), 4, S), dtype=np.complex128)
        read = np.zeros(len(sb["leaf"]), dtype=bool)
        read[m2l[:, 0]] = True
        read[m2m[:, 0]] = True
        for b in np.nonzero((sb["leaf"] != 0) & read)[0]:
            idx = self.leaf_panels(b)
            M[b] = O.single_p2m(1, p, R.QUAD_K, self.v[idx], None, x[idx], sb["center"][b], mu=R.MU)
        for c_, par in m2m:
            for s in range(4):
                M[par, s] += Tb.m2m(M[c_, s], sb["center"][par] - sb["center"][c_])
        L = np.zeros((len(tb["leaf"]), 4, S), dtype=np.complex128)
        for s_, t_ in m2l:
            for s in range(4):
                L[t_, s] += Tb.m2l(M[s_, s], tb["center"][t_] - sb["center"][s_])
        for par, c_ in l2l:
            for s in range(4):
                L[c_, s] += Tb.l2l(L[par, s], tb["center"][c_] - tb["center"][par])
        return L

    def far_half(self, key, p):
        """(q (distinct points,), u (distinct points, 3)): minus the trace of the gradients of slots 0..2, and the velocity rows
        u_k = (phi_k - x_e d_k phi_e + d_k phi_3) / (2 mu) of the same L"""
        if (key, p) not in self._far:
            L = self.expansions(self.vector(key), p)
            q, u = np.zeros(len(self.P)), np.zeros((len(self.P), 3))
            for b in np.nonzero(self.tb["leaf"])[0]:
                here = self.leaf_points(b)
                if len(here) == 0 or not np.any(L[b]):
                    continue
                _, gr = D.local_value_and_gradient(p, L[b], self.tb["center"][b], self.P[here])
                q[here] = -(gr[0, :, 0] + gr[1, :, 1] + gr[2, :, 2]).astype(np.float64)
                u[here] = D.velocity_rows_long(p, L[b], self.tb["center"][b], self.P[here]).astype(np.float64)
            self._far[(key, p)] = (q, u, L)
        return self._far[(key, p)]

    def pressure(self, p, key="x"):
        """(given targets,): the composed reference of an execute at order p"""
        return (self.near_half(key) + self.far_half(key, p)[0])[self.given]

    def velocity(self, p, key="x"):
        """(given targets, 3): the far half's velocity rows by the same L"""
        return self.far_half(key, p)[1][self.given]

    def _rest(self, key):
        if key not in self._limit:
            x = self.vector(key)
            out = self.near_half(key).copy()
            scale = np.zeros(len(self.P))
            for b in np.nonzero(self.tb["leaf"])[0]:
                rest = np.ones(len(self.v), dtype=bool)
                lists = [self.leaf_panels(s) for s in self.near.get(int(b), [])]
                for idx in lists:
                    rest[idx] = False
                far = np.nonzero(rest)[0]
                nr = np.concatenate(lists) if lists else np.zeros(0, dtype=np.int64)
                vf, gf, vn, gn = self.v[far], sub(self.g, far), self.v[nr], sub(self.g, nr)
                for k in self.leaf_points(b):
                    e = pi_entry(self.P[k], vf, gf, far_only=True)
                    out[k] += np.sum(e * x[far])
                    scale[k] = np.sum(np.abs(e) * np.abs(x[far]))
                    if len(nr):
                        scale[k] += np.sum(np.abs(pi_entry(self.P[k], vn, gn)) * np.abs(x[nr]))
            self._limit[key], self._scale[key] = out, float(scale.max())
        return self._limit[key]

    def limit(self, key="x"):
        """(given targets,): the near half plus the K-point pi of every panel not in the leaf's near list"""
        return self._rest(key)[self.given]

    def scale(self, key="x"):
        """max_i sum_j |pi_ij| . |x_j|"""
        self._rest(key)
        return self._scale[key]


_REFS = {}


def reference(name):
    if name not in _REFS:
        _REFS[name] = Reference(name)
    return _REFS[name]
