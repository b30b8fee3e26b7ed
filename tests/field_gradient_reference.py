"""The reference of the field gradient (fmmbem_plan_execute_gradient), composed on the CPU with no product code in it.

  gamma             the entry of include/fmmbem.h "Field gradient" in numpy, from the oracle's panel data (centre, area, normal, the K
                    stored points), the vertices and the 16-point rule O.quadrature(17): one (3,) vector per (target, panel).
  Reference         per case: oracle.TargetOracle's trees and lists; the NEAR half = gamma summed over the listed p2p pairs; the
                    FAR half = M per source leaf by O.single_p2m (slot 0 from a call with all-0 flags, slot 1 from one with all-1
                    flags), O.Tables(p).m2m / m2l / l2l over the listed pairs, then the value and the Cartesian gradient of L at the
                    targets by double_layer_reference.local_value_and_gradient (long double, nothing singular on the axis), + for
                    flag 0 and - for flag 1.  values() of the same L is what TargetOracle.matvec gives on far-only targets
                    (tests/test_field_gradient_host.py pins it), which ties the composition to the oracle.
  limit             the expansion-free number an execute converges to as p grows: the near half plus the K-point gamma of every
                    panel NOT in the leaf's near list.  (The all-regime direct sum is not that limit: a far box may hold panels that
                    are `nearby` for the quadrature.)

The cases are the smallest shapes at which the two kernels can go wrong; K = 3, theta = 0.5 throughout."""
import numpy as np

import double_layer_reference as D
from oracle import oracle as O

K = 3
THETA = 0.5


def two_spheres(rec, dist):
    a = O.unit_sphere(rec)
    return np.concatenate([a, O.unit_sphere(rec, center=(dist, 0.0, 0.0))])


def three_balls():                                     # the sources of tests/test_gpu_treecode.py
    s = O.unit_sphere(4) * 0.2
    return np.concatenate([s + np.array(c)[None, None, :] for c in ((0.0, 0.0, 0.0), (1.5, 0.0, 0.0), (12.0, 0.0, 0.0))])


def _dirs(rng, m):
    d = rng.normal(size=(m, 3))
    return d / np.linalg.norm(d, axis=1)[:, None]


def geometry(v):
    pan = O.Oracle(v, K=K, ncrit=1 << 30)
    out = pan.panels()
    pan.close()
    return out


def cloud(v, seed=0):
    """200 points on shells r 1.05 .. 2.45, 40 inside r < 0.9, 30 at 0.3 sqrt(2 A) above a panel's centroid (the near regime), 10
    copies of one point; 40 % flag 1"""
    rng = np.random.default_rng(seed)
    g = geometry(v)
    shell = _dirs(rng, 200) * (1.05 + 1.4 * rng.random(200))[:, None]
    inner = _dirs(rng, 40) * (0.9 * rng.random(40))[:, None]
    pick = rng.choice(len(v), 30, replace=False)
    close = g["center"][pick] + g["normal"][pick] * (0.3 * np.sqrt(2 * g["area"][pick]))[:, None]
    same = np.tile([[0.3, -0.2, 1.1]], (10, 1))
    pts = np.concatenate([shell, inner, close, same])
    flags = (rng.random(len(pts)) < 0.4).astype(np.uint8)
    flags[-10:] = np.arange(10) % 2                     # the copies: both flags, so two bodies of the target tree
    return pts, flags


N_AWKWARD = 16


def make_case(name):
    """dict(v, pts, flags, ncrit)"""
    if name == "two_r3":
        v = two_spheres(3, 3.0)
        pts, flags = cloud(v)
        return dict(v=v, pts=pts, flags=flags, ncrit=16)
    if name == "r4_ncrit8":
        v = O.unit_sphere(4)
        pts, flags = cloud(v)
        g = geometry(v)
        on = g["center"][[5, 140, 300, 500]]            # exactly on panel centroids: the self rule, two per flag
        return dict(v=v, pts=np.concatenate([pts, on]), flags=np.concatenate([flags, np.array([0, 1, 0, 1], np.uint8)]), ncrit=8)
    if name == "big_leaves":
        rng = np.random.default_rng(3)
        pts = _dirs(rng, 700) * (0.3 * rng.random(700) ** (1.0 / 3))[:, None]
        return dict(v=three_balls(), pts=pts, flags=(rng.random(700) < 0.4).astype(np.uint8), ncrit=600)
    if name == "one_row":
        rng = np.random.default_rng(4)
        pts = _dirs(rng, 40) * (1.05 + 1.4 * rng.random(40))[:, None]
        return dict(v=O.unit_sphere(2), pts=pts, flags=(np.arange(40) % 2).astype(np.uint8), ncrit=1)
    if name == "far_only":
        rng = np.random.default_rng(5)
        return dict(v=two_spheres(3, 3.0), pts=20.0 + rng.random((40, 3)), flags=(np.arange(40) % 2).astype(np.uint8), ncrit=16)
    if name == "no_far":
        rng = np.random.default_rng(6)
        pts = _dirs(rng, 30) * (1.05 + 0.25 * rng.random(30))[:, None]
        return dict(v=O.unit_sphere(2), pts=pts, flags=(np.arange(30) % 2).astype(np.uint8), ncrit=64)
    if name == "awkward":
        # two_r3's cloud plus, for eight of its target leaves, the leaf's centre and the point 0.3 side above it, one flag each way
        # (tests/test_gpu_stokes_double_layer.py::awkward): sin a ~ 0 in the spherical chain rule.  The added points are interior
        # to the cloud's and the panels' bounding cube, so the root cube stays; the leaves picked keep room for two more rows.
        base = make_case("two_r3")
        T = O.TargetOracle(base["v"], base["pts"], base["flags"], K=K, theta=THETA, ncrit=base["ncrit"])
        tb = T.boxes("target")
        T.close()
        rows = tb["be"] - tb["bb"]
        leaves = np.nonzero((tb["leaf"] != 0) & (rows >= 3) & (rows <= base["ncrit"] - 2))[0]
        pick = leaves[np.linspace(0, len(leaves) - 1, 8).astype(int)]
        assert len(set(pick.tolist())) == 8
        added = np.concatenate([tb["center"][pick], tb["center"][pick] + np.array([0.0, 0.0, 0.3]) * tb["side"][pick][:, None]])
        add_flags = (np.arange(N_AWKWARD) % 2).astype(np.uint8)
        add_flags[8:] = 1 - add_flags[8:]
        return dict(v=base["v"], pts=np.concatenate([base["pts"], added]), flags=np.concatenate([base["flags"], add_flags]),
                    ncrit=base["ncrit"], awkward_leaves=pick)
    raise KeyError(name)


CASES = ("two_r3", "r4_ncrit8", "big_leaves", "one_row", "far_only", "no_far", "awkward")
_QK = None


def _rules():
    global _QK
    if _QK is None:
        _QK = (O.quadrature(K)[1], O.quadrature(17))
    return _QK


def gamma(t, flag, v, g, far_only=False):
    """(P, 3): gamma(t, panel j) for the P panels of v (P, 3, 3) with geometry g (center, area, normal, quad restricted to them);
    far_only: the K stored points whatever the distance (the limit sum's far part)"""
    wK, (bF, wF) = _rules()
    c, A, n = g["center"], g["area"], g["normal"]
    d = np.linalg.norm(t[None] - c, axis=1)
    with np.errstate(divide="ignore"):
        near = (np.sqrt(2 * A) / d >= 0.5) & (not far_only)
    out = np.zeros((len(v), 3))
    for mask, y, w in ((~near, g["quad"], wK), (near, np.einsum("qk,pkx->pqx", bF, v), wF)):
        if not mask.any():
            continue
        dx = y[mask] - t[None, None]
        r2 = (dx * dx).sum(-1)
        r3 = r2 * np.sqrt(r2)
        wA = w[None] * A[mask][:, None]
        with np.errstate(divide="ignore", invalid="ignore"):     # a target on a centroid meets the rule's first point: the self rule below
            if flag == 0:
                out[mask] = (wA[..., None] * dx / r3[..., None]).sum(1)
            else:
                nm = n[mask][:, None]
                dn = (dx * nm).sum(-1)
                out[mask] = (wA[..., None] * (-nm / r3[..., None] + 3 * (dn / (r3 * r2))[..., None] * dx)).sum(1)
    if not far_only:
        self_ = d < 1e-8
        out[self_] = 2 * np.pi * n[self_] if flag == 0 else 0.0
    return out


def sub(g, idx):
    return {k: a[idx] for k, a in g.items()}


class Reference:
    """One case: the oracle's target plan, its lists, and the composed halves (cached per vector and order)"""

    def __init__(self, name):
        self.name = name
        self.c = c = make_case(name)
        self.v, self.pts, self.flags = c["v"], c["pts"], c["flags"]
        self.T = O.TargetOracle(self.v, self.pts, self.flags, K=K, theta=THETA, ncrit=c["ncrit"])
        self.info = self.T.info()
        self.g = geometry(self.v)
        self.sb, self.tb = self.T.boxes("source"), self.T.boxes("target")
        self.perm = self.T.perm().astype(np.int64)
        tree, given = self.T.target_perm()
        self.tree, self.given = tree.astype(np.int64), given.astype(np.int64)
        self.P, self.F = self.T.target_points()
        self.near = {}
        for s_, t_ in self.T.pairs("p2p"):
            self.near.setdefault(int(t_), []).append(int(s_))
        # the vector the bounds of tests/test_gpu_field_gradient.py were measured with.  One of them depends on it: far_only's error
        # against the limit sum at p = 16 is the truncation of its ONE M2L pair, (r_source / (d - r_target))^16 ~ 1e-7 of the
        # high-order content, and relative to |g| it is 9.1e-9 with this vector, 1.3e-7 .. 4.8e-7 with seeds 2, 3, 8, 99.
        self.x = np.random.default_rng(1).standard_normal(len(self.v))
        self.x2 = np.random.default_rng(99).standard_normal(len(self.v))
        self._near, self._far, self._limit = {}, {}, {}

    def leaf_points(self, b):
        return self.tree[self.tb["bb"][b]:self.tb["be"][b]]

    def leaf_panels(self, s):
        return self.perm[self.sb["bb"][s]:self.sb["be"][s]]

    def near_half(self, x, key):
        """(distinct points, 3)"""
        if key not in self._near:
            out = np.zeros((len(self.P), 3))
            for b in np.nonzero(self.tb["leaf"])[0]:
                lists = [self.leaf_panels(s) for s in self.near.get(int(b), [])]
                if not lists:
                    continue
                idx = np.concatenate(lists)
                vi, gi = self.v[idx], sub(self.g, idx)
                for k in self.leaf_points(b):
                    out[k] = gamma(self.P[k], int(self.F[k]), vi, gi).T @ x[idx]
            self._near[key] = out
        return self._near[key]

    def expansions(self, x, p):
        """L (target boxes, 2, S)"""
        sb, tb = self.sb, self.tb
        S = p * (p + 1) // 2
        Tb = O.Tables(p)
        m2m, m2l, l2l = self.T.pairs("m2m"), self.T.pairs("m2l"), self.T.pairs("l2l")
        M = np.zeros((len(sb["leaf"]), 2, S), dtype=np.complex128)
        read = np.zeros(len(sb["leaf"]), dtype=bool)
        read[m2l[:, 0]] = True
        read[m2m[:, 0]] = True
        for b in np.nonzero((sb["leaf"] != 0) & read)[0]:
            idx = self.leaf_panels(b)
            M[b, 0] = O.single_p2m(0, p, K, self.v[idx], np.zeros(len(idx), np.uint8), x[idx], sb["center"][b])[0]
            M[b, 1] = O.single_p2m(0, p, K, self.v[idx], np.ones(len(idx), np.uint8), x[idx], sb["center"][b])[1]
        for c_, par in m2m:
            for s in range(2):
                M[par, s] += Tb.m2m(M[c_, s], sb["center"][par] - sb["center"][c_])
        L = np.zeros((len(tb["leaf"]), 2, S), dtype=np.complex128)
        for s_, t_ in m2l:
            for s in range(2):
                L[t_, s] += Tb.m2l(M[s_, s], tb["center"][t_] - sb["center"][s_])
        for par, c_ in l2l:
            for s in range(2):
                L[c_, s] += Tb.l2l(L[par, s], tb["center"][c_] - tb["center"][par])
        return L

    def far_half(self, x, key, p):
        """(values (distinct points,), gradients (distinct points, 3)) of the local expansions, signed by flag"""
        if (key, p) not in self._far:
            L = self.expansions(x, p)
            val, grad = np.zeros(len(self.P)), np.zeros((len(self.P), 3))
            for b in np.nonzero(self.tb["leaf"])[0]:
                here = self.leaf_points(b)
                for f in (0, 1):
                    sel = here[self.F[here] == f]
                    if len(sel) == 0 or not np.any(L[b, f]):
                        continue
                    va, gr = D.local_value_and_gradient(p, L[b, f], self.tb["center"][b], self.P[sel])
                    sg = -1.0 if f else 1.0
                    val[sel] = sg * va[0].astype(np.float64)
                    grad[sel] = sg * gr[0].astype(np.float64)
            self._far[(key, p)] = (val, grad)
        return self._far[(key, p)]

    def vector(self, key):
        return self.x if key == "x" else self.x2

    def gradient(self, p, key="x"):
        """(given targets, 3): the composed reference of an execute at order p"""
        x = self.vector(key)
        return (self.near_half(x, key) + self.far_half(x, key, p)[1])[self.given]

    def values(self, p, key="x"):
        """(given targets,): the far half's VALUES by the same L (what TargetOracle.matvec gives where there is no near pair)"""
        return self.far_half(self.vector(key), key, p)[0][self.given]

    def limit(self, key="x"):
        """(given targets, 3): the near half plus the K-point gamma of every panel not in the leaf's near list"""
        if key not in self._limit:
            x = self.vector(key)
            out = self.near_half(x, key).copy()
            for b in np.nonzero(self.tb["leaf"])[0]:
                rest = np.ones(len(self.v), dtype=bool)
                for s in self.near.get(int(b), []):
                    rest[self.leaf_panels(s)] = False
                idx = np.nonzero(rest)[0]
                vi, gi = self.v[idx], sub(self.g, idx)
                for k in self.leaf_points(b):
                    out[k] += gamma(self.P[k], int(self.F[k]), vi, gi, far_only=True).T @ x[idx]
            self._limit[key] = out
        return self._limit[key][self.given]


_REFS = {}


def reference(name):
    if name not in _REFS:
        _REFS[name] = Reference(name)
    return _REFS[name]
