"""Inputs and the host reference shared by tests/test_field_near_cases_host.py and tests/test_gpu_field_near_soup.py: the matrix-free
near kernels of the field quantities (csrc/kernels_field.hip: near_field_kernel<GradientQ / PressureQ / VelocityGradientQ>,
near_flow_kernel, near_representation_kernel) and the field template of csrc/kernels_direct.hip on the ragged soups of
tests/near_form_cases.py, row by row against a sum in np.longdouble with no product code in it.

Sources   near_form_cases.case_input: Laplace (101) (102) (103) (106) (107), Stokes (201) (203).
Targets   targets(case): seeded, built from the panels' geometry -- above the centroids of groups of neighbouring panels at 0.05,
          0.3, 1.9 and 2.1 sqrt(2 A) (the last two on either side of the rule selection sqrt(2 A) / d >= 0.5; neighbours, so that the
          lanes of one wavefront disagree about the regime of one source panel), exactly on centroids (the self value), in the plane
          of a panel outside it, ten copies of one point, a handful far from every panel, and tight clusters round the point
          2 sqrt(2 A) above a centroid whose rows fall on both sides of the rule selection; CLUSTERS holds their sizes, chosen so that
          target leaves of 1, exactly 64, 65 and more than 128 rows occur (tests/test_field_near_cases_host.py holds that).  No point
          lies on a quadrature node, where include/fmmbem.h states no value.
No far field   plans take theta = THETA, at which the dual walk accepts no pair (stats()["m2l_pairs"] == 0, read from a host-only
          plan): an execute is the near kernel alone over every (target leaf, source leaf) pair, the same bits at every order.
Reference the pair functions of include/fmmbem.h "Field gradient", "Field pressure", "Field velocity gradient" and "Representation
          execute" in numpy, generic over the dtype (laplace_pairs, stokes_pairs, semi_analytic): the self value, the K-point rule
          on the oracle's stored points, the fine rule on the vertices, the semi-analytic G.  The regime of a pair is decided once, in
          double, by the header's expressions; the arithmetic then runs in np.longdouble from the same double vertices, stored points
          and weights, and a row is summed in long double over exactly the panels of the plan's p2p list (plan_layout).
Inputs    the five vectors of near_form_cases.vectors: normal, one entry x 1e8, three unit vectors.

The row bound, for quantity Q, row i, component c and input x:

    |got_ic - ref_ic| <= (C_Q + T_i) 2^-53 S_i,     S_i = sum_j |x_j| sum_q w_q A_j mu_Q(t_i, y_jq) (1 + |y_jq|_inf / r_jq)

mu_Q the integrand with every term of every inner sum in absolute value, |d_c| <= r and |n| = 1 used:
    G0  gradient of the single layer   1 / r^2              G1  gradient of the double layer   4 / r^3
    E0  value of the single layer      1 / r                E1  value of the double layer      sum_e |d_e| |n_e| / r^3
    PI  pressure                       1 / r^2  (|x_j| = |f_j|_1)
    VG  velocity gradient              6 / (2 mu r^2): (|f_k| |d_m| + delta_km |s| + |d_k| |f_m|) / r^3 <= 3 |f|_1 / r^2 and
                                       3 |s| |d_k| |d_m| / r^5 <= 3 |f|_1 / r^2
    E0 in the nearby regime (the semi-analytic G): per edge sum_k |w_k dt / 2| (R_k + |z|) (1 + |y|_inf / |a_x|), a_x the distance
    of the target's foot from the edge's line -- R - |z| taken as R + |z|, and the rounding of the rotated coordinates carried by
    1 / |a_x| as (1 + |y| / r) carries that of t - y.  Nothing caps 1 / |a_x|: a foot close to an edge's line loosens that pair's
    scale (the edge's term falls with a_x, so the product stays finite).  On the cases the factor reaches 1.7e5 and mE0 / |E0|
    6.9e6 at the worst nearby pair, 150 to 1000 at the median ((106): 2.4e4) (E0_AMP_MAX; tests/test_field_near_cases_host.py prints and holds them);
    c_ref(E0) = 10.6 says the float64 evaluation does err by that scale on its worst row.
(1 + |y| / r) carries the rounding of t - y and of fine-rule points formed from vertices.  A self entry adds |entry| |x_j|.  T_i: the
quadrature terms summed into the row that are not exact zeros -- points of the pair's rule over the panels with x_j != 0, times 3
for Stokes (a point adds d . f) and counted per layer for the representation; a term with x_j = 0 is an exact 0 and adding it rounds
nothing.  T_i 2^-53 S_i is the worst case of a double sum of T_i terms in any order, with or without FMA.  A row with S = 0 must be
exactly 0.  No row is exempt.  The representation takes the sum of its layers' bounds.

C_Q = 8 max(c_ref(Q), 1), c_ref(Q) = max |f64 - long double| / (2^-53 S) of THESE numpy functions over all cases, rules, rows and
vectors (C_REF below; tests/test_field_near_cases_host.py measures it again and holds it to the record).  The 8 is three bits for FMA
contraction, another order within a term and the device's reciprocal square root, which is not correctly rounded.

Measured.  c_ref on the reference (worst case and rule; every worst row is under the vector with one entry x 1e8), the constant
it gives, and the worst ratio of a device row to its bound on the MI355X (normal vector / one entry x 1e8 / unit vectors):

    Q    c_ref                    recorded  C_Q     kernel                                        worst device row / bound
    G0   16.043 (101) K = 4       16.05    128.4  near_field_kernel<GradientQ>, flags all 0     0.012 / 0.0095 / 0.037
                                                    direct_field_partial_kernel, gradient, all 0  0.0077 / 0.0065 / 0.016
    G1    6.150 (101) K = 1        6.16     49.3  near_field_kernel<GradientQ>, flags all 1     0.0077 / 0.013 / 0.060
                                                    direct_field_partial_kernel, gradient, all 1  0.0054 / 0.0083 / 0.032
    G0 / G1 by the row's flag                       near_field_kernel<GradientQ>, flags mixed     0.012 / 0.013 / 0.060
                                                    direct_field_partial_kernel, gradient, mixed  0.0054 / 0.0070 / 0.028
    E0   10.592 (107) K = 3       10.60     84.8  near_representation_kernel<true, false>       0.022 / 0.012 / 0.035
    E1    8.186 (101) K = 13       8.19     65.5  near_representation_kernel<false, true>       0.026 / 0.0094 / 0.032
                                                    near_representation_kernel<true, true>        0.026 / 0.012 / 0.035
    PI   19.630 (203)             19.63    157.0  near_field_kernel<PressureQ>                  1.8e-4 / 0.0021 / 0.022
                                                    near_flow_kernel, pressure                    1.8e-4 / 0.0021 / 0.022
                                                    direct_field_partial_kernel, pressure         1.8e-4 / 0.0053 / 0.022
    VG    3.028 (203)              3.03     24.2  near_field_kernel<VelocityGradientQ>          6.7e-5 / 0.0013 / 0.052
                                                    near_flow_kernel, velocity gradient           6.7e-5 / 0.0013 / 0.052
                                                    direct_field_partial_kernel, velocity grad.   6.7e-5 / 0.0011 / 0.052
         the trace |G00 + G11 + G22| against the    near_field_kernel<VelocityGradientQ>, flow    5.6e-5 / 9.4e-4 / 0.038
         row's own bound, once                      direct_field_partial_kernel                   4.7e-5 / 0.0016 / 0.038

No device ratio is above 1: no kernel was found wrong.  The worst rows are unit-vector rows -- one pair, T_i a single rule's points --
where the device is 16 to 45 times inside the bound, about what C_Q / c_ref = 8 and a device entry that errs less than the numpy
float64 evaluation leave."""
import numpy as np

import near_form_cases as N
from oracle import oracle as O

U53 = 2.0 ** -53
THETA = 1e-6
LAPLACE_CASES = (101, 102, 103, 106, 107)
STOKES_CASES = (201, 203)
LAPLACE_K = (1, 3, 4, 13)                              # the quad_k the gradient execute is run at; the representation: 3 and 13
HEIGHTS = (0.05, 0.3, 1.9, 2.1)
# case -> (points, radius / sqrt(2 A)) of the tight clusters; the first sits over the panel of largest area and reaches across the rule
# selection, the others are small enough for no box face to cut them: they size a leaf
CLUSTERS = {101: ((130, 0.3),), 102: ((130, 0.3), (58, 0.02)), 103: ((130, 0.3),), 106: ((130, 0.3),), 107: ((130, 0.3), (64, 0.02)),
            201: ((130, 0.3),), 203: ((150, 0.3),)}
# case -> (largest 1 + |y|_inf / |a_x| of a nearby pair's edges, largest mE0 / |E0|) as measured, rounded up: how loose the E0 scale gets
E0_AMP_MAX = {101: (1.7e5, 6.9e6), 102: (1.75e5, 3.2e6), 103: (3.4e4, 5.9e5), 106: (4.3e3, 2.1e5), 107: (9.3e4, 3.1e5)}
QUANTITIES = ("G0", "G1", "E0", "E1", "PI", "VG")
# c_ref(Q) as measured on this module's functions, rounded up in the second decimal
# (tests/test_field_near_cases_host.py::test_float64_reference_stays_within_c_ref measures it again)
C_REF = {"G0": 16.05, "G1": 6.16, "E0": 10.60, "E1": 8.19, "PI": 19.63, "VG": 3.03}
C_Q = {q: 8.0 * max(c, 1.0) for q, c in C_REF.items()}
# kernels_field.hip: panels per LDS batch of the near loops
REC_DOUBLES, REP_REC_DOUBLES = 1100, 64 * 18


def near_batch(k, rec=8):
    """near_batch(rec + 3 K) of kernels_field.hip: rec = 8 (gradient), 7 (pressure, velocity gradient, flow)"""
    return max(1, min(64, REC_DOUBLES // (rec + 3 * k)))


def representation_batch(k):
    return max(1, min(64, REP_REC_DOUBLES // (9 + 3 * k)))


def is_stokes(case):
    return case in STOKES_CASES


# ---------------------------------------------------------------------------------------------------------------- geometry
_GEOM = {}


def sources(case):
    return N.case_input(case, False)[0]


def geometry(case, K=None):
    """the oracle's panel data at rule K: center, normal, area, quad (P, K points, 3); Stokes: K = STOKES_K"""
    K = (N.STOKES_K if is_stokes(case) else 3) if K is None else K
    if (case, K) not in _GEOM:
        v = sources(case)
        o = (O.StokesOracle(v, K=K, K_fine=N.STOKES_KFINE, mu=N.STOKES_MU, ncrit=1 << 30) if is_stokes(case)
             else O.Oracle(v, K=K, ncrit=1 << 30))
        g = o.panels()
        o.close()
        for a in g.values():
            a.setflags(write=False)
        _GEOM[(case, K)] = g
    return _GEOM[(case, K)]


def rules(case, K=None):
    """(weights of the K rule, (barycentric points, weights) of the fine rule)"""
    if is_stokes(case):
        return O.quadrature(N.STOKES_K)[1], O.quadrature(N.STOKES_KFINE)
    return O.quadrature(3 if K is None else K)[1], O.quadrature(17)


def _ball(rng, m):
    d = rng.normal(size=(m, 3))
    return d / np.linalg.norm(d, axis=1)[:, None] * (rng.random(m) ** (1.0 / 3))[:, None]


_TARGETS = {}


def targets(case):
    """(points (M, 3), flags (M,) mixed, groups): groups names the slices of the point kinds"""
    if case in _TARGETS:
        return _TARGETS[case]
    rng = np.random.default_rng(1000 + case)
    v, g = sources(case), geometry(case)
    c, nrm, s = g["center"], g["normal"], np.sqrt(2 * g["area"])
    n = len(v)
    parts, groups, at = [], {}, 0

    def add(name, pts):
        nonlocal at
        parts.append(np.asarray(pts, dtype=np.float64).reshape(-1, 3))
        groups[name] = slice(at, at + len(parts[-1]))
        at += len(parts[-1])

    above = []
    for seed in rng.choice(n, min(8, n), replace=False):
        nb = np.argsort(np.linalg.norm(c - c[seed], axis=1))[:4]           # the panel and its nearest neighbours
        for j in nb:
            for h in HEIGHTS:
                above.append(c[j] + nrm[j] * (h * s[j]))
    add("above", above)
    on = rng.choice(n, min(6, n), replace=False)
    add("centroid", c[on])
    pl = rng.choice(n, min(6, n), replace=False)
    to_v0 = v[pl, 0] - c[pl]                                                # in the plane, through vertex 0 and beyond it
    add("in_plane", np.concatenate([c[pl] + 1.5 * to_v0, c[pl] + 4.0 * to_v0]))
    j = int(rng.integers(n))
    add("copies", np.tile(c[j] + nrm[j] * (0.7 * s[j]), (10, 1)))
    lo, hi = v.reshape(-1, 3).min(axis=0), v.reshape(-1, 3).max(axis=0)
    add("far", hi + (hi - lo).max() * (1.0 + rng.random((5, 3))))
    order = np.argsort(-g["area"])
    for k, (size, radius) in enumerate(CLUSTERS[case]):
        j = int(order[min(k, n - 1)])
        add("cluster%d" % k, c[j] + nrm[j] * (2.0 * s[j]) * (1 if k % 2 == 0 else -1) + radius * s[j] * _ball(rng, size))
    pts = np.concatenate(parts)
    flags = (rng.random(len(pts)) < 0.5).astype(np.uint8)
    flags[groups["copies"]] = np.arange(10) % 2
    pts.setflags(write=False)
    flags.setflags(write=False)
    _TARGETS[case] = (pts, flags, groups)
    return _TARGETS[case]


def flag_sets(case):
    pts, mixed, _ = targets(case)
    return {"all0": np.zeros(len(pts), np.uint8), "all1": np.ones(len(pts), np.uint8), "mixed": mixed}


# ---------------------------------------------------------------------------------------------------------------- plans
def make_plan(fb, case, K=None, flags=None, host_only=False, p_max=13):
    """The target plan (Laplace; flags: per target, None: all 0) or the field plan (Stokes, every target VELOCITY) of a case at THETA"""
    v, _, ncrit = N.case_input(case, False)
    pts = targets(case)[0]
    opts = fb.FMMOptions()
    opts.set_mac_theta(THETA)
    opts.set_max_per_box(ncrit)
    if is_stokes(case):
        kern = fb.StokesSphericalBEM(p_max, N.STOKES_K, N.STOKES_MU)
        kern.set_Kfine(N.STOKES_KFINE)
        return fb.FMM_plan(kern, v, opts, p_max=p_max, host_only=host_only).field_plan(pts)
    kern = fb.LaplaceSphericalBEM(p_max, 3 if K is None else K)
    return fb.FMM_plan(kern, v, opts, p_max=p_max, host_only=host_only, targets=pts, target_bc=flags)


def plan_layout(plan):
    """dict: leaves -- per target leaf in tree order (given-target index of each row in the kernel's row order, source leaves listed);
    mask (M, P) -- 1 where panel j is in the p2p list of target i's leaf; src_leaves -- tree-order (first row, rows) of the source
    leaves; perm -- tree position -> panel"""
    sb, tb = plan.boxes(), plan.target_boxes()
    perm = plan.perm().astype(np.int64)
    tree, given = (a.astype(np.int64) for a in plan.target_perm())
    first = np.full(len(tree), -1, dtype=np.int64)
    for k in range(len(given) - 1, -1, -1):
        first[given[k]] = k
    near = {}
    for s_, t_ in plan.pairs("p2p"):
        near.setdefault(int(t_), []).append(int(s_))
    mask = np.zeros((len(given), len(perm)))
    leaves = []
    for b in np.nonzero(tb["leaf"])[0]:
        pts_here = tree[tb["bb"][b]:tb["be"][b]]
        srcs = near.get(int(b), [])
        leaves.append((first[pts_here], srcs))
        for s_ in srcs:
            cols = perm[sb["bb"][s_]:sb["be"][s_]]
            rows = np.nonzero(np.isin(given, pts_here))[0]
            mask[np.ix_(rows, cols)] = 1
    src_leaves = sorted((int(sb["bb"][b]), int(sb["be"][b] - sb["bb"][b])) for b in np.nonzero(sb["leaf"])[0])
    return dict(leaves=leaves, mask=mask, src_leaves=src_leaves, perm=perm)


# ---------------------------------------------------------------------------------------------------------------- pair functions
_XK = (-9.06179846e-01, -5.38469310e-01, 1.78162900e-17, 9.06179846e-01, 5.38469310e-01)
_WK = (0.23692689, 0.47862867, 0.56888889, 0.23692689, 0.47862867)


def _edge_angle(z, x, v1, v2):
    """sum_k w_k (R_k - |z|) dt / 2 over the 5 Gauss points in the polar angle, and the same with every factor in absolute value
    and R + |z|"""
    t1, t2 = np.arctan2(v1, x), np.arctan2(v2, x)
    dt, tm = t2 - t1, (t2 + t1) / 2
    az = np.abs(z)
    G, Ga = np.zeros_like(z), np.zeros_like(z)
    for xk, wk in zip(_XK, _WK):
        tk = dt / 2 * z.dtype.type(xk) + tm
        Rt = x / np.cos(tk)
        R = np.sqrt(Rt * Rt + z * z)
        G = G + z.dtype.type(wk) * (R - az) * dt / 2
        Ga = Ga + np.abs(z.dtype.type(wk) * dt / 2) * (R + az)
    return G, Ga


def _edge_term(v1, v2, p):
    """one edge v1 -> v2 in the panel's plane, the target's foot at the origin, height p: (term, absolute sum, |a_x|)"""
    e = v2 - v1
    ln = np.sqrt((e * e).sum(-1))
    ux, uy = e[:, 0] / ln, e[:, 1] / ln
    ax, ay = -uy * v1[:, 0] + ux * v1[:, 1], ux * v1[:, 0] + uy * v1[:, 1]
    by = ux * v2[:, 0] + uy * v2[:, 1]
    flip = ax < 0
    ax, ay, by = np.where(flip, -ax, ax), np.where(flip, -ay, ay), np.where(flip, -by, by)
    zero = np.zeros_like(ax)
    cross = ((ay > 0) & (by < 0)) | ((ay < 0) & (by > 0))
    g1, a1 = _edge_angle(p, ax, zero, ay)
    g2, a2 = _edge_angle(p, ax, by, zero)
    g3, a3 = _edge_angle(p, ax, ay, by)
    return np.where(cross, g1 + g2, -g3), np.where(cross, a1 + a2, a3), ax, flip, cross


def semi_analytic(y0, y1, y2, x, seen=None):
    """int 1 / |x - y| dS over the flat triangles (n, 3) seen from the points x (n, 3), semi-analytically -- the E0 of a nearby pair
    (include/fmmbem.h "Representation execute": the entry of a flag-0 target) -- and its tolerance scale (module docstring).
    seen: a dict that receives, per edge, (n,) arrays: whether the edge took the mirrored frame (flip), was cut at the foot of the
    target (cross), and its 1 + |y|_inf / |a_x| (amp)"""
    dt = x.dtype
    xp, e1, e2 = x - y0, y1 - y0, y2 - y0
    X = e1 / np.sqrt((e1 * e1).sum(-1))[:, None]
    Z = np.cross(e1, e2)
    Z = Z / np.sqrt((Z * Z).sum(-1))[:, None]
    Y = np.cross(Z, X)
    rot = np.stack([X, Y, Z], axis=1)                                       # (n, 3, 3) rows X, Y, Z
    q1, q2, xq = (np.einsum("nab,nb->na", rot, a) for a in (e1, e2, xp))
    q0 = np.zeros_like(q1)
    f = [np.stack([q[:, 0] - xq[:, 0], q[:, 1] - xq[:, 1], q[:, 2]], axis=1) for q in (q0, q1, q2)]
    ymax = np.maximum(np.abs(x).max(-1), np.maximum(np.abs(y0).max(-1), np.maximum(np.abs(y1).max(-1), np.abs(y2).max(-1))))
    G, S = np.zeros(len(x), dtype=dt), np.zeros(len(x), dtype=dt)
    for a, b in ((0, 1), (1, 2), (2, 0)):
        g, ga, ax, flip, cross = _edge_term(f[a], f[b], xq[:, 2])
        amp = 1 + np.where(ax > 0, ymax / np.where(ax > 0, ax, 1), 0)
        G = G + g
        S = S + ga * amp
        if seen is not None:
            for name, a in (("flip", flip), ("cross", cross), ("amp", amp.astype(np.float64))):
                seen.setdefault(name, []).append(a)
    return G, S


def regimes(t, g):
    """(self, nearby) (T, P) bool, decided in double by the header's expressions: dist < 1e-8; sqrt(2 A) / dist >= 0.5"""
    d = np.linalg.norm(t[:, None, :] - g["center"][None, :, :], axis=2)
    self_ = d < 1e-8
    with np.errstate(divide="ignore"):
        near = (np.sqrt(2 * g["area"])[None, :] / d >= 0.5) & ~self_
    return self_, near


def _laplace_points(dt, dx, wA, nrm, ymax):
    """One rule's points for every pair of the leading axes: dx = y - t (..., q, 3), wA (..., q), nrm (..., 3), ymax (..., q).
    The four integrands summed over q and their absolute scales."""
    r2 = (dx * dx).sum(-1)
    r = np.sqrt(r2)
    r3 = r2 * r
    dn = (dx * nrm[..., None, :]).sum(-1)
    adn = (np.abs(dx) * np.abs(nrm[..., None, :])).sum(-1)
    amp = 1 + ymax / r
    f = wA / r3
    out = dict(E0=(wA / r).sum(-1), E1=(f * dn).sum(-1), G0=(f[..., None] * dx).sum(-2),
               G1=(f[..., None] * (3 * (dn / r2)[..., None] * dx - nrm[..., None, :])).sum(-2),
               mE0=(wA / r * amp).sum(-1), mE1=(f * adn * amp).sum(-1), mG0=(wA / r2 * amp).sum(-1), mG1=(4 * f * amp).sum(-1))
    return out


def laplace_pairs(t, v, g, K, dt=np.longdouble, chunk=32, force_far=None):
    """Every (target, panel) pair of a Laplace case in dtype dt: dict of E0, E1 (T, P), G0, G1 (T, P, 3) -- the entries of a flag-0 /
    flag-1 target and the two gradients gamma0 / gamma1 of include/fmmbem.h -- their scales mE0, mE1, mG0, mG1 (T, P) and the terms
    per pair nq (T, P; nqE0 for E0, whose nearby value is the semi-analytic G).  force_far: (target, panel) pairs taken by the K-point
    rule whatever their regime (the teeth of the host test)."""
    wK, (bF, wF) = O.quadrature(K)[1], O.quadrature(17)
    T, P = len(t), len(v)
    self_, near = regimes(t, g)
    if force_far is not None:
        for i, j in force_far:
            self_[i, j] = near[i, j] = False
    A, nrm, c = g["area"].astype(dt), g["normal"].astype(dt), g["center"]
    yK = g["quad"].astype(dt)
    ymaxK = np.maximum(np.abs(g["quad"]).max(-1)[None], np.abs(t).max(-1)[:, None, None]).astype(dt)       # (T, P, K)
    tl, vl = t.astype(dt), v.astype(dt)
    out = {k: np.zeros((T, P) + ((3,) if k in ("G0", "G1") else ()), dtype=dt) for k in ("E0", "E1", "G0", "G1", "mE0", "mE1", "mG0", "mG1")}
    far = ~self_ & ~near
    with np.errstate(divide="ignore", invalid="ignore"):
        for a in range(0, T, chunk):
            b = min(T, a + chunk)
            part = _laplace_points(dt, yK[None] - tl[a:b, None, None, :], wK.astype(dt)[None, None, :] * A[None, :, None],
                                   np.broadcast_to(nrm[None], (b - a, P, 3)), ymaxK[a:b])
            for k, arr in part.items():
                m = far[a:b] if arr.ndim == 2 else far[a:b, :, None]
                out[k][a:b] = np.where(m, arr, 0)
    nq = np.where(far, len(wK), 0)
    nqE0 = nq.copy()
    ti, pj = np.nonzero(near)
    if len(ti):
        y = np.einsum("qk,nkx->nqx", bF.astype(dt), vl[pj])
        ymax = np.maximum(np.abs(y).max(-1), np.abs(tl[ti]).max(-1)[:, None])
        part = _laplace_points(dt, y - tl[ti][:, None, :], wF.astype(dt)[None, :] * A[pj][:, None], nrm[pj], ymax)
        for k in ("E1", "G0", "G1", "mE1", "mG0", "mG1"):
            out[k][ti, pj] = part[k]
        nq[ti, pj] = len(wF)
    si, sj = np.nonzero(self_)
    two_pi = 2 * dt(np.pi)                                                  # the double 2 pi of the header, as the device takes it
    out["E1"][si, sj] = two_pi
    out["mE1"][si, sj] = two_pi
    out["G0"][si, sj] = two_pi * nrm[sj]
    out["mG0"][si, sj] = two_pi
    nq[si, sj] = 1
    ei, ej = np.nonzero(near | self_)                                       # E0: the semi-analytic G, at the self point too
    if len(ei):
        out["E0"][ei, ej], out["mE0"][ei, ej] = semi_analytic(vl[ej, 0], vl[ej, 1], vl[ej, 2], tl[ei])
        nqE0[ei, ej] = 30
    out.update(nq=nq, nqE0=nqE0, self_=self_, near=near)
    return out


def _stokes_points(dt, d, wA, ymax, mu):
    """One rule's points: d = t - y (..., q, 3): pi (..., 3), Gamma (..., 3, 3, 3) [k][m][e] and the two scales"""
    r2 = (d * d).sum(-1)
    ok = r2 >= 1e-8                                                         # a quadrature point with |d|^2 < 1e-8 contributes 0
    r = np.sqrt(np.where(ok, r2, 1))
    f3 = np.where(ok, wA / (r2 * r), 0)
    f5 = np.where(ok, wA / (r2 * r2 * r), 0)
    amp = 1 + ymax / r
    I = np.eye(3, dtype=dt)
    T3 = (-np.einsum("ke,...m->...kme", I, d) + np.einsum("km,...e->...kme", I, d) + np.einsum("me,...k->...kme", I, d))
    T5 = np.einsum("...k,...m,...e->...kme", d, d, d)
    gam = (f3[..., None, None, None] * T3 - 3 * f5[..., None, None, None] * T5).sum(-4) / (2 * dt(mu))
    m2 = np.where(ok, wA / r2 * amp, 0).sum(-1)
    return dict(PI=(f3[..., None] * d).sum(-2), VG=gam, mPI=m2, mVG=6 * m2 / (2 * dt(mu)))


def stokes_pairs(t, v, g, dt=np.longdouble, chunk=16, force_far=None, mu=N.STOKES_MU):
    """Every (target, panel) pair of a Stokes case in dtype dt: PI (T, P, 3), VG (T, P, 3, 3, 3) [k][m][e] with the 1 / (2 mu), the
    scales mPI, mVG (T, P) and the points per pair nq.  A self pair contributes 0 to both."""
    wK, (bF, wF) = O.quadrature(N.STOKES_K)[1], O.quadrature(N.STOKES_KFINE)
    T, P = len(t), len(v)
    self_, near = regimes(t, g)
    if force_far is not None:
        for i, j in force_far:
            self_[i, j] = near[i, j] = False
    A = g["area"].astype(dt)
    yK = g["quad"].astype(dt)
    ymaxK = np.maximum(np.abs(g["quad"]).max(-1)[None], np.abs(t).max(-1)[:, None, None]).astype(dt)
    tl, vl = t.astype(dt), v.astype(dt)
    out = dict(PI=np.zeros((T, P, 3), dtype=dt), VG=np.zeros((T, P, 3, 3, 3), dtype=dt), mPI=np.zeros((T, P), dtype=dt),
               mVG=np.zeros((T, P), dtype=dt))
    far = ~self_ & ~near
    for a in range(0, T, chunk):
        b = min(T, a + chunk)
        with np.errstate(divide="ignore", invalid="ignore"):
            part = _stokes_points(dt, tl[a:b, None, None, :] - yK[None], wK.astype(dt)[None, None, :] * A[None, :, None], ymaxK[a:b], mu)
        for k, arr in part.items():
            out[k][a:b] = np.where(far[a:b].reshape(far[a:b].shape + (1,) * (arr.ndim - 2)), arr, 0)
    nq = np.where(far, len(wK), 0)
    ti, pj = np.nonzero(near)
    if len(ti):
        y = np.einsum("qk,nkx->nqx", bF.astype(dt), vl[pj])
        ymax = np.maximum(np.abs(y).max(-1), np.abs(tl[ti]).max(-1)[:, None])
        with np.errstate(divide="ignore", invalid="ignore"):
            part = _stokes_points(dt, tl[ti][:, None, :] - y, wF.astype(dt)[None, :] * A[pj][:, None], ymax, mu)
        for k, arr in part.items():
            out[k][ti, pj] = arr
        nq[ti, pj] = len(wF)
    out.update(nq=nq, self_=self_, near=near)
    return out


_PAIRS = {}
PAIRS_KEPT = 4


def pairs(case, K=None, dt=np.longdouble):
    """the pair arrays of a case (cached, read-only): laplace_pairs at rule K or stokes_pairs"""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "np.longdouble is no extended type on this host: the reference would be double"
    K = None if is_stokes(case) else (3 if K is None else K)
    key = (case, K, np.dtype(dt).name)
    if key not in _PAIRS:
        t, v = targets(case)[0], sources(case)
        E = stokes_pairs(t, v, geometry(case), dt) if is_stokes(case) else laplace_pairs(t, v, geometry(case, K), K, dt)
        for a in E.values():
            a.setflags(write=False)
        while len(_PAIRS) >= PAIRS_KEPT:                                     # the rows made from them are what the tests share
            del _PAIRS[next(iter(_PAIRS))]
        _PAIRS[key] = E
    return _PAIRS[key]


# ---------------------------------------------------------------------------------------------------------------- rows and bounds
def vectors(case, seed_shift=0):
    """near_form_cases.vectors on the case's oracle: (5, unknowns) and the names"""
    o = N.make_oracle(O, case, False)
    X, names = N.vectors(o, case + seed_shift)
    o.close()
    return X, names


def _terms(x, nq, mask, per=1):
    """T_i: the quadrature terms of the row's listed panels whose x_j is not 0"""
    live = (np.abs(x).reshape(nq.shape[1], -1).sum(-1) != 0)
    return per * ((nq * mask) @ live.astype(np.float64))


def row(E, quantity, x, mask, flags=None):
    """(value, S, T) of one input vector over the listed panels, in E's dtype: value (M,) / (M, 3) / (M, 3, 3); S, T (M,).
    quantity: "gradient" (flags: per target), "pressure", "velocity_gradient", or ("representation", part) with x = (sigma, mu),
    either None, and part "value" / "gradient"; the representation's S is (S_sigma, S_mu) and T per layer."""
    dt = E["mPI" if "PI" in E else "mG0"].dtype
    full = bool(np.all(mask == 1))

    def listed(a):                                                          # the entries of the listed pairs
        return a if full else a * mask.astype(dt).reshape(mask.shape + (1,) * (a.ndim - 2))

    if quantity == "gradient":
        xl = np.asarray(x, dtype=dt)
        f = np.asarray(flags).astype(bool)
        val = np.where(f[:, None], np.einsum("tpc,p->tc", listed(E["G1"]), xl), np.einsum("tpc,p->tc", listed(E["G0"]), xl))
        S = np.where(f, listed(E["mG1"]) @ np.abs(xl), listed(E["mG0"]) @ np.abs(xl))
        return val, S, _terms(x, E["nq"], mask)
    if quantity == "pressure":
        xl = np.asarray(x, dtype=dt).reshape(-1, 3)
        return np.einsum("tpe,pe->t", listed(E["PI"]), xl), listed(E["mPI"]) @ np.abs(xl).sum(-1), _terms(x, E["nq"], mask, 3)
    if quantity == "velocity_gradient":
        xl = np.asarray(x, dtype=dt).reshape(-1, 3)
        return np.einsum("tpkme,pe->tkm", listed(E["VG"]), xl), listed(E["mVG"]) @ np.abs(xl).sum(-1), _terms(x, E["nq"], mask, 3)
    _, part = quantity
    sigma, mu = x
    shape = (len(mask),) + ((3,) if part == "gradient" else ())
    val, S, T = np.zeros(shape, dtype=dt), [np.zeros(len(mask), dtype=dt)] * 2, np.zeros(len(mask))
    for layer, (xs, sign) in enumerate(((sigma, 1), (mu, -1))):
        if xs is None:
            continue
        xl = np.asarray(xs, dtype=dt)
        key = ("G%d" if part == "gradient" else "E%d") % layer
        e = listed(E[key])
        val = val + sign * (np.einsum("tpc,p->tc", e, xl) if part == "gradient" else e @ xl)
        S[layer] = listed(E["m" + key]) @ np.abs(xl)
        T = T + _terms(xs, E["nqE0"] if key == "E0" else E["nq"], mask)
    return val, tuple(S), T


def bound(quantity, S, T, flags=None):
    """(C_Q + T_i) 2^-53 S_i per row (module docstring), in double"""
    if quantity == "gradient":
        C = np.where(np.asarray(flags).astype(bool), C_Q["G1"], C_Q["G0"])
    elif quantity == "pressure":
        C = C_Q["PI"]
    elif quantity == "velocity_gradient":
        C = C_Q["VG"]
    else:
        k = "G" if quantity[1] == "gradient" else "E"
        return ((C_Q[k + "0"] + T) * U53 * S[0] + (C_Q[k + "1"] + T) * U53 * S[1]).astype(np.float64)
    return ((C + T) * U53 * S).astype(np.float64)


def ratios(got, ref, bnd):
    """|got - ref| / bound per row (the worst component of the row); a row whose bound is 0 must be exactly 0: inf otherwise"""
    d = np.abs(np.asarray(got, dtype=np.longdouble) - ref).astype(np.float64).reshape(len(bnd), -1).max(-1)
    if not np.all(np.isfinite(d)):
        return np.full(len(bnd), np.inf)
    return np.where(bnd > 0, d / np.where(bnd > 0, bnd, 1.0), np.where(d > 0, np.inf, 0.0))


def c_ref_of(E64, El, quantity, x, mask, flags=None):
    """max |f64 - long double| / (2^-53 S) over the rows of one vector; per layer for the representation's parts"""
    v64, _, _ = row(E64, quantity, x, mask, flags)
    vl, S, _ = row(El, quantity, x, mask, flags)
    S = S[0] + S[1] if isinstance(S, tuple) else S
    d = np.abs(v64.astype(np.longdouble) - vl).reshape(len(mask), -1).max(-1)
    ok = S > 0
    assert np.all(d[~ok] == 0)
    return float((d[ok] / (U53 * S[ok])).max()) if ok.any() else 0.0
