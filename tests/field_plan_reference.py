"""Helpers of the field-plan tests (fmmbem_plan_create_field): the point sets, and the reference COMPOSED from the oracle's single
operators over the plan's own lists -- P2M per source leaf (oracle.single_p2m), M2M / M2L / L2L per listed pair and slot
(oracle.Tables), L2P at probe triangles per target leaf (oracle.single_l2p), plus the oracle's kernel entries over the p2p list.
The composition holds the VELOCITY rows (the single layer: the four potentials the oracle's Stokes operators carry).  On a single
plan's geometry (unit_sphere(4), ncrit 20, p = 6, 1 808 M2L pairs) it agrees with StokesOracle.matvec to 3.4e-16 relative L2 and
6.2e-16 of max |y| on the worst row (tests/test_field_plan_host.py holds it to 1e-14)."""
import numpy as np

from oracle import oracle as O

MU, QUAD_K, QUAD_K_FINE = 1e-3, 4, 19


def stokes_kernel(fb, p=5):
    K = fb.StokesSphericalBEM(p, QUAD_K, mu=MU)
    K.set_Kfine(QUAD_K_FINE)
    return K


def centroids(v):
    return (v[:, 0] + v[:, 1] + v[:, 2]) / 3


def point_panels(points, h=1e-9):
    """tiny triangles whose centroids stand for the points"""
    off = np.array([[h, 0, 0], [0, h, 0], [-h, -h, 0]])
    return np.asarray(points, dtype=np.float64)[:, None, :] + off[None, :, :]


def unit_dirs(rng, m):
    d = rng.normal(size=(m, 3))
    return d / np.linalg.norm(d, axis=1)[:, None]


def field_points(v, rng, m_shell, m_in, m_near, m_centroid, copies=20, r_max=1.5):
    """shells at 1.01 .. r_max radii, interior points, points within a tenth of a panel of the surface, `copies` copies of one
    point, and panel centroids (the self entries of both operators)"""
    c = centroids(v)
    nrm = c / np.linalg.norm(c, axis=1)[:, None]
    size = np.sqrt(np.linalg.norm(np.cross(v[:, 2] - v[:, 0], v[:, 1] - v[:, 0]), axis=1))        # sqrt(2 A)
    pick = rng.choice(len(v), m_near + m_centroid, replace=False)
    near = c[pick[:m_near]] + nrm[pick[:m_near]] * (size[pick[:m_near]] * 0.1 * (2 * rng.random(m_near) - 1))[:, None]
    shell = unit_dirs(rng, m_shell) * (1.01 + (r_max - 1.01) * rng.random(m_shell))[:, None]
    inner = unit_dirs(rng, m_in) * (0.95 * rng.random(m_in))[:, None]
    same = np.tile([[0.3, -0.2, 1.1]], (copies, 1))
    return np.concatenate([shell, inner, near, same, c[pick[m_near:]]])


def mixed_flags(rng, m):
    """half TRACTION (the copies of the one point fall into two bodies, one per flag)"""
    return (rng.random(m) < 0.5).astype(np.uint8)


def self_block_at(y1, y2, y3, x, mu=MU):
    """The velocity block of a VELOCITY target x in the plane of the panel (y1, y2, y3) inside the self window (|x - centroid| < 1e-8):
    the reference's closed form, FataAnalytical<STOKES>(y1, y2, y3, ., x = target.center, self = true, G) followed by
    Integration<STOKES>::integrate, times 1/(2 mu) (kernel/StokesSphericalBEM.hpp:266-281; examples/BEM/FataAnalytical.hpp:414-690,
    273-341), restated in numpy.  The oracle's own restatement (oracle/stokes.c stokes_self) evaluates at the PANEL's centroid,
    which is the same thing for a true self pair and 1e-9 relative off it for a target 1e-9 beside the centroid."""
    y1, y2, y3, x = (np.asarray(a, dtype=np.float64) for a in (y1, y2, y3, x))
    v1, v3 = y2 - y1, y3 - y1
    snrm = v1 @ v1
    e1 = v1 / np.sqrt(snrm)
    e2 = v3 - (v1 @ v3) / snrm * v1
    e2 = e2 / np.linalg.norm(e2)
    e3 = np.cross(e1, e2)
    bQ, aQ, cQ = v1 @ e1, v3 @ e2, v3 @ e1
    th0 = np.arccos(cQ / np.sqrt(cQ * cQ + aQ * aQ))
    th1 = np.arccos((bQ - cQ) / np.sqrt((bQ - cQ) ** 2 + aQ * aQ))
    alpha = np.array([0.0, np.pi - th1, np.pi + th0])
    cs, sn = np.cos(alpha), np.sin(alpha)
    r1 = x - y1
    xi, zt = r1 @ e1, r1 @ e2
    p11, p12, q0 = -xi, bQ - xi, -zt
    x3, z3 = cQ + p11, aQ + q0
    p22, p23, q1 = p12 * cs[1] + q0 * sn[1], x3 * cs[1] + z3 * sn[1], q0 * cs[1] - p12 * sn[1]
    p31, p33, q2 = p11 * cs[2] + q0 * sn[2], x3 * cs[2] + z3 * sn[2], q0 * cs[2] - p11 * sn[2]
    rho = np.array([np.hypot(p11, q0), np.hypot(p12, q0), np.hypot(p33, q2)])
    omega = (q0 * np.log((p11 + rho[0]) / (p12 + rho[1])) + q1 * np.log((p22 + rho[1]) / (p23 + rho[2]))
             + q2 * np.log((p33 + rho[2]) / (p31 + rho[0])))
    rb = np.array([rho[0] - rho[1], rho[1] - rho[2], rho[2] - rho[0]])
    Ixx, Izz, Izx = np.sum(rb * sn * cs), np.sum(-rb * cs * sn), np.sum(rb * sn * sn)
    coef = np.array([[omega + Ixx, Izx, 0.0], [Izx, omega + Izz, 0.0], [0.0, 0.0, omega]])
    E = np.stack([e1, e2, e3])
    return E.T @ coef @ E / (2 * mu)


class Probes:
    """the oracle context of the panels plus the targets as probe triangles: the centres the oracle places the targets at (what
    the plan must be handed) and K(t_i, s_j) of any listed pair"""

    def __init__(self, v, pts, flags):
        self.n, self.m = len(v), len(pts)
        self.v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1, 3, 3)
        self.flags = np.asarray(flags, np.uint8)
        self.tri = point_panels(pts)
        self.ctx = O.StokesOracle(np.concatenate([self.v, self.tri]), K=QUAD_K, K_fine=QUAD_K_FINE, mu=MU, ncrit=1 << 30,
                                  bc=np.concatenate([np.zeros(self.n, np.uint8), self.flags]))
        centres = self.ctx.panels()["center"]
        self.panel_centres, self.centres = centres[:self.n].copy(), centres[self.n:].copy()

    def entries(self, targets, sources):
        """(len(targets), len(sources), 3, 3): the oracle's K(t, s); where a VELOCITY target lies in a panel's self window without
        being its centroid, the closed form at the TARGET (self_block_at), as the reference evaluates it"""
        targets, sources = np.asarray(targets, dtype=np.int32), np.asarray(sources, dtype=np.int32)
        ti = np.repeat(targets + self.n, len(sources))
        sj = np.tile(sources, len(targets))
        E = self.ctx.kernel_entries(ti, sj).reshape(len(targets), len(sources), 3, 3)
        d = np.linalg.norm(self.centres[targets][:, None, :] - self.panel_centres[sources][None, :, :], axis=2)
        for a, b in zip(*np.nonzero((d < 1e-8) & (d > 0) & (self.flags[targets] == 0)[:, None])):
            tri = self.v[sources[b]]
            E[a, b] = self_block_at(tri[0], tri[1], tri[2], self.centres[targets[a]])
        return E

    def close(self):
        self.ctx.close()


def composed_reference(plan, probes, v, x, p):
    """(m, 3): near part by the oracle's entries over the plan's p2p list, far part by the oracle's single operators over the plan's
    m2m / m2l / l2l lists with every target read as a VELOCITY target.  plan: a field plan built on probes.centres.  Rows of
    TRACTION targets hold their (right) near part and the single layer's far part: compare the VELOCITY rows only."""
    sb, tb = plan.boxes(), plan.target_boxes()
    perm = plan.perm().astype(np.int64)
    tree, given = plan.target_perm()
    tree = tree.astype(np.int64)
    first = np.full(len(tree), -1, dtype=np.int64)         # distinct point -> the first given target at it
    for k in range(len(given) - 1, -1, -1):
        first[given[k]] = k
    S = p * (p + 1) // 2
    T = O.Tables(p)
    M = np.zeros((len(sb["leaf"]), 4, S), dtype=np.complex128)
    for b in np.nonzero(sb["leaf"])[0]:
        idx = perm[sb["bb"][b]:sb["be"][b]]
        M[b] = O.single_p2m(1, p, QUAD_K, v[idx], None, x[idx], sb["center"][b], mu=MU)
    for c, par in plan.pairs("m2m"):                       # deepest level first
        tr = sb["center"][par] - sb["center"][c]
        for s in range(4):
            M[par, s] += T.m2m(M[c, s], tr)
    L = np.zeros((len(tb["leaf"]), 4, S), dtype=np.complex128)
    for s_box, t_box in plan.pairs("m2l"):
        tr = tb["center"][t_box] - sb["center"][s_box]
        for s in range(4):
            L[t_box, s] += T.m2l(M[s_box, s], tr)
    for par, c in plan.pairs("l2l"):                       # top level first
        tr = tb["center"][c] - tb["center"][par]
        for s in range(4):
            L[c, s] += T.l2l(L[par, s], tr)
    y_points = np.zeros((len(tree), 3))
    near = {}
    for s_box, t_box in plan.pairs("p2p"):
        near.setdefault(int(t_box), []).append(int(s_box))
    for b in np.nonzero(tb["leaf"])[0]:
        pts_here = tree[tb["bb"][b]:tb["be"][b]]             # distinct points of the leaf
        tg = first[pts_here]
        y = O.single_l2p(1, p, QUAD_K, L[b], tb["center"][b], probes.tri[tg], None, mu=MU).reshape(-1, 3)
        for s_box in near.get(int(b), []):
            idx = perm[sb["bb"][s_box]:sb["be"][s_box]]
            y += np.einsum("ijab,jb->ia", probes.entries(tg, idx), x[idx])
        y_points[pts_here] = y
    return y_points[given]
