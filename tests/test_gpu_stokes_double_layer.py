"""The Stokes double layer's far field (the rows of TRACTION targets) on the GPU against the reference composed on the CPU
(tests/double_layer_reference.py, pinned by tests/test_double_layer_reference_host.py): the seven dipole potentials of
p2m_apply_kernel<3> / p2m_kernel<1> (wmode 5..11), the tree passes and M2L over slots 4..10, l2p_stokes_kernel<true, PT>.

A. M and L of slots 4..10 of every box, TOL_EXPANSION of the box's largest dipole coefficient;
B. the rows: relative L2 <= 1e-12 and every row within 1e-11 of the largest, both on the scale T of the terms a TRACTION row is
   the sum of (x_k d_i Psi_k and d_i Psi_0 cancel: double_layer_reference), the VELOCITY rows of the mixed plan on |y|;
C. every form that carries these slots, each against the reference and not against another device path;
D. field plans off the surface, both flag classes, over the plan's own two trees;
E. targets at the centre of their leaf and straight above it, where the spherical chain divides by sin a.

The composition is the host time of this file: one per (geometry, order), shared by every test that reads it, never changed.
The expansions do not depend on the targets' flags, so the all-TRACTION and the mixed plan of one geometry share them."""
import numpy as np
import pytest

import double_layer_reference as D
import field_plan_reference as R
import own_geometry
from test_double_layer_reference_host import DENSITY_SEED, two_spheres
from test_gpu_field_plan import plan_options
from test_gpu_parity import TOL_EXPANSION

pytestmark = pytest.mark.gpu

REL_TOL, ROW_TOL = 1e-12, 1e-11
LISTS = ("p2p", "m2l", "m2m", "l2l")


class Geometry:
    """panels, targets (None: the panels' own centroids, a single plan) and a density; per flag set the probes; per order the
    composed expansions, computed once over the lists of the first plan that asks and held to every later plan's lists"""

    def __init__(self, fb, v, pts, ncrit, singularity_free=False):
        self.fb, self.v, self.single, self.ncrit = fb, np.ascontiguousarray(v), pts is None, ncrit
        self.singularity_free = singularity_free            # the VELOCITY rows' far part too by the reference written here
        self.pts = R.centroids(self.v) if pts is None else np.ascontiguousarray(pts)
        self.x = np.random.default_rng(DENSITY_SEED).normal(size=(len(self.v), 3))
        self._probes, self._plans, self._exp, self._rows, self._lists = {}, {}, {}, {}, None

    def probes(self, name, flags):
        if name not in self._probes:
            self._probes[name] = R.Probes(self.v, self.pts, flags)
        return self._probes[name]

    def plan(self, name, flags, p_max=16, fresh=False):
        """(plan, kernel) of a flag set; fresh: a plan of its own (the environment is read while a plan is created)"""
        if fresh or name not in self._plans:
            K = R.stokes_kernel(self.fb, p_max)
            opts = plan_options(self.fb, 0.5, self.ncrit)
            if self.single:
                plan = self.fb.FMM_plan(K, self.v, opts, bc=flags, p_max=p_max)
            else:
                plan = self.fb.FMM_plan(K, self.v, opts, p_max=p_max).field_plan(self.probes(name, flags).centres, flags)
                assert plan.target_info()["tree_coder_levels"] == 10
            st = plan.stats()
            assert st["expansion_slots"] == 11 and st["m2l_pairs"] > 0
            lists = [plan.pairs(w) for w in LISTS]
            if self._lists is None:
                self._lists = lists
            for mine, first in zip(lists, self._lists):        # the flags and the switches change no list
                assert np.array_equal(mine, first)
            if fresh:
                return plan, K
            self._plans[name] = (plan, K)
        return self._plans[name]

    def expansions(self, plan, p):
        if p not in self._exp:
            self._exp[p] = D.compose_expansions(plan, self.v, self.x, p)
            for E in self._exp[p]:
                E.setflags(write=False)
        return self._exp[p]

    def rows(self, name, flags, plan, p):
        if (name, p) not in self._rows:
            self._rows[name, p] = D.compose_rows(plan, self.x, p, self.probes(name, flags), self.expansions(plan, p)[1],
                                                  self.singularity_free)
        return self._rows[name, p]


_GEOMETRIES = {}


def spheres(fb):
    """the geometry of the host pin (d): unit_sphere(4) + unit_sphere(3) at (2.6, 0.2, -0.3), 640 panels, ncrit 16, single plans"""
    if "spheres" not in _GEOMETRIES:
        _GEOMETRIES["spheres"] = Geometry(fb, two_spheres(fb), None, 16)
    return _GEOMETRIES["spheres"]


def sphere_flags(g, name):
    n = len(g.v)
    return {"traction": np.ones(n, np.uint8), "mixed": (np.arange(n) % 2).astype(np.uint8)}[name]


def cloud_points(fb):
    v = fb.unit_sphere(4)
    rng = np.random.default_rng(21)
    pts = R.field_points(v, rng, 300, 120, 100, 60)
    assert len(pts) == 600
    return v, pts, R.mixed_flags(rng, len(pts))


def cloud(fb):
    """unit_sphere(4) and the 600-point cloud of the field-plan tests (shells, interior, near the surface, copies, centroids)"""
    if "cloud" not in _GEOMETRIES:
        v, pts, flags = cloud_points(fb)
        g = _GEOMETRIES["cloud"] = Geometry(fb, v, pts, 20)
        g.flag_sets = {"mixed": flags, "traction": np.ones(len(pts), np.uint8)}
    return _GEOMETRIES["cloud"]


def check_rows(y, ref, T, flags, what, exempt=None):
    """B's pair of bounds per flag class; TRACTION rows on the scale T, VELOCITY rows on |y|.  exempt: rows held elsewhere."""
    assert y.shape == ref.shape and np.all(np.isfinite(y)), what
    keep = np.ones(len(y), bool) if exempt is None else ~exempt
    out = {}
    for f, name in ((1, "TRACTION"), (0, "VELOCITY")):
        rows = (flags == f) & keep
        if not rows.any():
            continue
        err = np.abs(y[rows] - ref[rows]).max(axis=1)
        if f:
            norm, top = np.linalg.norm(T[rows]), T[rows].max()
        else:
            norm, top = np.linalg.norm(ref[rows]), np.abs(ref[rows]).max()
        rel = float(np.linalg.norm(y[rows] - ref[rows]) / norm)
        print("%s %s: rel L2 %.3e, worst row %.3e of the scale (T / |t| up to %.1f)"
              % (what, name, rel, float(err.max() / top), float((T[rows] / np.linalg.norm(ref[rows], axis=1)).max()) if f else 1.0))
        assert rel <= REL_TOL, (what, name, rel)
        assert err.max() <= ROW_TOL * top, (what, name, int(np.argmax(err)), float(err.max()), float(top))
        out[name] = (rel, float(err.max() / top))
    return out


def check_expansions(got, ref, which, what):
    assert got.shape == ref.shape, what
    scale = np.abs(ref[:, D.DIPOLE]).max(axis=(1, 2), keepdims=True)
    if ref.shape[2] == 1:                                   # p = 1: the gradient of a constant, the double layer has no far field
        assert not np.any(ref[:, D.DIPOLE]) and not np.any(got[:, D.DIPOLE]), what
        return
    assert np.count_nonzero(scale) > 1 and np.abs(got[:, D.DIPOLE]).max() > 0, what        # the dipole slots are live
    err = np.abs(got[:, D.DIPOLE] - ref[:, D.DIPOLE]) / (scale + 1e-300)
    print("%s %s: slots 4..10 worst %.3e of the box's largest dipole coefficient" % (what, which, float(err.max())))
    assert err.max() <= TOL_EXPANSION, (what, which, np.unravel_index(np.argmax(err), err.shape), float(err.max()))


# ---- A, B ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 2, 5, 8, 12, 13, 16])
@pytest.mark.parametrize("name", ["traction", "mixed"])
def test_every_box_slot_by_slot_and_the_rows(fb, oracle_mod, name, p):
    g = spheres(fb)
    flags = sphere_flags(g, name)
    plan, K = g.plan(name, flags)
    K.set_p(p)
    y = plan.execute(g.x)
    Mref, Lref = g.expansions(plan, p)
    check_expansions(plan.expansions("M", p), Mref, "M", (name, p))
    check_expansions(plan.expansions("L", p), Lref, "L", (name, p))
    ref, T = g.rows(name, flags, plan, p)
    check_rows(y, ref, T, flags, (name, p))


# ---- C ---------------------------------------------------------------------------------------------------------------------------
FORMS = [
    ("recurrence P2M", {"FMMBEM_P2M_TABLE": "0"}, (6, 14), True),
    ("double-sum M2L", {"FMMBEM_M2L_ROT": "0"}, (5, 12), False),
    ("sparse shifts", {"FMMBEM_SHIFT_ROT": "0"}, (8,), False),
    ("shifts without lanes", {"FMMBEM_SHIFT_LANES": "0", "FMMBEM_SHIFT_ROT_MIN": "0"}, (8,), False),
]


@pytest.mark.parametrize("form", FORMS, ids=[f[0].replace(" ", "_") for f in FORMS])
def test_every_form_that_carries_the_slots(fb, oracle_mod, monkeypatch, form):
    what, env, orders, with_m = form
    g = spheres(fb)
    flags = sphere_flags(g, "mixed")
    # on a geometry of its own (the M2L and the tree passes' form are the geometry's; two forms here share p_max = 8)
    plan, K = own_geometry.under(monkeypatch, env, lambda: g.plan("mixed", flags, p_max=max(orders), fresh=True))
    for p in orders:
        K.set_p(p)
        y = plan.execute(g.x)
        assert plan.stats()["m2l_kernel"] == (2 if "FMMBEM_M2L_ROT" in env or p > 12 else 1), (what, p)
        if with_m:
            check_expansions(plan.expansions("M", p), g.expansions(plan, p)[0], "M", (what, p))
        ref, T = g.rows("mixed", flags, plan, p)
        check_rows(y, ref, T, flags, (what, p))
    plan.close()


def test_generic_l2p_at_an_unrolled_order(fb, oracle_mod, monkeypatch):
    """l2p_stokes_kernel<true, 0> at an order that has a kernel of its own (FMMBEM_L2P_GENERIC is read at every launch)"""
    g = spheres(fb)
    flags = sphere_flags(g, "mixed")
    plan, K = g.plan("mixed", flags)
    K.set_p(5)
    monkeypatch.setenv("FMMBEM_L2P_GENERIC", "1")
    y = plan.execute(g.x)
    monkeypatch.delenv("FMMBEM_L2P_GENERIC")
    ref, T = g.rows("mixed", flags, plan, 5)
    check_rows(y, ref, T, flags, ("generic L2P", 5))


def test_a_relaxed_sequence_and_a_graph_replay(fb, oracle_mod):
    g = spheres(fb)
    flags = sphere_flags(g, "mixed")
    plan, K = g.plan("mixed", flags)
    for p in (12, 3, 1, 12):                                # no state of a higher order survives into a lower one, and back
        K.set_p(p)
        ref, T = g.rows("mixed", flags, plan, p)
        check_rows(plan.execute(g.x), ref, T, flags, ("relaxed sequence", p))
    K.set_p(8)
    plain = plan.execute(g.x)
    ref, T = g.rows("mixed", flags, plan, 8)
    check_rows(plain, ref, T, flags, ("before the replay", 8))
    plan.set_graphs(True)
    try:
        for rep in range(3):
            assert np.array_equal(plan.execute(g.x), plain), rep
    finally:
        plan.set_graphs(False)


# ---- D ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 6, 12, 13, 16])
def test_field_plan_rows_off_the_surface(fb, oracle_mod, p):
    g = cloud(fb)
    flags = g.flag_sets["mixed"]
    plan, K = g.plan("mixed", flags)
    K.set_p(p)
    ref, T = g.rows("mixed", flags, plan, p)
    got = check_rows(plan.execute(g.x), ref, T, flags, ("field plan", p))
    assert set(got) == {"TRACTION", "VELOCITY"}


def test_all_traction_field_plan(fb, oracle_mod):
    """eleven slots and no reader of the first four"""
    g = cloud(fb)
    flags = g.flag_sets["traction"]
    plan, K = g.plan("traction", flags)
    K.set_p(8)
    ref, T = g.rows("traction", flags, plan, 8)
    check_rows(plan.execute(g.x), ref, T, flags, ("all-TRACTION field plan", 8))


# ---- E ---------------------------------------------------------------------------------------------------------------------------
def awkward(fb):
    """the cloud plus, for eight of its target leaves, the leaf's centre and the point 0.3 side above it, one flag each way.  The
    added points are interior to the cloud's bounding cube, so the root cube and the coder stay; the tree is built again."""
    if "awkward" not in _GEOMETRIES:
        v, pts, flags = cloud_points(fb)
        base, _ = cloud(fb).plan("mixed", flags)
        tb = base.target_boxes()
        leaves = np.nonzero(tb["leaf"] & (tb["be"] - tb["bb"] >= 4) & (tb["be"] - tb["bb"] <= 18))[0]     # 20 at most with the two added
        pick = leaves[np.linspace(0, len(leaves) - 1, 8).astype(int)]
        assert len(set(pick)) == 8
        added = np.concatenate([tb["center"][pick], tb["center"][pick] + np.array([0.0, 0.0, 0.3]) * tb["side"][pick][:, None]])
        lo, hi = pts.min(axis=0), pts.max(axis=0)
        assert np.all(added > lo) and np.all(added < hi)
        add_flags = (np.arange(16) % 2).astype(np.uint8)
        add_flags[8:] = 1 - add_flags[8:]
        g = _GEOMETRIES["awkward"] = Geometry(fb, v, np.concatenate([pts, added]), 20, singularity_free=True)
        g.flag_sets = {"mixed": np.concatenate([flags, add_flags])}
        g.base_root = (tb["center"][0].copy(), float(tb["side"][0]))
    return _GEOMETRIES["awkward"]


@pytest.mark.parametrize("p", [8, 13])
def test_targets_at_the_centre_of_their_leaf_and_above_it(fb, oracle_mod, p):
    """The 16 added rows: finite, and within 10 x ON_AXIS_DEVIATION (what the oracle's own double-precision chain loses there
    against the singularity-free reference, host pin (e); the margin is for another rounding order of the same formula) of the
    largest scale of their class.  Every other row keeps B's bounds: no row is exempt from both.  An order with a kernel of its
    own (8) and one of the generic kernel (13)."""
    g = awkward(fb)
    flags = g.flag_sets["mixed"]
    plan, K = g.plan("mixed", flags)
    tb = plan.target_boxes()
    assert np.array_equal(tb["center"][0], g.base_root[0]) and tb["side"][0] == g.base_root[1]
    tree, given = plan.target_perm()
    pos = np.empty(len(tree), dtype=np.int64)
    pos[tree.astype(np.int64)] = np.arange(len(tree))
    added = np.arange(600, 616)
    leaf_of = np.nonzero(tb["leaf"])[0]
    for k in added:                                         # each added point sits where intended in the leaf that holds it
        at = pos[given[k]]
        b = leaf_of[(tb["bb"][leaf_of] <= at) & (at < tb["be"][leaf_of])]
        assert len(b) == 1
        d = g.pts[k] - tb["center"][b[0]]
        assert abs(d[0]) + abs(d[1]) < D.EPS, (k, d)
        if abs(d[2]) > 0:
            assert 0.05 * tb["side"][b[0]] < abs(d[2]) <= 0.5 * tb["side"][b[0]], (k, d)
    on_centre = sum(1 for k in added if np.all(g.pts[k] == tb["center"][leaf_of[
        (tb["bb"][leaf_of] <= pos[given[k]]) & (pos[given[k]] < tb["be"][leaf_of])][0]]))
    assert on_centre >= 1
    K.set_p(p)
    y = plan.execute(g.x)
    ref, T = g.rows("mixed", flags, plan, p)
    exempt = np.zeros(len(y), bool)
    exempt[added] = True
    check_rows(y, ref, T, flags, ("awkward targets, the other rows", p), exempt=exempt)
    assert np.all(np.isfinite(y[added]))
    for f in (0, 1):
        rows = added[flags[added] == f]
        assert len(rows) == 8
        top = T[flags == 1].max() if f else np.abs(ref[flags == 0]).max()
        err = np.abs(y[rows] - ref[rows]).max()
        print("awkward targets p = %d, flag %d: %.3e of the scale" % (p, f, float(err / top)))
        assert err <= 10 * D.ON_AXIS_DEVIATION * top, (p, f, float(err / top))
