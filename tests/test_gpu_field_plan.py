"""Field plans (fmmbem_plan_create_field, FMM_plan.field_plan) on the GPU: the Stokes velocity (single layer, VELOCITY targets) and
double layer (TRACTION targets) at points of their own, and the Laplace field plan as the targets= plan it is.

1. no far field (theta 0.05): every row is the CPU oracle's sum of kernel entries, both operators, to 1e-12;
2. the full FMM: the VELOCITY rows row by row against the reference composed from the oracle's single operators over the plan's own
   lists (field_plan_reference.composed_reference), orders 1 .. 16 on one plan and a relaxed sequence, 8 and 11 expansion slots;
3. centroid targets: bit for bit the single Stokes plan, all VELOCITY, all TRACTION and mixed -- the double layer's far field
   stands on the single plan's own checks;
4. TRACTION rows off the surface against the device Direct sum, calibrated on the VELOCITY rows' own loss (see the test);
5. the item shapes of near_spmv_sym3 on rectangular blocks (the geometries of test_target_plan_oracle_host.CASES);
6. execute_torch on a side stream, execute_batch, graph replays, and the Laplace field plan bit for bit the targets= plan.

Two bounds per flag class, as the target plans' own tests: relative L2 <= 1e-12, and every row within 1e-11 of the class's
max |y| -- an error confined to one leaf cannot hide in the norm."""
import numpy as np
import pytest

import field_plan_reference as R
import own_geometry
from test_gpu_direct import stokes_oracle_at
from test_target_plan_oracle_host import CASES, HOST_CASES, case

pytestmark = pytest.mark.gpu


def check(y, ref, rows, what, rel_tol=1e-12, row_tol=1e-11):
    assert y.shape == ref.shape and np.all(np.isfinite(y)), what
    assert rows.any(), what
    err = np.abs(y[rows] - ref[rows])
    scale = np.max(np.abs(ref[rows]))
    rel = float(np.linalg.norm(y[rows] - ref[rows]) / np.linalg.norm(ref[rows]))
    print("%s: rel L2 %.3e, worst row %.3e of max |y|" % (what, rel, float(err.max() / scale)))
    assert rel <= rel_tol, (what, rel)
    assert err.max() <= row_tol * scale, (what, int(np.argmax(err.max(axis=1))), float(err.max()), float(scale))


def plan_options(fb, theta, ncrit):
    opts = fb.FMMOptions()
    opts.set_mac_theta(theta)
    opts.set_max_per_box(ncrit)
    return opts


# ---- 1. no far field: exact ----------------------------------------------------------------------------------------------------
def test_no_far_field_is_the_oracles_sum(fb, oracle_mod):
    v = fb.unit_sphere(3)
    rng = np.random.default_rng(31)
    pts = R.field_points(v, rng, 150, 60, 60, 10)          # 150 shell, 60 interior, 60 near, 20 copies, 10 centroids
    flags = R.mixed_flags(rng, len(pts))
    assert len(pts) == 300
    x = rng.normal(size=(len(v), 3))
    ref, centres = stokes_oracle_at(oracle_mod, v, pts, flags, x)
    K = R.stokes_kernel(fb, 5)
    plan = fb.FMM_plan(K, v, plan_options(fb, 0.05, 8)).field_plan(centres, flags)
    assert plan.target_info()["tree_coder_levels"] == 10
    assert plan.stats()["m2l_pairs"] == 0 and plan.stats()["expansion_slots"] == 11
    y = plan.execute(x)
    assert y.shape == (300, 3)
    for f in (0, 1):
        check(y, ref, flags == f, ("near only", f))
    x2 = rng.normal(size=(len(v), 3))                      # a second vector on the same plan: no stale rows
    ref2, _ = stokes_oracle_at(oracle_mod, v, pts, flags, x2)
    y2 = plan.execute(x2)
    for f in (0, 1):
        check(y2, ref2, flags == f, ("near only, second vector", f))


# ---- 2. the full FMM, VELOCITY rows against the composed reference -------------------------------------------------------------
class Composed:
    """a field plan on the oracle's centres, and the composed reference per order (computed once)"""

    def __init__(self, fb, v, pts, flags, theta, ncrit, p_max=16, seed=1):
        self.v, self.flags = np.ascontiguousarray(v), flags
        self.probes = R.Probes(self.v, pts, flags)
        self.K = R.stokes_kernel(fb, p_max)
        self.plan = fb.FMM_plan(self.K, self.v, plan_options(fb, theta, ncrit), p_max=p_max).field_plan(self.probes.centres, flags)
        assert self.plan.target_info()["tree_coder_levels"] == 10
        self.x = np.random.default_rng(seed).normal(size=(len(self.v), 3))
        self._ref = {}

    def ref(self, p):
        if p not in self._ref:
            self._ref[p] = R.composed_reference(self.plan, self.probes, self.v, self.x, p)
        return self._ref[p]

    def run(self, p):
        self.K.set_p(p)
        return self.plan.execute(self.x)


@pytest.fixture(scope="module")
def sphere4(fb):
    v = fb.unit_sphere(4)
    rng = np.random.default_rng(21)
    pts = R.field_points(v, rng, 300, 120, 100, 60)
    assert len(pts) == 600
    return v, pts, R.mixed_flags(rng, len(pts))


@pytest.mark.parametrize("mixed", [False, True])
def test_velocity_rows_equal_the_composed_reference(fb, oracle_mod, sphere4, mixed):
    v, pts, mixed_flags = sphere4
    flags = mixed_flags if mixed else np.zeros(len(pts), np.uint8)
    F = Composed(fb, v, pts, flags, 0.5, 20)
    st = F.plan.stats()
    assert st["m2l_pairs"] > 0 and st["expansion_slots"] == (11 if mixed else 8)
    for p in (1, 6, 12, 13, 16, 12, 3, 16):                 # every path of the far field, then a relaxed sequence
        check(F.run(p), F.ref(p), flags == 0, ("composed", "mixed" if mixed else "velocity", p))
    F.probes.close()


# ---- 3. centroid targets: the single plan, bit for bit -------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["velocity", "traction", "mixed"])
def test_centroid_targets_are_the_single_plan_bit_for_bit(fb, which):
    v = fb.unit_sphere(5)
    n = len(v)
    rng = np.random.default_rng(41)
    bc = {"velocity": np.zeros(n, np.uint8), "traction": np.ones(n, np.uint8), "mixed": (rng.random(n) < 0.5).astype(np.uint8)}[which]
    x = rng.normal(size=(n, 3))
    orders = (5, 10, 12, 16) if which == "velocity" else (5, 10, 12)
    K = R.stokes_kernel(fb, 5)
    single = fb.FMM_plan(K, v, bc=bc, p_max=max(orders))
    field = single.field_plan(R.centroids(v), bc)
    assert field.target_info()["tree_coder_levels"] == 10
    assert single.stats()["expansion_slots"] == field.stats()["expansion_slots"] == {"velocity": 8, "traction": 11, "mixed": 11}[which]
    for p in orders:
        K.set_p(p)
        a, b = single.execute(x), field.execute(x)
        assert a.shape == b.shape == (n, 3)
        assert np.array_equal(a, b), (which, p, float(np.linalg.norm(a - b) / np.linalg.norm(a)))


# ---- 4. TRACTION rows off the surface against Direct ---------------------------------------------------------------------------
TRACTION_FACTOR = 4.0


def test_traction_rows_off_the_surface_against_direct(fb):
    """e_ft <= TRACTION_FACTOR * max(e_st, e_st * e_fv / e_sv): the VELOCITY rows are right to 1e-12 (test 2), so e_fv / e_sv is the
    truncation loss this point set really has over the surface's own rows; the double layer is allowed the same loss over the single
    plan's own double-layer rows, times a margin for its extra derivative.  Measured on an MI355X ("Field
    plans"), e_fv e_ft | e_sv e_st, ratio of e_ft to the bound without its factor:
      p =  4: 1.435e-02 2.035e-02 | 5.204e-03 2.289e-03, 3.22
      p =  8: 5.787e-04 1.477e-03 | 1.115e-04 9.071e-05, 3.14
      p = 12: 5.048e-05 1.738e-04 | 6.060e-06 6.902e-06, 3.02"""
    v = fb.unit_sphere(5)
    n = len(v)
    rng = np.random.default_rng(51)
    pts = R.unit_dirs(rng, 4000) * (1.05 + 0.95 * rng.random(4000))[:, None]
    flags = R.mixed_flags(rng, 4000)
    bc = R.mixed_flags(rng, n)
    x = rng.normal(size=(n, 3))
    K = R.stokes_kernel(fb, 12)
    D = fb.Direct(K, v)
    ref_f = D.matvec(x, targets=pts, target_bc=flags)
    ref_s = D.matvec(x, targets=R.centroids(v), target_bc=bc)
    D.close()
    single = fb.FMM_plan(K, v, bc=bc, p_max=12)
    field = single.field_plan(pts, flags)
    assert field.target_info()["tree_coder_levels"] == 10 and field.stats()["m2l_pairs"] > 0

    def rel(y, ref, s):
        return float(np.linalg.norm(y[s] - ref[s]) / np.linalg.norm(ref[s]))

    e_ft = {}
    for p in (4, 8, 12):
        K.set_p(p)
        yf, ys = field.execute(x), single.execute(x)
        e_fv, e_ft[p] = rel(yf, ref_f, flags == 0), rel(yf, ref_f, flags == 1)
        e_sv, e_st = rel(ys, ref_s, bc == 0), rel(ys, ref_s, bc == 1)
        print("p = %2d: field VELOCITY %.3e TRACTION %.3e; single plan VELOCITY %.3e TRACTION %.3e; TRACTION ratio %.2f"
              % (p, e_fv, e_ft[p], e_sv, e_st, e_ft[p] / max(e_st, e_st * e_fv / e_sv)))
        assert e_ft[p] <= TRACTION_FACTOR * max(e_st, e_st * e_fv / e_sv), p
    assert e_ft[4] > e_ft[8] > e_ft[12]


# ---- 5. the item shapes of near_spmv_sym3 on rectangular blocks -----------------------------------------------------------------
SHAPE_ORDER = 4          # the composition of shells_dgdn (64 353 M2L pairs) takes 5 s of host time whatever the order; the shapes are the near field's


def shape_case(name):
    c = case(name)
    if name == "tight_cloud":                               # its first 200 points need the 21-level coder, which is not this file's
        c["pts"] = np.ascontiguousarray(c["pts"][200:])
    return c


@pytest.fixture(scope="module")
def shape_plans():
    return {}


def shape_fixture(fb, shape_plans, name):
    if name not in shape_plans:
        c = shape_case(name)
        shape_plans[name] = Composed(fb, c["v"], c["pts"], np.zeros(len(c["pts"]), np.uint8), c["theta"], c["ncrit"], p_max=SHAPE_ORDER,
                                     seed=len(name))
    return shape_plans[name]


@pytest.mark.parametrize("name", HOST_CASES)
def test_spmv_item_shapes_against_the_composed_reference(fb, oracle_mod, shape_plans, name):
    assert name in CASES
    F = shape_fixture(fb, shape_plans, name)
    check(F.run(SHAPE_ORDER), F.ref(SHAPE_ORDER), F.flags == 0, (name, SHAPE_ORDER))


def leaf_shapes(tp):
    """(rows, near columns) per target leaf, from the p2p list and the box ranges"""
    sb, tb = tp.boxes(), tp.target_boxes()
    cols = np.zeros(len(tb["leaf"]), dtype=np.int64)
    p2p = tp.pairs("p2p")
    if len(p2p):
        np.add.at(cols, p2p[:, 1], (sb["be"] - sb["bb"])[p2p[:, 0]])
    leaves = np.nonzero(tb["leaf"])[0]
    return (tb["be"] - tb["bb"])[leaves], cols[leaves]


def test_fixtures_reach_the_sym3_item_shapes(fb, oracle_mod, shape_plans):
    shapes = [leaf_shapes(shape_fixture(fb, shape_plans, name).plan) for name in HOST_CASES]
    rows = np.concatenate([r for r, _ in shapes])
    cols = np.concatenate([c for _, c in shapes])
    assert np.any(cols > 2048)                          # three or more chunks of kSymChunk = 1024 source panels
    assert np.any((rows < 8) & (cols > 1024))           # a column split of a short leaf, plus chunks
    assert np.any((rows == 1) & (cols > 0))             # one-row leaves
    assert np.any(cols == 0)                            # target leaves with no near pair
    r, c = leaf_shapes(shape_fixture(fb, shape_plans, "far_only").plan)
    assert np.all(c == 0)                               # a case with no near pair at all


# ---- 6. other paths ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def general(fb, sphere4):
    v, pts, flags = sphere4
    K = R.stokes_kernel(fb, 10)
    plan = fb.FMM_plan(K, v, plan_options(fb, 0.5, 20), p_max=12).field_plan(pts, flags)
    x = np.random.default_rng(61).normal(size=(len(v), 3))
    return plan, K, x


def test_execute_torch_on_a_side_stream(fb, general):
    import torch
    plan, K, x = general
    K.set_p(10)
    host = plan.execute(x)
    xd = torch.from_numpy(x).to("cuda:0")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        y = plan.execute_torch(xd)
    s.synchronize()
    assert tuple(y.shape) == (plan.n_targets, 3)
    assert np.array_equal(y.cpu().numpy(), host)


def test_execute_batch(fb, general):
    import torch
    plan, K, x = general
    K.set_p(8)
    assert plan.batch_width() == 1
    X = np.random.default_rng(62).normal(size=(5,) + x.shape)
    X[3] *= 1e3
    X[4] = 0.0
    single = [plan.execute(X[j]) for j in range(5)]
    for k in (1, 2, 3, 5):
        Y = plan.execute_batch(X[:k])
        assert Y.shape == (k, plan.n_targets, 3)
        for j in range(k):
            assert np.array_equal(Y[j], single[j]), (k, j)
        if k == 5:
            assert np.all(Y[4] == 0)
    Yd = plan.execute_batch_torch(torch.from_numpy(X[:3].reshape(3, -1)).to("cuda:0"))
    torch.cuda.synchronize()
    assert tuple(Yd.shape) == (3, plan.n_targets * 3)
    for j in range(3):
        assert np.array_equal(Yd[j].cpu().numpy().reshape(-1, 3), single[j]), j


def test_graph_replays(fb, general):
    plan, K, x = general
    K.set_p(9)
    x2 = -0.5 * x + 1.0
    plain, plain2 = plan.execute(x), plan.execute(x2)
    plan.set_graphs(True)
    try:
        for rep in range(3):
            assert np.array_equal(plan.execute(x), plain), rep
            assert np.array_equal(plan.execute(x2), plain2), rep
    finally:
        plan.set_graphs(False)


def test_nine_value_rows(fb, oracle_mod, sphere4, monkeypatch):
    """FMMBEM_STOKES_SYM=0 (read while the plan is created): the blocks as rows of nine values per pair, near_spmv_kernel instead of
    near_spmv_sym3.  The VELOCITY rows against the composed reference; the TRACTION rows against the default plan's, whose entries are
    the same numbers added in another order (1e-12: far above m 2^-53 for rows of a few hundred entries)."""
    v, pts, flags = sphere4
    sym = Composed(fb, v, pts, flags, 0.5, 20, p_max=6)
    rows9 = own_geometry.under(monkeypatch, {"FMMBEM_STOKES_SYM": "0"}, lambda: Composed(fb, v, pts, flags, 0.5, 20, p_max=6),
                               plan_of=lambda c: c.plan)         # sym is alive: the storage form is the geometry's
    assert rows9.plan.stats()["near_bytes"] > 1.4 * sym.plan.stats()["near_bytes"]
    y9, ys = rows9.run(6), sym.run(6)
    check(y9, rows9.ref(6), flags == 0, "9-value rows, VELOCITY against the composed reference")
    check(y9, ys, flags == 1, "9-value rows, TRACTION against the symmetric blocks")
    sym.probes.close()
    rows9.probes.close()


def test_laplace_field_plan_is_the_targets_plan_bit_for_bit(fb, sphere4):
    v, pts, flags = sphere4
    K = fb.LaplaceSphericalBEM(5, 3)
    opts = plan_options(fb, 0.5, 20)
    field = fb.FMM_plan(K, v, opts, p_max=13).field_plan(pts, flags)
    targets = fb.FMM_plan(K, v, opts, p_max=13, targets=pts, target_bc=flags)
    x = np.random.default_rng(63).normal(size=len(v))
    for p in (5, 13):
        K.set_p(p)
        a, b = field.execute(x), targets.execute(x)
        assert a.shape == (len(pts),)
        assert np.array_equal(a, b), p
