"""The Laplace L2P after its rewrite: seven FP64 operations per (n, m) term -- the harmonic's prefactor and weight folded into
the staged coefficient, the Legendre recurrence carried on q_n = rho^n P_n^m with z = rho cos(alpha) and rho^2 -- and the result
scatter folded into its last store where the L2P groups cover every row of the plan (csrc/kernels_far.hip l2p_kernel,
csrc/plan.hip l2p_delivers; FMMBEM_L2P_SCATTER=0 runs the separate scatter kernel).

Tolerances are the project's: TOL_MATVEC for a matvec against the oracle, and for L2P on its own the single-operator bound of
tests/test_gpu_single_operators.py, 1e-12 of the largest value (= TOL_EXPANSION)."""
import numpy as np
import pytest

from test_gpu_parity import TOL_EXPANSION, TOL_MATVEC

from conftest import rel_l2

pytestmark = pytest.mark.gpu

ORDERS = (1, 2, 9, 10, 12, 13, 16)                     # both ends of the unrolled kernels (1 ... 12) and the run-time one


def flags(kind, n):
    if kind == "mixed":                                # both slots live, the -r1 branch on about half of the rows
        return (np.random.default_rng(11).random(n) < 0.5).astype(np.uint8)
    return np.full(n, 1 if kind == "ones" else 0, dtype=np.uint8)


@pytest.fixture(scope="module")
def two_spheres(oracle_mod):
    v = np.concatenate([oracle_mod.unit_sphere(5), oracle_mod.unit_sphere(3, center=(2.5, 0.3, -0.2))])   # leaves of 1 ... 64 panels
    x = np.random.default_rng(21).standard_normal(len(v))
    return v, x


@pytest.fixture(scope="module")
def sides(fb, oracle_mod, two_spheres):
    """per kind of flags: the plan (p_max 16), its kernel object, the oracle; references are computed once per (kind, p)"""
    v, x = two_spheres
    made, refs = {}, {}

    def get(kind, p):
        if kind not in made:
            bc = flags(kind, len(v))
            K = fb.LaplaceSphericalBEM(16, 3)
            made[kind] = (fb.FMM_plan(K, v, bc=bc), K, oracle_mod.Oracle(v, bc=bc))
        if (kind, p) not in refs:
            ref = made[kind][2].matvec(x, p)
            ref.setflags(write=False)
            refs[kind, p] = ref
        return made[kind][0], made[kind][1], refs[kind, p]
    return get


@pytest.mark.parametrize("kind", ["zeros", "ones", "mixed"])
@pytest.mark.parametrize("p", ORDERS)
def test_matvec_against_the_oracle(sides, two_spheres, p, kind):
    pl, K, ref = sides(kind, p)
    K.set_p(p)
    err = rel_l2(pl.execute(two_spheres[1]), ref)
    print("p = %d, bc %s: rel. L2 vs oracle %.3e" % (p, kind, err))
    assert err <= TOL_MATVEC


def test_leaf_of_more_than_64_rows(fb, oracle_mod, two_spheres):
    """max_per_box 128: a leaf holds more rows than a wavefront has lanes and is walked in chunks"""
    v, x = two_spheres
    bc = flags("mixed", len(v))
    opts = fb.FMMOptions()
    opts.set_max_per_box(128)
    pl = fb.FMM_plan(fb.LaplaceSphericalBEM(10, 3), v, opts, bc=bc)
    b = pl.boxes()
    assert np.max((b["be"] - b["bb"])[b["leaf"] != 0]) > 64
    err = rel_l2(pl.execute(x), oracle_mod.Oracle(v, bc=bc, ncrit=128).matvec(x, 10))
    print("ncrit 128: rel. L2 vs oracle %.3e" % err)
    assert err <= TOL_MATVEC


def axis_panels(center):
    """Targets where a recurrence in rho cos(alpha) and rho^2 could go wrong: centroids on the local z axis (sin alpha = 0, above and
    below the centre), a hair beside it (inside and outside the EPS of cart2sph's degenerate azimuth), at the centre itself
    (rho = EPS) and next to it, in the equatorial plane (cos alpha = 0); then points all over the box.  70 targets: two chunks."""
    rng = np.random.default_rng(5)
    off = [(0, 0, 0.25), (0, 0, -0.25), (0, 0, 2.0 ** -20), (0, 0, -2.0 ** -30), (1e-13, 0, 0.125), (0, -1e-13, -0.125), (1e-9, 1e-9, 0.25),
           (1e-6, 0, -0.5), (0, 0, 0), (1e-13, 0, 0), (0, 1e-14, 1e-14), (1e-9, -1e-9, 1e-9), (0.25, 0, 0), (0, -0.25, 0), (0.125, 0.125, 0),
           (-0.25, 2.0 ** -40, 0)]
    off = np.array(off + list(0.3 * rng.uniform(-1, 1, (70 - len(off), 3))))
    c = np.asarray(center) + off
    a, b = np.array([2.0 ** -6, 0, 0]), np.array([0, 2.0 ** -6, 0])         # vertex offsets that sum to zero exactly
    return np.ascontiguousarray(np.stack([c + a, c + b, c - a - b], axis=1))


@pytest.mark.parametrize("p", ORDERS)
def test_far_field_alone_on_the_axis_and_at_the_centre(fb, oracle_mod, p):
    """L2P of a given L through the single-operator entry against the oracle's orc_l2p, both flags"""
    rng = np.random.default_rng(300 + p)
    center = np.array([0.25, -0.5, 0.125])
    panels = axis_panels(center)
    n = len(panels)
    bc = (np.arange(n) % 3 == 1).astype(np.uint8)
    S = p * (p + 1) // 2
    L = rng.standard_normal((2, S)) + 1j * rng.standard_normal((2, S))
    for k in range(p):
        L[:, k * (k + 1) // 2] = L[:, k * (k + 1) // 2].real
    L = np.ascontiguousarray(L)
    K = fb.LaplaceSphericalBEM(p, 3)
    for flags_ in (bc, 1 - bc):
        r0 = rng.standard_normal(n)
        r = r0.copy()
        K.L2P(L, center, panels, r, bc=flags_)
        ref = oracle_mod.single_l2p(0, p, 3, L, center, panels, flags_)
        assert np.all(np.isfinite(r))
        scale = np.abs(ref).max()
        err = np.abs((r - r0) - ref).max() / scale
        print("p = %d: L2P alone, max error / max value %.3e" % (p, err))
        assert scale > 0 and err <= TOL_EXPANSION


# ------------------------------------------------ the scatter fold ------------------------------------------------
@pytest.fixture(scope="module")
def odd_mesh(oracle_mod):
    v = np.concatenate([oracle_mod.unit_sphere(4), oracle_mod.unit_sphere(3, center=(2.5, 0.3, -0.2))])[:-5]
    assert len(v) % 64 != 0
    rng = np.random.default_rng(8)
    return v, (rng.random(len(v)) < 0.4).astype(np.uint8), rng.standard_normal((4, len(v)))


def test_fold_and_separate_scatter_give_the_same_bits(fb, oracle_mod, monkeypatch, odd_mesh):
    import torch
    v, bc, xs = odd_mesh
    K = fb.LaplaceSphericalBEM(10, 3)
    pl = fb.FMM_plan(K, v, bc=bc)
    assert not np.array_equal(pl.perm(), np.arange(len(v)))
    xd = [torch.from_numpy(x).cuda() for x in xs]

    def run_all():
        got = [pl.execute(xs[0])]
        buf = torch.full((len(v),), np.nan, dtype=torch.float64, device="cuda")
        for x in (xd[1], xd[2]):                                     # twice into the same buffer
            out = pl.execute_torch(x, out=buf)
            assert out.data_ptr() == buf.data_ptr()
            got.append(buf.cpu().numpy())
        got.append(pl.execute_torch(xd[1]).cpu().numpy())            # and into another one
        got.append(pl.execute_batch(xs[:3]))
        return got

    folded = run_all()
    assert rel_l2(folded[0], oracle_mod.Oracle(v, bc=bc).matvec(xs[0], 10)) <= TOL_MATVEC
    assert np.array_equal(folded[1], folded[3]) and np.array_equal(folded[4][1], folded[1]) and np.array_equal(folded[4][0], folded[0])
    monkeypatch.setenv("FMMBEM_L2P_SCATTER", "0")
    separate = run_all()
    for a, b in zip(folded, separate):
        assert np.array_equal(a, b)
    # replayed as a graph: the captured chain holds no pointer of the caller's, so another output buffer is honoured
    monkeypatch.delenv("FMMBEM_L2P_SCATTER")
    pl.set_graphs(True)
    for _ in range(3):
        for j in (1, 2):
            out = torch.full((len(v),), np.nan, dtype=torch.float64, device="cuda")
            pl.execute_torch(xd[j], out=out)
            assert np.array_equal(out.cpu().numpy(), folded[j])
    pl.set_graphs(False)
    # with events around every stage the stages keep their places: L2P is timed, the scatter stage brackets nothing
    pl.set_timing(True)
    assert np.array_equal(pl.execute(xs[0]), folded[0])
    st = pl.stats()
    assert st["timed_executes"] >= 1 and st["ms_l2p"] > 0 and st["ms_total"] >= st["ms_l2p"]
    pl.set_timing(False)


def both_ways(monkeypatch, run):
    monkeypatch.delenv("FMMBEM_L2P_SCATTER", raising=False)
    a = run()
    monkeypatch.setenv("FMMBEM_L2P_SCATTER", "0")
    b = run()
    monkeypatch.delenv("FMMBEM_L2P_SCATTER")
    assert np.array_equal(a, b)
    return a


def test_plans_that_keep_the_scatter_kernel(fb, oracle_mod, monkeypatch, odd_mesh):
    import torch
    v, bc, xs = odd_mesh
    x = xs[0]
    p = 8
    ref = oracle_mod.Oracle(v, bc=bc).matvec(x, p)
    # one leaf: no L2P at all
    v0 = oracle_mod.unit_sphere(0)
    x0 = np.arange(1.0, len(v0) + 1)
    pl0 = fb.FMM_plan(fb.LaplaceSphericalBEM(p, 3), v0)
    assert pl0.stats()["l2p_leaves"] == 0
    assert rel_l2(both_ways(monkeypatch, lambda: pl0.execute(x0)), oracle_mod.Oracle(v0).matvec(x0, p)) <= TOL_MATVEC
    # a target plan
    pts = np.random.default_rng(22).normal(size=(300, 3)) * 2.0 + np.array([1.5, 0.0, 0.0])
    plt = fb.FMM_plan(fb.LaplaceSphericalBEM(p, 3), v, targets=pts)
    yt = both_ways(monkeypatch, lambda: plt.execute(x))
    assert rel_l2(yt, oracle_mod.TargetOracle(v, pts).matvec(x, p)) <= TOL_MATVEC
    # the two shards of a plan: each delivers its rows and zeros elsewhere
    shards = [fb.FMM_plan(fb.LaplaceSphericalBEM(p, 3), v, bc=bc, shard=(r, 2)) for r in range(2)]
    y0 = both_ways(monkeypatch, lambda: shards[0].execute(x))
    y1 = shards[1].execute(x)
    assert np.count_nonzero(y0) > 0 and np.count_nonzero(y1) > 0 and not np.any((y0 != 0) & (y1 != 0))
    assert rel_l2(y0 + y1, ref) <= TOL_MATVEC
    # result slices: the rows in tree order at the head of y
    pls = fb.FMM_plan(fb.LaplaceSphericalBEM(p, 3), v, bc=bc)
    xd = torch.from_numpy(x).cuda()
    y = pls.execute_torch(xd).cpu().numpy()
    assert rel_l2(y, ref) <= TOL_MATVEC
    pls.set_result_slices(True)
    sl = both_ways(monkeypatch, lambda: pls.execute_torch(xd).cpu().numpy())
    assert np.array_equal(sl, y[pls.perm()])
    pls.set_result_slices(False)
    assert np.array_equal(pls.execute_torch(xd).cpu().numpy(), y)
