"""The field gradient (fmmbem_plan_execute_gradient), host side: the composed CPU reference pinned to the oracle, its entry formula
against central differences, the shapes of the cases the GPU tests run, and the refusals of the C ABI.  No device needed."""
import ctypes

import numpy as np
import pytest

import field_gradient_reference as G
from oracle import oracle as O


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# ---- the reference ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [4, 7, 10, 13, 16])
def test_composition_gives_the_oracles_values(p):
    """The VALUES of the local expansions the gradient is taken of, by the same L, are TargetOracle.matvec where no target has a near
    pair.  Measured 2e-16 .. 4e-16; held to 1e-14."""
    R = G.reference("far_only")
    assert R.info["p2p_pairs"] == 0
    for key in ("x", "x2"):
        got, want = R.values(p, key), R.T.matvec(R.vector(key), p)
        for f in (0, 1):
            s = R.flags == f
            assert rel(got[s], want[s]) <= 1e-14, (p, key, f, rel(got[s], want[s]))


def test_gamma_is_the_gradient_of_the_k_point_potentials():
    """Central differences, h = 1e-5, of sum_q w_q A / |y_q - t| (flag 0) and sum_q w_q A (y_q - t) . n / |y_q - t|^3 (flag 1) on
    far-regime pairs.  Measured 1e-10 and 2e-10 of the largest entry; held to 1e-8."""
    v = O.unit_sphere(3)
    g = G.geometry(v)
    w = O.quadrature(G.K)[1]
    rng = np.random.default_rng(2)
    h = 1e-5

    def potential(t, flag):
        dx = g["quad"] - t[None, None]
        r = np.linalg.norm(dx, axis=2)
        wA = w[None] * g["area"][:, None]
        if flag == 0:
            return (wA / r).sum(1)
        return (wA * (dx * g["normal"][:, None]).sum(2) / r ** 3).sum(1)

    for flag in (0, 1):
        worst, top = 0.0, 0.0
        for _ in range(8):
            t = rng.normal(size=3)
            t *= (1.6 + rng.random()) / np.linalg.norm(t)
            far = np.sqrt(2 * g["area"]) / np.linalg.norm(t[None] - g["center"], axis=1) < 0.5
            assert far.sum() >= 30
            got = G.gamma(t, flag, v, g)[far]
            fd = np.stack([(potential(t + h * e, flag) - potential(t - h * e, flag)) / (2 * h) for e in np.eye(3)], axis=1)[far]
            worst, top = max(worst, float(np.abs(got - fd).max())), max(top, float(np.abs(fd).max()))
        print("gamma vs central differences, flag %d: %.2e of the largest entry" % (flag, worst / top))
        assert worst <= 1e-8 * top, (flag, worst / top)


def test_normal_component_of_flag0_is_the_oracles_dgdn_entry():
    """n_j . gamma(t, s_j), flag 0, is the oracle's K(t, s_j) of a NORMAL_DERIV target in the far and near regimes and on the panel"""
    v = O.unit_sphere(3)
    g = G.geometry(v)
    orc = O.Oracle(v, bc=np.ones(len(v), np.uint8), K=G.K)
    n = len(v)
    for ti in (0, 17, 100):
        # a target PANEL of the oracle stands for its centroid
        got = np.einsum("pk,pk->p", G.gamma(g["center"][ti], 0, v, g), g["normal"])
        want = orc.kernel_entries(np.full(n, ti), np.arange(n))
        assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
        assert got[ti] == pytest.approx(2 * np.pi, rel=1e-14)
    orc.close()


# ---- the cases ----------------------------------------------------------------------------------------------------------------
def regimes(R):
    """(near-regime pairs, far-regime pairs, self pairs) among the listed near pairs"""
    near = far = self_ = 0
    for b, lists in R.near.items():
        idx = np.concatenate([R.leaf_panels(s) for s in lists])
        for k in R.leaf_points(b):
            d = np.linalg.norm(R.P[k][None] - R.g["center"][idx], axis=1)
            with np.errstate(divide="ignore"):
                nb = np.sqrt(2 * R.g["area"][idx]) / d >= 0.5
            self_ += int((d < 1e-8).sum())
            near += int(nb.sum())
            far += int((~nb).sum())
    return near, far, self_


def leaf_rows(R):
    leaves = np.nonzero(R.tb["leaf"])[0]
    return (R.tb["be"] - R.tb["bb"])[leaves]


def test_case_shapes():
    shapes = {}
    for name in G.CASES:
        R = G.reference(name)
        shapes[name] = {k: R.info[k] for k in ("n_target_points", "n_target_leaves", "p2p_pairs", "m2l_pairs", "l2l_ops", "live_slots")}
    print("\n" + "\n".join("%-10s %s" % kv for kv in shapes.items()))
    R = G.reference("two_r3")
    near, far, self_ = regimes(R)
    assert near > 30 and far > 1000 and self_ == 0                     # both regimes among the listed pairs
    assert R.info["n_target_points"] == 272 and len(R.pts) == 280      # the copies: one body per flag
    assert R.info["m2l_pairs"] > 100 and R.info["l2l_ops"] > 0 and R.info["p2p_pairs"] > 100
    assert set(R.flags.tolist()) == {0, 1}
    R = G.reference("r4_ncrit8")
    assert regimes(R)[2] == 4                                          # the four targets on centroids meet their panels
    assert R.info["l2l_ops"] > 0 and R.info["m2l_pairs"] > 1000
    R = G.reference("big_leaves")
    assert leaf_rows(R).max() > 64 and R.info["p2p_pairs"] > 0 and R.info["m2l_pairs"] > 0     # several chunks per leaf, both kernels
    R = G.reference("one_row")
    assert np.all(leaf_rows(R) == 1)
    R = G.reference("far_only")
    assert R.info["p2p_pairs"] == 0 and R.info["m2l_pairs"] >= 1 and R.info["l2l_ops"] >= 1
    R = G.reference("no_far")
    assert R.info["m2l_pairs"] == 0 and R.info["p2p_pairs"] > 0
    R = G.reference("awkward")
    base = G.reference("two_r3")
    assert np.array_equal(R.tb["center"][0], base.tb["center"][0]) and R.tb["side"][0] == base.tb["side"][0]
    leaves = np.nonzero(R.tb["leaf"])[0]
    pos = np.empty(len(R.tree), dtype=np.int64)
    pos[R.tree] = np.arange(len(R.tree))
    on_centre = 0
    for k in range(len(R.pts) - G.N_AWKWARD, len(R.pts)):               # each added point sits on the axis of the leaf that holds it
        at = pos[R.given[k]]
        b = leaves[(R.tb["bb"][leaves] <= at) & (at < R.tb["be"][leaves])]
        assert len(b) == 1
        d = R.pts[k] - R.tb["center"][b[0]]
        assert abs(d[0]) + abs(d[1]) < 1e-12, (k, d)
        on_centre += int(np.all(d == 0))
        assert abs(d[2]) <= 0.5 * R.tb["side"][b[0]]
    assert on_centre >= 1
    assert R.info["m2l_pairs"] > 100


def test_limit_sum_is_what_the_composed_reference_converges_to():
    """on two_r3: the error against the limit sum falls by at least 3 x per four orders and is <= 1e-4 at p = 16, per flag class"""
    R = G.reference("two_r3")
    lim = R.limit()
    errs = {p: [rel(R.gradient(p)[R.flags == f], lim[R.flags == f]) for f in (0, 1)] for p in (4, 8, 12, 16)}
    print("\ncomposed reference vs limit sum:", errs)
    for f in (0, 1):
        for a, b in ((4, 8), (8, 12), (12, 16)):
            assert errs[b][f] * 3 <= errs[a][f], (f, a, b, errs)
        assert errs[16][f] <= 1e-4


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_symbols_present(fb):
    L = fb.lib()
    for name in ("fmmbem_plan_execute_gradient", "fmmbem_plan_execute_gradient_device", "fmmbem_kernel_gradient_entries"):
        assert name in fb.SYMBOLS
        getattr(L, name)
    assert L.fmmbem_version() == 1
    assert callable(fb.kernel_gradient_entries) and hasattr(fb.FMM_plan, "execute_gradient")
    assert hasattr(fb.FMM_plan, "execute_gradient_torch") and hasattr(fb.FMM_plan, "execute_gradient_device")


def test_refusals_in_order_and_the_handle_stays_usable(fb):
    L = fb.lib()
    v = fb.unit_sphere(3)
    pts = np.random.default_rng(1).normal(size=(50, 3)) * 2
    K = fb.LaplaceSphericalBEM(5, 3)
    tp = fb.FMM_plan(K, v, host_only=True, targets=pts)
    single = fb.FMM_plan(K, v, host_only=True)
    stokes = fb.FMM_plan(fb.StokesSphericalBEM(5, 3), v, host_only=True).field_plan(pts)
    buf = np.zeros(3 * len(v) + 3 * len(pts))
    bp, null = buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p()
    before = tp.pairs("m2l").copy()
    forms = (lambda h, p, x, g: L.fmmbem_plan_execute_gradient(h, p, x, g),
             lambda h, p, x, g: L.fmmbem_plan_execute_gradient_device(h, p, x, g, null))
    for call in forms:
        assert call(None, 5, bp, bp) == 1                               # null plan
        assert call(tp._h, 5, None, bp) == 1 and call(tp._h, 5, bp, None) == 1
        assert call(single._h, 5, None, bp) == 1                        # null before everything else
        assert call(tp._h, 0, bp, bp) == 1 and call(tp._h, 6, bp, bp) == 1       # p outside 1..p_max
        assert call(single._h, 0, bp, bp) == 1 and call(stokes._h, 17, bp, bp) == 1   # ... before the kind of plan
        assert call(single._h, 5, bp, bp) == 6                          # not over separate targets
        assert "separate targets" in L.fmmbem_last_error().decode()
        assert call(stokes._h, 5, bp, bp) == 6                          # a Stokes plan (before host-only)
        assert "Laplace" in L.fmmbem_last_error().decode()
        assert call(tp._h, 5, bp, bp) == 6                              # host-only, as execute
        assert "host-only" in L.fmmbem_last_error().decode()
    assert np.all(buf == 0)
    with pytest.raises(fb.FmmBemError) as e:
        tp.execute_gradient(np.ones(len(v)))
    assert e.value.status == 6
    with pytest.raises(fb.FmmBemError) as e:
        single.execute_gradient(np.ones(len(v)))
    assert e.value.status == 6
    with pytest.raises(ValueError):
        tp.execute_gradient(np.ones(len(v) + 1))
    # the handles are still usable
    assert np.array_equal(tp.pairs("m2l"), before)
    assert tp.stats()["n_panels"] == len(v) and tp.target_info()["n_targets"] == 50
    assert single.stats()["n_panels"] == len(v)
    assert stokes.target_info()["n_targets"] == 50


def test_gradient_entries_arguments(fb):
    L = fb.lib()
    o = fb.Options()
    L.fmmbem_options_default(ctypes.byref(o))
    out = np.zeros(9)
    op = out.ctypes.data_as(ctypes.c_void_p)
    assert L.fmmbem_kernel_gradient_entries(ctypes.byref(o), 1, None, None, None, None) == 1
    assert L.fmmbem_kernel_gradient_entries(None, 1, op, None, op, op) == 1
    assert L.fmmbem_kernel_gradient_entries(ctypes.byref(o), 0, op, None, op, op) == 0
    o.kernel = 1
    assert L.fmmbem_kernel_gradient_entries(ctypes.byref(o), 1, op, None, op, op) == 6      # Stokes
    o.kernel, o.quad_k = 0, 5
    assert L.fmmbem_kernel_gradient_entries(ctypes.byref(o), 1, op, None, op, op) == 1      # no such rule
    with pytest.raises(ValueError):
        fb.kernel_gradient_entries(fb.LaplaceSphericalBEM(5, 3), np.zeros((2, 3, 3)), np.zeros((3, 3, 3)))
