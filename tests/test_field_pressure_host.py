"""The field pressure (fmmbem_plan_execute_pressure), host side: the entry formula against the gradient's and against the momentum
equation of the velocity entries the oracle gives, the composed CPU reference pinned to the oracle's operators, its convergence, the
shapes of the cases the GPU tests run, and the refusals of the C ABI.  No device needed."""
import ctypes

import numpy as np
import pytest

import field_gradient_reference as G
import field_plan_reference as R
import field_pressure_reference as Q
from oracle import oracle as O


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# ---- the entry ----------------------------------------------------------------------------------------------------------------
def test_pi_is_minus_the_flag0_gamma_of_the_gradient():
    """with the K stored points, pi(t, s) = -gamma(t, s) of flag 0 at the same K, to 1e-14 of the entry"""
    v = O.unit_sphere(3)
    g = G.geometry(v)                                       # K = 3, the gradient reference's rule
    rng = np.random.default_rng(7)
    for _ in range(6):
        t = rng.normal(size=3)
        t *= (1.1 + 1.5 * rng.random()) / np.linalg.norm(t)
        got = Q.pi_entry(t, v, g, far_only=True, rules=G._rules())
        want = -G.gamma(t, 0, v, g, far_only=True)
        scale = np.abs(want).max(axis=1)
        assert np.all(np.abs(got - want).max(axis=1) <= 1e-14 * scale)


def test_momentum_equation_of_the_oracles_velocity_entries():
    """mu lap(U f) = grad(pi . f) for single far-regime pairs: U the oracle's velocity entries (Probes.entries, with their 1/(2 mu)),
    both sides by central differences with step h = 1e-3 at targets 1.6 .. 2.6 from the centre of unit_sphere(3).  The differences'
    own accuracy: truncation h^2 / 12 times the ratio of the fourth to the second derivatives (~ 20 / r^2) ~ 1e-6, rounding
    2^-53 |U| / h^2 against |lap U| ~ |U| / r^2, ~ 1e-9.  Measured disagreement: 1.73e-06 of the largest |grad(pi . f)| of the pairs;
    asserted: 10 x that.  This pins the sign and the 1/(2 mu) against the velocity the library returns, with no pressure code of the
    library in it."""
    v = O.unit_sphere(3)
    g = Q.geometry(v)
    rng = np.random.default_rng(12)
    h = 1e-3
    T = 6
    t0 = G._dirs(rng, T) * (1.6 + rng.random(T))[:, None]
    steps = np.concatenate([np.zeros((1, 3)), h * np.eye(3), -h * np.eye(3)])        # centre, +x +y +z, -x -y -z
    pts = (t0[:, None, :] + steps[None, :, :]).reshape(-1, 3)
    probes = R.Probes(v, pts, np.zeros(len(pts), np.uint8))
    placed = probes.centres.reshape(T, 7, 3)
    f = rng.normal(size=(len(v), 3))
    worst, top, pairs = 0.0, 0.0, 0
    for a in range(T):
        _, near = Q.regimes(placed[a, 0], g)
        src = np.nonzero(~near)[0][:40]
        assert len(src) == 40
        E = probes.entries(np.arange(7 * a, 7 * a + 7), src)                           # (7, 40, 3, 3)
        u = np.einsum("kjab,jb->kja", E, f[src])                                       # (7, 40, 3): U f per pair
        lap = (u[1:].sum(0) - 6 * u[0]) / (h * h)                                      # (40, 3)
        q = np.stack([np.sum(Q.pi_entry(placed[a, k], v[src], Q.sub(g, src), far_only=True) * f[src], axis=1) for k in range(7)])
        grad = np.stack([(q[1 + k] - q[4 + k]) / (2 * h) for k in range(3)], axis=1)   # (40, 3)
        worst = max(worst, float(np.abs(R.MU * lap - grad).max()))
        top = max(top, float(np.abs(grad).max()))
        pairs += len(src)
    probes.close()
    print("momentum equation, %d far pairs, h = %g: %.2e of the largest |grad(pi . f)|" % (pairs, h, worst / top))
    assert worst <= 10 * 1.73e-06 * top, worst / top


# ---- the reference ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [4, 9, 13, 16])
def test_far_half_and_slot_order_give_the_oracles_velocity(fb, p):
    """The VALUES and gradients of slots 0..3 through the same L the pressure is taken of, recombined as l2p_stokes_kernel does,
    are the velocity the oracle's single operators give over the field plan's lists (field_plan_reference.composed_reference) where
    no target has a near pair: to 1e-14.  Ties the composition and its slot order to the oracle."""
    ref = Q.reference("far_only")
    assert ref.info["p2p_pairs"] == 0
    probes = R.Probes(ref.v, ref.c["pts"], np.zeros(len(ref.pts), np.uint8))
    _, plan = Q.host_plan(fb, ref.v, probes.centres, ref.c["ncrit"])
    assert np.array_equal(probes.centres, ref.pts)
    for key in ("x", "x2"):
        want = R.composed_reference(plan, probes, ref.v, ref.vector(key), p)
        got = ref.velocity(p, key)
        print("far_only p = %d %s: velocity by the pressure's L vs the oracle's operators %.2e" % (p, key, rel(got, want)))
        assert rel(got, want) <= 1e-14
    probes.close()


def test_reference_converges_to_the_limit_sum():
    """|reference(p) - limit| / |limit| falls monotonically over p = 4, 8, 12, 16 (a wrong sign of the far half does not converge).
    Measured: two_r3 7.3e-03, 5.0e-04, 3.0e-05, 7.6e-06; far_only 3.9e-02, 4.9e-04, 4.5e-06, 4.2e-08."""
    for name in ("two_r3", "far_only"):
        ref = Q.reference(name)
        lim = ref.limit()
        errs = [rel(ref.pressure(p), lim) for p in (4, 8, 12, 16)]
        print("%s vs limit sum at p = 4, 8, 12, 16: %s" % (name, " ".join("%.1e" % e for e in errs)))
        assert errs[0] > errs[1] > errs[2] > errs[3], (name, errs)
        assert errs[0] < 0.1, (name, errs)                    # (a wrong sign gives ~ 2 |far| / |q|, at every order)


# ---- the cases ----------------------------------------------------------------------------------------------------------------
def count_regimes(ref):
    """(near-regime pairs, far-regime pairs, self pairs) among the listed near pairs"""
    near = far = self_ = 0
    for b, lists in ref.near.items():
        idx = np.concatenate([ref.leaf_panels(s) for s in lists])
        gi = Q.sub(ref.g, idx)
        for k in ref.leaf_points(b):
            s_, n_ = Q.regimes(ref.P[k], gi)
            self_ += int(s_.sum())
            near += int(n_.sum())
            far += int((~n_ & ~s_).sum())
    return near, far, self_


def leaf_rows(ref):
    leaves = np.nonzero(ref.tb["leaf"])[0]
    return (ref.tb["be"] - ref.tb["bb"])[leaves]


def test_case_shapes():
    shapes = {name: {k: Q.reference(name).info[k] for k in ("n_target_points", "n_target_leaves", "p2p_pairs", "m2l_pairs")} for name in Q.CASES}
    print("\n" + "\n".join("%-10s %s" % kv for kv in shapes.items()))
    ref = Q.reference("two_r3")
    near, far, self_ = count_regimes(ref)
    print("two_r3: near-regime pairs %d, far-regime %d" % (near, far))
    assert near >= 20 and far > 1000 and self_ == 0                    # both regimes among the listed pairs
    assert ref.info["n_target_points"] == 271 and len(ref.pts) == 280  # the ten copies: one distinct point
    assert np.all(ref.given[-10:] == ref.given[-10])
    assert ref.info["m2l_pairs"] > 100 and len(ref.lists["l2l"]) > 0 and ref.info["p2p_pairs"] > 100
    ref = Q.reference("r4_ncrit8")
    assert count_regimes(ref)[2] == 4                                  # the four targets on centroids meet their panels
    assert len(ref.lists["l2l"]) > 0 and ref.info["m2l_pairs"] > 1000
    ref = Q.reference("big_leaves")
    assert leaf_rows(ref).max() > 64 and ref.info["p2p_pairs"] > 0 and ref.info["m2l_pairs"] > 0   # several chunks per leaf, both kernels
    ref = Q.reference("one_row")
    assert np.all(leaf_rows(ref) == 1)
    ref = Q.reference("far_only")
    assert ref.info["p2p_pairs"] == 0 and ref.info["m2l_pairs"] >= 1 and len(ref.lists["l2l"]) >= 1
    ref = Q.reference("no_far")
    assert ref.info["m2l_pairs"] == 0 and ref.info["p2p_pairs"] > 0
    ref = Q.reference("awkward")
    leaves = np.nonzero(ref.tb["leaf"])[0]
    pos = np.empty(len(ref.tree), dtype=np.int64)
    pos[ref.tree] = np.arange(len(ref.tree))
    on_axis = on_centre = 0
    for k in range(len(ref.pts) - Q.N_AWKWARD, len(ref.pts)):            # the added points: on the axis of the leaf that holds them
        at = pos[ref.given[k]]
        b = leaves[(ref.tb["bb"][leaves] <= at) & (at < ref.tb["be"][leaves])]
        assert len(b) == 1
        d = ref.pts[k] - ref.tb["center"][b[0]]
        on_axis += int(abs(d[0]) + abs(d[1]) < 1e-12)
        on_centre += int(np.abs(d).max() < 1e-12)
    print("awkward: %d of the %d added points on the axis of their leaf, %d at its centre" % (on_axis, Q.N_AWKWARD, on_centre))
    assert on_axis == Q.N_AWKWARD and on_centre >= 1
    assert ref.info["m2l_pairs"] > 100


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_symbols_present(fb):
    L = fb.lib()
    for name in ("fmmbem_plan_execute_pressure", "fmmbem_plan_execute_pressure_device", "fmmbem_kernel_pressure_entries"):
        assert name in fb.SYMBOLS
        getattr(L, name)
    assert L.fmmbem_version() == 1
    assert callable(fb.kernel_pressure_entries) and hasattr(fb.FMM_plan, "execute_pressure")
    assert hasattr(fb.FMM_plan, "execute_pressure_torch") and hasattr(fb.FMM_plan, "execute_pressure_device")


def test_refusals_in_order_and_the_handle_stays_usable(fb):
    L = fb.lib()
    v = fb.unit_sphere(3)
    pts = np.random.default_rng(1).normal(size=(50, 3)) * 2
    KS, KL = fb.StokesSphericalBEM(5, 3), fb.LaplaceSphericalBEM(5, 3)
    tp = fb.FMM_plan(KS, v, host_only=True).field_plan(pts)
    single = fb.FMM_plan(KS, v, host_only=True)
    laplace = fb.FMM_plan(KL, v, host_only=True).field_plan(pts)
    flags = np.zeros(50, np.uint8)
    flags[7] = 1
    traction = fb.FMM_plan(KS, v, host_only=True).field_plan(pts, flags)
    buf = np.zeros(3 * len(v) + len(pts))
    bp, null = buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p()
    before = tp.pairs("m2l").copy()
    forms = (lambda h, p, x, q: L.fmmbem_plan_execute_pressure(h, p, x, q),
             lambda h, p, x, q: L.fmmbem_plan_execute_pressure_device(h, p, x, q, null))
    for call in forms:
        assert call(None, 5, bp, bp) == 1                               # 1 null plan
        assert call(tp._h, 5, None, bp) == 1 and call(tp._h, 5, bp, None) == 1
        assert call(single._h, 5, None, bp) == 1                        #   null before everything else
        assert call(tp._h, 0, bp, bp) == 1 and call(tp._h, 6, bp, bp) == 1       # 2 p outside 1..p_max
        assert "p_max" in L.fmmbem_last_error().decode()
        assert call(single._h, 0, bp, bp) == 1 and call(laplace._h, 17, bp, bp) == 1 and call(traction._h, 0, bp, bp) == 1   #   before the kind of plan
        assert call(single._h, 5, bp, bp) == 6                          # 3 not over separate targets
        assert "separate targets" in L.fmmbem_last_error().decode()
        assert call(laplace._h, 5, bp, bp) == 6                         # 4 a Laplace plan
        assert "Stokes" in L.fmmbem_last_error().decode()
        assert call(traction._h, 5, bp, bp) == 6                        # 5 a TRACTION target (before host-only)
        assert "VELOCITY" in L.fmmbem_last_error().decode()
        assert call(tp._h, 5, bp, bp) == 6                              # 6 host-only, as execute
        assert "host-only" in L.fmmbem_last_error().decode()
    assert np.all(buf == 0)
    for plan, x in ((tp, np.ones((len(v), 3))), (single, np.ones(3 * len(v))), (laplace, np.ones(len(v))), (traction, np.ones((len(v), 3)))):
        with pytest.raises(fb.FmmBemError) as e:
            plan.execute_pressure(x)
        assert e.value.status == 6
    for bad in (np.ones(len(v)), np.ones(3 * len(v) + 1), np.ones((len(v), 2)), np.ones((3, len(v)))):
        with pytest.raises(ValueError):
            tp.execute_pressure(bad)
    # the handles are still usable
    assert np.array_equal(tp.pairs("m2l"), before)
    assert tp.stats()["n_panels"] == len(v) and tp.target_info()["n_targets"] == 50
    assert single.stats()["n_panels"] == len(v)
    assert laplace.target_info()["n_targets"] == 50 and traction.target_info()["n_targets"] == 50


def test_pressure_entries_arguments(fb):
    L = fb.lib()
    o = fb.Options()
    L.fmmbem_options_default(ctypes.byref(o))
    o.kernel = 1
    out = np.zeros(9)
    op = out.ctypes.data_as(ctypes.c_void_p)
    assert L.fmmbem_kernel_pressure_entries(ctypes.byref(o), 1, None, None, None) == 1
    assert L.fmmbem_kernel_pressure_entries(ctypes.byref(o), 1, op, op, None) == 1
    assert L.fmmbem_kernel_pressure_entries(None, 1, op, op, op) == 1
    assert L.fmmbem_kernel_pressure_entries(ctypes.byref(o), 0, op, op, op) == 0
    o.kernel = 0
    assert L.fmmbem_kernel_pressure_entries(ctypes.byref(o), 1, op, op, op) == 6             # Laplace
    o.kernel, o.quad_k = 1, 5
    assert L.fmmbem_kernel_pressure_entries(ctypes.byref(o), 1, op, op, op) == 1             # no such rule
    o.quad_k, o.quad_k_fine = 4, 5
    assert L.fmmbem_kernel_pressure_entries(ctypes.byref(o), 1, op, op, op) == 1             # no such fine rule
    assert np.all(out == 0)
    with pytest.raises(ValueError):
        fb.kernel_pressure_entries(fb.StokesSphericalBEM(5, 3), np.zeros((2, 3, 3)), np.zeros((3, 3, 3)))
