"""The inputs and the reference of tests/test_gpu_field_near_soup.py, held on the host (tests/field_near_cases.py):

1 per case, from host-only plans: no M2L pair at THETA, every target leaf lists every source leaf (more than one run wherever the
  source tree has more than one leaf: (106), two panels, is one leaf), pairs in the self, the nearby and the far regime, a 64-row
  chunk whose rows disagree about the regime of one panel; over the cases target leaves of 1, exactly 64, 65 and more than 128 rows
2 c_ref: the numpy pair functions in float64 against np.longdouble stay within the recorded C_REF
3 the pair functions against the entries of the existing references (field_gradient_reference.gamma, field_pressure_reference.pi_entry,
  field_velocity_gradient_reference.gamma_entry), which this work leaves as they were, on those modules' own cases
4 teeth: the row bound fails on a unit-vector row when the reference is corrupted the way a kernel can be wrong -- a panel dropped
  from a row, the last panel of a PB-sized batch replaced by its neighbour, a nearby pair taken by the K-point rule, an entry off by
  1e-9 relative -- and passes without the corruption"""
import numpy as np
import pytest

import field_gradient_reference as G
import field_plan_reference
import field_near_cases as F
import field_pressure_reference as Q
import field_velocity_gradient_reference as V
import near_form_cases as N

CASES = F.LAPLACE_CASES + F.STOKES_CASES


def _host_plans(fb, case):
    if F.is_stokes(case):
        return {"velocity": F.make_plan(fb, case, host_only=True)}
    return {name: F.make_plan(fb, case, flags=fl, host_only=True) for name, fl in F.flag_sets(case).items()}


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
def _check_case(fb, case):
    """the properties of one case, asserted; returns the rows of its target leaves over its plans"""
    t, g = F.targets(case)[0], F.geometry(case)
    self_, near = F.regimes(t, g)
    far = ~self_ & ~near
    assert self_.sum() > 0 and near.sum() > 0 and far.sum() > 0, (self_.sum(), near.sum(), far.sum())
    sizes = set()
    for name, plan in _host_plans(fb, case).items():
        assert plan.stats()["m2l_pairs"] == 0, (case, name)
        L = F.plan_layout(plan)
        assert np.all(L["mask"] == 1), (case, name)                 # no far field: every panel is in every row's near list
        n_src = len(L["src_leaves"])
        assert (n_src == 1) == (case == 106)
        split = False
        for rows, srcs in L["leaves"]:
            assert len(srcs) == n_src and len(set(srcs)) == n_src, (case, name)
            sizes.add(len(rows))
            for a in range(0, len(rows), 64):
                chunk = rows[a:a + 64]
                split = split or bool(np.any(near[chunk].any(axis=0) & far[chunk].any(axis=0)))
        assert split, (case, name)
        plan.close()
    return sizes


_SIZES = {}


def leaf_sizes(fb, case):
    if case not in _SIZES:
        _SIZES[case] = _check_case(fb, case)
    return _SIZES[case]


@pytest.mark.parametrize("case", CASES)
def test_case_is_what_it_is_meant_to_be(fb, case):
    assert leaf_sizes(fb, case)


def test_leaf_sizes_over_the_cases(fb):
    sizes = set().union(*(leaf_sizes(fb, case) for case in CASES))
    assert 1 in sizes and 64 in sizes and 65 in sizes and max(sizes) > 128, sorted(sizes)
    assert 64 in leaf_sizes(fb, 107) and 65 in leaf_sizes(fb, 102) and max(leaf_sizes(fb, 203)) > 128


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
def _c_ref(case):
    out = {}

    def upd(q, c):
        out[q] = max(out.get(q, 0.0), c)

    X, names = F.vectors(case)
    M = len(F.targets(case)[0])
    if F.is_stokes(case):
        mask = np.ones((M, X.shape[1] // 3))
        El, E64 = F.pairs(case), F.pairs(case, None, np.float64)
        for x in X:
            upd("PI", F.c_ref_of(E64, El, "pressure", x, mask))
            upd("VG", F.c_ref_of(E64, El, "velocity_gradient", x, mask))
        return out
    mask = np.ones((M, X.shape[1]))
    fs = F.flag_sets(case)
    for K in F.LAPLACE_K:
        El, E64 = F.pairs(case, K), F.pairs(case, K, np.float64)
        for x in X:
            upd("G0", F.c_ref_of(E64, El, "gradient", x, mask, fs["all0"]))
            upd("G1", F.c_ref_of(E64, El, "gradient", x, mask, fs["all1"]))
            upd("E0", F.c_ref_of(E64, El, ("representation", "value"), (x, None), mask))
            upd("E1", F.c_ref_of(E64, El, ("representation", "value"), (None, x), mask))
    return out


@pytest.mark.parametrize("case", CASES)
def test_float64_reference_stays_within_c_ref(case):
    got = _c_ref(case)
    print("(%d) c_ref: %s" % (case, ", ".join("%s %.3g" % kv for kv in sorted(got.items()))))
    for q, c in got.items():
        assert c <= F.C_REF[q], (case, q, c)


def test_constants():
    assert F.C_Q == {q: 8.0 * max(c, 1.0) for q, c in F.C_REF.items()} and set(F.C_REF) == set(F.QUANTITIES)
    assert (F.near_batch(13), F.near_batch(13, 7), F.representation_batch(13), F.near_batch(3), F.representation_batch(3)) == (23, 23, 24, 64, 64)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
def _close(a, b, scale):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b)) / scale)


def test_pair_functions_agree_with_the_existing_entries():
    """One equality per module, on its own case r4_ncrit8 (shell, close and centroid targets): the float64 evaluation of this
    module's pair functions is the entry of the existing reference to rounding, 1e-13 of the target's largest entry"""
    R = G.reference("r4_ncrit8")
    t = np.ascontiguousarray(R.pts[-40:])                          # close points, the copies of one point and the four centroids
    E = F.laplace_pairs(t, R.v, R.g, G.K, np.float64)
    for flag, key in ((0, "G0"), (1, "G1")):
        ref = np.stack([G.gamma(p, flag, R.v, R.g) for p in t])
        assert _close(E[key], ref, np.abs(ref).max()) <= 1e-13
    Rq = Q.reference("r4_ncrit8")
    t = np.ascontiguousarray(Rq.pts[-40:])
    assert (Q.R.QUAD_K, Q.R.QUAD_K_FINE) == (N.STOKES_K, N.STOKES_KFINE)
    E = F.stokes_pairs(t, Rq.v, Rq.g, np.float64, mu=Q.R.MU)
    ref = np.stack([Q.pi_entry(p, Rq.v, Rq.g) for p in t])
    assert _close(E["PI"], ref, np.abs(ref).max()) <= 1e-13
    ref = np.stack([V.gamma_entry(p, Rq.v, Rq.g) for p in t])
    assert _close(E["VG"], ref, np.abs(ref).max()) <= 1e-13


def test_values_agree_with_the_oracle_entries(oracle_mod):
    """E0 and E1 -- the semi-analytic G with its mirrored and cut edges, the K-point rule, the fine rule, the two self values --
    against the CPU oracle's own entries K(t, s) of flag-0 and flag-1 targets at the same points, pair by pair in every regime:
    within 1e-12 of the pair's scale mE0 / mE1 (the oracle is double arithmetic in another order)"""
    case = 103
    v, (pts, _, groups) = F.sources(case), F.targets(case)
    pick = np.concatenate([np.arange(s.start, s.stop) for s in (groups["above"], groups["centroid"], groups["in_plane"])]
                          + [np.arange(groups["cluster0"].start, groups["cluster0"].start + 20)])
    n, m = len(v), len(pick)
    tri = field_plan_reference.point_panels(pts[pick])
    for flag, key in ((0, "E0"), (1, "E1")):
        o = oracle_mod.Oracle(np.concatenate([v, tri]), bc=np.concatenate([np.zeros(n, np.uint8), np.full(m, flag, np.uint8)]), K=3,
                              ncrit=1 << 30)
        g = {k: a[:n] for k, a in o.panels().items()}
        t = np.ascontiguousarray(o.panels()["center"][n:])            # the targets where the oracle places them
        ref = o.kernel_entries(np.repeat(np.arange(m) + n, n), np.tile(np.arange(n), m)).reshape(m, n)
        o.close()
        E = F.laplace_pairs(t, v, g, 3, np.float64)
        assert E["self_"].sum() > 0 and E["near"].sum() > 0 and (~E["self_"] & ~E["near"]).sum() > 0
        q = np.abs(E[key] - ref) / E["m" + key]
        print("%s against the oracle: worst %.3g of the pair's scale" % (key, q.max()))
        assert q.max() <= 1e-12, (key, np.unravel_index(np.argmax(q), q.shape), float(q.max()))
    ei, ej = np.nonzero(E["near"] | E["self_"])
    seen = {}
    F.semi_analytic(v[ej, 0], v[ej, 1], v[ej, 2], t[ei], seen)
    for branch in ("flip", "cross"):                                # both sides of both branches of an edge's term are met
        taken = np.stack(seen[branch])
        assert taken.any() and not taken.all(), branch


@pytest.mark.parametrize("case", F.LAPLACE_CASES)
def test_semi_analytic_scale_is_not_loose(case):
    """The E0 scale of a nearby pair carries 1 + |y|_inf / |a_x| per edge, unbounded as the target's foot nears an edge's line.
    What it comes to on the cases: the largest factor and the largest mE0 / |E0| over the nearby and self pairs, held to the record"""
    E = F.pairs(case, 3, np.float64)
    t, v = F.targets(case)[0], F.sources(case)
    ei, ej = np.nonzero(E["near"] | E["self_"])
    seen = {}
    F.semi_analytic(v[ej, 0], v[ej, 1], v[ej, 2], t[ei], seen)
    amp = float(np.stack(seen["amp"]).max())
    ratio = E["mE0"][ei, ej] / np.abs(E["E0"][ei, ej])
    loose = float(ratio.max())
    print("(%d) E0 nearby: largest 1 + |y| / |a_x| %.3g, mE0 / |E0| largest %.3g, median %.3g over %d pairs"
          % (case, amp, loose, float(np.median(ratio)), len(ei)))
    assert amp <= F.E0_AMP_MAX[case][0] and loose <= F.E0_AMP_MAX[case][1]


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
VALUE_KEYS = ("E0", "E1", "G0", "G1", "PI", "VG")
TEETH = [("gradient flag 0", 102, 13, "gradient", 0), ("gradient flag 1", 102, 13, "gradient", 1),
         ("representation value", 102, 13, ("representation", "value"), None),
         ("representation gradient", 107, 13, ("representation", "gradient"), None),
         ("pressure", 203, None, "pressure", None), ("velocity gradient", 203, None, "velocity_gradient", None)]


def _unit(case, j, quantity):
    if F.is_stokes(case):
        x = np.zeros((len(F.sources(case)), 3))
        x[j, 1] = 1.0
        return x.reshape(-1)
    x = np.zeros(len(F.sources(case)))
    x[j] = 1.0
    return (x, x) if isinstance(quantity, tuple) else x


def _worst(E2, E, quantity, x, mask2, mask, flags):
    got = F.row(E2, quantity, x, mask2, flags)[0].astype(np.float64)
    ref, S, T = F.row(E, quantity, x, mask, flags)
    return float(F.ratios(got, ref, F.bound(quantity, S, T, flags)).max())


@pytest.mark.parametrize("what,case,K,quantity,flag", TEETH, ids=[t[0] for t in TEETH])
def test_teeth(fb, what, case, K, quantity, flag):
    E = F.pairs(case, K)
    t, v = F.targets(case)[0], F.sources(case)
    M, P = len(t), len(v)
    flags = None if flag is None else np.full(M, flag, np.uint8)
    mask = np.ones((M, P))
    keys = [k for k in VALUE_KEYS if k in E]
    L = F.plan_layout(F.make_plan(fb, case, K=K, flags=flags, host_only=True))

    def copy():
        return {k: (a.copy() if k in keys else a) for k, a in E.items()}

    # a well-conditioned nearby pair: the point 0.3 sqrt(2 A) above a centroid and its panel
    above = F.targets(case)[2]["above"]
    d = np.linalg.norm(t[above][:, None] - F.geometry(case, K)["center"][None], axis=2)
    i = above.start + 1                                             # heights cycle 0.05, 0.3, 1.9, 2.1 over a panel's four points
    j = int(np.argmin(d[1]))
    assert E["near"][i, j]
    x = _unit(case, j, quantity)
    assert _worst(E, E, quantity, x, mask, mask, flags) <= 1.0      # the uncorrupted reference, rounded to double, passes
    # (a) one panel dropped from one row
    m2 = mask.copy()
    m2[i, j] = 0
    assert _worst(E, E, quantity, x, m2, mask, flags) > 1.0, what
    # (c) one nearby pair by the K-point rule
    far1 = (F.stokes_pairs(t[i:i + 1], v, F.geometry(case), force_far=[(0, j)]) if F.is_stokes(case)
            else F.laplace_pairs(t[i:i + 1], v, F.geometry(case, K), K, force_far=[(0, j)]))
    E2 = copy()
    for k in keys:
        E2[k][i, j] = far1[k][0, j]
    assert _worst(E2, E, quantity, x, mask, mask, flags) > 1.0, what
    # (d) one entry off by 1e-9 relative
    E2 = copy()
    for k in keys:
        E2[k][i, j] *= np.longdouble(1) + np.longdouble(1e-9)
    assert _worst(E2, E, quantity, x, mask, mask, flags) > 1.0, what
    # (b) the last panel of a PB-sized batch replaced by its neighbour, in every row
    PB = (F.representation_batch(K) if isinstance(quantity, tuple) else F.near_batch(K) if not F.is_stokes(case)
          else F.near_batch(len(F.rules(case)[0]), 7))
    row0, length = max(L["src_leaves"], key=lambda leaf: leaf[1])
    assert length > PB, (length, PB)
    pb, nb = int(L["perm"][row0 + PB - 1]), int(L["perm"][row0 + PB])
    E2 = copy()
    for k in keys:
        E2[k][:, pb] = E[k][:, nb]
    assert _worst(E2, E, quantity, _unit(case, pb, quantity), mask, mask, flags) > 1.0, what
