"""The double-sum M2L (csrc/kernels_m2l.hip) in every form launch_m2l dispatches at p <= 12, against the CPU oracle.

A plan created under FMMBEM_M2L_ROT=0 runs these kernels at every order -- the documented way to run without the rotation
kernels -- where the default plan runs them at p = 13 ... 16 only, one slot per pass:

    m2l_small_kernel<1..4>      p <= 4, lanes = sources, one slot per pass
    m2l_kernel<P, NS, NSLOT>    p >= 5; NS = 2 wavefronts per target at p = 10; NSLOT = 4 slots per pass where the live slots are a
                                multiple of four and p <= 10 (Stokes velocity), 2 where even and p <= 12 (Laplace with mixed flags;
                                Stokes velocity at p = 11, 12), else 1

Per (case, flag set) of tests/m2l_form_cases.py two plans, each the only holder of its geometry (own_geometry): the FALLBACK
(FMMBEM_M2L_ROT=0) and the CONTROL (the default path), both with p_max = 16, so that every order runs with the strides s_max,
g_max, p_max of another order.  Per order, for both plans: which kernel ran (stats m2l_kernel: 3 at p <= 4, 2 above; the control's
1), every live slot of L of every box against the oracle's, per box and slot relative to that slot's largest coefficient, and the
rows against the oracle's matvec by relative L2; the fallback's L against the control's on the same scale.  Once per (case, flag
set): the fallback repeated, replayed as a graph and in a batch of three gives the bits of its single execute.

Gates: TOL_EXPANSION and TOL_MATVEC of tests/test_gpu_parity.py (1e-12); the rows on the two soups 1e-11, as tests/test_random_meshes.py
holds soups.  The control is the default path, gated elsewhere, and comes first in every comparison: a gate the control misses would
be a property of the case, not of the fallback -- two cases have one, for L at p = 1 (L_GATE below: ten times the control's
measured worst, capped at 1e-10).  No gate here was measured on the fallback.  Every order is walked and printed before the
first miss fails the test.

The eleven-slot Stokes plan (mixed3) has no oracle far field: its reference is the composition of tests/double_layer_reference.py
over the plan's own lists, which tests/test_gpu_stokes_double_layer.py holds the default path to; rows by that file's bounds."""
import numpy as np
import pytest

import m2l_form_cases as mfc
import own_geometry
from conftest import rel_l2
from test_gpu_parity import TOL_EXPANSION, TOL_MATVEC

pytestmark = pytest.mark.gpu

TOL_ROWS_SOUP = 1e-11                                  # tests/test_random_meshes.py
ROW_GATE = {"two_r54": TOL_MATVEC, "tiny48": TOL_MATVEC, "stokes_r43": TOL_MATVEC, "soup2500": TOL_ROWS_SOUP, "stokes_soup1500": TOL_ROWS_SOUP}
# L per box and slot: TOL_EXPANSION, but on two cases the CONTROL (the default path) is above it at p = 1, where a box's slot is ONE
# coefficient, the sum of up to 191 translations of both signs, held against itself and not against a larger neighbour:
#     soup2500     control 7.09e-12 (all POTENTIAL, p = 1; every other order and flag set of the case <= 9.3e-13)   -> 7.1e-11
#     stokes_r43   control 3.04e-12 (all VELOCITY, p = 1; the eleven-slot plan <= 1.5e-13)                          -> 3.1e-11
# ten times the control's measured worst (MI355X), below the cap of 1e-10; the fallback is held to the same figure.
L_GATE = {"two_r54": TOL_EXPANSION, "tiny48": TOL_EXPANSION, "stokes_soup1500": TOL_EXPANSION, "soup2500": 7.1e-11, "stokes_r43": 3.1e-11}
P_MAX = 16

ORDERS = {
    "two_r54": tuple(range(1, 13)), "soup2500": (1, 3, 4, 5, 8, 10, 12), "tiny48": (2, 4, 5, 10),
    ("stokes_r43", "velocity"): tuple(range(1, 13)), ("stokes_soup1500", "velocity"): (2, 4, 6, 10, 11), ("stokes_r43", "mixed3"): (3, 8, 12),
}
RUNS = ([(name, fs) for name in ("two_r54", "soup2500", "tiny48") for fs in mfc.LAPLACE_FLAG_SETS]
        + [("stokes_r43", "velocity"), ("stokes_soup1500", "velocity"), ("stokes_r43", "mixed3")])


def _orders(name, flag_set):
    return ORDERS[name] if name in ORDERS else ORDERS[name, flag_set]


def _plans(fb, monkeypatch, name, flag_set, p_max=P_MAX):
    """(fallback, its kernel object, control, its kernel object)"""
    Kf, args, kw = mfc.make_plan_args(fb, name, flag_set, p_max)
    fallback = own_geometry.plan_under(fb, monkeypatch, {"FMMBEM_M2L_ROT": "0"}, *args, **kw)
    Kc, args, kw = mfc.make_plan_args(fb, name, flag_set, p_max)
    control = own_geometry.plan_under(fb, monkeypatch, None, *args, **kw)
    return fallback, Kf, control, Kc


def _slot_errors(L, ref, slots, dipole_at_p1=()):
    """per box and slot, relative to that slot's largest coefficient in the reference; every live slot's reference is nonzero
    somewhere.  dipole_at_p1: at p = 1 the slots of a double layer (Laplace slot 1, Stokes 4..10) hold the gradient of a constant:
    the reference is zero everywhere there, and so must the device be, exactly"""
    worst = 0.0
    for s in slots:
        scale = np.abs(ref[:, s]).max(axis=1, keepdims=True)
        if s in dipole_at_p1:
            assert not np.any(ref[:, s]) and not np.any(L[:, s]), "slot %d at p = 1" % s
            continue
        assert scale.max() > 0, "slot %d of the reference is zero everywhere" % s
        worst = max(worst, float(np.max(np.abs(L[:, s] - ref[:, s]) / (scale + 1e-300))))
    return worst


def _walk(name, flag_set, orders, fallback, Kf, control, Kc, x, reference, row_error):
    """every order: stats, L and rows of both plans; the figures are printed before anything is asserted.
    reference(p) -> (L, rows data); row_error(y, rows data, what) -> the figure held to the case's row gate"""
    slots = mfc.live_slots(name, flag_set)
    worst = {"control L": 0.0, "fallback L": 0.0, "control rows": 0.0, "fallback rows": 0.0, "fallback L - control L": 0.0}
    missed = []
    for p in orders:
        Lref, rows = reference(p)
        got = {}
        for what, plan, K, kernel in (("control", control, Kc, 1), ("fallback", fallback, Kf, 3 if p <= 4 else 2)):
            K.set_p(p)
            y = plan.execute(x)
            assert plan.stats()["m2l_kernel"] == kernel and plan.stats()["last_p"] == p, (what, p, plan.stats()["m2l_kernel"])
            L = plan.expansions("L", p)
            assert L.shape[0] == Lref.shape[0] and L.shape[2] == Lref.shape[2] and np.all(np.isfinite(L)) and np.all(np.isfinite(y)), (what, p)
            dipole = () if p > 1 else tuple(range(4, 11)) if mfc.is_stokes(name) else (1,)
            got[what] = (L, _slot_errors(L, Lref, slots, dipole), row_error(y, rows, (name, flag_set, what, p)))
        ab = 0.0
        for s in slots:
            scale = np.abs(Lref[:, s]).max(axis=1, keepdims=True) + 1e-300
            ab = max(ab, float(np.max(np.abs(got["fallback"][0][:, s] - got["control"][0][:, s]) / scale)))
        print("m2l forms %s %s p = %2d: L control %.3e fallback %.3e, rows control %.3e fallback %.3e, fallback L - control L %.3e"
              % (name, flag_set, p, got["control"][1], got["fallback"][1], got["control"][2], got["fallback"][2], ab))
        for what in ("control", "fallback"):               # the control first
            if got[what][1] > L_GATE[name]:
                missed.append((what, "L", p, got[what][1]))
            if got[what][2] > ROW_GATE[name]:
                missed.append((what, "rows", p, got[what][2]))
            worst[what + " L"] = max(worst[what + " L"], got[what][1])
            worst[what + " rows"] = max(worst[what + " rows"], got[what][2])
        if ab > L_GATE[name]:
            missed.append(("fallback L - control L", p, ab))
        worst["fallback L - control L"] = max(worst["fallback L - control L"], ab)
    print("m2l forms %s %s worst over p = %s: %s" % (name, flag_set, list(orders), ", ".join("%s %.2e" % kv for kv in worst.items())))
    assert not missed, missed                              # every order is walked and printed before the first one fails the test


def _same_bits_again(name, fallback, Kf, x, p):
    """the fallback repeated, replayed as a graph, and in a batch of three: the bits of its single execute"""
    Kf.set_p(p)
    y = fallback.execute(x)
    assert np.array_equal(fallback.execute(x), y), "repeated"
    X = mfc.density(name, len(x), k=3)
    singles = [fallback.execute(X[i]) for i in range(3)]
    batch = fallback.execute_batch(X)
    for i in range(3):
        assert np.array_equal(batch[i], singles[i]), ("batch", i)
    fallback.set_graphs(True)
    try:
        for rep in range(3):                               # launch by launch, captured, replayed
            assert np.array_equal(fallback.execute(x), y), ("graph", rep)
            assert fallback.stats()["m2l_kernel"] == (3 if p <= 4 else 2)
    finally:
        fallback.set_graphs(False)


def _oracle_reference(oracle_mod, name, flag_set):
    def reference(p):
        r = mfc.reference(oracle_mod, name, flag_set, p)
        return r["L"], r["y"]
    return reference, lambda y, yo, what: rel_l2(y, yo)


def _composed_reference(fb, oracle_mod, name, flag_set, control, v, x):
    """mixed3: the double layer's composed reference over the control plan's lists (the flags and the switches change no list: held
    below), rows by check_rows of tests/test_gpu_stokes_double_layer.py -- its own two bounds; the figure returned is the largest
    relative L2 of the two flag classes"""
    import double_layer_reference as D
    import field_plan_reference as R
    from test_gpu_stokes_double_layer import check_rows
    assert (R.QUAD_K, R.QUAD_K_FINE, R.MU) == (mfc.STOKES_K, mfc.STOKES_KFINE, mfc.STOKES_MU)
    fl = mfc.flags(name, flag_set, len(v))
    probes = R.Probes(v, R.centroids(v), fl)
    o = mfc.make_oracle(oracle_mod, name, "velocity")
    assert np.array_equal(control.pairs("m2l"), o.pairs("m2l"))          # the lists the composition walks are the oracle's
    o.close()
    cache = {}

    def reference(p):
        if p not in cache:
            M, L = D.compose_expansions(control, v, x, p)
            cache[p] = (L, D.compose_rows(control, x, p, probes, L))
        return cache[p]

    def row_error(y, rows, what):
        ref, T = rows
        out = check_rows(y, ref, T, fl, what)
        assert set(out) == {"TRACTION", "VELOCITY"}
        return max(rel for rel, _ in out.values())
    return reference, row_error


@pytest.mark.parametrize("name,flag_set", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_every_form_against_the_oracle(fb, oracle_mod, monkeypatch, name, flag_set):
    fallback, Kf, control, Kc = _plans(fb, monkeypatch, name, flag_set)
    v = mfc.vertices(fb, name)
    x = mfc.density(name, len(v))
    st = fallback.stats()
    assert st["m2l_pairs"] == mfc.FIGURES[name]["pairs"] and st["n_boxes"] == mfc.FIGURES[name]["boxes"]
    assert st["expansion_slots"] == (2 if not mfc.is_stokes(name) else 11 if flag_set == "mixed3" else 8)
    assert np.array_equal(fallback.pairs("m2l"), control.pairs("m2l"))
    if flag_set == "mixed3":
        reference, row_error = _composed_reference(fb, oracle_mod, name, flag_set, control, v, x)
    else:
        reference, row_error = _oracle_reference(oracle_mod, name, flag_set)
    orders = _orders(name, flag_set)
    _walk(name, flag_set, orders, fallback, Kf, control, Kc, x, reference, row_error)
    for p in sorted({min(orders, key=lambda q: abs(q - 4)), max(q for q in orders if q <= 10)}):     # m2l_small_kernel and m2l_kernel
        _same_bits_again(name, fallback, Kf, x, p)
    fallback.close()
    control.close()


@pytest.mark.parametrize("flag_set", ["potential", "mixed"])
@pytest.mark.parametrize("p", [4, 10])
def test_strides_equal_to_the_order(fb, oracle_mod, monkeypatch, flag_set, p):
    """p_max equal to the order: s_max = S, the strides the kernels' own order gives (every other test here runs below p_max)"""
    name = "two_r54"
    fallback, Kf, control, Kc = _plans(fb, monkeypatch, name, flag_set, p_max=p)
    x = mfc.density(name, fallback.n)
    reference, row_error = _oracle_reference(oracle_mod, name, flag_set)
    _walk(name, flag_set, (p,), fallback, Kf, control, Kc, x, reference, row_error)
    fallback.close()
    control.close()
