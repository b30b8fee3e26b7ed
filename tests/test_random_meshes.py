"""Randomised parity (hypothesis): arbitrary triangle soups -- clustered, stretched, with panels of very different
sizes -- through the host list builder (CPU, against the oracle's lists) and through the whole GPU matvec (against the
oracle's matvec).  The reference's own tests only ever use its sphere generator; these are the inputs it would meet with
a user's mesh."""
import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

from near_form_cases import _soup


def _coverage(pl, n):
    """The counting-kernel check of the reference (tests/correctness.cpp:69-78 with kernel/UnitKernel.hpp: every result
    must equal the number of sources) on the plan's LISTS: sources reaching each leaf through its near blocks, through
    M2L into the leaf or an ancestor, and down the L2L edges the plan applies."""
    bx = pl.boxes()
    cnt = (bx["be"] - bx["bb"]).astype(np.int64)
    far = np.zeros(len(cnt), dtype=np.int64)
    m2l = pl.pairs("m2l")
    np.add.at(far, m2l[:, 1], cnt[m2l[:, 0]])
    for parent, child in pl.pairs("l2l"):              # parents first (level order)
        far[child] += far[parent]
    near = np.zeros(len(cnt), dtype=np.int64)
    p2p = pl.pairs("p2p")
    np.add.at(near, p2p[:, 1], cnt[p2p[:, 0]])
    leaves = np.nonzero(bx["leaf"])[0]
    return near[leaves] + far[leaves]



soup_args = dict(seed=st.integers(0, 2 ** 31 - 1), n=st.integers(2, 900), clusters=st.integers(1, 6),
                 stretch=st.sampled_from([1.0, 3.0, 10.0]), size_spread=st.sampled_from([0.0, 1.0, 2.0]),
                 ncrit=st.sampled_from([8, 32, 64, 126]), theta=st.sampled_from([0.4, 0.5, 0.7]))


@settings(max_examples=25, deadline=None, suppress_health_check=[HealthCheck.function_scoped_fixture])
@given(**soup_args)
def test_host_lists_equal_oracle_on_random_soups(fb, oracle_mod, seed, n, clusters, stretch, size_spread, ncrit, theta):
    v = _soup(seed, n, clusters, stretch, size_spread)
    opts = fb.FMMOptions()
    opts.set_mac_theta(theta)
    opts.set_max_per_box(ncrit)
    try:
        pl = fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), v, opts, host_only=True)
    except fb.FmmBemError as e:                        # clumps the 10-level keys cannot separate
        assert e.status == 5
        return
    o = oracle_mod.Oracle(v, theta=theta, ncrit=ncrit)
    assert np.array_equal(pl.perm(), o.perm())
    assert np.array_equal(pl.pairs("p2p"), o.pairs("p2p")) and np.array_equal(pl.pairs("m2l"), o.pairs("m2l"))
    s, so = pl.stats(), o.stats()
    assert (s["n_boxes"], s["n_leaves"], s["near_nnz_total"]) == (so["boxes"], so["leaves"], so["near_nnz"])
    # downward pass: the default applies every parent->child edge, the reference's lazy rule leaves some out
    # (EvalInteractionLazySparse.hpp:199-237); both lists against the oracle's
    assert s["l2l_reference_omitted"] == so["l2l_skipped"]
    assert s["l2l_ops"] == so["l2l_ops"] + so["l2l_skipped"]
    assert np.all(_coverage(pl, n) == n)              # counting kernel: every source reaches every target exactly once
    opts.reference_l2l = True
    ref = fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), v, opts, host_only=True)
    assert ref.stats()["l2l_ops"] == so["l2l_ops"]
    assert np.all(_coverage(ref, n) == n) == (so["l2l_skipped"] == 0)


@pytest.mark.gpu
@settings(max_examples=30, deadline=None, suppress_health_check=[HealthCheck.function_scoped_fixture])
@given(p=st.integers(1, 16), k=st.sampled_from([1, 3, 4, 7]), mixed=st.booleans(), ref_rule=st.booleans(), **soup_args)
def test_gpu_matvec_equals_oracle_on_random_soups(fb, oracle_mod, seed, n, clusters, stretch, size_spread, ncrit, theta, p, k, mixed,
                                                  ref_rule):
    v = _soup(seed, n, clusters, stretch, size_spread)
    rng = np.random.default_rng(seed + 1)
    bc = (rng.random(n) < 0.5).astype(np.uint8) if mixed else None
    x = rng.standard_normal(n)
    opts = fb.FMMOptions()
    opts.set_mac_theta(theta)
    opts.set_max_per_box(ncrit)
    opts.reference_l2l = ref_rule                      # the reference's L2L list, or the complete one (default)
    try:
        pl = fb.FMM_plan(fb.LaplaceSphericalBEM(p, k), v, opts, bc=bc)
    except fb.FmmBemError as e:
        assert e.status == 5
        return
    y = pl.execute(x)
    yo = oracle_mod.Oracle(v, bc=bc, K=k, theta=theta, ncrit=ncrit, complete_l2l=not ref_rule).matvec(x, p)
    assert np.all(np.isfinite(y))
    assert np.linalg.norm(y - yo) <= 1e-11 * np.linalg.norm(yo)


@pytest.mark.gpu
@settings(max_examples=12, deadline=None, suppress_health_check=[HealthCheck.function_scoped_fixture])
@given(seed=st.integers(0, 2 ** 31 - 1), n=st.integers(2, 400), clusters=st.integers(1, 4), p=st.integers(1, 12),
       kfine=st.sampled_from([7, 13, 19, 25]), ncrit=st.sampled_from([16, 64]), ref_rule=st.booleans())
def test_gpu_stokes_matvec_equals_oracle_on_random_soups(fb, oracle_mod, seed, n, clusters, p, kfine, ncrit, ref_rule):
    v = _soup(seed, n, clusters, 1.0, 1.0)
    rng = np.random.default_rng(seed + 2)
    f = rng.standard_normal((n, 3))
    opts = fb.FMMOptions()
    opts.set_max_per_box(ncrit)
    opts.reference_l2l = ref_rule
    K = fb.StokesSphericalBEM(p, 4, 1e-3)
    K.set_Kfine(kfine)
    try:
        pl = fb.FMM_plan(K, v, opts)
    except fb.FmmBemError as e:
        assert e.status == 5
        return
    u = pl.execute(f)
    uo = oracle_mod.StokesOracle(v, K=4, K_fine=kfine, mu=1e-3, ncrit=ncrit, complete_l2l=not ref_rule).matvec(f, p)
    assert np.all(np.isfinite(u))
    assert np.linalg.norm(u - uo) <= 1e-11 * np.linalg.norm(uo)
