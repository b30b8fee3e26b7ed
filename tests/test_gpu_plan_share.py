"""Plans of the same panels that differ in the boundary-condition flags share one tree, one set of lists and tables
(fmmbem_plan_create_like; fmmbem_plan_create recognises the geometry of a live plan by itself): the drivers' right-hand-side plan
(examples/LaplaceBEM.cpp:218-232, StokesBEM.cpp:266-270) costs the near-matrix assembly and the P2M table, not a second tree build
and traversal.  The shared plan must give the bits of an independent one, and either plan may be destroyed first."""
import os

import numpy as np
import pytest

from conftest import drand48

pytestmark = pytest.mark.gpu


def test_second_plan_with_flipped_flags_shares_the_geometry_and_gives_the_same_bits(fb, monkeypatch):
    v = np.concatenate([fb.unit_sphere(6), fb.unit_sphere(5, center=(2.5, 0.0, 0.3))])
    n = len(v)
    ones = np.ones(n, dtype=np.uint8)
    mixed = (np.arange(n) % 3 == 0).astype(np.uint8)
    x = drand48(n, seed=5)
    # independent plans (the recognition switched off): the reference results
    monkeypatch.setenv("FMMBEM_PLAN_SHARE", "0")
    ref = {}
    for name, bc in (("pot", None), ("nd", ones), ("mixed", mixed)):
        p = fb.FMM_plan(fb.LaplaceSphericalBEM(10, 3), v, bc=bc, p_max=10)
        assert p.stats()["geometry_shared"] == 1
        ref[name] = (p.execute(x), p.diagonal())
        p.close()
    monkeypatch.delenv("FMMBEM_PLAN_SHARE")
    K = fb.LaplaceSphericalBEM(10, 3)
    base = fb.FMM_plan(K, v, p_max=10)
    assert base.stats()["geometry_shared"] == 1
    rhs = fb.FMM_plan(fb.LaplaceSphericalBEM(10, 3), v, bc=ones, p_max=10)          # recognised: same vertices, same options
    third = base.like(mixed)                                                        # asked for
    assert base.stats()["geometry_shared"] == 3 and rhs.stats()["geometry_shared"] == 3
    assert np.array_equal(base.perm(), rhs.perm())
    for p, name in ((base, "pot"), (rhs, "nd"), (third, "mixed")):
        assert np.array_equal(p.execute(x), ref[name][0]), name
        assert np.array_equal(p.diagonal(), ref[name][1]), name
    # other options, other geometry: not shared
    other = fb.FMM_plan(fb.LaplaceSphericalBEM(8, 3), v, bc=ones, p_max=8)
    assert other.stats()["geometry_shared"] == 1
    moved = fb.FMM_plan(fb.LaplaceSphericalBEM(10, 3), v + 1e-9, bc=ones, p_max=10)
    assert moved.stats()["geometry_shared"] == 1
    other.close()
    moved.close()
    # the base goes first: the shared block lives on with the plans that still point to it
    base.close()
    assert rhs.stats()["geometry_shared"] == 2
    K2 = rhs.kernel()
    for p_ in (10, 4):
        K2.set_p(p_)
        y = rhs.execute(x)
        assert np.all(np.isfinite(y))
    K2.set_p(10)
    assert np.array_equal(rhs.execute(x), ref["nd"][0])
    fourth = fb.FMM_plan(fb.LaplaceSphericalBEM(10, 3), v, p_max=10)                 # recognised through a plan that shares it
    assert fourth.stats()["geometry_shared"] == 3
    assert np.array_equal(fourth.execute(x), ref["pot"][0])


def test_stokes_traction_plan_shares_the_velocity_plans_geometry(fb, monkeypatch):
    """StokesBEM.cpp:266-270: the right-hand side comes from a plan whose targets are TRACTION (11 expansion slots per box instead
    of 8, three gradient records per panel): a different set of flag-dependent arrays on the same tree."""
    v = fb.unit_sphere(5)
    n = len(v)
    K = fb.StokesSphericalBEM(7, 4, 1e-3)
    K.set_Kfine(19)
    x = drand48(3 * n, seed=9).reshape(n, 3)
    monkeypatch.setenv("FMMBEM_PLAN_SHARE", "0")
    ref_v = fb.FMM_plan(K, v).execute(x)
    ref_t = fb.FMM_plan(K, v, bc=np.ones(n, dtype=np.uint8)).execute(x)
    monkeypatch.delenv("FMMBEM_PLAN_SHARE")
    fo = fb.FMMOptions()
    fo.near_stream_fraction = 0.5                                                   # hybrid plans share their leaf choice and items too
    for opts in (None, fo):
        vel = fb.FMM_plan(K, v, opts)
        trac = fb.FMM_plan(K, v, opts, bc=np.ones(n, dtype=np.uint8))
        assert vel.stats()["geometry_shared"] == 2 and trac.stats()["expansion_slots"] == 11 and vel.stats()["expansion_slots"] == 8
        yv, yt = vel.execute(x), trac.execute(x)
        if opts is None:
            assert np.array_equal(yv, ref_v) and np.array_equal(yt, ref_t)
        else:
            assert np.linalg.norm(yv - ref_v) <= 1e-13 * np.linalg.norm(ref_v) and np.linalg.norm(yt - ref_t) <= 1e-13 * np.linalg.norm(ref_t)
        vel.close()
        trac.close()


def test_shards_share_per_shard(fb):
    v = fb.unit_sphere(6)
    n = len(v)
    x = drand48(n, seed=2)
    K = fb.LaplaceSphericalBEM(8, 3)
    whole = fb.FMM_plan(K, v, p_max=8).execute(x)
    ones = np.ones(n, dtype=np.uint8)
    whole_nd = fb.FMM_plan(K, v, bc=ones, p_max=8).execute(x)
    tot, tot_nd = np.zeros(n), np.zeros(n)
    for r in range(2):
        a = fb.FMM_plan(K, v, p_max=8, shard=(r, 2))
        b = fb.FMM_plan(K, v, bc=ones, p_max=8, shard=(r, 2))
        assert b.stats()["geometry_shared"] == 2
        tot += a.execute(x)
        tot_nd += b.execute(x)
    assert np.array_equal(tot, whole) and np.array_equal(tot_nd, whole_nd)


# ---- a plan is built on the shared geometry, never copied from a live plan: what a derived plan owns is its own ----
# The mesh: two spheres of 2 048 + 512 panels -- at p_max = 8 four levels, 88 leaves, 2 913 M2L pairs, 83 M2M and 83 L2L operations:
# the smallest found on which every stage of the chain does work (unit_sphere(5) alone gives no L2L).  Every reference is an
# independent plan (FMMBEM_PLAN_SHARE=0), every comparison bit for bit.
def _independent(fb, make):
    keep = os.environ.get("FMMBEM_PLAN_SHARE")
    os.environ["FMMBEM_PLAN_SHARE"] = "0"
    try:
        return make()
    finally:
        if keep is None:
            del os.environ["FMMBEM_PLAN_SHARE"]
        else:
            os.environ["FMMBEM_PLAN_SHARE"] = keep


@pytest.fixture(scope="module")
def two(fb):
    v = np.concatenate([fb.unit_sphere(5), fb.unit_sphere(4, center=(2.5, 0.0, 0.3))])
    n = len(v)
    assert n == 2560
    d = {"v": v, "x": drand48(n, seed=11), "X": drand48(3 * n, seed=12).reshape(3, n),
         "bc": {"pot": None, "mixed": (np.arange(n) % 3 == 0).astype(np.uint8), "nd": np.ones(n, dtype=np.uint8)}, "ref": {}}

    def refs():
        for name, bc in d["bc"].items():
            p = fb.FMM_plan(fb.LaplaceSphericalBEM(8, 3), v, bc=bc, p_max=8)
            st = p.stats()
            assert st["geometry_shared"] == 1 and st["l2l_ops"] > 0 and st["m2m_ops"] > 0 and st["m2l_pairs"] > 0
            d["ref"][name] = (p.execute(d["x"]), p.execute_batch(d["X"]))
            p.close()
    _independent(fb, refs)
    for a in d["ref"].values():
        for b in a:
            b.setflags(write=False)
    return d


def test_a_derived_plan_starts_clean_and_owns_its_own_state(fb, two):
    """The base has a captured graph, recorded stage times, an order it last ran at and batch buffers; a plan made from it has
    none of these, gives the bits of an independent plan, and neither plan's end touches the other."""
    v, x, X, ref = two["v"], two["x"], two["X"], two["ref"]
    base = fb.FMM_plan(fb.LaplaceSphericalBEM(8, 3), v, p_max=8)
    base.set_graphs(True)
    for _ in range(3):                                  # launch by launch, captured, replayed
        assert np.array_equal(base.execute(x), ref["pot"][0])
    base.set_timing(True)                               # (timed executes go out launch by launch)
    for _ in range(3):
        assert np.array_equal(base.execute(x), ref["pot"][0])
    assert base.batch_width() > 1                       # the batch allocates its buffers
    assert np.array_equal(base.execute_batch(X), ref["pot"][1])
    st = base.stats()
    assert st["timed_executes"] > 0 and st["last_p"] == 8
    like = base.like(two["bc"]["mixed"])
    st = like.stats()
    assert st["timed_executes"] == 0 and st["last_p"] == 0 and st["geometry_shared"] == 2
    assert np.array_equal(like.execute(x), ref["mixed"][0])
    assert np.array_equal(like.execute_batch(X), ref["mixed"][1])
    assert np.array_equal(base.execute(x), ref["pot"][0])
    like.close()
    assert np.array_equal(base.execute(x), ref["pot"][0])
    assert np.array_equal(base.execute_batch(X), ref["pot"][1])
    second = base.like(two["bc"]["nd"])
    base.close()
    assert second.stats()["geometry_shared"] == 1
    assert np.array_equal(second.execute(x), ref["nd"][0])
    assert np.array_equal(second.execute_batch(X), ref["nd"][1])
    second.close()


@pytest.mark.parametrize("first", ["base", "like"])
def test_a_derived_plan_has_no_block_inverse_until_it_builds_its_own(fb, first):
    v = fb.unit_sphere(5)
    n = len(v)
    o = fb.FMMOptions()
    o.local_evaluation, o.lazy_evaluation, o.sparse_local, o.block_diagonal = False, False, True, True
    mixed = (np.arange(n) % 3 == 0).astype(np.uint8)
    w = drand48(n, seed=13)
    K = fb.LaplaceSphericalBEM(8, 3)

    def refs():
        out = []
        for bc in (None, mixed):
            p = fb.FMM_plan(K, v, o, bc=bc)
            p.block_inverse_build()
            out.append(p.block_inverse_apply(w))
            p.close()
        return out
    ref_base, ref_like = _independent(fb, refs)
    assert not np.array_equal(ref_base, ref_like)
    base = fb.FMM_plan(K, v, o)
    base.block_inverse_build()
    assert base.block_inverse_bytes() > 0
    like = base.like(mixed)
    assert like.stats()["geometry_shared"] == 2 and like.block_inverse_bytes() == 0
    with pytest.raises(fb.FmmBemError):
        like.block_inverse_apply(w)
    like.block_inverse_build()
    assert like.block_inverse_bytes() == base.block_inverse_bytes()
    assert np.array_equal(base.block_inverse_apply(w), ref_base) and np.array_equal(like.block_inverse_apply(w), ref_like)
    (base if first == "base" else like).close()
    if first == "base":
        assert np.array_equal(like.block_inverse_apply(w), ref_like)
        like.close()
    else:
        assert np.array_equal(base.block_inverse_apply(w), ref_base)
        base.close()


def test_the_cache_forgets_a_geometry_whose_plans_are_gone(fb, two):
    """A plan created after the only holder of its geometry was closed builds its own.  (A geometry that lives on in a derived
    plan after its first plan is closed is still recognised: `fourth` in the first test of this file.)  p_max = 9: a geometry
    no other test of this process holds."""
    v, x = two["v"], two["x"]
    make = lambda: fb.FMM_plan(fb.LaplaceSphericalBEM(8, 3), v, p_max=9)

    def ref():
        p = make()
        y = p.execute(x)
        p.close()
        return y
    y_ref = _independent(fb, ref)
    a = make()
    assert a.stats()["geometry_shared"] == 1
    a.close()
    b = make()
    assert b.stats()["geometry_shared"] == 1
    assert np.array_equal(b.execute(x), y_ref)
    c = make()                                          # ... and b's is recognised
    assert b.stats()["geometry_shared"] == 2
    assert np.array_equal(c.execute(x), y_ref)
    b.close()
    c.close()


def test_a_batch_leaves_the_plan_as_it_was(fb, two):
    """execute_batch runs vector j's far field on vector j's buffers; the plan's own are what a single execute uses afterwards."""
    v, x, X, ref = two["v"], two["x"], two["X"], two["ref"]
    p = fb.FMM_plan(fb.LaplaceSphericalBEM(8, 3), v, bc=two["bc"]["mixed"], p_max=8)
    assert p.batch_width() > 1
    before = p.execute(x)
    assert np.array_equal(before, ref["mixed"][0])
    assert np.array_equal(p.execute_batch(X), ref["mixed"][1])
    assert np.array_equal(p.execute(x), before)
    p.close()
