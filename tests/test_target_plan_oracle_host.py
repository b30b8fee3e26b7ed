"""Plans over separate target points against the oracle's target plan (oracle.TargetOracle, oracle/targets.c), host side:
the oracle against itself (centroid targets give its single plan, one leaf gives its Direct sum, the error decays with p),
and the product's host lists -- both trees, the target permutation, the p2p / M2L / M2M / L2L pairs and the counts --
entry for entry against the oracle's independent derivation.  No device needed.

The target geometries are shared with tests/test_gpu_target_plan_oracle.py: points inside the surface and in shells within a
tenth of a panel size of it, points straddling the near-regime switch sqrt(2A)/dist = 0.5, points ON the surface (exact
centroids, 1e-9 off a centroid, vertices, edge midpoints, interior points of a panel), points far outside the panels' box,
coincident duplicates, a single target, one leaf of targets, targets with no near pair at all, and a cloud tight enough to
need the 21-level coder."""
import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

from oracle import oracle as O
from test_random_meshes import _soup


def centroids(v):
    return (v[:, 0] + v[:, 1] + v[:, 2]) / 3


def frame(v):
    """(centroid, unit normal, sqrt(2A)) per panel -- the normal of LaplaceSphericalBEM's Panel, (p2 - p0) x (p1 - p0)"""
    c = np.cross(v[:, 2] - v[:, 0], v[:, 1] - v[:, 0])
    a2 = np.linalg.norm(c, axis=1)
    return centroids(v), c / a2[:, None], np.sqrt(a2)


def near_points(v, rng, m):
    """m // 3 points inside (radius < 0.9 of a unit sphere's), m // 3 within +-0.1 panel sizes of a panel, the rest on the
    normal through a centroid at 2 sqrt(2A) (1 -+ 1e-7): just inside and just outside the switch of both kernels"""
    c, nrm, size = frame(v)
    k = rng.integers(0, len(v), m)
    d = rng.normal(size=(m // 3, 3))
    inside = d / np.linalg.norm(d, axis=1)[:, None] * 0.9 * rng.random((m // 3, 1))
    w = rng.random((m // 3, 3))
    w /= w.sum(axis=1)[:, None]
    ks = k[: m // 3]
    shell = (w[:, 0:1] * v[ks, 0] + w[:, 1:2] * v[ks, 1] + w[:, 2:3] * v[ks, 2]
             + ((rng.random(m // 3) - 0.5) * 0.2 * size[ks])[:, None] * nrm[ks])
    r = m - 2 * (m // 3)
    kk = k[m - r:]
    side = np.where(np.arange(r) % 2 == 0, 1 - 1e-7, 1 + 1e-7) * np.where(np.arange(r) % 4 < 2, 1.0, -1.0)
    switch = c[kk] + (2 * size[kk] * side)[:, None] * nrm[kk]
    return np.concatenate([inside, shell, switch])


def surface_points(v, rng, m):
    """points ON the surface: exact centroids (the dist < 1e-10 / 1e-8 self rules), centroids moved 1e-9 in the panel's plane
    (between the two), vertices, edge midpoints and interior barycentric points, m // 5 of each"""
    c, nrm, _ = frame(v)
    q = m // 5
    k = rng.choice(len(v), q, replace=False) if q <= len(v) else rng.integers(0, len(v), q)
    inplane = np.cross(nrm[k], [0.3, 0.5, 0.7])
    inplane /= np.linalg.norm(inplane, axis=1)[:, None]
    w = rng.random((q, 3)) + 0.05
    w /= w.sum(axis=1)[:, None]
    j = rng.integers(0, 3, q)
    return np.concatenate([c[k], c[k] + 1e-9 * inplane, v[k, j], (v[k, j] + v[k, (j + 1) % 3]) / 2,
                           w[:, 0:1] * v[k, 0] + w[:, 1:2] * v[k, 1] + w[:, 2:3] * v[k, 2]])


def unit_dirs(rng, m):
    d = rng.normal(size=(m, 3))
    return d / np.linalg.norm(d, axis=1)[:, None]


def flags_of(rng, m, mode):
    if mode == "g":
        return np.zeros(m, np.uint8)
    if mode == "dgdn":
        return np.ones(m, np.uint8)
    return (rng.random(m) < 0.5).astype(np.uint8)


def _shells(rec, mode, m):
    def make(rng):
        v = O.unit_sphere(rec)
        pts = near_points(v, rng, m)
        return v, pts, flags_of(rng, len(pts), mode)
    return make


def _surface(rng):
    v = O.unit_sphere(5)
    pts = np.concatenate([surface_points(v, rng, 1500), near_points(v, rng, 600)])
    fl = flags_of(rng, len(pts), "mixed")
    # coincident duplicates: copies with the same flag, and copies of the same points with the other flag
    k = rng.integers(0, len(pts), 300)
    pts = np.concatenate([pts, pts[k[:150]], pts[k[150:]]])
    fl = np.concatenate([fl, fl[k[:150]], 1 - fl[k[150:]]]).astype(np.uint8)
    return v, pts, fl


def _far_outside(rng):
    """the root cube set by the targets, the panels deep in one octant of it"""
    v = O.unit_sphere(5)
    pts = np.concatenate([20 + 30 * rng.random((1500, 3)), near_points(v, rng, 600)])
    return v, pts, flags_of(rng, len(pts), "mixed")


def _far_only(rng):
    """every target far from every panel: no near pair anywhere, every target row is far field only"""
    v = O.unit_sphere(4)
    pts = np.array([30.0, 30.0, 30.0]) + 2 * rng.normal(size=(800, 3))
    return v, pts, flags_of(rng, len(pts), "mixed")


def _single(rng):
    v = O.unit_sphere(4)
    c, nrm, size = frame(v)
    return v, (c[7] + 0.05 * size[7] * nrm[7])[None, :], np.array([1], np.uint8)


def _one_leaf(m):
    """m targets spread over the surface and no more than ncrit: the target tree is one leaf whose near block is every panel"""
    def make(rng):
        v = O.unit_sphere(6)
        pts = unit_dirs(rng, m) * (1 + 0.01 * (rng.random((m, 1)) - 0.5))
        return v, pts, flags_of(rng, m, "mixed")
    return make


def _tight(rng):
    """a cloud 1e-3 wide: the target tree alone needs more than the 10-level coder (15 levels)"""
    v = O.unit_sphere(4)
    pts = np.concatenate([np.array([0.3, -0.2, 0.95]) + 1e-3 * rng.random((200, 3)), near_points(v, rng, 300)])
    return v, pts, flags_of(rng, len(pts), "mixed")


def _ncrit1(rng):
    """one body per leaf (no pair of targets 1e-9 apart: a 21-level cell is 1e-6 wide here)"""
    v = O.unit_sphere(3)
    pts = np.concatenate([near_points(v, rng, 240)[:160], centroids(v)[::4]])     # inside and shell points
    return v, pts, flags_of(rng, len(pts), "mixed")


# name -> (builder(rng), quadrature K, theta, ncrit); every theta in {0.4, 0.5, 0.7}, ncrit in {1, 8, 64, 200} and K in
# {1, 3, 4, 7} is reached
CASES = {
    "shells_g": (_shells(5, "g", 3000), 3, 0.5, 64),
    "shells_dgdn": (_shells(5, "dgdn", 3000), 4, 0.4, 8),
    "shells_mixed_two_spheres": (None, 3, 0.5, 64),
    "surface_duplicates": (_surface, 7, 0.7, 200),
    "far_outside": (_far_outside, 1, 0.5, 64),
    "far_only": (_far_only, 3, 0.4, 64),
    "single": (_single, 4, 0.5, 8),
    "one_leaf_40": (_one_leaf(40), 3, 0.5, 64),
    "one_leaf_5": (_one_leaf(5), 1, 0.7, 8),
    "tight_cloud": (_tight, 3, 0.5, 8),
    "ncrit1": (_ncrit1, 7, 0.5, 1),
}


def _two_spheres(rng):
    v = np.concatenate([O.unit_sphere(6), O.unit_sphere(6, center=(3.0, 0.0, 0.0))])
    d = unit_dirs(rng, 12000)
    r = np.concatenate([1.01 + 1.99 * rng.random(6000), 0.9 * rng.random(3000), 5 + 20 * rng.random(3000)])
    centre = np.where(rng.random(12000) < 0.5, 0.0, 3.0)[:, None] * np.array([1.0, 0, 0])
    pts = np.concatenate([centre + d * r[:, None], near_points(v, rng, 6000)])
    return v, pts, flags_of(rng, len(pts), "mixed")


CASES["shells_mixed_two_spheres"] = (_two_spheres, 3, 0.5, 64)
HOST_CASES = [k for k in CASES if k != "shells_mixed_two_spheres"]     # the largest one runs on the GPU box only


def case(name, seed=0):
    make, K, theta, ncrit = CASES[name]
    v, pts, fl = make(np.random.default_rng(seed))
    return dict(v=np.ascontiguousarray(v), pts=np.ascontiguousarray(pts), flags=np.ascontiguousarray(fl, dtype=np.uint8),
                K=K, theta=theta, ncrit=ncrit)


def product_plan(fb, c, p=5, host_only=True, p_max=None):
    opts = fb.FMMOptions()
    opts.set_mac_theta(c["theta"])
    opts.set_max_per_box(c["ncrit"])
    K = fb.LaplaceSphericalBEM(p, c["K"])
    return fb.FMM_plan(K, c["v"], opts, host_only=host_only, p_max=p_max, targets=c["pts"], target_bc=c["flags"]), K


def oracle_plan(c):
    return O.TargetOracle(c["v"], c["pts"], c["flags"], K=c["K"], theta=c["theta"], ncrit=c["ncrit"])


def assert_lists_equal(tp, to):
    """the product's host lists against the oracle's, entry for entry"""
    tree, given = tp.target_perm()
    otree, ogiven = to.target_perm()
    assert np.array_equal(given, ogiven)
    assert np.array_equal(tree, otree)
    assert np.array_equal(tp.perm(), to.perm())
    for mine, theirs in ((tp.boxes(), to.boxes("source")), (tp.target_boxes(), to.boxes("target"))):
        for k in ("center", "side", "level", "leaf", "parent", "bb", "be"):
            assert np.array_equal(mine[k], theirs[k]), k
    for which in ("p2p", "m2l"):                       # walk order
        assert np.array_equal(tp.pairs(which), to.pairs(which)), which
    for which in ("m2m", "l2l"):
        a, b = tp.pairs(which), to.pairs(which)
        assert len(a) == len(b) and set(map(tuple, a.tolist())) == set(map(tuple, b.tolist())), which
    info, oi = tp.target_info(), to.info()
    for k in info:
        assert info[k] == oi[k], (k, info[k], oi[k])
    st = tp.stats()
    assert (st["m2l_pairs"], st["m2m_ops"], st["l2l_ops"]) == (oi["m2l_pairs"], oi["m2m_ops"], oi["l2l_ops"])


@pytest.mark.parametrize("name", HOST_CASES)
def test_host_lists_equal_target_oracle(fb, oracle_mod, name):
    c = case(name)
    tp, _ = product_plan(fb, c)
    to = oracle_plan(c)
    assert_lists_equal(tp, to)
    info = to.info()
    if name == "far_only":
        assert info["p2p_pairs"] == 0 and info["m2l_pairs"] > 0
    if name == "tight_cloud":
        assert info["tree_coder_levels"] == 21
        assert O.TargetOracle(c["v"], c["pts"][200:], c["flags"][200:], ncrit=c["ncrit"]).info()["tree_coder_levels"] == 10
    if name.startswith("one_leaf"):
        assert info["n_target_leaves"] == 1 and info["m2l_pairs"] == 0
    if name == "surface_duplicates":
        assert info["n_target_points"] < len(c["pts"]) - 150


@settings(max_examples=25, deadline=None, suppress_health_check=[HealthCheck.function_scoped_fixture])
@given(seed=st.integers(0, 2 ** 31 - 1), n=st.integers(2, 900), clusters=st.integers(1, 6),
       stretch=st.sampled_from([1.0, 3.0, 10.0]), size_spread=st.sampled_from([0.0, 1.0, 2.0]), m=st.integers(1, 1500),
       cloud=st.sampled_from(["box", "clusters", "far", "duplicates"]), theta=st.sampled_from([0.4, 0.5, 0.7]),
       ncrit=st.sampled_from([1, 8, 64]))
def test_host_lists_equal_target_oracle_random(fb, oracle_mod, seed, n, clusters, stretch, size_spread, m, cloud, theta, ncrit):
    v = _soup(seed, n, clusters, stretch, size_spread)
    rng = np.random.default_rng(seed + 3)
    c = centroids(v)
    lo, hi = c.min(axis=0), c.max(axis=0)
    if cloud == "box":
        pts = lo + (hi - lo) * rng.random((m, 3))
    elif cloud == "clusters":
        pts = c[rng.integers(0, n, m)] + rng.normal(0, 0.05, (m, 3))
    elif cloud == "far":
        pts = hi + 10 * (1 + rng.random((m, 3)))
    else:
        base = c[rng.integers(0, n, max(1, m // 10))]
        pts = base[rng.integers(0, len(base), m)]
    fl = (rng.random(m) < 0.5).astype(np.uint8)
    cs = dict(v=v, pts=np.ascontiguousarray(pts), flags=fl, K=3, theta=theta, ncrit=ncrit)
    try:
        tp, _ = product_plan(fb, cs)
    except fb.FmmBemError as e:                        # deeper than the 21-level coder resolves
        assert e.status == 5
        return
    assert_lists_equal(tp, oracle_plan(cs))


# ---- the oracle against itself ----

@pytest.mark.parametrize("flag", [0, 1])
def test_oracle_centroid_targets_give_its_single_plan(oracle_mod, flag):
    # targets at the centroids with the panels' flag: the same tree twice, the same lists, every source in the one live slot
    # (the single plan's P2M puts a panel in the slot of its own flag) -- the single oracle with the complete L2L rule
    v = O.unit_sphere(5)
    bc = np.full(len(v), flag, np.uint8)
    x = np.random.default_rng(1).standard_normal(len(v))
    to = O.TargetOracle(v, centroids(v), bc, ncrit=32)
    so = O.Oracle(v, bc=bc, ncrit=32, complete_l2l=True)
    assert np.array_equal(to.pairs("m2l"), so.pairs("m2l")) and np.array_equal(to.pairs("p2p"), so.pairs("p2p"))
    for p in (1, 4, 12, 16):
        a, b = to.matvec(x, p), so.matvec(x, p)
        assert np.linalg.norm(a - b) <= 1e-13 * np.linalg.norm(b), p
    d = to.direct(x)
    assert np.linalg.norm(d - so.direct(x)) <= 1e-13 * np.linalg.norm(d)


def test_oracle_one_leaf_is_its_direct_sum(oracle_mod):
    c = case("surface_duplicates")
    to = O.TargetOracle(c["v"], c["pts"], c["flags"], K=c["K"], ncrit=len(c["v"]) + len(c["pts"]))
    info = to.info()
    assert info["m2l_pairs"] == 0 and info["p2p_pairs"] == 1
    x = np.random.default_rng(2).standard_normal(len(c["v"]))
    d = to.direct(x)
    assert np.all(np.isfinite(d))
    assert np.linalg.norm(to.matvec(x, 5) - d) <= 1e-13 * np.linalg.norm(d)


def test_oracle_error_decays_with_p(oracle_mod):
    c = case("far_outside")
    to = oracle_plan(c)
    x = np.random.default_rng(3).standard_normal(len(c["v"]))
    d = to.direct(x)
    for f in (0, 1):
        s = c["flags"] == f
        err = [np.linalg.norm(to.matvec(x, p)[s] - d[s]) / np.linalg.norm(d[s]) for p in (2, 6, 12)]
        assert err[0] > 10 * err[1] > 100 * err[2], (f, err)


def test_oracle_duplicates_and_order(oracle_mod):
    # duplicates are copies of their first occurrence; the same point with the other flag is a body of its own
    v = O.unit_sphere(4)
    rng = np.random.default_rng(4)
    base = rng.normal(size=(30, 3)) * 1.2
    idx = rng.integers(0, 30, 400)
    fl = (idx % 3 == 0).astype(np.uint8)
    to = O.TargetOracle(v, base[idx], fl)
    tree, given = to.target_perm()
    pts, pfl = to.target_points()
    assert np.array_equal(pts[given], base[idx]) and np.array_equal(pfl[given], fl)
    first = sorted({(int(i), int(f)): k for k, (i, f) in reversed(list(enumerate(zip(idx, fl))))}.values())
    assert np.array_equal(pts, base[idx[first]])             # distinct targets in first-occurrence order
    assert sorted(tree.tolist()) == list(range(len(pts)))
    x = rng.standard_normal(len(v))
    ref = O.TargetOracle(v, pts, pfl).direct(x)
    assert np.array_equal(to.direct(x), ref[given])
