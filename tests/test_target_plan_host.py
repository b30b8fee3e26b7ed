"""Plans over separate target points (fmmbem_plan_create_targets), host side: the two trees on one lattice, the dual
traversal's lists, coverage of every (target, source) pair, and the status codes.  No device needed."""
import ctypes

import numpy as np
import pytest

from test_random_meshes import _soup


def centroids(v):
    return (v[:, 0] + v[:, 1] + v[:, 2]) / 3


def target_plan(fb, v, targets, target_bc=None, opts=None, K=None):
    K = K if K is not None else fb.LaplaceSphericalBEM(5, 3)
    return fb.FMM_plan(K, v, opts, host_only=True, targets=targets, target_bc=target_bc)


def assert_same_lists(fb, v, opts=None):
    K = fb.LaplaceSphericalBEM(5, 3)
    single = fb.FMM_plan(K, v, opts, host_only=True)
    tp = target_plan(fb, v, centroids(v), opts=opts)
    for which in ("p2p", "m2l", "m2m", "l2l"):
        assert np.array_equal(single.pairs(which), tp.pairs(which)), which
    bs, bt = single.boxes(), tp.target_boxes()
    for k in bs:
        assert np.array_equal(bs[k], bt[k]), k
        assert np.array_equal(bs[k], tp.boxes()[k]), k
    assert np.array_equal(tp.target_perm()[0], single.perm())
    assert np.array_equal(tp.perm(), single.perm())
    s, t = single.stats(), tp.stats()
    for k in ("n_boxes", "n_leaves", "n_levels", "near_nnz_total", "m2l_classes", "tree_coder_levels"):
        assert s[k] == t[k], k


@pytest.mark.parametrize("r", [4, 5, 6])
def test_centroid_targets_give_the_single_plans_lists_sphere(fb, r):
    assert_same_lists(fb, fb.unit_sphere(r))


@pytest.mark.parametrize("seed,n,clusters,stretch,spread,ncrit,theta", [
    (1, 900, 3, 3.0, 1.0, 32, 0.5), (2, 400, 1, 1.0, 0.0, 8, 0.4), (3, 700, 6, 10.0, 2.0, 64, 0.7),
    (4, 50, 2, 1.0, 2.0, 126, 0.5), (5, 850, 4, 3.0, 0.0, 16, 0.5)])
def test_centroid_targets_give_the_single_plans_lists_random(fb, seed, n, clusters, stretch, spread, ncrit, theta):
    v = _soup(seed, n, clusters, stretch, spread)
    opts = fb.FMMOptions()
    opts.set_mac_theta(theta)
    opts.set_max_per_box(ncrit)
    assert_same_lists(fb, v, opts)


def covered_sources(tp, n_src):
    """per target-tree leaf: the source panels (source-tree positions) its lists reach, with multiplicity"""
    sb, tb = tp.boxes(), tp.target_boxes()
    anc = {}
    for b in range(len(tb["leaf"])):
        chain, a = [b], b
        while a != 0:
            a = int(tb["parent"][a])
            chain.append(a)
        anc[b] = set(chain)
    near, far = {}, {}
    for s, t in tp.pairs("p2p"):
        near.setdefault(int(t), []).append(int(s))
    for s, t in tp.pairs("m2l"):
        far.setdefault(int(t), []).append(int(s))
    out = {}
    for b in np.nonzero(tb["leaf"])[0]:
        cols = [np.arange(sb["bb"][s], sb["be"][s]) for s in near.get(int(b), [])]
        for a in anc[int(b)]:
            cols += [np.arange(sb["bb"][s], sb["be"][s]) for s in far.get(a, [])]
        out[int(b)] = np.sort(np.concatenate(cols)) if cols else np.zeros(0, dtype=np.int64)
    return out


@pytest.mark.parametrize("theta", [0.5, 0.7])
def test_every_pair_covered_exactly_once(fb, theta):
    v = fb.unit_sphere(5)
    rng = np.random.default_rng(7)
    d = rng.normal(size=(600, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    pts = np.concatenate([d[:200] * 0.9 * rng.random((200, 1)),          # inside the surface
                          d[200:400] * (1 + 0.2 * rng.random((200, 1))),   # near it
                          d[400:] * 50,                                     # far outside the panels' box
                          np.tile([[0.3, -0.2, 0.1]], (1000, 1))])         # 1 000 copies of one point
    flags = (np.arange(len(pts)) % 2).astype(np.uint8)
    opts = fb.FMMOptions()
    opts.set_mac_theta(theta)
    tp = target_plan(fb, v, pts, flags, opts)
    info = tp.target_info()
    assert info["n_targets"] == len(pts) and info["n_target_points"] == 600 + 2      # the copies: one per flag
    tree, given = tp.target_perm()
    assert sorted(tree.tolist()) == list(range(info["n_target_points"]))
    assert len(set(given[600:].tolist())) == 2
    for b, cols in covered_sources(tp, len(v)).items():
        assert np.array_equal(cols, np.arange(len(v))), b
    # every M2L pair is well separated (DefaultMAC, radius = side / 2)
    sb, tb = tp.boxes(), tp.target_boxes()
    m2l = tp.pairs("m2l")
    assert len(m2l) > 0
    dist = np.linalg.norm(sb["center"][m2l[:, 0]] - tb["center"][m2l[:, 1]], axis=1)
    assert np.all(dist > (sb["side"][m2l[:, 0]] / 2 + tb["side"][m2l[:, 1]] / 2) / theta)
    # both trees sit on one lattice: the same root cube
    assert np.array_equal(sb["center"][0], tb["center"][0]) and sb["side"][0] == tb["side"][0]
    # the downward pass runs on the target tree, the upward one on the source tree
    l2l, m2m = tp.pairs("l2l"), tp.pairs("m2m")
    assert len(m2m) > 0 and m2m.max() < info["n_source_boxes"]
    assert l2l.size == 0 or l2l.max() < info["n_target_boxes"]


def test_many_coincident_targets_build(fb):
    v = fb.unit_sphere(3)
    pts = np.tile([[0.25, 0.5, -0.125]], (5000, 1))
    tp = target_plan(fb, v, pts)
    info = tp.target_info()
    assert info["n_target_points"] == 1 and info["n_target_leaves"] == 1 and info["tree_coder_levels"] == 10


def options(fb, **kw):
    o = fb.Options()
    fb.lib().fmmbem_options_default(ctypes.byref(o))
    o.host_only = 1
    for k, val in kw.items():
        setattr(o, k, val)
    return o


def create(fb, o, v, pts, out=True):
    h = ctypes.c_void_p()
    vp = v.ctypes.data_as(ctypes.c_void_p) if v is not None else None
    tp = pts.ctypes.data_as(ctypes.c_void_p) if pts is not None else None
    rc = fb.lib().fmmbem_plan_create_targets(ctypes.byref(o) if o is not None else None, 0 if v is None else len(v), vp, None,
                                             0 if pts is None else len(pts), tp, None, ctypes.byref(h) if out else None)
    if rc == 0:
        fb.lib().fmmbem_plan_destroy(h)
    return rc


def test_status_codes(fb):
    v = np.ascontiguousarray(fb.unit_sphere(3))
    pts = np.ascontiguousarray(np.random.default_rng(0).normal(size=(100, 3)))
    assert create(fb, options(fb), v, pts) == 0
    assert create(fb, options(fb, kernel=1), v, pts) == 6                       # Stokes
    o = options(fb, n_devices=2)
    o.devices[0], o.devices[1] = 0, 1
    assert create(fb, o, v, pts) == 6                                           # a device list
    assert create(fb, options(fb, shard_world=2), v, pts) == 6
    assert create(fb, options(fb, sparse_local=0), v, pts) == 6
    assert create(fb, options(fb, evaluator=1), v, pts) == 6                    # LOCAL
    assert create(fb, options(fb, evaluator=2), v, pts) == 6                    # BLOCK_DIAGONAL
    assert create(fb, options(fb, l2l_rule=1), v, pts) == 6                     # REFERENCE
    assert create(fb, None, v, pts) == 1
    assert create(fb, options(fb), None, pts) == 1
    assert create(fb, options(fb), v, None) == 1
    assert create(fb, options(fb), v, pts, out=False) == 1
    bad = pts.copy()
    bad[3, 1] = np.nan
    assert create(fb, options(fb), v, bad) == 1
    with pytest.raises(fb.FmmBemError) as e:
        target_plan(fb, v, pts, K=fb.StokesSphericalBEM(5, 3))
    assert e.value.status == 6
    with pytest.raises(ValueError):
        target_plan(fb, v, pts, target_bc=np.zeros(3, np.uint8))


def test_single_plan_calls_refused_handle_kept(fb):
    v = fb.unit_sphere(4)
    pts = np.random.default_rng(1).normal(size=(300, 3)) * 2
    tp = target_plan(fb, v, pts)
    before = tp.pairs("m2l").copy()
    L, h = fb.lib(), tp._h
    null = ctypes.c_void_p()
    out = ctypes.c_void_p()
    n64 = ctypes.c_int64(0)
    sz = ctypes.c_size_t(0)
    buf = np.zeros(4 * len(v) + 64)
    bp = buf.ctypes.data_as(ctypes.c_void_p)
    so = fb._capi.SolverOpts()
    L.fmmbem_solver_options_default(ctypes.byref(so))
    calls = [
        lambda: L.fmmbem_plan_create_like(h, None, ctypes.byref(out)),
        lambda: L.fmmbem_plan_exchange_doubles(h, 5, ctypes.byref(sz)),
        lambda: L.fmmbem_plan_exchange_counts(h, 5, bp, bp),
        lambda: L.fmmbem_plan_upward_device(h, 5, bp, bp, null),
        lambda: L.fmmbem_plan_downward_device(h, 5, bp, bp, null),
        lambda: L.fmmbem_plan_near_split_device(h, bp, null),
        lambda: L.fmmbem_plan_shard_rows(h, bp),
        lambda: L.fmmbem_plan_set_result_slices(h, 1),
        lambda: L.fmmbem_plan_assemble_slices_device(h, bp, 1, bp, null),
        lambda: L.fmmbem_plan_get_near_row(h, 0, None, None, ctypes.byref(n64)),
        lambda: L.fmmbem_plan_get_diagonal(h, bp),
        lambda: L.fmmbem_plan_get_expansions(h, 0, 5, bp),
        lambda: L.fmmbem_gmres(h, ctypes.byref(so), bp, bp, None, None),
    ]
    for i, call in enumerate(calls):
        assert call() == 6, i
        assert "separate targets" in L.fmmbem_last_error().decode(), i
    # a host-only target plan has no execute
    with pytest.raises(fb.FmmBemError) as e:
        tp.execute(np.ones(len(v)))
    assert e.value.status == 6
    # the handle is still usable
    assert np.array_equal(tp.pairs("m2l"), before)
    st = tp.stats()
    assert st["n_panels"] == len(v) and st["owned_row_end"] == 300
    assert tp.target_info()["n_targets"] == 300
    # the target-plan calls on a single plan
    single = fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), v, host_only=True)
    info = fb._capi.TargetInfo()
    assert L.fmmbem_plan_target_info(single._h, ctypes.byref(info)) == 1
    assert L.fmmbem_plan_get_target_perm(single._h, None, None) == 1
