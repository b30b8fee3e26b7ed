"""Field plans (fmmbem_plan_create_field, FMM_plan.field_plan), host side: the host lists do not depend on the kernel, so a Stokes
field plan's trees, permutations and pair lists are a Laplace target plan's entry for entry; the Laplace field plan IS
fmmbem_plan_create_targets; the status codes of every refusal and argument error; the Python refusals.  No device needed."""
import ctypes

import numpy as np
import pytest

import field_plan_reference as R


@pytest.fixture(scope="module")
def sphere(fb):
    v = np.ascontiguousarray(fb.unit_sphere(4))
    v.setflags(write=False)
    return v


@pytest.fixture(scope="module")
def cloud(sphere):
    """about 600 points: shells, interior, near the surface, 20 copies of one point, points on panel centroids; mixed flags"""
    rng = np.random.default_rng(21)
    pts = np.ascontiguousarray(R.field_points(sphere, rng, 300, 120, 100, 60))
    flags = R.mixed_flags(rng, len(pts))
    assert len(pts) == 600
    return pts, flags


def options(fb, **kw):
    o = fb.Options()
    fb.lib().fmmbem_options_default(ctypes.byref(o))
    o.host_only = 1
    for k, val in kw.items():
        setattr(o, k, val)
    return o


def create_field(fb, o, v, pts, flags=None, out=True, n=None, m=None, keep=False):
    h = ctypes.c_void_p()
    vp = v.ctypes.data_as(ctypes.c_void_p) if v is not None else None
    tp = pts.ctypes.data_as(ctypes.c_void_p) if pts is not None else None
    fp = flags.ctypes.data_as(ctypes.c_void_p) if flags is not None else None
    rc = fb.lib().fmmbem_plan_create_field(ctypes.byref(o) if o is not None else None, (0 if v is None else len(v)) if n is None else n,
                                           vp, (0 if pts is None else len(pts)) if m is None else m, tp, fp,
                                           ctypes.byref(h) if out else None)
    if keep:
        return rc, h
    if rc == 0:
        fb.lib().fmmbem_plan_destroy(h)
    return rc


def host_opts(fb, ncrit=20, theta=0.5):
    opts = fb.FMMOptions()
    opts.set_max_per_box(ncrit)
    opts.set_mac_theta(theta)
    return opts


def assert_same_host_plan(a, b):
    """target_info, both box tables, both permutations, the p2p / m2l / m2m / l2l lists: entry for entry"""
    assert a.target_info() == b.target_info()
    for mine, theirs in ((a.boxes(), b.boxes()), (a.target_boxes(), b.target_boxes())):
        assert set(mine) == set(theirs)
        for k in mine:
            assert np.array_equal(mine[k], theirs[k]), k
    assert np.array_equal(a.perm(), b.perm())
    for x, y in zip(a.target_perm(), b.target_perm()):
        assert np.array_equal(x, y)
    for which in ("p2p", "m2l", "m2m", "l2l"):
        assert np.array_equal(a.pairs(which), b.pairs(which)), which


def test_stokes_field_plan_has_the_laplace_target_plans_lists(fb, sphere, cloud):
    pts, flags = cloud
    opts = host_opts(fb)
    stokes = fb.FMM_plan(R.stokes_kernel(fb), sphere, opts, host_only=True).field_plan(pts, flags)
    laplace = fb.FMM_plan(fb.LaplaceSphericalBEM(5, R.QUAD_K), sphere, opts, host_only=True, targets=pts, target_bc=flags)
    info = stokes.target_info()
    assert info["tree_coder_levels"] == 10
    assert info["n_targets"] == 600 and info["n_target_points"] == 600 - 20 + 2      # the copies: one body per flag
    assert stokes.stats()["m2l_pairs"] > 0
    assert_same_host_plan(stokes, laplace)
    assert stokes.dof == 3 and stokes.n_targets == 600 and stokes.batch_width() == 1
    assert stokes.stats()["n_panels"] == len(sphere) and stokes.stats()["owned_row_end"] == info["n_target_points"]


def test_laplace_field_plan_is_create_targets(fb, sphere, cloud):
    pts, flags = cloud
    opts = host_opts(fb)
    K = fb.LaplaceSphericalBEM(5, 3)
    field = fb.FMM_plan(K, sphere, opts, host_only=True).field_plan(pts, flags)
    targets = fb.FMM_plan(K, sphere, opts, host_only=True, targets=pts, target_bc=flags)
    assert field.target_info()["tree_coder_levels"] == 10
    assert_same_host_plan(field, targets)
    sa, sb = field.stats(), targets.stats()
    assert field.dof == 1 and all(sa[k] == sb[k] for k in sa if not k.startswith("build_"))
    # triangles stand for their centroids, as targets= takes them
    tri = R.point_panels(pts)
    a = fb.FMM_plan(K, sphere, opts, host_only=True).field_plan(tri, flags)
    b = fb.FMM_plan(K, sphere, opts, host_only=True, targets=tri, target_bc=flags)
    assert_same_host_plan(a, b)


@pytest.mark.parametrize("kernel", [0, 1])
def test_status_codes(fb, sphere, kernel):
    v = sphere
    pts = np.ascontiguousarray(np.random.default_rng(0).normal(size=(100, 3)))
    fl = (np.arange(100) % 2).astype(np.uint8)
    kw = dict(kernel=kernel)
    assert create_field(fb, options(fb, **kw), v, pts) == 0
    assert create_field(fb, options(fb, **kw), v, pts, fl) == 0
    # accepted without effect
    assert create_field(fb, options(fb, near_f32_max_p=8, stokes_batch_width=3, near_stream_fraction=0.5, **kw), v, pts, fl) == 0
    o = options(fb, n_devices=2, **kw)
    o.devices[0], o.devices[1] = 0, 1
    assert create_field(fb, o, v, pts) == 6                                     # a device list
    assert create_field(fb, options(fb, shard_world=2, **kw), v, pts) == 6
    assert create_field(fb, options(fb, sparse_local=0, **kw), v, pts) == 6     # matrix-free
    assert create_field(fb, options(fb, evaluator=1, **kw), v, pts) == 6        # LOCAL
    assert create_field(fb, options(fb, evaluator=2, **kw), v, pts) == 6        # BLOCK_DIAGONAL
    assert create_field(fb, options(fb, evaluator=4, **kw), v, pts) == 6        # TREECODE
    assert create_field(fb, options(fb, l2l_rule=1, **kw), v, pts) == 6         # REFERENCE
    assert create_field(fb, options(fb, kernel=7), v, pts) == 6                 # an unknown kernel id
    # argument errors
    assert create_field(fb, None, v, pts) == 1
    assert create_field(fb, options(fb, **kw), None, pts) == 1
    assert create_field(fb, options(fb, **kw), v, None) == 1
    assert create_field(fb, options(fb, **kw), v, pts, out=False) == 1
    assert create_field(fb, options(fb, **kw), v, pts, m=0) == 1
    assert create_field(fb, options(fb, **kw), v, pts, n=0) == 1
    assert create_field(fb, options(fb, **kw), v, pts, m=2 ** 31) == 1          # more than INT32_MAX bodies: refused before any read
    assert create_field(fb, options(fb, near_f32_max_p=17, **kw), v, pts) == 1
    assert create_field(fb, options(fb, stokes_batch_width=5, **kw), v, pts) == 1
    bad = pts.copy()
    bad[3, 1] = np.nan
    assert create_field(fb, options(fb, **kw), v, bad) == 1
    bad[3, 1] = np.inf
    assert create_field(fb, options(fb, **kw), v, bad) == 1
    if kernel == 1:
        assert create_field(fb, options(fb, kernel=1, mu=0.0), v, pts) == 1


def test_create_targets_still_refuses_stokes(fb, sphere):
    pts = np.ascontiguousarray(np.random.default_rng(0).normal(size=(100, 3)))
    h = ctypes.c_void_p()
    o = options(fb, kernel=1)
    rc = fb.lib().fmmbem_plan_create_targets(ctypes.byref(o), len(sphere), sphere.ctypes.data_as(ctypes.c_void_p), None, len(pts),
                                             pts.ctypes.data_as(ctypes.c_void_p), None, ctypes.byref(h))
    assert rc == 6 and not h.value
    with pytest.raises(fb.FmmBemError) as e:
        fb.FMM_plan(fb.StokesSphericalBEM(5, 3), sphere, host_only=True, targets=pts)
    assert e.value.status == 6


@pytest.mark.parametrize("kernel", [0, 1])
def test_whole_operator_calls_refused_handle_kept(fb, sphere, cloud, kernel):
    pts, flags = cloud
    rc, h = create_field(fb, options(fb, kernel=kernel, ncrit=20), sphere, pts, flags, keep=True)
    assert rc == 0
    L = fb.lib()
    n64 = ctypes.c_int64(0)
    assert L.fmmbem_plan_get_pairs(h, 1, None, ctypes.byref(n64)) == 0
    m2l_before = n64.value
    null, out, sz = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t(0)
    buf = np.zeros(12 * len(sphere) + 64)
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
    # a host-only field plan builds the lists and has no execute, as a host-only target plan
    assert L.fmmbem_plan_execute(h, 5, bp, bp) == 6
    assert L.fmmbem_plan_execute_batch(h, 5, 2, bp, 3 * len(sphere), bp, 3 * len(pts)) == 6
    assert L.fmmbem_plan_execute_device(h, 5, bp, bp, null) == 6
    # the handle is still usable, and reports what a target plan reports
    assert L.fmmbem_plan_get_pairs(h, 1, None, ctypes.byref(n64)) == 0 and n64.value == m2l_before
    info = fb._capi.TargetInfo()
    assert L.fmmbem_plan_target_info(h, ctypes.byref(info)) == 0
    assert info.n_panels == len(sphere) and info.n_targets == len(pts) and info.tree_coder_levels == 10
    st = fb._capi.Stats()
    assert L.fmmbem_plan_stats(h, ctypes.byref(st)) == 0
    assert st.n_panels == len(sphere) and st.owned_row_end == info.n_target_points
    w = ctypes.c_int(0)
    assert L.fmmbem_plan_batch_width(h, ctypes.byref(w)) == 0 and w.value == 1
    assert L.fmmbem_plan_set_timing(h, 1) == 0 and L.fmmbem_plan_set_graphs(h, 1) == 0
    L.fmmbem_plan_destroy(h)


def test_python_refusals(fb, sphere, cloud):
    pts, flags = cloud

    def refused(plan):
        with pytest.raises(fb.FmmBemError) as e:
            plan.field_plan(pts, flags)
        assert e.value.status == 6

    for K in (fb.LaplaceSphericalBEM(5, 3), R.stokes_kernel(fb)):
        ok = fb.FMM_plan(K, sphere, host_only=True)
        field = ok.field_plan(pts, flags)
        refused(field)                                                          # itself a target plan
        local, diag, matfree = fb.FMMOptions(), fb.FMMOptions(), fb.FMMOptions()
        local.lazy_evaluation, local.local_evaluation = False, True
        diag.lazy_evaluation, diag.block_diagonal = False, True
        matfree.sparse_local = False
        for opts in (local, diag, matfree):
            refused(fb.FMM_plan(K, sphere, opts, host_only=True))
        refused(fb.FMM_plan(K, sphere, host_only=True, shard=(0, 2)))           # a shard of an operator
        # a plan over a device list cannot be built without devices: a host-only plan whose options name one
        listed = fb.FMM_plan(K, sphere, host_only=True)
        listed._created_from[1].n_devices = 2
        listed._created_from[1].devices[1] = 1
        refused(listed)
        with pytest.raises(ValueError):
            ok.field_plan(pts, flags[:3])
        with pytest.raises(ValueError):
            ok.field_plan(pts[:, :2])
    tree = fb.FMMOptions()
    tree.evaluator = "TREECODE"
    refused(fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), sphere, tree, host_only=True))
    refused(fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), sphere, host_only=True, targets=pts))


def test_composed_reference_is_the_oracles_matvec(fb, oracle_mod, sphere):
    """the reference the GPU tests hold the VELOCITY rows to, on a single plan's geometry: centroid targets give the single plan's
    lists, and the five composed steps give StokesOracle.matvec to rounding"""
    v = np.array(sphere)
    x = np.random.default_rng(1).normal(size=(len(v), 3))
    probes = R.Probes(v, R.centroids(v), np.zeros(len(v), np.uint8))
    plan = fb.FMM_plan(R.stokes_kernel(fb, 6), v, host_opts(fb), host_only=True).field_plan(probes.centres)
    assert plan.target_info()["tree_coder_levels"] == 10 and plan.stats()["m2l_pairs"] == 1808
    ref = R.composed_reference(plan, probes, v, x, 6)
    so = oracle_mod.StokesOracle(v, K=R.QUAD_K, K_fine=R.QUAD_K_FINE, mu=R.MU, ncrit=20, complete_l2l=True)
    y = so.matvec(x, 6)
    probes.close()
    assert np.linalg.norm(ref - y) <= 1e-14 * np.linalg.norm(y)
    assert np.abs(ref - y).max() <= 1e-14 * np.abs(y).max()


def test_self_block_at_the_target_is_the_oracles_at_the_centroid(oracle_mod, sphere):
    """the helper's restatement of the reference's closed form: at a panel's own centroid it is the oracle's self entry to rounding;
    1e-9 beside the centroid (still inside the self window) it moves by about 1e-9 relative, which the oracle's entry does not"""
    v = np.array(sphere)
    k = np.arange(0, len(v), 7)
    on = R.Probes(v, R.centroids(v)[k], np.zeros(len(k), np.uint8))
    nrm = np.cross(v[k, 2] - v[k, 0], v[k, 1] - v[k, 0])
    inplane = np.cross(nrm, [0.3, 0.5, 0.7])
    inplane /= np.linalg.norm(inplane, axis=1)[:, None]
    off = R.Probes(v, R.centroids(v)[k] + 1e-9 * inplane, np.zeros(len(k), np.uint8))
    for a, j in enumerate(k):
        oracle_self = on.ctx.kernel_entries([on.n + a], [j])[0]
        scale = np.abs(oracle_self).max()
        mine = R.self_block_at(v[j, 0], v[j, 1], v[j, 2], on.panel_centres[j])
        assert np.abs(mine - oracle_self).max() <= 1e-14 * scale
        assert np.array_equal(off.ctx.kernel_entries([off.n + a], [j])[0], oracle_self)          # the oracle: the panel's centroid
        moved = off.entries([a], [j])[0, 0]
        assert 1e-11 * scale < np.abs(moved - oracle_self).max() < 1e-7 * scale
    on.close()
    off.close()
