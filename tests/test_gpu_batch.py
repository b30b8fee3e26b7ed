"""Batched execute (fmmbem_plan_execute_batch(_device), FMM_plan.execute_batch / execute_batch_torch) on the GPU: every result
vector of a batch is bit for bit (np.array_equal) the single execute of that vector at the same p, on every kind of plan --
the fast path (one near-field pass for several vectors) and the plans that run a batch vector by vector."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PS = (1, 2, 5, 8, 10, 12, 16)
KS = (1, 2, 3, 4, 7, 8, 9)
SENTINEL = -12345.678


def two_spheres(fb, rec):
    return np.concatenate([fb.unit_sphere(rec), fb.unit_sphere(rec, center=(3.0, 0.0, 0.0))])


def _out_len(plan):
    return plan.n * plan.dof if plan.n_targets is None else plan.n_targets


def singles(plan, X, p):
    """the single device execute of every row of X (numpy (k, n * dof)) at order p -> numpy (k, m)"""
    import torch
    xd = torch.from_numpy(np.ascontiguousarray(X)).to("cuda:%d" % plan.device)
    out = [plan.execute_torch(xd[j].contiguous(), p=p) for j in range(X.shape[0])]
    torch.cuda.synchronize()
    return np.stack([o.cpu().numpy() for o in out])


def batch(plan, X, p, gx=5, gy=3):
    """the device batch with leading dimensions n + gx and m + gy, the gaps holding a sentinel that must survive"""
    import torch
    k, nx = X.shape
    ny = _out_len(plan)
    dev = "cuda:%d" % plan.device
    xb = torch.full((k, nx + gx), SENTINEL, dtype=torch.float64, device=dev)
    xb[:, :nx] = torch.from_numpy(np.ascontiguousarray(X)).to(dev)
    yb = torch.full((k, ny + gy), SENTINEL, dtype=torch.float64, device=dev)
    plan.execute_batch_device(k, xb.data_ptr(), nx + gx, yb.data_ptr(), ny + gy,
                              torch.cuda.current_stream(dev).cuda_stream, p)
    torch.cuda.synchronize()
    y = yb.cpu().numpy()
    assert (y[:, ny:] == SENTINEL).all(), "a gap between result vectors was written"
    assert (xb[:, nx:] == SENTINEL).all().item()
    return y[:, :ny]


def charges(n, k, seed=0):
    return np.random.default_rng(seed).random((k, n)) - 0.3


def assert_batches(plan, X, ps=PS, ks=KS):
    for p in ps:
        ref = singles(plan, X[:max(ks)], p)
        for k in ks:
            got = batch(plan, X[:k], p)
            for j in range(k):
                assert np.array_equal(got[j], ref[j]), (p, k, j, float(np.abs(got[j] - ref[j]).max()))


@pytest.mark.parametrize("rec", [6, 7])
@pytest.mark.parametrize("flags", ["potential", "normal_deriv", "mixed"])
def test_fast_path_every_order_and_batch_size(fb, rec, flags):
    v = two_spheres(fb, rec)
    n = len(v)
    bc = {"potential": np.zeros(n, np.uint8), "normal_deriv": np.ones(n, np.uint8),
          "mixed": (np.arange(n) % 3 == 0).astype(np.uint8)}[flags]
    plan = fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), v, bc=bc, p_max=16)
    assert plan.batch_width() > 1
    assert_batches(plan, charges(n, max(KS), seed=rec))


def test_host_form_and_numpy_shapes(fb):
    v = two_spheres(fb, 6)
    K = fb.LaplaceSphericalBEM(10, 3)
    plan = fb.FMM_plan(K, v)
    X = charges(len(v), 7, seed=1)
    got = plan.execute_batch(X)
    assert got.shape == X.shape
    for j in range(7):
        assert np.array_equal(got[j], plan.execute(X[j]))


def test_create_like_plan(fb):
    v = two_spheres(fb, 6)
    n = len(v)
    base = fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), v, p_max=16)
    X = charges(n, 9, seed=2)
    base.execute_batch(X[:3])                         # the base plan's batch buffers exist before the like plan is made
    like = base.like((np.arange(n) % 2).astype(np.uint8))
    assert like.batch_width() > 1
    assert_batches(like, X, ps=(2, 8, 10, 16), ks=(1, 3, 4, 9))
    assert_batches(base, X, ps=(5,), ks=(2, 9))


def test_target_plan_with_coincident_targets(fb):
    v = two_spheres(fb, 6)
    g = np.linspace(-1.5, 4.5, 11)
    pts = np.stack(np.meshgrid(g, g[:7] - 1.0, g[:5] - 0.5, indexing="ij"), axis=-1).reshape(-1, 3)
    pts = np.concatenate([pts, pts[::7], v[:50].mean(axis=1)])         # repeated grid points, points on the surface
    flags = (np.arange(len(pts)) % 4 == 1).astype(np.uint8)
    plan = fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), v, p_max=16, targets=pts, target_bc=flags)
    assert plan.batch_width() > 1
    assert_batches(plan, charges(len(v), 9, seed=3), ps=(1, 2, 8, 10, 16), ks=(1, 2, 3, 8, 9))


@pytest.mark.parametrize("evaluator", ["local", "block_diagonal"])
def test_local_and_block_diagonal(fb, evaluator):
    v = two_spheres(fb, 6)
    o = fb.FMMOptions()
    o.lazy_evaluation = False
    o.local_evaluation = evaluator == "local"
    o.block_diagonal = evaluator == "block_diagonal"
    plan = fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), v, o, p_max=12)
    assert plan.batch_width() > 1
    assert_batches(plan, charges(len(v), 9, seed=4), ps=(2, 10), ks=(1, 3, 9))


@pytest.mark.parametrize("traction", [False, True])
def test_stokes_runs_vector_by_vector(fb, traction):
    v = two_spheres(fb, 5)
    n = len(v)
    bc = np.ones(n, np.uint8) if traction else None
    plan = fb.FMM_plan(fb.StokesSphericalBEM(6, 3, 1e-3), v, bc=bc, p_max=8)
    assert plan.batch_width() == 1
    X = np.random.default_rng(5).random((3, n, 3))
    got = plan.execute_batch(X)
    assert got.shape == (3, n, 3)
    for j in range(3):
        assert np.array_equal(got[j], plan.execute(X[j]))
    assert_batches(plan, X.reshape(3, 3 * n), ps=(3, 8), ks=(1, 3))


def test_hybrid_width_follows_what_the_plan_built(fb):
    v = two_spheres(fb, 6)
    o = fb.FMMOptions()
    o.near_stream_fraction = 0.5
    plan = fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), v, o, p_max=12)
    hybrid = plan.stats()["near_recomputed_pairs"] > 0
    assert (plan.batch_width() == 1) == hybrid
    assert_batches(plan, charges(len(v), 4, seed=6), ps=(2, 10), ks=(1, 4))


def test_matrix_free_runs_vector_by_vector(fb):
    v = two_spheres(fb, 6)
    o = fb.FMMOptions()
    o.sparse_local = False
    plan = fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), v, o, p_max=12)
    assert plan.batch_width() == 1
    assert_batches(plan, charges(len(v), 3, seed=7), ps=(2, 10), ks=(1, 3))


def test_device_list_runs_vector_by_vector(fb):
    v = two_spheres(fb, 6)
    plan = fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), v, p_max=10, devices=[0, 0])
    assert plan.batch_width() == 1
    assert_batches(plan, charges(len(v), 3, seed=8), ps=(2, 10), ks=(1, 3))
    X = charges(len(v), 3, seed=9)
    got = plan.execute_batch(X)
    for j in range(3):
        assert np.array_equal(got[j], plan.execute(X[j]))


def test_graphs_on_plan(fb):
    v = two_spheres(fb, 6)
    K = fb.LaplaceSphericalBEM(10, 3)
    plan = fb.FMM_plan(K, v, p_max=12)
    plan.set_graphs(True)
    X = charges(len(v), 5, seed=10)
    for _ in range(3):                                # singles captured and replayed as graphs
        ref = singles(plan, X, 10)
    assert plan.batch_width() > 1
    assert_batches(plan, X, ps=(10, 4), ks=(1, 5))
    assert np.array_equal(singles(plan, X, 10), ref)


def test_state_between_single_and_batch(fb):
    v = two_spheres(fb, 6)
    K = fb.LaplaceSphericalBEM(10, 3)
    plan = fb.FMM_plan(K, v, bc=(np.arange(len(v)) % 5 == 0).astype(np.uint8), p_max=12)
    X = charges(len(v), 6, seed=11)
    before = plan.execute(X[0])
    b10 = batch(plan, X, 10)
    after = plan.execute(X[0])
    assert np.array_equal(before, after)
    b3 = batch(plan, X, 3)
    assert all(np.array_equal(b10[j], r) for j, r in enumerate(singles(plan, X, 10)))
    assert all(np.array_equal(b3[j], r) for j, r in enumerate(singles(plan, X, 3)))


def test_torch_form_on_a_side_stream(fb):
    import torch
    v = two_spheres(fb, 6)
    K = fb.LaplaceSphericalBEM(8, 3)
    plan = fb.FMM_plan(K, v)
    X = charges(len(v), 4, seed=12)
    ref = plan.execute_batch(X)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        xd = torch.from_numpy(X).cuda()
        out = plan.execute_batch_torch(xd)
        got = out.cpu().numpy()
    assert np.array_equal(got, ref)
    with pytest.raises(ValueError):
        plan.execute_batch_torch(xd[:, :-1].contiguous())
    with pytest.raises(ValueError):
        plan.execute_batch_torch(xd.float())


def test_full_size_two_spheres(fb):
    """2 x UnitSphere(9), N = 1 048 576, p = 10, k = 4: all 4 x N results bit-equal to four single executes."""
    v = two_spheres(fb, 9)
    plan = fb.FMM_plan(fb.LaplaceSphericalBEM(10, 3), v)
    assert plan.batch_width() > 1
    X = charges(len(v), 4, seed=13)
    got = batch(plan, X, 10)
    ref = singles(plan, X, 10)
    for j in range(4):
        assert np.array_equal(got[j], ref[j]), j
