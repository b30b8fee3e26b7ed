"""The multi-vector near field of Stokes plans (fmmbem_options.stokes_batch_width, near_spmv_sym3_multi) on the GPU: with the
option a Stokes plan reports the width it was asked for, and every result vector of a batch -- any batch size, either execute_batch
form, any leading dimension -- is bit for bit (np.array_equal) the single execute of that vector, on the plan itself and on a plan
built without the option.  Plans on which the option is not active keep width 1 and batch as before."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

WIDTHS = (2, 3, 4)
PS = (3, 8)
KS = (1, 2, 3, 4, 5, 7)
SENTINEL = -12345.678


def two_spheres(fb, rec):
    return np.concatenate([fb.unit_sphere(rec), fb.unit_sphere(rec, center=(3.0, 0.0, 0.0))])


def stokes(p=6):
    import fmm_bem_relaxed_amd as fb
    return fb.StokesSphericalBEM(p, 3, 1e-3)


def flags_of(kind, n):
    return {"velocity": None, "traction": np.ones(n, np.uint8), "mixed": (np.arange(n) % 3 == 0).astype(np.uint8)}[kind]


def charges(n, k, seed=0):
    return np.random.default_rng(seed).random((k, 3 * n)) - 0.3


def singles(plan, X, p):
    """the single device execute of every row of X (numpy (k, 3 n)) at order p -> numpy (k, 3 n)"""
    import torch
    xd = torch.from_numpy(np.ascontiguousarray(X)).to("cuda:%d" % plan.device)
    out = [plan.execute_torch(xd[j].contiguous(), p=p) for j in range(X.shape[0])]
    torch.cuda.synchronize()
    return np.stack([o.cpu().numpy() for o in out])


def batch(plan, X, p, gx=5, gy=3):
    """the device batch with leading dimensions 3 n + gx and 3 n + gy, the gaps holding a sentinel that must survive"""
    import torch
    k, nx = X.shape
    dev = "cuda:%d" % plan.device
    xb = torch.full((k, nx + gx), SENTINEL, dtype=torch.float64, device=dev)
    xb[:, :nx] = torch.from_numpy(np.ascontiguousarray(X)).to(dev)
    yb = torch.full((k, nx + gy), SENTINEL, dtype=torch.float64, device=dev)
    plan.execute_batch_device(k, xb.data_ptr(), nx + gx, yb.data_ptr(), nx + gy, torch.cuda.current_stream(dev).cuda_stream, p)
    torch.cuda.synchronize()
    y = yb.cpu().numpy()
    assert (y[:, nx:] == SENTINEL).all(), "a gap between result vectors was written"
    assert (xb[:, nx:] == SENTINEL).all().item()
    return y[:, :nx]


def host_batch(plan, X, p, gx=2, gy=7):
    """the host form (fmmbem_plan_execute_batch) with leading dimensions larger than the vector and sentinels in the gaps"""
    import ctypes as C
    from fmm_bem_relaxed_amd import _capi
    k, nx = X.shape
    xb = np.full((k, nx + gx), SENTINEL)
    xb[:, :nx] = X
    yb = np.full((k, nx + gy), SENTINEL)
    _capi.check(_capi.lib().fmmbem_plan_execute_batch(plan._h, p, k, xb.ctypes.data_as(C.c_void_p), nx + gx,
                                                      yb.ctypes.data_as(C.c_void_p), nx + gy))
    assert (yb[:, nx:] == SENTINEL).all() and (xb[:, nx:] == SENTINEL).all()
    return yb[:, :nx]


def assert_batches(plan, X, ps=PS, ks=KS, ref=None, host_ks=None):
    """every batch size at every order, device and host form, against the plan's own singles and -- ref[p], when given -- the
    singles of a plan built without the option"""
    host_ks = ks if host_ks is None else host_ks       # the host form over the same batch sizes as the device form
    for p in ps:
        own = singles(plan, X[:max(ks)], p)
        if ref is not None:
            assert np.array_equal(own, ref[p][:max(ks)]), ("single executes differ from the plan without the option", p)
        for k in ks:
            got = batch(plan, X[:k], p)
            for j in range(k):
                assert np.array_equal(got[j], own[j]), (p, k, j, float(np.abs(got[j] - own[j]).max()))
        for k in host_ks:
            got = host_batch(plan, X[:k], p)
            for j in range(k):
                assert np.array_equal(got[j], own[j]), ("host", p, k, j)


# one mesh, one charge set and -- per kind of targets -- one plan WITHOUT the option with its single executes, for the module
_REF = {}


def reference(fb, kind):
    if "mesh" not in _REF:
        v = two_spheres(fb, 5)
        _REF["mesh"] = (v, charges(len(v), max(KS), seed=5))
    v, X = _REF["mesh"]
    if kind not in _REF:
        plain = fb.FMM_plan(stokes(), v, bc=flags_of(kind, len(v)), p_max=8)
        assert plain.batch_width() == 1
        _REF[kind] = {p: singles(plain, X, p) for p in PS}
        plain.close()
    return v, X, _REF[kind]


def test_option_sets_the_width(fb):
    """Fails without the feature: FMM_plan has no stokes_batch_width, and a Stokes plan's width is 1."""
    v = two_spheres(fb, 5)
    plan = fb.FMM_plan(fb.StokesSphericalBEM(6, 3, 1e-3), v, p_max=8, stokes_batch_width=3)
    assert plan.batch_width() == 3
    assert fb.FMM_plan(fb.StokesSphericalBEM(6, 3, 1e-3), v, p_max=8).batch_width() == 1
    opts = fb.FMMOptions()
    opts.stokes_batch_width = 2                        # the same through FMMOptions
    assert fb.FMM_plan(fb.StokesSphericalBEM(6, 3, 1e-3), v, opts, p_max=8).batch_width() == 2
    for off in (0, 1):
        assert fb.FMM_plan(fb.StokesSphericalBEM(6, 3, 1e-3), v, p_max=8, stokes_batch_width=off).batch_width() == 1


@pytest.mark.parametrize("kind", ["velocity", "traction", "mixed"])
@pytest.mark.parametrize("width", WIDTHS)
def test_bit_identity_over_widths_and_batch_sizes(fb, width, kind):
    v, X, ref = reference(fb, kind)
    plan = fb.FMM_plan(stokes(), v, bc=flags_of(kind, len(v)), p_max=8, stokes_batch_width=width)
    assert plan.batch_width() == width
    assert_batches(plan, X, ref=ref)
    # the numpy and torch forms of the Python plan, at the kernel's own order
    n = len(v)
    got = plan.execute_batch(X[:5].reshape(5, n, 3))
    assert got.shape == (5, n, 3)
    for j in range(5):
        assert np.array_equal(got[j], plan.execute(X[j].reshape(n, 3)))
    import torch
    out = plan.execute_batch_torch(torch.from_numpy(X[:4]).cuda(), p=8).cpu().numpy()
    assert np.array_equal(out, ref[8][:4])


def near_source_panels(plan):
    """near source panels of every target leaf (box index -> count), from the plan's P2P list and boxes"""
    b = plan.boxes()
    size = (b["be"] - b["bb"]).astype(np.int64)
    pairs = plan.pairs("p2p")                          # (source leaf, target leaf)
    count = np.zeros(len(size), dtype=np.int64)
    np.add.at(count, pairs[:, 1], size[pairs[:, 0]])
    return count, size, b


@pytest.mark.parametrize("n_panels", [1301, 1400])
def test_leaf_with_more_than_one_chunk_of_columns(fb, n_panels):
    """some leaf sees more than 1024 near source panels: the chunk loop takes its add-into-y branch; odd and even panel counts"""
    v = fb.unit_sphere(5)[:n_panels]
    o = fb.FMMOptions()
    o.set_max_per_box(300)
    plan = fb.FMM_plan(stokes(), v, o, p_max=8, stokes_batch_width=4)
    assert plan.batch_width() == 4
    count, size, b = near_source_panels(plan)
    t = int(np.argmax(count))
    assert count[t] > 1024, int(count[t])
    cols, _ = plan.near_row(3 * int(b["bb"][t]), values=False)          # the assembled row agrees with the list: 3 unknowns per panel
    assert len(cols) == 3 * count[t]
    X = charges(n_panels, 5, seed=n_panels)
    plain = fb.FMM_plan(stokes(), v, o, p_max=8)
    assert_batches(plan, X, ks=(2, 3, 4, 5), ref={p: singles(plain, X, p) for p in PS})
    for w in (2, 3):
        assert_batches(fb.FMM_plan(stokes(), v, o, p_max=8, stokes_batch_width=w), X, ps=(8,), ks=(w, 5), host_ks=())


@pytest.mark.parametrize("ncrit", [8, 13])
@pytest.mark.parametrize("n_panels", [301, 400])
def test_panel_soup_with_short_and_ragged_leaves(fb, n_panels, ncrit):
    """a random soup of small triangles.  ncrit = 8: leaves with fewer than 8 panel rows, which split the columns over the
    wavefronts; ncrit = 13: leaves whose row counts are a multiple neither of 4 nor of 8 (kRows x wavefronts of every shape)"""
    rng = np.random.default_rng(n_panels)
    c = rng.random((n_panels, 1, 3))
    v = c + 0.04 * (rng.random((n_panels, 3, 3)) - 0.5)
    o = fb.FMMOptions()
    o.set_max_per_box(ncrit)
    X = charges(n_panels, 5, seed=ncrit)
    plain = fb.FMM_plan(stokes(), v, o, p_max=8)
    ref = {p: singles(plain, X, p) for p in PS}
    for w in WIDTHS:
        plan = fb.FMM_plan(stokes(), v, o, p_max=8, stokes_batch_width=w)
        assert plan.batch_width() == w
        b = plan.boxes()
        rows = (b["be"] - b["bb"])[b["leaf"] != 0]
        if ncrit == 8:
            assert ((rows > 0) & (rows < 8)).any()
        else:
            assert ((rows >= 8) & (rows % 4 != 0)).any()
        assert_batches(plan, X, ks=(1, 2, 3, 4, 5), ref=ref)


@pytest.mark.parametrize("evaluator", ["local", "block_diagonal"])
def test_local_and_block_diagonal(fb, evaluator):
    v = two_spheres(fb, 5)
    o = fb.FMMOptions()
    o.lazy_evaluation = False
    o.local_evaluation = evaluator == "local"
    o.block_diagonal = evaluator == "block_diagonal"
    X = charges(len(v), 7, seed=4)
    plain = fb.FMM_plan(stokes(), v, o, p_max=8)
    assert plain.batch_width() == 1
    ref = {p: singles(plain, X, p) for p in PS}
    for w in WIDTHS:
        plan = fb.FMM_plan(stokes(), v, o, p_max=8, stokes_batch_width=w)
        assert plan.batch_width() == w
        assert_batches(plan, X, ks=(1, w, 7), ref=ref)


def test_inactive_plans_keep_width_one_and_still_batch(fb):
    v = two_spheres(fb, 5)
    n = len(v)
    X = charges(n, 4, seed=6)
    o = fb.FMMOptions()
    o.near_stream_fraction = 0.5
    hybrid = fb.FMM_plan(stokes(), v, o, p_max=8, stokes_batch_width=3)
    assert hybrid.stats()["near_recomputed_pairs"] > 0, "the mesh was chosen so that the plan IS hybrid"
    assert hybrid.batch_width() == 1
    assert_batches(hybrid, X, ks=(1, 4))
    f32 = fb.FMM_plan(stokes(), v, p_max=8, near_f32_max_p=4, stokes_batch_width=3)
    assert f32.stats()["near_f32_bytes"] > 0 and f32.batch_width() == 1
    assert_batches(f32, X, ks=(1, 4))
    two = fb.FMM_plan(stokes(), v, p_max=8, devices=[0, 0], stokes_batch_width=3)
    assert two.batch_width() == 1
    assert_batches(two, X, ks=(1, 3), host_ks=())
    for w in (0, 2, 3):                                # a Laplace plan keeps its own width, whatever the option says
        lap = fb.FMM_plan(fb.LaplaceSphericalBEM(6, 3), v, p_max=8, stokes_batch_width=w)
        own = fb.FMM_plan(fb.LaplaceSphericalBEM(6, 3), v, p_max=8).batch_width()
        assert lap.batch_width() == own and own > 1
    import torch
    x1 = np.random.default_rng(7).random((5, n))
    out = lap.execute_batch_torch(torch.from_numpy(x1).cuda(), p=8).cpu().numpy()
    for j in range(5):
        assert np.array_equal(out[j], lap.execute_torch(torch.from_numpy(x1[j]).cuda(), p=8).cpu().numpy())


def test_create_like_inherits_the_width(fb):
    v = two_spheres(fb, 5)
    n = len(v)
    X = charges(n, 7, seed=8)
    base = fb.FMM_plan(stokes(), v, p_max=8, stokes_batch_width=3)
    batch(base, X[:3], 8)                              # the base plan's batch buffers exist before the like plan is made
    like = base.like((np.arange(n) % 2).astype(np.uint8))
    assert like.batch_width() == 3
    plain = fb.FMM_plan(stokes(), v, bc=(np.arange(n) % 2).astype(np.uint8), p_max=8)
    assert_batches(like, X, ks=(1, 3, 7), ref={p: singles(plain, X, p) for p in PS})
    assert_batches(base, X, ps=(8,), ks=(2, 7))    # the base plan's own buffers are untouched by the like plan's


def test_state_between_single_and_batch(fb):
    v, X, ref = reference(fb, "mixed")
    plan = fb.FMM_plan(stokes(), v, bc=flags_of("mixed", len(v)), p_max=8, stokes_batch_width=4)
    before = singles(plan, X[:1], 8)
    b8 = batch(plan, X, 8)
    assert np.array_equal(singles(plan, X[:1], 8), before) and np.array_equal(before[0], ref[8][0])
    b3 = batch(plan, X, 3)                             # p = 8, then p = 3 on the same batch buffers
    assert np.array_equal(b8, ref[8]) and np.array_equal(b3, ref[3])
    assert np.array_equal(singles(plan, X, 3), ref[3]) and np.array_equal(singles(plan, X, 8), ref[8])
    assert np.array_equal(batch(plan, X, 8), ref[8])


def test_gmres_batch_of_three_right_hand_sides(fb):
    import torch
    v = fb.unit_sphere(4)
    n = len(v)
    K = fb.StokesSphericalBEM(8, 4, 1e-3)
    K.set_Kfine(19)
    plan = fb.FMM_plan(K, v, p_max=8, stokes_batch_width=3)
    assert plan.batch_width() == 3
    so = fb.SolverOptions(residual=1e-5, max_iters=100, max_p=8, p_min=5)
    B = np.zeros((3, n, 3))
    for j in range(3):
        B[j, :, j] = 4 * math.pi                       # the three unit translations of the driver
    dev = "cuda:%d" % plan.device
    ref = []
    for j in range(3):
        x = torch.zeros(3 * n, dtype=torch.float64, device=dev)
        log = []
        _, it, res, _ = fb.gmres_capi(plan, x, torch.from_numpy(B[j].reshape(-1)).to(dev), so, log=log, stokes=True)
        ref.append((x.cpu().numpy(), it, res, log))
    logs = [[], [], []]
    Xb = torch.zeros((3, n, 3), dtype=torch.float64, device=dev)
    _, its, ress, _ = fb.gmres_capi_batch(plan, Xb, torch.from_numpy(B).to(dev), so, logs=logs, stokes=True)
    torch.cuda.synchronize()
    got = Xb.cpu().numpy().reshape(3, 3 * n)
    for j in range(3):
        assert its[j] == ref[j][1] and ress[j] == ref[j][2], (j, its[j], ref[j][1])
        assert [p for _, p, _ in logs[j]] == [p for _, p, _ in ref[j][3]]
        assert logs[j] == ref[j][3]
        assert np.array_equal(got[j], ref[j][0]), (j, float(np.abs(got[j] - ref[j][0]).max()))
    assert min(its) > 1


def test_driver_resistance_matrix():
    """examples/StokesBEM.py -resistance with -stokes_batch 3 on the sphere of the driver test: the matrix's deviation from
    6 pi mu I, relative to 6 pi mu, is no larger than 1.5 x the relative drag error the same run prints for its x solve (y and z
    see the triangulation in another orientation)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "StokesBEM.py"), "-recursions", "4", "-p", "10",
                        "-stokes_batch", "3", "-resistance"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-600:] + r.stderr[-600:]
    lines = r.stdout.splitlines()
    assert "batched near field: one pass serves 3 vectors" in lines
    drag = float([ln for ln in lines if ln.startswith("error on a sphere")][0].split(":")[1])
    dev = float([ln for ln in lines if ln.startswith("resistance deviation from 6 pi mu I")][0].split(":")[1])
    at = [i for i, ln in enumerate(lines) if ln.startswith("resistance matrix")][0]
    R = np.array([[float(t) for t in lines[at + 1 + i].split()] for i in range(3)])
    mu6 = 6 * math.pi * 1e-3
    print("drag error %.5e, resistance deviation %.5e" % (drag, dev))
    print(R)
    # the line reports the matrix above it (printed with seven digits: entries to 5e-9, 3e-7 of 6 pi mu)
    assert abs(float(np.abs(R - mu6 * np.eye(3)).max()) / mu6 - dev) <= 1e-6
    assert dev <= 1.5 * drag, (dev, drag)
