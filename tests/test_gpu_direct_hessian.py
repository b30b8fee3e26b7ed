"""The Hessian of the device Direct sum (fb.Direct.hessian, fmmbem_direct_hessian): the all-pairs sum that FMM_plan.execute_hessian
approximates.  Every pair's value is kernel_hessian_entries' bit for bit, the order of addition is fixed (bit for bit across launch
shapes), the sum agrees with eta of tests/field_hessian_reference.py in numpy, and on a plan without a far field the execute is the
same sum in another order."""
import ctypes

import numpy as np
import pytest

import field_gradient_reference as G
import field_hessian_reference as H
from conftest import rel_l2
from test_gpu_direct_field import centroids, field_points, point_panels, unit_dirs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sphere(fb):
    v = fb.unit_sphere(5)
    v.setflags(write=False)
    return v


@pytest.fixture(scope="module")
def few(fb, sphere):
    """the first 2 chunks + 77 panels: two full chunks and a ragged third"""
    n = 2 * fb.lib().fmmbem_direct_chunk() + 77
    assert n <= len(sphere)
    return sphere[:n]


def kernel(fb):
    return fb.LaplaceSphericalBEM(5, H.K)


# ---- 1. one source: every term is the entries function's -----------------------------------------------------------------------
@pytest.mark.parametrize("flag", [0, 1])
def test_one_source_is_the_entries_bit_for_bit(fb, sphere, flag):
    """500 points at 1e-3 .. 5 sqrt(2 A) from panel 17's centroid, and the centroid: the self, 16-point and K-point regimes"""
    src = sphere[17:18]
    c = centroids(src)[0]
    size = np.sqrt(np.linalg.norm(np.cross(src[0, 2] - src[0, 0], src[0, 1] - src[0, 0])))       # sqrt(2 A)
    rng = np.random.default_rng(3)
    dist = size * 10 ** rng.uniform(np.log10(1e-3), np.log10(5), 500)
    tri = np.concatenate([point_panels(c + unit_dirs(rng, 500) * dist[:, None]), src])
    d = np.linalg.norm(centroids(tri) - c, axis=1)
    nearby = (size / np.maximum(d, 1e-300) >= 0.5) & (d >= 1e-8)
    assert (d < 1e-8).sum() == 1 and d[-1] < 1e-8 and nearby.sum() >= 100 and (~nearby).sum() - 1 >= 20
    K = kernel(fb)
    bc = np.full(len(tri), flag, np.uint8)
    E = fb.kernel_hessian_entries(K, tri, np.repeat(src, len(tri), axis=0), target_bc=bc)
    D = fb.Direct(K, src)
    y = D.hessian(np.ones(1), tri, bc)
    D.close()
    assert y.shape == (len(tri), 3, 3) and np.all(np.isfinite(y))
    assert np.array_equal(y, E)
    assert np.array_equal(y, y.transpose(0, 2, 1))
    assert np.all(y[-1] == 0)                                # the centroid row: 0 for both flags
    assert np.all(np.abs(y[:-1]).max(axis=(1, 2)) > 0)


# ---- 2. the sum ----------------------------------------------------------------------------------------------------------------
def test_sum_against_eta_in_numpy(fb, few):
    """1101 panels, 300 points (shells, interior, 50 within a tenth of a panel of the surface), both flags: <= 1e-12 relative"""
    rng = np.random.default_rng(5)
    tri = point_panels(field_points(rng, few, 200, 50, 50))
    flags = (rng.random(len(tri)) < 0.5).astype(np.uint8)
    x = rng.normal(size=len(few))
    pts = centroids(tri)
    v = np.ascontiguousarray(few)
    g = G.geometry(v)
    ref = np.stack([np.einsum("pab,p->ab", H.eta(pts[i], int(flags[i]), v, g), x) for i in range(len(pts))])
    D = fb.Direct(kernel(fb), few)
    y = D.hessian(x, tri, flags)
    D.close()
    err = rel_l2(y, ref)
    print("Direct Hessian vs eta . x in numpy: rel L2 %.3e" % err)
    assert y.shape == ref.shape and np.array_equal(y, y.transpose(0, 2, 1))
    assert err <= 1e-12


# ---- 3. the bits do not depend on the launch -----------------------------------------------------------------------------------
def test_launch_independence(fb, few):
    import torch
    rng = np.random.default_rng(17)
    pts = np.ascontiguousarray(field_points(rng, few, 1500, 400, 100))
    flags = (rng.random(len(pts)) < 0.5).astype(np.uint8)
    x = rng.normal(size=len(few))
    D = fb.Direct(kernel(fb), few)
    y = D.hessian(x, pts, flags)
    assert np.all(np.isfinite(y)) and np.array_equal(y, y.transpose(0, 2, 1))
    assert np.array_equal(y, D.hessian(x, pts, flags))                                            # two runs
    for i in range(20):                                                                           # one target at a time
        assert np.array_equal(D.hessian(x, pts[i:i + 1], flags[i:i + 1])[0], y[i]), i
    halves = np.concatenate([D.hessian(x, pts[:1000], flags[:1000]), D.hessian(x, pts[1000:], flags[1000:])])
    assert np.array_equal(halves, y)
    assert np.array_equal(D.hessian(x, pts), D.hessian(x, pts, np.zeros(len(pts), np.uint8)))     # target_bc None: all 0
    dev = torch.device("cuda:0")
    xd, pd, fd = torch.from_numpy(x).to(dev), torch.from_numpy(pts).to(dev), torch.from_numpy(flags).to(dev)
    yd = D.hessian_torch(xd, pd, fd)
    out = torch.empty_like(yd)
    assert D.hessian_torch(xd, pd, fd, out=out) is out
    torch.cuda.synchronize()
    assert tuple(yd.shape) == y.shape and np.array_equal(yd.cpu().numpy(), y) and np.array_equal(out.cpu().numpy(), y)
    with pytest.raises(ValueError):
        D.hessian_torch(xd, pd, fd, out=out[:-1])
    with pytest.raises(ValueError):
        D.hessian(x[:-1], pts, flags)
    D.close()


# ---- 4. against the field execute ----------------------------------------------------------------------------------------------
def test_no_far_field_execute_equals_direct(fb):
    """32 panels, 30 points, one source leaf: every pair is a near pair, and the two differ only in the order of addition"""
    c = G.make_case("no_far")
    v, pts = np.ascontiguousarray(c["v"]), np.ascontiguousarray(c["pts"])
    opts = fb.FMMOptions()
    opts.set_mac_theta(G.THETA)
    opts.set_max_per_box(c["ncrit"])
    K = fb.LaplaceSphericalBEM(8, G.K)
    x = np.random.default_rng(1).standard_normal(len(v))
    plan = fb.FMM_plan(K, v, opts, p_max=8, targets=pts, target_bc=c["flags"])
    got = plan.execute_hessian(x)
    assert plan.stats()["m2l_pairs"] == 0
    plan.close()
    D = fb.Direct(K, v)
    d = D.hessian(x, pts, c["flags"])
    D.close()
    err = rel_l2(got, d)
    print("no_far: execute_hessian vs Direct.hessian rel L2 %.3e" % err)
    assert len(d) == 30 and err <= 1e-12


# ---- 5. status codes, handle kept ----------------------------------------------------------------------------------------------
def test_status_codes_handle_kept(fb, few):
    L, vp = fb.lib(), ctypes.c_void_p
    ptr = lambda a: a.ctypes.data_as(vp)                                                         # noqa: E731
    n = len(few)
    pts = np.ascontiguousarray(centroids(few)[:40] * 2)
    bad = pts.copy()
    bad[5, 2] = np.nan
    x1, x3 = np.ones(n), np.ones((n, 3))
    DL, DS = fb.Direct(kernel(fb), few), fb.Direct(fb.StokesSphericalBEM(5, 4), few)
    m = len(pts)
    SENT = 7.25
    host = lambda h, mm, p, x, o: L.fmmbem_direct_hessian(h, mm, p, None, x, o)                   # noqa: E731
    device = lambda h, mm, p, x, o: L.fmmbem_direct_hessian_device(h, mm, p, None, x, o, None)    # noqa: E731
    before = DL.hessian(x1, pts)
    out = np.full((m, 9), SENT)
    assert host(DS._h, m, ptr(pts), ptr(x3), ptr(out)) == 6                                       # the wrong kind of handle
    msg = L.fmmbem_last_error().decode()
    assert "Laplace" in msg and "Hessian" in msg, msg
    assert device(DS._h, m, ptr(pts), ptr(x3), ptr(out)) == 6                                     # (refused before any pointer is read)
    assert host(DL._h, m, ptr(bad), ptr(x1), ptr(out)) == 1                                       # a NaN in a target point
    assert host(DL._h, 0, ptr(pts), ptr(x1), ptr(out)) == 1
    assert host(DL._h, m, ptr(pts), None, ptr(out)) == 1
    assert host(DL._h, m, ptr(pts), ptr(x1), None) == 1
    assert host(DL._h, m, None, ptr(x1), ptr(out)) == 1
    assert device(DL._h, 0, ptr(pts), ptr(x1), ptr(out)) == 1
    assert device(DL._h, m, None, ptr(x1), ptr(out)) == 1
    # the order of the checks: no targets comes before the wrong kind of handle, the wrong kind before the NaN
    assert host(DS._h, 0, ptr(pts), ptr(x3), ptr(out)) == 1 and host(DS._h, m, ptr(bad), ptr(x3), ptr(out)) == 6
    assert np.all(out == SENT)                                                                    # the output is untouched
    assert np.array_equal(DL.hessian(x1, pts), before)                                            # and the handles usable
    assert np.array_equal(DS.matvec(x3, targets=pts), DS.matvec(x3, targets=pts))
    with pytest.raises(fb.FmmBemError) as e:
        DS.hessian(x3, pts)
    assert e.value.status == 6
    with pytest.raises(ValueError):
        DL.hessian(x1, pts, np.zeros(3, np.uint8))
    DL.close()
    DS.close()
