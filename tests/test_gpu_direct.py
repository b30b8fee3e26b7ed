"""The device Direct sum (fb.Direct, fmmbem_direct_*): y_i = sum_j K(t_i, s_j) x_j for all pairs in one kernel, Laplace and Stokes.
Every entry is the assembly's (bit for bit against kernel_entries), the order of addition is fixed (bit for bit across launch shapes),
and the sums agree with the CPU oracle's Direct to the project's 1e-12."""
import ctypes

import numpy as np
import pytest

from conftest import rel_l2

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def point_panels(points, h=1e-9):
    """tiny triangles whose centroids stand for the points (the trick of test_gpu_target_plan.py)"""
    off = np.array([[h, 0, 0], [0, h, 0], [-h, -h, 0]])
    return np.asarray(points, dtype=np.float64)[:, None, :] + off[None, :, :]


def centroids(v):
    return (v[:, 0] + v[:, 1] + v[:, 2]) / 3


def kernels(fb):
    KS = fb.StokesSphericalBEM(5, 4, mu=1e-3)
    KS.set_Kfine(19)
    return {"laplace": fb.LaplaceSphericalBEM(5, 3), "stokes": KS}


def unit_dirs(rng, m):
    d = rng.normal(size=(m, 3))
    return d / np.linalg.norm(d, axis=1)[:, None]


@pytest.fixture(scope="module")
def sphere(fb):
    v = fb.unit_sphere(5)
    v.setflags(write=False)
    return v


@pytest.fixture(scope="module")
def few(fb, sphere):
    """the first 2 chunk + 77 panels: two full chunks and a ragged third"""
    n = 2 * fb.lib().fmmbem_direct_chunk() + 77
    assert n <= len(sphere)
    return sphere[:n]


def field_points(rng, v, m_shell, m_in, m_near):
    """shells at 1.01 .. 3 radii, interior points, and points within a tenth of a panel of the surface"""
    c = centroids(v)
    nrm = c / np.linalg.norm(c, axis=1)[:, None]
    size = np.sqrt(2 * 0.5 * np.linalg.norm(np.cross(v[:, 2] - v[:, 0], v[:, 1] - v[:, 0]), axis=1))
    pick = rng.choice(len(v), m_near, replace=False)
    near = c[pick] + nrm[pick] * (size[pick] * 0.1 * (2 * rng.random(m_near) - 1))[:, None]
    shell = unit_dirs(rng, m_shell) * (1.01 + 1.99 * rng.random(m_shell))[:, None]
    inner = unit_dirs(rng, m_in) * (0.95 * rng.random(m_in))[:, None]
    return np.concatenate([shell, inner, near])


# ---- 1. one source: every term is the assembly's entry -------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["laplace", "stokes"])
@pytest.mark.parametrize("flag", [0, 1])
def test_one_source_is_kernel_entries_bit_for_bit(fb, sphere, kind, flag):
    K = kernels(fb)[kind]
    src = sphere[17:18]
    c = centroids(src)[0]
    size = np.sqrt(np.linalg.norm(np.cross(src[0, 2] - src[0, 0], src[0, 1] - src[0, 0])))       # sqrt(2 A)
    rng = np.random.default_rng(3)
    dist = size * 10 ** rng.uniform(np.log10(1e-3), np.log10(5), 500)
    tri = np.concatenate([point_panels(c + unit_dirs(rng, 500) * dist[:, None]), src])             # ... plus its own centroid
    bc = np.full(len(tri), flag, np.uint8)
    E = fb.kernel_entries(K, tri, np.repeat(src, len(tri), axis=0), target_bc=bc)
    D = fb.Direct(K, src)
    if kind == "laplace":
        y = D.matvec(np.ones(1), targets=tri, target_bc=bc)
        assert np.array_equal(y, E)
        assert np.all(np.isfinite(y)) and (flag == 0 or y[-1] == 2 * np.pi)
    else:
        for k in range(3):
            x = np.zeros((1, 3))
            x[0, k] = 1.0
            y = D.matvec(x, targets=tri, target_bc=bc)
            assert np.array_equal(y, E[:, :, k]), k
            assert np.all(np.isfinite(y))
    D.close()


# ---- 2. the sum: n fused multiply-adds in a fixed order ------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["laplace", "stokes"])
def test_sum_within_the_fma_bound(fb, few, kind):
    K = kernels(fb)[kind]
    n = len(few)
    rng = np.random.default_rng(5)
    pts = field_points(rng, few, 200, 50, 50)
    tri = point_panels(pts)
    m = len(tri)
    bc = (rng.random(m) < 0.5).astype(np.uint8)
    E = fb.kernel_entries(K, np.repeat(tri, n, axis=0), np.tile(few, (m, 1, 1)), target_bc=np.repeat(bc, n))
    D = fb.Direct(K, few)
    ld = np.longdouble                                   # the reference sum in extended precision: its own error is 2^-11 of the bound
    if kind == "laplace":
        x = rng.normal(size=n)
        terms = E.reshape(m, n).astype(ld) * x.astype(ld)[None, :]
        nterms = n
    else:
        x = rng.normal(size=(n, 3))
        terms = (E.reshape(m, n, 3, 3).astype(ld) * x.astype(ld)[None, :, None, :]).transpose(0, 2, 1, 3).reshape(m, 3, 3 * n)
        nterms = 3 * n
    y = D.matvec(x, targets=tri, target_bc=bc)
    ref, mag = terms.sum(axis=-1), np.abs(terms).sum(axis=-1)
    err = np.abs(y.astype(ld) - ref)
    bound = nterms * U * mag
    print("%s: max |y - ref| / (n u sum|E x|) = %.3e" % (kind, float(np.max(err / bound))))
    assert np.all(err <= bound)
    D.close()


# ---- 3. the symmetric form against the oracle ----------------------------------------------------------------------------------
def flags_for(which, n):
    if which == "first":
        return np.zeros(n, np.uint8)
    if which == "second":
        return np.ones(n, np.uint8)
    return (np.arange(n) % 3 == 1).astype(np.uint8)


@pytest.mark.parametrize("which", ["first", "second", "mixed"])
def test_symmetric_laplace_matches_oracle(fb, oracle_mod, sphere, which):
    bc = flags_for(which, len(sphere))
    x = np.random.default_rng(7).normal(size=len(sphere))
    D = fb.Direct(fb.LaplaceSphericalBEM(5, 3), sphere)
    y = D.matvec(x, target_bc=bc)
    ref = oracle_mod.Oracle(sphere, bc=bc, K=3).direct(x)
    err = rel_l2(y, ref)
    print("laplace symmetric %s: rel L2 vs oracle %.3e" % (which, err))
    assert err <= 1e-12
    D.close()


@pytest.mark.parametrize("which", ["first", "mixed"])
def test_symmetric_stokes_matches_oracle(fb, oracle_mod, sphere, which):
    bc = flags_for(which, len(sphere))
    x = np.random.default_rng(8).normal(size=(len(sphere), 3))
    D = fb.Direct(kernels(fb)["stokes"], sphere)
    y = D.matvec(x, target_bc=bc)
    ref = oracle_mod.StokesOracle(sphere, K=4, K_fine=19, mu=1e-3, bc=bc).direct(x)
    err = rel_l2(y, ref)
    print("stokes symmetric %s: rel L2 vs oracle %.3e" % (which, err))
    assert err <= 1e-12
    D.close()


# ---- 4. points against the oracle ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def thousand(sphere):
    rng = np.random.default_rng(11)
    pts = field_points(rng, sphere, 700, 250, 50)
    flags = (rng.random(len(pts)) < 0.5).astype(np.uint8)
    pts.setflags(write=False)
    flags.setflags(write=False)
    return pts, flags


def test_points_laplace_match_oracle(fb, oracle_mod, sphere, thousand):
    pts, flags = thousand
    x = np.random.default_rng(12).normal(size=len(sphere))
    D = fb.Direct(fb.LaplaceSphericalBEM(5, 3), sphere)
    y = D.matvec(x, targets=pts, target_bc=flags)
    ref = oracle_mod.TargetOracle(sphere, pts, target_bc=flags, K=3).direct(x)
    err = rel_l2(y, ref)
    print("laplace points: rel L2 vs oracle %.3e" % err)
    assert err <= 1e-12
    D.close()


def stokes_oracle_at(oracle_mod, v, pts, flags, x):
    """(the oracle's sum of kernel_entries(t_i, s_j) x_j at probe triangles, the centres the oracle reports for them)"""
    n, m = len(v), len(pts)
    ctx = oracle_mod.StokesOracle(np.concatenate([v, point_panels(pts)]), K=4, K_fine=19, mu=1e-3, ncrit=1 << 30,
                                  bc=np.concatenate([np.zeros(n, np.uint8), flags]))
    centres = ctx.panels()["center"][n:].copy()
    y = np.empty((m, 3))
    sj = np.tile(np.arange(n, dtype=np.int32), 100)
    for b in range(0, m, 100):
        e = min(b + 100, m)
        ti = np.repeat(np.arange(n + b, n + e, dtype=np.int32), n)
        E = ctx.kernel_entries(ti, sj[:len(ti)]).reshape(e - b, n, 3, 3)
        y[b:e] = np.einsum("ijab,jb->ia", E, x)
    ctx.close()
    return y, centres


def test_points_stokes_match_oracle(fb, oracle_mod, sphere, thousand):
    pts, flags = thousand
    x = np.random.default_rng(13).normal(size=(len(sphere), 3))
    ref, centres = stokes_oracle_at(oracle_mod, sphere, pts, flags, x)
    D = fb.Direct(kernels(fb)["stokes"], sphere)
    y = D.matvec(x, targets=centres, target_bc=flags)
    err = rel_l2(y, ref)
    print("stokes points: rel L2 vs oracle %.3e" % err)
    assert err <= 1e-12
    D.close()


# ---- 5. the bits do not depend on the launch -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["laplace", "stokes"])
def test_launch_independence(fb, few, kind):
    import torch
    K = kernels(fb)[kind]
    rng = np.random.default_rng(17)
    pts = field_points(rng, few, 1500, 400, 100)
    flags = (rng.random(len(pts)) < 0.5).astype(np.uint8)
    assert len(pts) == 2000
    x = rng.normal(size=len(few) if kind == "laplace" else (len(few), 3))
    D = fb.Direct(K, few)
    y = D.matvec(x, targets=pts, target_bc=flags)
    assert np.array_equal(y, D.matvec(x, targets=pts, target_bc=flags))                           # two runs
    for i in range(20):                                                                           # one target at a time
        assert np.array_equal(D.matvec(x, targets=pts[i:i + 1], target_bc=flags[i:i + 1])[0], y[i]), i
    halves = np.concatenate([D.matvec(x, targets=pts[:1000], target_bc=flags[:1000]),
                             D.matvec(x, targets=pts[1000:], target_bc=flags[1000:])])
    assert np.array_equal(halves, y)
    dev = torch.device("cuda:0")
    yd = D.matvec_torch(torch.from_numpy(x).to(dev), torch.from_numpy(pts.copy()).to(dev), torch.from_numpy(flags.copy()).to(dev))
    assert np.array_equal(yd.cpu().numpy(), y)                                                    # host form == device form
    # the symmetric form on device tensors, and the same thing through explicit points
    bc = (np.arange(len(few)) % 2).astype(np.uint8)
    ys = D.matvec(x, target_bc=bc)
    ysd = D.matvec_torch(torch.from_numpy(x).to(dev), None, torch.from_numpy(bc).to(dev))
    assert np.array_equal(ysd.cpu().numpy(), ys)
    assert np.array_equal(D.matvec(x, targets=few, target_bc=bc), ys)
    D.close()


def test_apply_status_codes_handle_kept(fb, few):
    K = fb.LaplaceSphericalBEM(5, 3)
    D = fb.Direct(K, few)
    L, vp = fb.lib(), ctypes.c_void_p
    n = len(few)
    x, y = np.ones(n), np.zeros(n)
    pts = np.ascontiguousarray(centroids(few) * 2)
    ptr = lambda a: a.ctypes.data_as(vp)                                                         # noqa: E731
    bad = pts.copy()
    bad[5, 2] = np.nan
    assert L.fmmbem_direct_apply(D._h, n, ptr(bad), None, ptr(x), ptr(y)) == 1                    # a NaN in a target point
    assert L.fmmbem_direct_apply(D._h, n - 1, None, None, ptr(x), ptr(y)) == 1                    # symmetric form, n_targets != n_sources
    assert L.fmmbem_direct_apply(D._h, 0, ptr(pts), None, ptr(x), ptr(y)) == 1
    assert L.fmmbem_direct_apply(D._h, n, ptr(pts), None, None, ptr(y)) == 1
    assert L.fmmbem_direct_apply(D._h, n, ptr(pts), None, ptr(x), None) == 1
    assert L.fmmbem_direct_apply_device(D._h, n - 1, None, None, ptr(x), ptr(y), None) == 1
    assert np.all(y == 0)
    with pytest.raises(ValueError):
        D.matvec(x, targets=pts, target_bc=np.zeros(3, np.uint8))
    assert D.chunk == L.fmmbem_direct_chunk()
    ref = D.matvec(x, targets=pts)                                                                # target_bc None: all 0
    assert np.array_equal(ref, D.matvec(x, targets=pts, target_bc=np.zeros(n, np.uint8)))
    D.close()
    D.close()


# ---- 6. agrees with the FMM ----------------------------------------------------------------------------------------------------
def test_fmm_error_is_the_same_against_either_direct(fb, oracle_mod, sphere):
    v = np.concatenate([sphere, sphere + np.array([3.0, 0.5, 0.25])])
    x = np.random.default_rng(19).normal(size=len(v))
    K = fb.LaplaceSphericalBEM(12, 3)
    plan = fb.FMM_plan(K, v, p_max=12)
    yf = plan.execute(x)
    plan.close()
    D = fb.Direct(K, v)
    yd = D.matvec(x)
    D.close()
    yo = oracle_mod.Oracle(v, K=3).direct(x)
    e_gpu, e_orc = rel_l2(yf, yd), rel_l2(yf, yo)
    print("FMM p=12 vs device Direct %.6e, vs oracle Direct %.6e" % (e_gpu, e_orc))
    assert abs(e_gpu - e_orc) <= 1e-12


# ---- 7. analytic: the single layer of a uniform density on the unit sphere -------------------------------------------------------
def test_stokes_uniform_density_on_a_sphere(fb, oracle_mod, sphere):
    K = kernels(fb)["stokes"]
    g = np.array([0.3, -1.1, 0.7])
    rng = np.random.default_rng(23)
    pts = np.concatenate([unit_dirs(rng, 150) * (1.5 + 1.5 * rng.random(150))[:, None], unit_dirs(rng, 50) * (0.7 * rng.random(50))[:, None]])
    r = np.linalg.norm(pts, axis=1)[:, None]
    xh = pts / r
    gx = (xh @ g)[:, None]
    c = (1 / (2 * K.Mu)) * (16 * np.pi / 3)
    exact = np.where(r > 1, c * ((3 / (4 * r)) * (g[None, :] + gx * xh) + (1 / (4 * r ** 3)) * (g[None, :] - 3 * gx * xh)), c * g[None, :])
    x = np.tile(g, (len(sphere), 1))
    ref, centres = stokes_oracle_at(oracle_mod, sphere, pts, np.zeros(len(pts), np.uint8), x)
    # the oracle places a probe's centre within an ulp or two of the point: far below the discretisation error measured here
    D = fb.Direct(K, sphere)
    y = D.matvec(x, targets=centres)
    D.close()
    dev_gpu, dev_orc = np.linalg.norm(y - exact), np.linalg.norm(ref - exact)
    print("uniform density: |gpu - exact| / |exact| = %.3e, oracle %.3e" % (dev_gpu / np.linalg.norm(exact), dev_orc / np.linalg.norm(exact)))
    assert dev_orc / np.linalg.norm(exact) < 5e-2          # the formula and the discretisation are talking about the same field
    assert dev_gpu <= 2 * dev_orc
