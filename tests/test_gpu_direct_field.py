"""The field quantities of the device Direct sum (fb.Direct.gradient / pressure / velocity_gradient / stress, fmmbem_direct_*): the
all-pairs sums that the field executes approximate.  Every pair's value is the entries functions' (bit for bit against
kernel_gradient_entries / kernel_pressure_entries / kernel_velocity_gradient_entries), the order of addition is fixed (bit for bit
across launch shapes), the sums agree with the numpy pair functions of tests/field_*_reference.py, and the field executes converge
to them.

Measured on an MI355X (the figures the tests print):
  1  the 501 targets: 1 self, 457 nearby, 43 far
  2  gradient / pressure: largest |y - ref| / (nterms u sum|E x|) 2.3e-02 / 5.2e-03;
     velocity gradient against the long-double sum of entries: rel L2 1.8e-15, worst row 1.6e-15 of the scale;
     against the numpy pair functions: rel L2 4.6e-14 (gradient), 3.4e-13 (pressure), 2.1e-13 (velocity gradient) -- the 50 points
     within a tenth of a panel of the surface carry the norm
  4  no_far, the execute against the Direct quantity: 0 (gradient), 3.6e-16 (pressure), 0 (velocity gradient)
  5  two_r3, the execute against the Direct quantity, p = 8 / p = 12:
     gradient 3.676e-04 / 1.847e-04, pressure 4.962e-04 / 3.059e-05, velocity gradient 2.347e-03 / 2.943e-04; the same six figures
     against the numpy all-pairs sum.  (The gradient's floor is not truncation: a far box of the 16-panel leaves holds panels that
     are `nearby` for the quadrature, which the Direct sum gives the 16-point rule and P2M the K stored points --
     tests/field_gradient_reference.py, "limit".)
  7  the driver at 512 panels, p = 8, 200 points at r = 3 -- eight leaves that are all neighbours, no far field: field (FMM)
     against field 1.124e-15; pressure against Direct 1.228e-15, velocity gradient against Direct 1.728e-15 (the bound: 4 x the
     first figure)
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import field_gradient_reference as G
import field_plan_reference as R
import field_pressure_reference as Q
import field_velocity_gradient_reference as V
from conftest import rel_l2

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
LD = np.longdouble
QUANTITIES = ("gradient", "pressure", "velocity_gradient")


def point_panels(points, h=1e-9):
    """tiny triangles whose centroids stand for the points (tests/test_gpu_direct.py)"""
    off = np.array([[h, 0, 0], [0, h, 0], [-h, -h, 0]])
    return np.asarray(points, dtype=np.float64)[:, None, :] + off[None, :, :]


def centroids(v):
    return (v[:, 0] + v[:, 1] + v[:, 2]) / 3


def unit_dirs(rng, m):
    d = rng.normal(size=(m, 3))
    return d / np.linalg.norm(d, axis=1)[:, None]


def field_points(rng, v, m_shell, m_in, m_near):
    """shells at 1.01 .. 3 radii, interior points, and points within a tenth of a panel of the surface (tests/test_gpu_direct.py)"""
    c = centroids(v)
    nrm = c / np.linalg.norm(c, axis=1)[:, None]
    size = np.sqrt(2 * 0.5 * np.linalg.norm(np.cross(v[:, 2] - v[:, 0], v[:, 1] - v[:, 0]), axis=1))
    pick = rng.choice(len(v), m_near, replace=False)
    near = c[pick] + nrm[pick] * (size[pick] * 0.1 * (2 * rng.random(m_near) - 1))[:, None]
    shell = unit_dirs(rng, m_shell) * (1.01 + 1.99 * rng.random(m_shell))[:, None]
    inner = unit_dirs(rng, m_in) * (0.95 * rng.random(m_in))[:, None]
    return np.concatenate([shell, inner, near])


def kernels(fb):
    return {"laplace": fb.LaplaceSphericalBEM(5, G.K), "stokes": R.stokes_kernel(fb, 5)}       # K = 3; K = 4, K_fine = 19, mu = 1e-3


def kind_of(quantity):
    return "laplace" if quantity == "gradient" else "stokes"


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


def run(D, quantity, x, pts, flags=None):
    if quantity == "gradient":
        return D.gradient(x, pts, flags)
    return getattr(D, quantity)(x, pts)


# ---- 1. one source: every term is the entries function's -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_source(sphere):
    src = sphere[17:18]
    c = centroids(src)[0]
    size = np.sqrt(np.linalg.norm(np.cross(src[0, 2] - src[0, 0], src[0, 1] - src[0, 0])))       # sqrt(2 A)
    rng = np.random.default_rng(3)
    dist = size * 10 ** rng.uniform(np.log10(1e-3), np.log10(5), 500)
    tri = np.concatenate([point_panels(c + unit_dirs(rng, 500) * dist[:, None]), src])             # ... plus its own centroid
    tri.setflags(write=False)
    return src, tri


def test_one_source_hits_all_three_regimes(sphere, one_source):
    src, tri = one_source
    g = Q.sub(Q.geometry(np.ascontiguousarray(sphere)), [17])
    masks = np.array([Q.regimes(t, g) for t in centroids(tri)])[:, :, 0]                           # (targets, [self, nearby])
    n_self, n_near, n_far = int(masks[:, 0].sum()), int(masks[:, 1].sum()), int((~masks.any(axis=1)).sum())
    print("regimes of the 501 targets: self %d, nearby %d, far %d" % (n_self, n_near, n_far))
    assert n_self == 1 and masks[-1, 0] and n_near >= 100 and n_far >= 20 and n_self + n_near + n_far == len(tri)


@pytest.mark.parametrize("flag", [0, 1])
def test_one_source_gradient_is_the_entries_bit_for_bit(fb, sphere, one_source, flag):
    src, tri = one_source
    K = kernels(fb)["laplace"]
    bc = np.full(len(tri), flag, np.uint8)
    E = fb.kernel_gradient_entries(K, tri, np.repeat(src, len(tri), axis=0), target_bc=bc)
    D = fb.Direct(K, src)
    y = D.gradient(np.ones(1), tri, bc)
    D.close()
    assert y.shape == (len(tri), 3) and np.all(np.isfinite(y))
    assert np.array_equal(y, E)
    if flag == 0:                                            # the centroid row: 2 pi n_j
        nrm = G.geometry(np.ascontiguousarray(sphere))["normal"][17]
        assert np.allclose(y[-1], 2 * np.pi * nrm, rtol=0, atol=1e-13) and abs(np.linalg.norm(y[-1]) - 2 * np.pi) <= 1e-13
    else:
        assert np.all(y[-1] == 0)
    assert np.all(np.abs(y[:-1]).max(axis=1) > 0)


def test_one_source_pressure_is_the_entries_bit_for_bit(fb, one_source):
    src, tri = one_source
    K = kernels(fb)["stokes"]
    E = fb.kernel_pressure_entries(K, tri, np.repeat(src, len(tri), axis=0))
    D = fb.Direct(K, src)
    for k in range(3):
        x = np.zeros((1, 3))
        x[0, k] = 1.0
        y = D.pressure(x, tri)
        assert y.shape == (len(tri),) and np.all(np.isfinite(y))
        assert np.array_equal(y, E[:, k]), k
        assert y[-1] == 0 and np.all(y[:-1] != 0)
    D.close()


def test_one_source_velocity_gradient_is_the_entries_bit_for_bit(fb, one_source):
    src, tri = one_source
    K = kernels(fb)["stokes"]
    E = fb.kernel_velocity_gradient_entries(K, tri, np.repeat(src, len(tri), axis=0))
    D = fb.Direct(K, src)
    for e in range(3):
        x = np.zeros((1, 3))
        x[0, e] = 1.0
        y = D.velocity_gradient(x, tri)
        assert y.shape == (len(tri), 3, 3) and np.all(np.isfinite(y))
        assert np.array_equal(y, E[..., e]), e
        assert np.all(y[-1] == 0) and np.all(np.abs(y[:-1]).reshape(len(tri) - 1, 9).max(axis=1) > 0)
    D.close()


# ---- 2. the sum ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sum_case(few):
    rng = np.random.default_rng(5)
    pts = field_points(rng, few, 200, 50, 50)
    tri = point_panels(pts)
    flags = (rng.random(len(tri)) < 0.5).astype(np.uint8)
    x1, x3 = rng.normal(size=len(few)), rng.normal(size=(len(few), 3))
    for a in (tri, flags, x1, x3):
        a.setflags(write=False)
    return tri, flags, x1, x3


def pairs(tri, v):
    return np.repeat(tri, len(v), axis=0), np.tile(v, (len(tri), 1, 1))


@pytest.mark.parametrize("quantity", ["gradient", "pressure"])
def test_sum_within_the_fma_bound(fb, few, sum_case, quantity):
    """|y - ref| <= nterms 2^-53 sum|E x| row by row, ref the long-double sum of the device entries times x: a chunk is nterms fused
    multiply-adds in a row, the chunks' partial sums add two more roundings (the bound of tests/test_gpu_direct.py)"""
    tri, flags, x1, x3 = sum_case
    n, m = len(few), len(tri)
    K = kernels(fb)[kind_of(quantity)]
    T, S = pairs(tri, few)
    D = fb.Direct(K, few)
    if quantity == "gradient":
        E = fb.kernel_gradient_entries(K, T, S, target_bc=np.repeat(flags, n)).reshape(m, n, 3)
        terms = (E.astype(LD) * x1.astype(LD)[None, :, None]).transpose(0, 2, 1)                  # (m, 3, n)
        y, nterms = D.gradient(x1, tri, flags), n
    else:
        E = fb.kernel_pressure_entries(K, T, S).reshape(m, n, 3)
        terms = (E.astype(LD) * x3.astype(LD)[None]).reshape(m, 3 * n)
        y, nterms = D.pressure(x3, tri), 3 * n
    D.close()
    ref, mag = terms.sum(axis=-1), np.abs(terms).sum(axis=-1)
    err = np.abs(y.astype(LD) - ref)
    bound = nterms * U * mag
    print("%s: max |y - ref| / (nterms u sum|E x|) = %.3e" % (quantity, float(np.max(err / bound))))
    assert np.all(np.isfinite(y)) and np.all(mag > 0)
    assert np.all(err <= bound)


def test_velocity_gradient_sum_against_the_entries(fb, few, sum_case):
    """The tensor is contracted with f inside the quadrature, so no entrywise bound is derivable: held against the long-double sum of
    entries times x to the project's parity figures, those of tests/test_gpu_field_velocity_gradient.py -- relative L2 <= 1e-12,
    worst row <= 1e-11 of the scale, here the largest sum_j sum_e |Gamma_ij,e| |x_je| of a component of a row"""
    tri, _, _, x3 = sum_case
    n, m = len(few), len(tri)
    K = kernels(fb)["stokes"]
    T, S = pairs(tri, few)
    E = fb.kernel_velocity_gradient_entries(K, T, S).reshape(m, n, 3, 3, 3)
    terms = E.astype(LD) * x3.astype(LD)[None, :, None, None, :]
    ref = terms.sum(axis=(1, 4))
    scale = float(np.abs(terms).sum(axis=(1, 4)).max())
    D = fb.Direct(K, few)
    y = D.velocity_gradient(x3, tri)
    D.close()
    rel = float(np.linalg.norm((y.astype(LD) - ref).ravel()) / np.linalg.norm(ref.ravel()))
    row = float(np.abs(y.astype(LD) - ref).max() / scale)
    print("velocity gradient vs long-double sum of entries: rel L2 %.3e, worst row %.3e of the scale" % (rel, row))
    assert np.all(np.isfinite(y))
    assert rel <= 1e-12
    assert row <= 1e-11


@pytest.mark.parametrize("quantity", QUANTITIES)
def test_sum_against_the_numpy_pair_functions(fb, few, sum_case, quantity):
    tri, flags, x1, x3 = sum_case
    pts = centroids(tri)
    v = np.ascontiguousarray(few)
    K = kernels(fb)[kind_of(quantity)]
    D = fb.Direct(K, few)
    if quantity == "gradient":
        g = G.geometry(v)
        ref = np.stack([G.gamma(pts[i], int(flags[i]), v, g).T @ x1 for i in range(len(pts))])
        y = D.gradient(x1, tri, flags)
    elif quantity == "pressure":
        g = Q.geometry(v)
        ref = np.array([np.sum(Q.pi_entry(pts[i], v, g) * x3) for i in range(len(pts))])
        y = D.pressure(x3, tri)
    else:
        g = Q.geometry(v)
        ref = np.stack([np.einsum("pkme,pe->km", V.gamma_entry(pts[i], v, g), x3) for i in range(len(pts))])
        y = D.velocity_gradient(x3, tri)
    D.close()
    err = rel_l2(y, ref)
    print("%s vs the numpy pair functions: rel L2 %.3e" % (quantity, err))
    assert y.shape == ref.shape and err <= 1e-12


# ---- 3. the bits do not depend on the launch -----------------------------------------------------------------------------------
@pytest.mark.parametrize("quantity", QUANTITIES)
def test_launch_independence(fb, few, quantity):
    import torch
    K = kernels(fb)[kind_of(quantity)]
    rng = np.random.default_rng(17)
    pts = np.ascontiguousarray(field_points(rng, few, 1500, 400, 100))
    flags = (rng.random(len(pts)) < 0.5).astype(np.uint8)
    assert len(pts) == 2000
    x = rng.normal(size=len(few) if quantity == "gradient" else (len(few), 3))
    D = fb.Direct(K, few)
    y = run(D, quantity, x, pts, flags)
    assert np.all(np.isfinite(y))
    assert np.array_equal(y, run(D, quantity, x, pts, flags))                                     # two runs
    for i in range(20):                                                                           # one target at a time
        assert np.array_equal(run(D, quantity, x, pts[i:i + 1], flags[i:i + 1])[0], y[i]), i
    halves = np.concatenate([run(D, quantity, x, pts[:1000], flags[:1000]), run(D, quantity, x, pts[1000:], flags[1000:])])
    assert np.array_equal(halves, y)
    dev = torch.device("cuda:0")
    xd, pd = torch.from_numpy(x).to(dev), torch.from_numpy(pts).to(dev)
    if quantity == "gradient":
        yd = D.gradient_torch(xd, pd, torch.from_numpy(flags).to(dev))
        assert np.array_equal(D.gradient(x, pts), D.gradient(x, pts, np.zeros(len(pts), np.uint8)))   # target_bc None: all 0
    else:
        yd = getattr(D, quantity + "_torch")(xd, pd)
    torch.cuda.synchronize()
    assert tuple(yd.shape) == y.shape and np.array_equal(yd.cpu().numpy(), y)                     # host form == device form
    out = torch.empty_like(yd)
    args = (xd, pd, torch.from_numpy(flags).to(dev)) if quantity == "gradient" else (xd, pd)
    assert getattr(D, quantity + "_torch")(*args, out=out) is out
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), y)
    with pytest.raises(ValueError):
        getattr(D, quantity + "_torch")(*args, out=out[:-1])
    with pytest.raises(ValueError):
        run(D, quantity, x[:-1], pts, flags)
    D.close()


# ---- 4, 5. against the field executes ------------------------------------------------------------------------------------------
def execute_and_direct(fb, name, quantity, orders):
    """({p: the field execute at order p}, the Direct quantity, the numpy all-pairs sum) on the case's panels and points; the flags as
    the case gives them for Laplace, all 0 for Stokes"""
    c = G.make_case(name)
    v, pts = np.ascontiguousarray(c["v"]), np.ascontiguousarray(c["pts"])
    opts = fb.FMMOptions()
    opts.set_mac_theta(G.THETA)
    opts.set_max_per_box(c["ncrit"])
    p_max = max(orders)
    if quantity == "gradient":
        K = fb.LaplaceSphericalBEM(p_max, G.K)
        x = np.random.default_rng(1).standard_normal(len(v))
        plan = fb.FMM_plan(K, v, opts, p_max=p_max, targets=pts, target_bc=c["flags"])
        g = G.geometry(v)
        ref = np.stack([G.gamma(pts[i], int(c["flags"][i]), v, g).T @ x for i in range(len(pts))])
    else:
        K = R.stokes_kernel(fb, p_max)
        x = np.random.default_rng(1).standard_normal((len(v), 3))
        plan = fb.FMM_plan(K, v, opts, p_max=p_max).field_plan(pts)
        g = Q.geometry(v)
        if quantity == "pressure":
            ref = np.array([np.sum(Q.pi_entry(pts[i], v, g) * x) for i in range(len(pts))])
        else:
            ref = np.stack([np.einsum("pkme,pe->km", V.gamma_entry(pts[i], v, g), x) for i in range(len(pts))])
    got = {}
    for p in orders:
        K.set_p(p)
        got[p] = getattr(plan, "execute_" + quantity)(x)
    stats = plan.stats()
    plan.close()
    D = fb.Direct(K, v)
    d = run(D, quantity, x, pts, c["flags"])
    D.close()
    return got, d, ref, stats


@pytest.mark.parametrize("quantity", QUANTITIES)
def test_no_far_field_execute_equals_direct(fb, quantity):
    """32 panels, 30 points, one source leaf: every pair is a near pair, and the two differ only in the order of addition"""
    got, d, ref, stats = execute_and_direct(fb, "no_far", quantity, (8,))
    assert stats["m2l_pairs"] == 0 and len(d) == 30
    err = rel_l2(got[8], d)
    print("no_far %s: execute vs Direct rel L2 %.3e (Direct vs numpy %.3e)" % (quantity, err, rel_l2(d, ref)))
    assert err <= 1e-12


@pytest.mark.parametrize("quantity", QUANTITIES)
def test_fmm_error_is_the_same_against_either_sum(fb, quantity):
    """the form of test_fmm_error_is_the_same_against_either_direct (tests/test_gpu_direct.py)"""
    got, d, ref, stats = execute_and_direct(fb, "two_r3", quantity, (8, 12))
    assert stats["m2l_pairs"] > 0
    e_gpu = {p: rel_l2(got[p], d) for p in got}
    e_np = {p: rel_l2(got[p], ref) for p in got}
    print("two_r3 %s: execute vs device Direct p = 8: %.6e, p = 12: %.6e; vs the numpy all-pairs sum %.6e, %.6e"
          % (quantity, e_gpu[8], e_gpu[12], e_np[8], e_np[12]))
    for p in got:
        assert abs(e_gpu[p] - e_np[p]) <= 1e-12, p
    assert e_gpu[12] < e_gpu[8]


# ---- 6. status codes, handle kept ----------------------------------------------------------------------------------------------
def test_status_codes_handle_kept(fb, few):
    L, vp = fb.lib(), ctypes.c_void_p
    ptr = lambda a: a.ctypes.data_as(vp)                                                         # noqa: E731
    n = len(few)
    pts = np.ascontiguousarray(centroids(few)[:40] * 2)
    bad = pts.copy()
    bad[5, 2] = np.nan
    x1, x3 = np.ones(n), np.ones((n, 3))
    DL, DS = fb.Direct(kernels(fb)["laplace"], few), fb.Direct(kernels(fb)["stokes"], few)
    m = len(pts)
    SENT = 7.25
    calls = {
        "gradient": (DL, DS, x1, x3, 3, lambda h, mm, p, x, o: L.fmmbem_direct_gradient(h, mm, p, None, x, o),
                     lambda h, mm, p, x, o: L.fmmbem_direct_gradient_device(h, mm, p, None, x, o, None)),
        "pressure": (DS, DL, x3, x1, 1, lambda h, mm, p, x, o: L.fmmbem_direct_pressure(h, mm, p, x, o),
                     lambda h, mm, p, x, o: L.fmmbem_direct_pressure_device(h, mm, p, x, o, None)),
        "velocity_gradient": (DS, DL, x3, x1, 9, lambda h, mm, p, x, o: L.fmmbem_direct_velocity_gradient(h, mm, p, x, o),
                              lambda h, mm, p, x, o: L.fmmbem_direct_velocity_gradient_device(h, mm, p, x, o, None)),
    }
    for quantity, (good, wrong, x, x_wrong, w, host, device) in calls.items():
        before = run(good, quantity, x, pts)
        out = np.full((m, w), SENT)
        assert host(wrong._h, m, ptr(pts), ptr(x_wrong), ptr(out)) == 6, quantity                 # the wrong kind of handle
        msg = L.fmmbem_last_error().decode()
        assert ("Laplace" if quantity == "gradient" else "Stokes") in msg and quantity.replace("_", " ") in msg, msg
        assert device(wrong._h, m, ptr(pts), ptr(x_wrong), ptr(out)) == 6, quantity               # (refused before any pointer is read)
        assert host(good._h, m, ptr(bad), ptr(x), ptr(out)) == 1, quantity                        # a NaN in a target point
        assert host(good._h, 0, ptr(pts), ptr(x), ptr(out)) == 1, quantity
        assert host(good._h, m, ptr(pts), None, ptr(out)) == 1, quantity
        assert host(good._h, m, ptr(pts), ptr(x), None) == 1, quantity
        assert host(good._h, m, None, ptr(x), ptr(out)) == 1, quantity
        assert device(good._h, 0, ptr(pts), ptr(x), ptr(out)) == 1, quantity
        assert device(good._h, m, None, ptr(x), ptr(out)) == 1, quantity
        # the order of the checks: no targets comes before the wrong kind of handle, the wrong kind before the NaN
        assert host(wrong._h, 0, ptr(pts), ptr(x_wrong), ptr(out)) == 1 and host(wrong._h, m, ptr(bad), ptr(x_wrong), ptr(out)) == 6
        assert np.all(out == SENT), quantity                                                      # the output is untouched
        assert np.array_equal(run(good, quantity, x, pts), before), quantity                      # and the handle usable
        assert np.array_equal(wrong.matvec(x_wrong, targets=pts), wrong.matvec(x_wrong, targets=pts))
    with pytest.raises(fb.FmmBemError) as e:
        DS.gradient(x3, pts)
    assert e.value.status == 6
    with pytest.raises(fb.FmmBemError) as e:
        DL.stress(x1, pts)
    assert e.value.status == 6
    with pytest.raises(ValueError):
        DL.gradient(x1, pts, np.zeros(3, np.uint8))
    # stress is -q I + mu (G + G^T) of the two other methods, bit for bit
    rng = np.random.default_rng(29)
    xs = rng.normal(size=(n, 3))
    q, g = DS.pressure(xs, pts), DS.velocity_gradient(xs, pts)
    s = DS.stress(xs, pts)
    assert s.shape == (m, 3, 3) and np.array_equal(s, -q[:, None, None] * np.eye(3)[None] + R.MU * (g + g.transpose(0, 2, 1)))
    assert np.array_equal(s, s.transpose(0, 2, 1)) and np.abs(s).max() > 0
    DL.close()
    DS.close()


# ---- 7. the driver -------------------------------------------------------------------------------------------------------------
def driver(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "examples", "StokesBEM.py")] + list(args), capture_output=True, text=True, timeout=600)


def test_driver_field_direct():
    """-field_direct prints the two "against Direct" lines, at or below 4 x the level of the "field (FMM) against field" line of the
    same run -- the margin DESIGN.md section 8 gives the double layer over the velocity, for the extra derivative.  That line needs
    -field 200 beside -field_fmm 200, so the run carries it."""
    base = ("-recursions", "4", "-p", "8", "-field", "200", "-field_fmm", "200", "-field_pressure", "-field_stress")
    r = driver(*base, "-field_direct")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()

    def figure(prefix):
        hit = [ln for ln in lines if ln.startswith(prefix)]
        assert len(hit) == 1, (prefix, lines[-14:])
        return float(hit[0].split("relative L2 difference")[1]), lines.index(hit[0])

    level, _ = figure("field (FMM) against field:")
    dq, iq = figure("field pressure (FMM) against Direct:")
    dg, ig = figure("field velocity gradient (FMM) against Direct:")
    print("driver: field (FMM) against field %.3e; pressure against Direct %.3e, velocity gradient against Direct %.3e" % (level, dq, dg))
    assert lines[iq - 1].startswith("field pressure (FMM):") and lines[ig - 1].startswith("field velocity gradient (FMM):")
    assert sum("against Direct" in ln for ln in lines) == 2
    assert 0 < dq <= 4 * level and 0 < dg <= 4 * level
    # without the flag: none of the new lines, every other line of the field report as it was
    r0 = driver(*base)
    assert r0.returncode == 0, r0.stderr[-2000:]
    lines0 = r0.stdout.splitlines()
    assert not any("against Direct" in ln for ln in lines0)
    tail = lambda ls: [ln for ln in ls if ln.startswith("field") and "against Direct" not in ln]  # noqa: E731
    assert tail(lines) == tail(lines0) and len(tail(lines0)) >= 6
    for args in (("-field_direct",), ("-field_fmm", "200", "-field_direct")):
        bad = driver("-recursions", "4", "-p", "8", *args)
        assert bad.returncode != 0 and "-field_direct" in bad.stderr, args
