"""The block inverse (csrc/kernels_blockinv.hip) on leaves that pivot and on blocks of 63 to 768 unknowns.  The meshes of
tests/test_gpu_block_inverse.py give column-dominant blocks of at most 192 unknowns: no row is ever exchanged there and no loop of
the kernels takes a second trip.  Here the blocks come from tight triangle soups (tests/block_inverse_cases.py); each case counts,
on the blocks it reads back from its own plan, the exchanges that a float64 restatement of the kernel's elimination makes, and
holds z = apply(v) to a long-double elimination of the same blocks:
    |z_dev - z_ld| <= 4 max(|inv(A) v - z_ld|, |z_emul - z_ld|) + 4 m 2^-52 |z_ld|        per leaf,
LAPACK's explicit inverse and the restatement being the yardsticks (on the CPU oracle's blocks the restatement stays within
0.1 - 2.8 x LAPACK; the factor 4 is for the device's fma and the order of the sums in its apply)."""
import ctypes as C
import time

import numpy as np
import pytest

import block_inverse_cases as bic
from test_gpu_block_inverse import _bd_options

pytestmark = pytest.mark.gpu

U = bic.U
NAMES = sorted(bic.SINGLE) + list(bic.MULTI)

_cache = {}


def _kernel(fb, kern):
    if kern == "laplace":
        return fb.LaplaceSphericalBEM(5, 3)
    K = fb.StokesSphericalBEM(5, bic.STOKES_K)
    K.set_Kfine(bic.STOKES_KFINE)
    return K


def _plan(fb, kern, v, bc, ncrit):
    return fb.FMM_plan(_kernel(fb, kern), v, _bd_options(fb, ncrit), bc=bc)


def _leaves(plan):
    bx = plan.boxes()
    return sorted((int(bx["bb"][b]), int(bx["be"][b])) for b in range(len(bx["leaf"])) if bx["leaf"][b])      # the plan's leaf order


def _blocks(plan):
    """every leaf's self block read back through the near-row getter, and the positions of its unknowns in a flattened vector
    in the caller's order"""
    dof = plan.dof
    perm = plan.perm().astype(np.int64)
    blocks, index = [], []
    for bb, be in _leaves(plan):
        m = dof * (be - bb)
        A = np.empty((m, m))
        for i in range(m):
            cols, vals = plan.near_row(dof * bb + i)
            assert cols.tolist() == list(range(dof * bb, dof * be))
            A[i] = vals
        blocks.append(A)
        index.append((perm[bb:be, None] * dof + np.arange(dof)[None, :]).reshape(-1))
    return blocks, index


def _case(fb, name, key=None):
    """Built once per case and shared, never modified: the plan with its inverse, its leaf blocks on the host, the references of
    every leaf (block_inverse_cases.leaf_references), a seeded Gaussian v and z = apply(v)."""
    key = key or name
    if key in _cache:
        return _cache[key]
    kern, verts, bc, ncrit = bic.case_input(name)
    n = len(verts)
    plan = _plan(fb, kern, verts, bc, ncrit)
    dof = plan.dof
    blocks, index = _blocks(plan)
    assert sum(len(ix) for ix in index) == n * dof
    if name in bic.SINGLE:
        assert [len(A) for A in blocks] == [dof * n]
    else:
        assert sorted(len(A) for A in blocks) == [1, 1, 31, 270, 297]
    assert plan.block_inverse_bytes() == 0
    t0 = time.perf_counter()
    plan.block_inverse_build()
    build_s = time.perf_counter() - t0
    assert plan.block_inverse_bytes() == 8 * sum(A.size for A in blocks)
    v = np.random.default_rng(sum(name.encode())).standard_normal((n,) if dof == 1 else (n, dof))
    z = plan.block_inverse_apply(v)
    assert np.isfinite(z).all()
    vf = v.reshape(-1)
    refs = [bic.leaf_references(A, vf[ix]) for A, ix in zip(blocks, index)]
    _cache[key] = dict(plan=plan, n=n, dof=dof, verts=verts, bc=bc, ncrit=ncrit, kern=kern, blocks=blocks, index=index, v=v, z=z, refs=refs,
                       build_s=build_s)
    return _cache[key]


def _forward_check(d, label):
    """the bound of the module's docstring on every leaf; returns the largest ratio 4 |z_dev - z_ld| / bound, i.e. the error over
    max(|inv(A) v - z_ld|, |z_emul - z_ld|) + m u |z_ld| -- the assertion is ratio <= 4"""
    zf = d["z"].reshape(-1)
    worst = 0.0
    for leaf, (ix, r) in enumerate(zip(d["index"], d["refs"])):
        err = float(np.linalg.norm(zf[ix] - r["z_ld"]))
        ratio = 4.0 * err / r["bound"]
        worst = max(worst, ratio)
        print("%s leaf %d (m = %d): |z_dev - z_ld| / |z_ld| = %.3g, LAPACK %.3g, restatement %.3g, m u = %.3g, ratio to the yardstick %.3g" %
              (label, leaf, len(ix), err / r["norm_z"], r["e_lapack"] / r["norm_z"], r["e_emul"] / r["norm_z"], len(ix) * U, ratio))
        assert err <= r["bound"], (label, leaf, err, r["bound"])
    return worst


# ---- 1. the inputs do what they are here for, counted on the plan's own blocks ---------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_blocks_exchange_rows(fb, name):
    d = _case(fb, name)
    counts = [bic.exchanges(r["piv"]) for r in d["refs"]]
    print("%s: blocks %s, exchanges per leaf %s, with a pivot row >= 256: %s, >= 512: %s; build %.4f s" %
          (name, [len(A) for A in d["blocks"]], counts, [bic.exchanges(r["piv"], 256) for r in d["refs"]],
           [bic.exchanges(r["piv"], 512) for r in d["refs"]], d["build_s"]))
    if name in bic.SINGLE:
        beyond = bic.SINGLE[name][3]
        if beyond is not None:
            assert counts[0] >= 1 and bic.exchanges(d["refs"][0]["piv"], beyond) >= 1
    else:
        assert sum(1 for c in counts if c > 0) >= 2
        assert all(c > 0 for c, A in zip(counts, d["blocks"]) if len(A) > 256)          # both blocks of more than 256 rows


# ---- 2. forward error against the long-double elimination ------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_forward_error_against_long_double(fb, name):
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63
    d = _case(fb, name)
    print("%s: largest ratio to the yardstick %.3g (bound 4)" % (name, _forward_check(d, name)))


# ---- 3. the checks of test_gpu_block_inverse.py, unchanged in form ---------------------------------------------------------------

def _residual_bounds(d):
    if "bounds" not in d:
        vf, zf = d["v"].reshape(-1), d["z"].reshape(-1)
        out = []
        for A, ix, r in zip(d["blocks"], d["index"], d["refs"]):
            m = len(ix)
            nA = np.linalg.norm(A, 2)
            zl, vl = zf[ix], vf[ix]
            zr = r["lapack_inv"] @ vl                                # the yardstick: LAPACK's explicit inverse
            dev = np.linalg.norm(A @ zl - vl) / (nA * np.linalg.norm(zl))
            ref = np.linalg.norm(A @ zr - vl) / (nA * np.linalg.norm(zr))
            out.append((dev, 4.0 * max(ref, m * U), nA * np.linalg.norm(zl)))
        d["bounds"] = out
    return d["bounds"]


@pytest.mark.parametrize("name", NAMES)
def test_residual_against_the_plans_own_blocks(fb, name):
    d = _case(fb, name)
    bounds = _residual_bounds(d)
    print("%s: max residual ratio to max(LAPACK, m u): %.3g" % (name, max(dev / (bound / 4.0) for dev, bound, _ in bounds)))
    for leaf, (dev, bound, _) in enumerate(bounds):
        assert dev <= bound, (name, leaf, dev, bound)


@pytest.mark.parametrize("name", NAMES)
def test_execute_of_apply_returns_v(fb, name):
    d = _case(fb, name)
    y = d["plan"].execute(d["z"]).reshape(-1)
    vf = d["v"].reshape(-1)
    worst = 0.0
    for leaf, (ix, (_, bound, scale)) in enumerate(zip(d["index"], _residual_bounds(d))):
        err = np.linalg.norm(y[ix] - vf[ix])
        worst = max(worst, err / (bound * scale))
        assert err <= bound * scale, (name, leaf, err, bound * scale)
    print("%s: max |execute(apply(v)) - v| over its bound: %.3g" % (name, worst))


# ---- 4. the whole inverse of a pivoting block of more than 256 rows ---------------------------------------------------------------

def _unit_vector_images(d, ix):
    """apply of the unit vectors of the unknowns ix, in one call: (len(ix), n dof)"""
    n, dof = d["n"], d["dof"]
    E = np.zeros((len(ix), n * dof))
    E[np.arange(len(ix)), ix] = 1.0
    return d["plan"].block_inverse_apply(E.reshape((len(ix), n) if dof == 1 else (len(ix), n, dof))).reshape(len(ix), n * dof)


@pytest.mark.parametrize("name", ["laplace-300-f1", "multi-f1"])
def test_whole_inverse_of_a_pivoting_block(fb, name):
    """Every entry of the inverse of the case's largest leaf (300 rows; 297 rows beside four other leaves), relative to the largest
    entry, against the long-double inverse; the yardsticks are LAPACK's inverse and the restatement's, as in the forward check."""
    d = _case(fb, name)
    leaf = int(np.argmax([len(ix) for ix in d["index"]]))
    ix, r = d["index"][leaf], d["refs"][leaf]
    m = len(ix)
    assert m > 256 and bic.exchanges(r["piv"], 256) >= 1
    Z = _unit_vector_images(d, ix)
    outside = np.ones(Z.shape[1], dtype=bool)
    outside[ix] = False
    assert outside.sum() == Z.shape[1] - m and (Z[:, outside] == 0.0).all()
    dev = Z[:, ix].T                                                  # image c is column c of the inverse
    inv_ld = bic.ld_solve(r["fac"], np.eye(m))
    top = float(np.abs(inv_ld).max())
    e_dev = float(np.abs(dev - inv_ld).max()) / top
    e_lapack = float(np.abs(r["lapack_inv"] - inv_ld).max()) / top
    e_emul = float(np.abs(r["emul_inv"] - inv_ld).max()) / top
    print("%s leaf %d (m = %d): max entry error over the largest entry: device %.3g, LAPACK %.3g, restatement %.3g" %
          (name, leaf, m, e_dev, e_lapack, e_emul))
    assert e_dev <= 4.0 * max(e_lapack, e_emul) + 4.0 * m * U


# ---- 5. bits -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["laplace-300-f1", "multi-mixed"])
def test_same_bits_for_every_k_every_stride_and_a_second_plan(fb, monkeypatch, name):
    import torch
    d = _case(fb, name)
    plan, n = d["plan"], d["n"]
    assert d["dof"] == 1
    V = np.random.default_rng(17).standard_normal((9, n))
    V[4] = d["v"]
    single = np.stack([plan.block_inverse_apply(V[j]) for j in range(9)])
    assert np.array_equal(single[4], d["z"])
    for k in (1, 2, 3, 4, 5, 9):
        assert np.array_equal(plan.block_inverse_apply(V[:k]), single[:k]), k
    # the device entry with ldv != ldz, both larger than a vector: the gaps keep their sentinel
    k, ldv, ldz, sentinel = 5, n + 3, n + 11, -7.25
    vd = torch.full((k, ldv), sentinel, dtype=torch.float64, device="cuda")
    vd[:, :n] = torch.from_numpy(V[:k]).cuda()
    zd = torch.full((k, ldz), sentinel, dtype=torch.float64, device="cuda")
    st = fb.lib().fmmbem_plan_block_inverse_apply_device(plan._h, k, C.c_void_p(vd.data_ptr()), ldv, C.c_void_p(zd.data_ptr()), ldz,
                                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0
    torch.cuda.synchronize()
    zh, vh = zd.cpu().numpy(), vd.cpu().numpy()
    assert np.array_equal(zh[:, :n], single[:k])
    assert (zh[:, n:] == sentinel).all() and (vh[:, n:] == sentinel).all() and np.array_equal(vh[:, :n], V[:k])
    # a second plan of the same inputs, sharing nothing with the first (its own tree, lists and assembly): the same inverse,
    # entry by entry
    monkeypatch.setenv("FMMBEM_PLAN_SHARE", "0")
    twin = _plan(fb, d["kern"], d["verts"], d["bc"], d["ncrit"])
    twin.block_inverse_build()
    d2 = dict(d, plan=twin)
    everything = np.arange(n)
    assert np.array_equal(_unit_vector_images(d2, everything), _unit_vector_images(d, everything))


# ---- 6. a singular block found late: an ordinary refusal -----------------------------------------------------------------------------

def _refused(fb, plan, x, bad_leaves):
    y0 = plan.execute(x)
    assert np.isfinite(y0).all()
    with pytest.raises(fb.FmmBemError) as e:
        plan.block_inverse_build()
    assert e.value.status == 1
    assert "leaf %d " % min(bad_leaves) in str(e.value) and "singular" in str(e.value)
    assert plan.block_inverse_bytes() == 0
    with pytest.raises(fb.FmmBemError) as e:
        plan.block_inverse_apply(x)
    assert e.value.status == 1
    assert np.array_equal(plan.execute(x), y0)


@pytest.mark.parametrize("flag", [0, 1])
def test_singular_block_found_at_step_256(fb, flag):
    """Panel 256 of the 257-panel soup repeats panel 1: two equal columns, and the second is exactly zero from the first's step
    on, so the search of step 256 -- the first of the second trip of the 256-thread loops -- finds nothing, after real exchanges"""
    _, verts, _, ncrit = bic.single_input("laplace-257-f%d" % flag)
    verts = verts.copy()
    verts[256] = verts[1]
    plan = _plan(fb, "laplace", verts, np.full(257, flag, dtype=np.uint8), ncrit)
    (A,), _ = _blocks(plan)
    _, piv, bad = bic.gauss_jordan(A)
    print("flag %d: the restatement meets a zero pivot at step %s after %d exchanges" % (flag, bad, bic.exchanges(piv)))
    assert bad is not None and bad >= 256 and bic.exchanges(piv) >= 1
    _refused(fb, plan, np.random.default_rng(5).standard_normal(257), [0])


def test_singular_blocks_in_two_large_leaves_name_the_lower(fb):
    _, verts, bc, ncrit = bic.multi_input("multi-f0")
    host = fb.FMM_plan(_kernel(fb, "laplace"), verts, _bd_options(fb, ncrit), bc=bc, host_only=True)
    perm = host.perm().astype(np.int64)
    verts = verts.copy()
    pairs = []
    for bb, be in _leaves(host):
        if be - bb > 256:                                            # one panel repeated in each of the two large leaves
            verts[perm[be - 3]] = verts[perm[bb + 5]]
            pairs.append(sorted((int(perm[bb + 5]), int(perm[be - 3]))))
    assert len(pairs) == 2
    plan = _plan(fb, "laplace", verts, bc, ncrit)
    perm = plan.perm().astype(np.int64)
    blocks, _ = _blocks(plan)
    bad_leaves = []
    for leaf, ((bb, be), A) in enumerate(zip(_leaves(plan), blocks)):
        _, piv, bad = bic.gauss_jordan(A)
        if bad is not None:
            assert any(set(p) <= set(perm[bb:be].tolist()) for p in pairs) and len(A) > 256 and bad >= 256 and bic.exchanges(piv) >= 1
            bad_leaves.append(leaf)
    print("leaves", [len(A) for A in blocks], "singular:", bad_leaves)
    assert len(bad_leaves) == 2
    _refused(fb, plan, np.random.default_rng(6).standard_normal(len(verts)), bad_leaves)


# ---- 7. Stokes blocks read from the nine-value rows -----------------------------------------------------------------------------------

def test_nine_value_stokes_rows(fb, monkeypatch):
    """FMMBEM_STOKES_SYM=0 stores the Stokes blocks as rows of nine values per panel pair and the build kernel reads them as it
    reads Laplace rows.  A plan created while one of the same panels is alive is a copy that keeps its storage form, so plan
    sharing is off here, and the form is asserted through the bytes of the stored blocks."""
    sym = _case(fb, "stokes-86-vel")
    monkeypatch.setenv("FMMBEM_PLAN_SHARE", "0")
    monkeypatch.setenv("FMMBEM_STOKES_SYM", "0")
    d = _case(fb, "stokes-86-vel", key="stokes-86-vel/nine")
    assert d["plan"].stats()["geometry_shared"] == 1
    monkeypatch.undo()
    m = 258
    b9, b6 = d["plan"].stats()["near_bytes"], sym["plan"].stats()["near_bytes"]
    print("stored near blocks: %d bytes as nine-value rows, %d bytes in the symmetric form; 8 m^2 = %d" % (b9, b6, 8 * m * m))
    assert b9 >= 8 * m * m > b6 >= 8 * 6 * 86 * 86                  # nine, not six, values per panel pair
    assert bic.exchanges(d["refs"][0]["piv"], 256) >= 1
    print("nine-value rows: largest ratio to the yardstick %.3g (bound 4)" % _forward_check(d, "stokes-86-vel/nine"))
    A9, A6 = d["blocks"][0], sym["blocks"][0]
    same = np.array_equal(A9, A6)
    print("blocks bitwise those of the symmetric plan: %s (largest difference over the largest entry %.3g)" %
          (same, np.abs(A9 - A6).max() / np.abs(A6).max()))
    assert np.abs(A9 - A6).max() <= 1e-13 * np.abs(A6).max()         # the same operator, entries to rounding
    if same:                                                         # the same block bits must give the same result bits
        assert np.array_equal(d["z"], sym["z"])


# ---- the cost of the largest block served ----------------------------------------------------------------------------------------------

def test_build_time_of_a_768_unknown_block_is_reported(fb):
    """One workgroup runs 768 elimination steps over 4.7 MB; printed beside the build of a Stokes TRACTION plan on
    unit_sphere(4), whose leaves hold up to 192 unknowns (a first build each: allocation, launch and synchronisation included)."""
    big = _case(fb, "stokes-256-vel")
    n = 512
    plan = fb.FMM_plan(fb.StokesSphericalBEM(5, 3), fb.unit_sphere(4), _bd_options(fb, 64), bc=np.ones(n, dtype=np.uint8))
    t0 = time.perf_counter()
    plan.block_inverse_build()
    small_s = time.perf_counter() - t0
    assert max(3 * (e - b) for b, e in _leaves(plan)) == 192
    print("build of one 768-unknown block: %.4f s (traction: %.4f s); of unit_sphere(4) Stokes, %d leaves, largest block 192: %.4f s" %
          (big["build_s"], _case(fb, "stokes-256-tra")["build_s"], len(_leaves(plan)), small_s))
    assert big["plan"].block_inverse_bytes() == 8 * 768 * 768
