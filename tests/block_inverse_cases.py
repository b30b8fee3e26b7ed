"""Inputs and host references shared by tests/test_gpu_block_inverse_pivot.py and tests/test_block_inverse_host.py: triangle soups
whose leaf blocks make a partial-pivot elimination exchange rows (the blocks of a smooth closed mesh never do), a float64 numpy
restatement of the device's Gauss-Jordan inversion (csrc/kernels_blockinv.hip: same pivot rule, same in-place order) that
records the exchanges, and a plain Gaussian elimination in np.longdouble as the high-precision yardstick."""
import numpy as np

U = 2.0 ** -52


def soup(seed, n, clusters, stretch, size_spread, sigma):
    """tests/near_form_cases.py::_soup with the spread of a cluster as a parameter (there 0.15): at sigma = 0.03 the panels
    of a cluster sit within a few panel sizes of each other and the off-diagonal entries of a leaf block outgrow the diagonal"""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-1, 1, (clusters, 3)) * np.array([stretch, 1.0, 1.0 / stretch])
    which = rng.integers(0, clusters, n)
    c = centres[which] + rng.normal(0, sigma, (n, 3))
    h = 0.02 * np.exp(rng.uniform(-size_spread, size_spread, n))
    e0, e1 = rng.normal(size=(n, 3)), rng.normal(size=(n, 3))
    e0 /= np.linalg.norm(e0, axis=1, keepdims=True)
    e1 -= (e1 * e0).sum(axis=1, keepdims=True) * e0
    e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
    return np.stack([c, c + h[:, None] * e0, c + h[:, None] * (0.3 * e0 + e1)], axis=1)


# Single-leaf plans: n <= ncrit, the root is the only leaf and m = dof * n.
#   name: (kernel, panels, flag of every panel, lowest pivot row that at least one exchange must reach -- None: a size-only case)
SINGLE = {
    "laplace-63-f0": ("laplace", 63, 0, 0), "laplace-63-f1": ("laplace", 63, 1, 0),
    "laplace-64-f0": ("laplace", 64, 0, None), "laplace-64-f1": ("laplace", 64, 1, 0),
    "laplace-65-f0": ("laplace", 65, 0, None), "laplace-65-f1": ("laplace", 65, 1, 0),
    "laplace-255-f0": ("laplace", 255, 0, 0), "laplace-255-f1": ("laplace", 255, 1, 0),
    "laplace-256-f0": ("laplace", 256, 0, 0), "laplace-256-f1": ("laplace", 256, 1, 0),
    "laplace-257-f0": ("laplace", 257, 0, 0), "laplace-257-f1": ("laplace", 257, 1, 0),
    "laplace-300-f0": ("laplace", 300, 0, 256), "laplace-300-f1": ("laplace", 300, 1, 256),
    "stokes-21-vel": ("stokes", 21, 0, 0), "stokes-21-tra": ("stokes", 21, 1, 0),
    "stokes-22-vel": ("stokes", 22, 0, None),
    "stokes-86-vel": ("stokes", 86, 0, 0), "stokes-86-tra": ("stokes", 86, 1, 0),
    "stokes-256-vel": ("stokes", 256, 0, 512), "stokes-256-tra": ("stokes", 256, 1, 512),
}
# One plan of five leaves (297, 1, 1, 31 and 270 panels): 1 x 1 blocks beside blocks of more than 256 rows.
MULTI = ("multi-f0", "multi-f1", "multi-mixed")
MULTI_N, MULTI_NCRIT = 600, 300
STOKES_K, STOKES_KFINE = 3, 19


def single_input(name):
    """(kernel, vertices, flags, ncrit) of a SINGLE case"""
    kern, n, flag, _ = SINGLE[name]
    v = soup((1000 if kern == "laplace" else 2000) + n, n, 1, 1.0, 2.0, 0.03)
    return kern, v, np.full(n, flag, dtype=np.uint8), n


def multi_input(name):
    v = soup(1, MULTI_N, 2, 1.0, 2.0, 0.03)
    if name == "multi-mixed":
        bc = (np.random.default_rng(3).random(MULTI_N) < 0.5).astype(np.uint8)
    else:
        bc = np.full(MULTI_N, 0 if name == "multi-f0" else 1, dtype=np.uint8)
    return "laplace", v, bc, MULTI_NCRIT


def case_input(name):
    return single_input(name) if name in SINGLE else multi_input(name)


def gauss_jordan(A):
    """The build kernel's elimination in float64 numpy: at step k the pivot is the largest |W(i, k)|, i >= k, the lowest such
    row; rows k and pivot change places; W(k, k) = 1 and row k is divided by the pivot; every other row i takes
    f = W(i, k), W(i, k) = 0, W(i, :) -= f W(k, :); the exchanges are undone on the columns, last first.  Returns
    (inverse or None, pivot rows so far, the step that met a zero or non-finite pivot or None)."""
    W = np.array(A, dtype=np.float64)
    m = W.shape[0]
    piv = []
    for k in range(m):
        p = k + int(np.argmax(np.abs(W[k:, k])))
        pv = W[p, k]
        if not abs(pv) > 0.0 or np.isinf(pv):
            return None, piv, k
        piv.append(p)
        if p != k:
            W[[k, p]] = W[[p, k]]
        W[k, k] = 1.0
        W[k] /= pv
        f = W[:, k].copy()
        f[k] = 0.0
        W[:, k] = 0.0
        W[k, k] = 1.0 / pv
        W -= np.outer(f, W[k])
    for k in range(m - 1, -1, -1):
        if piv[k] != k:
            W[:, [k, piv[k]]] = W[:, [piv[k], k]]
    return W, piv, None


def exchanges(piv, at_least=0):
    """row exchanges among the pivot rows of gauss_jordan whose pivot row is at_least or beyond"""
    return sum(1 for k, p in enumerate(piv) if p != k and p >= at_least)


def ld_factor(A):
    """P A = L U by partial-pivot Gaussian elimination in np.longdouble (numpy has no extended-precision LAPACK)"""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "np.longdouble is no extended type on this host: the yardstick would be double"
    L = np.array(A, dtype=np.longdouble)
    m = L.shape[0]
    piv = np.empty(m, dtype=np.int64)
    for k in range(m):
        p = k + int(np.argmax(np.abs(L[k:, k])))
        piv[k] = p
        if p != k:
            L[[k, p]] = L[[p, k]]
        L[k + 1:, k] /= L[k, k]
        L[k + 1:, k + 1:] -= np.outer(L[k + 1:, k], L[k, k + 1:])
    return L, piv


def ld_solve(fac, B):
    """A X = B for the columns of B (m, r) or the vector B (m,), from ld_factor's factors, in np.longdouble"""
    L, piv = fac
    m = L.shape[0]
    X = np.array(B, dtype=np.longdouble).reshape(m, -1)
    for k in range(m):
        if piv[k] != k:
            X[[k, piv[k]]] = X[[piv[k], k]]
    for k in range(m - 1):
        X[k + 1:] -= np.outer(L[k + 1:, k], X[k])
    for k in range(m - 1, -1, -1):
        X[k] /= L[k, k]
        X[:k] -= np.outer(L[:k, k], X[k])
    return X.reshape(np.shape(B))


def oracle_blocks(oracle_mod, name):
    """The leaf self blocks of a case from the CPU oracle's block-diagonal near matrix, in the tree's leaf order"""
    kern, v, bc, ncrit = case_input(name)
    if kern == "laplace":
        o = oracle_mod.Oracle(v, bc=bc, K=STOKES_K, ncrit=ncrit, evaluator=2)
    else:
        o = oracle_mod.StokesOracle(v, K=STOKES_K, K_fine=STOKES_KFINE, ncrit=ncrit, evaluator=2, bc=bc)
    rp, col, val = o.near_csr()
    bx = o.boxes()
    leaves = sorted((int(bx["bb"][b]), int(bx["be"][b])) for b in range(len(bx["leaf"])) if bx["leaf"][b])
    dof = 1 if kern == "laplace" else 3
    blocks = []
    for bb, be in leaves:
        q = be - bb
        A = np.empty((dof * q, dof * q))
        for i in range(q):
            assert col[rp[bb + i]:rp[bb + i + 1]].tolist() == list(range(bb, be))
            rows = val[rp[bb + i]:rp[bb + i + 1]]
            if dof == 1:
                A[i] = rows
            else:
                A[3 * i:3 * i + 3] = rows.transpose(1, 0, 2).reshape(3, 3 * q)      # [pair][a][c] -> row a, column 3 pair + c
        blocks.append(A)
    return blocks


def leaf_references(A, vl):
    """Everything the forward check of one leaf needs that is not the code under test: the long-double solution z_ld of
    A z = vl (and the factors, for more right-hand sides), LAPACK's inv(A) @ vl, the float64 restatement's inverse applied to vl
    with its pivot rows, and the distance of both from z_ld."""
    fac = ld_factor(A)
    z_ld = ld_solve(fac, vl)
    lapack_inv = np.linalg.inv(A)
    emul_inv, piv, bad = gauss_jordan(A)
    assert bad is None
    nz = float(np.linalg.norm(z_ld))
    e_lapack = float(np.linalg.norm(lapack_inv @ vl - z_ld))
    e_emul = float(np.linalg.norm(emul_inv @ vl - z_ld))
    return dict(fac=fac, z_ld=z_ld, norm_z=nz, e_lapack=e_lapack, e_emul=e_emul, piv=piv, lapack_inv=lapack_inv, emul_inv=emul_inv,
                bound=4.0 * max(e_lapack, e_emul) + 4.0 * len(A) * U * nz)
