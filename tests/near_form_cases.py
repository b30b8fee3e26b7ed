"""Inputs and the host reference shared by tests/test_near_form_cases_host.py and tests/test_gpu_near_forms_soup.py: fixed, seeded
triangle soups -- clustered, stretched, panel areas three orders of magnitude apart, leaves of one row up to more than a hundred --
for every form of the near field (streamed, matrix-free, hybrid, float, multi-vector), and the near-field product of the CPU oracle's
own matrix (Oracle.near_csr / StokesOracle.near_csr) accumulated in np.longdouble, row by row.

The row bound every form is held to,

    |y_i - r_i| <= (eps_entry + m_i 2^-53) (|A| |x|)_i,

is derived, not measured: m_i 2^-53 is the worst case of a double sum of m_i terms in any order, with or without FMA (m_i: the
stored entries of row i; Stokes: 3 per block); eps_entry = 1e-13 is the project's tolerance for a near entry against the oracle's
(TOL_ENTRY of tests/test_gpu_parity.py).  The float form adds 2^-24, the one float rounding of an entry.

eps_entry on these soups.  1e-13 holds entry by entry for POTENTIAL targets (int 1/r: worst measured 5.9e-15).  It does not for
the entries that are sums of terms of both signs -- dG/dn of a NORMAL_DERIV target, sum w A (d . n) / r^3, where a target close to
the source's plane leaves d . n a small difference, and every value of a Stokes 3 x 3 block, sum w A (delta r^2 + d_a d_c) / r^3
(TRACTION: (d . n) d_a d_c / r^5).  Against an evaluation of the same rule in np.longdouble from the same double vertices the
device and the oracle are equally far off on the worst entries (MI355X; device / oracle, relative): (102) mixed 7.0e-11 / 6.4e-11
at a cancellation sum|terms| / |entry| of 2.4e5; (108) mixed 3.6e-11 / 3.5e-11; (202) velocity 2.1e-11 / 3.0e-11; (203) mixed
7.7e-11 / 7.6e-11 -- both sit at the rounding level of the sum, neither is the further one.  So these entries take a measured
tolerance, 4 x the worst |device - oracle| / |oracle| over all cases:
    NORMAL_DERIV rows (Laplace)   worst 1.20e-11 ((102) mixed)      -> EPS_ENTRY_DN     = 4.8e-11
    Stokes rows, entry by entry   worst 1.70e-11 ((202) velocity)   -> EPS_ENTRY_STOKES = 6.8e-11
(a Stokes row against its LARGEST entry, as tests/test_stokes.py holds it, stays within 1e-13: worst 1.2e-14).  POTENTIAL rows
keep 1e-13, also inside a plan of mixed flags.

Not reached here: NearForm::Plain on a Laplace plan (near_spmv_kernel with one unknown per panel) needs a leaf with more than 256
runs of source rows; no switch forces it and no known input reaches it.  The Stokes 9-value rows (FMMBEM_STOKES_SYM=0) run that
kernel and are covered."""
import numpy as np

U53 = 2.0 ** -53
EPS_ENTRY = 1e-13                  # TOL_ENTRY of tests/test_gpu_parity.py
EPS_ENTRY_DN = 4.8e-11             # measured, see above
EPS_ENTRY_STOKES = 6.8e-11
EPS_F32 = 2.0 ** -24

# (seed, n, clusters, stretch, size_spread, ncrit), theta = 0.5; what each gives is held by tests/test_near_form_cases_host.py
LAPLACE = {
    101: (101, 700, 3, 1.0, 2.0, 8),        # 281 leaves of 1-8 rows, 101 of them one row; area ratio 2906; 14967 M2L pairs
    102: (102, 900, 1, 3.0, 1.0, 126),      # 20 leaves, up to 119 rows; the near matrix is 98 % of n^2
    103: (103, 333, 6, 10.0, 2.0, 32),      # 6 levels, stretched; area ratio 2803
    105: (105, 65, 1, 1.0, 2.0, 64),        # 7 leaves, no M2L pair at all
    106: (106, 2, 1, 1.0, 0.0, 8),          # two panels, one leaf
    107: (107, 850, 4, 3.0, 2.0, 64),       # leaves of 1-59 rows; 402 M2L pairs
    108: (108, 600, 2, 1.0, 2.0, 200),      # leaves up to 116 rows
}
# (seed, n, clusters, ncrit): _soup(seed, n, clusters, 1.0, 1.0)
STOKES = {
    201: (201, 400, 3, 16),                 # leaves of 1-15 rows
    202: (202, 300, 1, 64),                 # 15-60; no M2L pair
    203: (203, 350, 2, 300),                # 3-182; three leaves, no M2L pair
}
STOKES_K, STOKES_KFINE, STOKES_MU = 4, 19, 1e-3
# Every pair of leaves is a near pair: no M2L pair, no far field.  Under the FMM evaluator such a plan takes near_f32_max_p as 0
# (plan.hip, f32_premise), so the float form meets these inputs under the LOCAL evaluator, which keeps the option and lists the
# same near field.
NO_FAR_FIELD = (105, 106, 202, 203)


def _soup(seed, n, clusters, stretch, size_spread):
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-1, 1, (clusters, 3)) * np.array([stretch, 1.0, 1.0 / stretch])
    which = rng.integers(0, clusters, n)
    c = centres[which] + rng.normal(0, 0.15, (n, 3))
    h = 0.02 * np.exp(rng.uniform(-size_spread, size_spread, n))
    e0, e1 = rng.normal(size=(n, 3)), rng.normal(size=(n, 3))
    e0 /= np.linalg.norm(e0, axis=1, keepdims=True)
    e1 -= (e1 * e0).sum(axis=1, keepdims=True) * e0
    e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
    return np.stack([c, c + h[:, None] * e0, c + h[:, None] * (0.3 * e0 + e1)], axis=1)


def is_stokes(case):
    return case in STOKES


def case_input(case, mixed):
    """(vertices, flags or None, ncrit).  mixed: rng(seed + 1).random(n) < 0.5 picks the panels with flag 1 (NORMAL_DERIV / TRACTION)"""
    if case in LAPLACE:
        seed, n, clusters, stretch, spread, ncrit = LAPLACE[case]
    else:
        seed, n, clusters, ncrit = STOKES[case]
        stretch, spread = 1.0, 1.0
    v = _soup(seed, n, clusters, stretch, spread)
    bc = (np.random.default_rng(seed + 1).random(n) < 0.5).astype(np.uint8) if mixed else None
    return v, bc, ncrit


def eps_rows(case, mixed):
    """eps_entry of every unknown's row, the caller's order (module docstring)"""
    v, bc, _ = case_input(case, mixed)
    if case in STOKES:
        return np.full(3 * len(v), EPS_ENTRY_STOKES)
    return np.where(bc != 0, EPS_ENTRY_DN, EPS_ENTRY) if mixed else np.full(len(v), EPS_ENTRY)


def make_oracle(oracle_mod, case, mixed, K=None, evaluator=0, complete_l2l=False):
    v, bc, ncrit = case_input(case, mixed)
    if case in LAPLACE:
        return oracle_mod.Oracle(v, bc=bc, K=3 if K is None else K, ncrit=ncrit, evaluator=evaluator, complete_l2l=complete_l2l)
    return oracle_mod.StokesOracle(v, K=STOKES_K if K is None else K, K_fine=STOKES_KFINE, mu=STOKES_MU, ncrit=ncrit, evaluator=evaluator,
                                   complete_l2l=complete_l2l, bc=bc)


def make_plan(fb, case, mixed, K=None, p_max=8, evaluator="fmm", **options):
    """The device plan of a case.  options: sparse_local, near_stream_fraction, stokes_batch_width (FMMOptions fields) and
    near_f32_max_p (FMM_plan's own).  evaluator "local": the LOCAL evaluator (near field only)."""
    v, bc, ncrit = case_input(case, mixed)
    opts = fb.FMMOptions()
    opts.set_max_per_box(ncrit)
    if evaluator == "local":
        opts.lazy_evaluation, opts.local_evaluation = False, True
    f32 = options.pop("near_f32_max_p", 0)
    for name, value in options.items():
        assert hasattr(opts, name), name
        setattr(opts, name, value)
    if case in LAPLACE:
        kern = fb.LaplaceSphericalBEM(p_max, 3 if K is None else K)
    else:
        kern = fb.StokesSphericalBEM(p_max, STOKES_K if K is None else K, STOKES_MU)
        kern.set_Kfine(STOKES_KFINE)
    return fb.FMM_plan(kern, v, opts, bc=bc, p_max=p_max, near_f32_max_p=f32)


def near_product(plan, x):
    """fmmbem_plan_near_device: the near field alone, caller's order in and out"""
    import torch
    xd = torch.from_numpy(np.array(x, dtype=np.float64).reshape(-1)).to("cuda:%d" % plan.device)
    yd = torch.full_like(xd, np.nan)                                      # a row the near field does not write shows
    plan.near_device(xd.data_ptr(), yd.data_ptr(), torch.cuda.current_stream(xd.device).cuda_stream)
    torch.cuda.synchronize()
    return yd.cpu().numpy()


def leaf_rows(o):
    """(first tree-order row, rows) of every leaf, in tree order"""
    bx = o.boxes()
    return sorted((int(bx["bb"][b]), int(bx["be"][b] - bx["bb"][b])) for b in range(len(bx["leaf"])) if bx["leaf"][b])


def dense_near(o):
    """The oracle's near matrix in the CALLER's order of unknowns, dense, in np.longdouble (the cases are 900 unknowns at the most;
    Stokes: 1200), and the stored entries per row m_i.  near_csr is in tree order: perm()[tree position] = panel."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "np.longdouble is no extended type on this host: the reference would be double"
    rp, col, val = o.near_csr()
    perm = o.perm().astype(np.int64)
    dof = 1 if val.ndim == 1 else 3
    n = o.n
    A = np.zeros((n * dof, n * dof), dtype=np.longdouble)
    m = np.zeros(n * dof, dtype=np.int64)
    for t in range(n):
        cs = perm[col[rp[t]:rp[t + 1]].astype(np.int64)]
        i = perm[t]
        if dof == 1:
            A[i, cs] = val[rp[t]:rp[t + 1]]
        else:
            blk = val[rp[t]:rp[t + 1]]                                      # [pair][a][c]
            for a in range(3):
                for c in range(3):
                    A[3 * i + a, 3 * cs + c] = blk[:, a, c]
        m[dof * i:dof * i + dof] = dof * len(cs)
    return A, m


def vectors(o, seed):
    """The input vectors of a case, (5, unknowns) in the caller's order, and their names: one standard normal vector, one with a
    single entry scaled by 1e8, and three unit vectors -- the first tree-order panel, the last, and one in the middle of the leaf
    with the most rows (Stokes: components 0, 2, 1 of those panels).  Under a unit vector a row is ONE entry: a wrong column
    cannot hide in a sum."""
    n = o.n
    dof = 3 if hasattr(o, "mu") else 1
    rng = np.random.default_rng(seed + 7)
    X = np.zeros((5, n * dof))
    X[0] = rng.standard_normal(n * dof)
    X[1] = rng.standard_normal(n * dof)
    X[1, int(np.argmax(np.abs(X[1])))] *= 1e8
    perm = o.perm().astype(np.int64)
    r0, nr = max(leaf_rows(o), key=lambda leaf: leaf[1])
    for k, (t, comp) in enumerate(((0, 0), (n - 1, 2), (r0 + nr // 2, 1))):
        X[2 + k, dof * perm[t] + (comp if dof == 3 else 0)] = 1.0
    return X, ("normal", "one entry x 1e8", "e_first", "e_last", "e_mid_largest_leaf")


def reference(o, X):
    """r = A x in np.longdouble, the row sums (|A| |x|)_i (rounded to double once) and the stored entries per row m_i, for
    every row of X ((k, unknowns), the caller's order): (k, unknowns), (k, unknowns), (unknowns,)"""
    A, m = dense_near(o)
    Xl = np.asarray(X, dtype=np.longdouble)
    r = Xl @ A.T
    s = np.abs(Xl) @ np.abs(A).T
    return r, s.astype(np.float64), m


def row_bound(s, m, eps_entry=EPS_ENTRY, extra=0.0):
    return (eps_entry + extra + m * U53) * s


def worst_ratio(y, r, bound):
    """max_i |y_i - r_i| / bound_i; a row whose bound is 0 (no entry meets a non-zero of x) must be exactly 0: inf otherwise"""
    d = np.abs(np.asarray(y, dtype=np.longdouble).reshape(np.shape(r)) - r).astype(np.float64)
    if not np.all(np.isfinite(d)):
        return float("inf")
    q = np.where(bound > 0, d / np.where(bound > 0, bound, 1.0), np.where(d > 0, np.inf, 0.0))
    return float(q.max())


_REFERENCES = {}


def case_reference(oracle_mod, case, mixed, K=None, evaluator=0):
    """The oracle of a case (complete L2L list, as the device's default), its input vectors and the long-double reference of
    its near field: computed once per process, shared, never written to"""
    key = (case, bool(mixed), K, evaluator)
    if key not in _REFERENCES:
        o = make_oracle(oracle_mod, case, mixed, K=K, evaluator=evaluator, complete_l2l=True)
        X, names = vectors(o, case)
        r, s, m = reference(o, X)
        for a in (X, r, s, m):
            a.setflags(write=False)
        eps = eps_rows(case, mixed)
        eps.setflags(write=False)
        _REFERENCES[key] = dict(o=o, X=X, names=names, r=r, s=s, m=m, eps=eps)
    return _REFERENCES[key]


def near_ratios(plan, R, extra=0.0):
    """worst |y_i - r_i| / bound_i of the plan's near field, per input vector of the reference R"""
    return {name: worst_ratio(near_product(plan, R["X"][k]), R["r"][k], row_bound(R["s"][k], R["m"], R["eps"], extra))
            for k, name in enumerate(R["names"])}
