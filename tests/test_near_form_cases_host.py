"""The case table of tests/near_form_cases.py held to what it claims, from the CPU oracle alone: every case builds, the one-row
leaves, the leaves of more than 64 rows, the area ratios, the cases without an M2L pair and the share of near pairs inside the
near-regime band d^2 <= 8 A are there, and the oracle's own near-field product obeys the row bound against the long-double
reference.  An edit of the table that loses an edge fails here, not silently on the GPU."""
import numpy as np
import pytest

import near_form_cases as nfc

ALL = sorted(nfc.LAPLACE) + sorted(nfc.STOKES)


@pytest.fixture(scope="module")
def oracles(oracle_mod):
    return {c: nfc.make_oracle(oracle_mod, c, False) for c in ALL}


def _area_ratio(o):
    a = o.panels()["area"]
    return float(a.max() / a.min())


def _band_share(o):
    """share of the near pairs OTHER than a panel with itself whose centres are within the near regime of the source,
    |c_t - c_s|^2 <= 8 A_s (kernels_near.hip, mf_listed), among all near pairs"""
    rp, col, _ = o.near_csr()
    pn = o.panels()
    c, area = pn["center"], pn["area"]
    perm = o.perm().astype(np.int64)
    rows = np.repeat(np.arange(o.n), np.diff(rp))
    t, s = perm[rows], perm[col.astype(np.int64)]
    d2 = ((c[t] - c[s]) ** 2).sum(axis=1)
    return float(((d2 <= 8.0 * area[s]) & (t != s)).sum() / len(col))


@pytest.mark.parametrize("case", ALL)
def test_case_builds_with_the_seeded_input(oracles, case):
    o = oracles[case]
    v, _, _ = nfc.case_input(case, False)
    v2, bc, _ = nfc.case_input(case, True)
    assert np.array_equal(v, v2) and o.n == len(v) <= 900              # the same soup on every call; every GPU test stays small
    assert bc.dtype == np.uint8 and 0 < bc.sum() < len(v)
    rows = nfc.leaf_rows(o)
    assert sum(nr for _, nr in rows) == o.n and o.stats()["leaves"] == len(rows)
    X, names = nfc.vectors(o, case)
    assert X.shape == (5, o.n * (3 if nfc.is_stokes(case) else 1)) and len(names) == 5
    assert [(X[k] != 0).sum() for k in (2, 3, 4)] == [1, 1, 1] and len({int(np.argmax(X[k])) for k in (2, 3, 4)}) == (3 if o.n > 2 else 2)
    assert np.abs(X[1]).max() > 1e6 * np.sort(np.abs(X[1]))[-2]         # one entry stands 1e8 above the others


def test_leaf_sizes(oracles):
    rows = {c: [nr for _, nr in nfc.leaf_rows(oracles[c])] for c in ALL}
    assert rows[101].count(1) >= 50 and max(rows[101]) <= 8
    assert min(rows[107]) == 1 and min(rows[201]) == 1
    for c in (102, 108, 203):
        assert max(rows[c]) > 64, (c, max(rows[c]))
    assert max(rows[203]) > 128                                          # more than one chunk of 128 source panels in a self block
    assert len(rows[106]) == 1 and rows[106] == [2]
    assert len(rows[105]) > 1
    # row blocks of 24 (matrix-free), 5 (Stokes hybrid) and items of 60 / 64 rows: leaves that are no multiple of either
    assert any(nr % 24 and nr > 24 for nr in rows[102]) and any(nr % 5 and nr > 60 for nr in rows[203])


def test_column_counts_are_ragged(oracles):
    """columns of a leaf's rows that are no multiple of 2, 4, 64 or 128 (row padding, float padding, lanes, LDS chunks)"""
    for c in (101, 103, 107, 201):
        rp, _, _ = oracles[c].near_csr()
        ncols = np.unique(np.diff(rp))
        assert (ncols % 2 == 1).any() and (ncols % 4 == 2).any() and (ncols > 128).any(), c
        assert all((ncols % k != 0).any() for k in (64, 128))


def test_area_ratios(oracles):
    for c in (101, 103):
        assert _area_ratio(oracles[c]) >= 1000.0, c


def test_far_field_presence(oracles):
    assert (105 in nfc.NO_FAR_FIELD) and (106 in nfc.NO_FAR_FIELD)
    for c in ALL:
        st = oracles[c].stats()
        assert (st["m2l_pairs"] == 0) == (c in nfc.NO_FAR_FIELD), c
        assert (st["p2p_pairs"] == st["leaves"] ** 2) == (c in nfc.NO_FAR_FIELD), c      # the rule of plan.hip's f32_premise
    assert oracles[103].stats()["levels"] >= 6


def test_band_share(oracles):
    for c in (101, 105):
        assert _band_share(oracles[c]) >= 0.01, c


def test_near_only_evaluators_list_the_same_near_field(oracle_mod, oracles):
    """the cases without a far field run the float form under the LOCAL evaluator: the same near matrix"""
    for c in nfc.NO_FAR_FIELD:
        a, b = oracles[c].near_csr(), nfc.make_oracle(oracle_mod, c, False, evaluator=1).near_csr()
        assert all(np.array_equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("case", sorted(nfc.LAPLACE))
def test_oracle_near_only_obeys_the_row_bound(oracle_mod, oracles, case, mixed):
    """The oracle's own double-precision product of the same matrix: no entry error at all, m_i 2^-53 alone (measured: 0.53
    of it at the most, on the two panels of (106); below 0.2 on every other case)."""
    o = nfc.make_oracle(oracle_mod, case, True) if mixed else oracles[case]
    X, names = nfc.vectors(o, case)
    r, s, m = nfc.reference(o, X)
    assert (m >= 1).all() and m.sum() == o.stats()["near_nnz"]
    for k, name in enumerate(names):
        y = o.near_only(X[k])
        q = nfc.worst_ratio(y, r[k], nfc.row_bound(s[k], m, eps_entry=0.0))
        print("case %d %s %s: oracle near_only / (m 2^-53 |A||x|) = %.3f" % (case, "mixed" if mixed else "potential", name, q))
        assert q <= 1.0, (case, name, q)


def test_rows_cancel(oracles):
    """the rows a global norm would hide: |r_i| far below (|A| |x|)_i under the normal vector"""
    for c in (101, 102, 107):
        o = oracles[c]
        X, _ = nfc.vectors(o, c)
        r, s, _ = nfc.reference(o, X[:1])
        assert (np.abs(r[0]).astype(np.float64) / s[0]).min() < 1e-2, c


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("case", sorted(nfc.STOKES))
def test_stokes_reference_is_the_oracle_matrix(oracle_mod, oracles, case, mixed):
    """The Stokes reference against a plain double product of near_csr's blocks (the oracle has no Stokes near_only)"""
    o = nfc.make_oracle(oracle_mod, case, True) if mixed else oracles[case]
    X, _ = nfc.vectors(o, case)
    r, s, m = nfc.reference(o, X)
    rp, col, val = o.near_csr()
    perm = o.perm().astype(np.int64)
    assert m.sum() == 9 * len(col)
    for k in range(len(X)):
        xt = X[k].reshape(o.n, 3)[perm]
        y = np.zeros((o.n, 3))
        for t in range(o.n):
            y[perm[t]] = np.einsum("jac,jc->a", val[rp[t]:rp[t + 1]], xt[col[rp[t]:rp[t + 1]].astype(np.int64)])
        assert nfc.worst_ratio(y.reshape(-1), r[k], nfc.row_bound(s[k], m, eps_entry=0.0)) <= 1.0
