"""CPU checks of tournament pivoting's ground work: the numpy model (tests/pivot_tp_model.py) the device's mpf_dgetf2_tp and
pivot_search = 2 are compared with -- against the partial-pivoting model where the rule says the two agree, against the oracle's
no-pivot panel everywhere -- and the header's statement of the rule.  All for fused = 0."""
import os

import numpy as np
import pytest

import pivot64_model as M1
import pivot_tp_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _panel(rows, cols, kind):
    rng = np.random.default_rng(rows * 131 + cols)
    if kind == "ints":
        P = rng.integers(-3, 4, (rows, cols)).astype(np.float64)      # ties: the smallest position must win
    else:
        P = rng.standard_normal((rows, cols))
    if kind == "zero_col":                                             # every key 0 from column cols // 2 on (NaNs after it)
        P[:, cols // 2] = 0.0
    return np.asfortranarray(P)


@pytest.mark.parametrize("kind", ["normal", "ints", "zero_col"])
@pytest.mark.parametrize("rows,cols", [(1, 1), (2, 2), (33, 32), (256, 32), (200, 64)])
def test_one_group_is_partial_pivoting(rows, cols, kind):
    """rows <= 256: one group at level 0 at every sub-panel, so pivots and bits are LAPACK's."""
    P = _panel(rows, cols, kind)
    a, b = P.copy(order="F"), P.copy(order="F")
    piv_t, info_t = M.panel_tp(a, ipiv_offset=7)
    piv_p, info_p = M1.panel_piv(b, ipiv_offset=7)
    assert np.array_equal(piv_t, piv_p) and info_t == info_p
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("kind", ["normal", "ints"])
@pytest.mark.parametrize("rows,cols", [(257, 32), (300, 40), (2049, 32), (2305, 64), (1000, 256), (4099, 64)])
def test_model_panel_bits_equal_the_oracle_panel_on_permuted_rows(oracle, rows, cols, kind):
    """Unfused: the tournament panel == orc_dgetf2_npv on the panel with its rows pre-permuted by the pivots, bit for bit."""
    P = _panel(rows, cols, kind)
    got = P.copy(order="F")
    ipiv, info = M.panel_tp(got, ipiv_offset=7)
    assert ipiv.min() >= 1 + 7 and ipiv.max() <= rows + 7
    want = M.permute_rows(P, ipiv, ipiv_offset=7)
    with np.errstate(all="ignore"):
        oracle.dgetf2_npv(want)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    if kind == "normal":
        assert info == 0


def test_select_tie_and_nan_rules():
    # positions 1 and 2 tie at 3 in column 0: the smaller position wins; the NaN counts as 0
    S = np.array([[1.0, 2.0], [-3.0, 1.0], [3.0, 5.0], [np.nan, 1.0]])
    keep = S.copy()
    assert M.select(S) == [1, 2]                                # then position 2 has |5 + 1| = 6, the largest
    assert np.array_equal(S[:3], keep[:3])                      # a private copy: the stack is not changed
    # every key 0 (zeros and NaNs): the smallest position not yet chosen, step after step
    Z = np.array([[0.0, 0.0], [np.nan, 0.0], [0.0, np.nan], [0.0, 0.0]])
    assert M.select(Z) == [0, 1]
    # a NaN does not beat a number, however small
    T = np.array([[np.nan, 1.0], [1e-300, 1.0], [0.0, 2.0], [np.nan, 3.0]])
    assert M.select(T)[0] == 1
    # fewer rows than columns: every row, in pivot order
    assert M.select(np.array([[1.0, 5.0, 2.0], [4.0, 1.0, 1.0]])) == [1, 0]
    # positions are dgetf2's: taking row 2 first moves row 0 to position 2, so rows 1 and 0 (both 1 in column 1) tie with row 1 in front
    D = np.array([[1.0, 1.0], [0.0, 1.0], [2.0, 0.0], [0.0, 0.5]])
    assert M.select(D) == [2, 1]
    # ... and a zero column keeps the row that stands at position s, as idamax does
    E = np.array([[0.0, 0.0], [0.0, 0.0], [1.0, 0.0], [0.0, 0.0]])
    assert M.select(E) == [2, 1]
    for Q in (S, Z, T, D, E):                                   # one group: the model of partial pivoting takes the same rows
        piv, _ = M1.panel_piv(np.asfortranarray(Q.copy()))
        ref = list(range(Q.shape[0]))
        for j, g in enumerate(piv):
            ref[j], ref[g - 1] = ref[g - 1], ref[j]
        assert M.select(Q) == ref[:len(piv)]


def test_the_rules_can_be_told_apart():
    """300 x 40: two groups (256 + 44 rows), and the tournament takes other rows than partial pivoting."""
    P = _panel(300, 40, "normal")
    a, b = P.copy(order="F"), P.copy(order="F")
    piv_t, _ = M.panel_tp(a)
    piv_p, _ = M1.panel_piv(b)
    assert not np.array_equal(piv_t, piv_p)
    assert np.abs(np.tril(b, -1)).max() <= 1.0


@pytest.mark.parametrize("n,nb", [(515, 128)])
def test_factor_model_residual_and_scale_invariance(n, nb):
    A = np.random.default_rng(n).standard_normal((n, n))
    LU, ipiv = M.factor_tp(A, nb)
    LU1, ipiv1 = M1.factor_piv(A, nb)
    r2, r1 = M.plu_residual(A, LU, ipiv), M1.plu_residual(A, LU1, ipiv1)
    print(f"||PA - LU||_F / ||A||_F: tournament {r2:.2e}, partial pivoting {r1:.2e}, max |l_ij| {np.abs(np.tril(LU, -1)).max():.2f}")
    assert r2 <= 8.0 * r1
    s = 2.0 ** -40
    LUs, ipivs = M.factor_tp(A * s, nb)
    assert np.array_equal(ipiv, ipivs)


def test_header_documents_the_rule(mpf):
    hdr = open(os.path.join(ROOT, "include", "mpf_c.h")).read()
    assert "int mpf_dgetf2_tp(" in hdr
    assert "2: tournament pivoting" in hdr
    assert "MPF_PIVOT_FP64=2" in hdr
    assert "mpf_dgetf2_tp" in mpf.C_ABI_SYMBOLS
