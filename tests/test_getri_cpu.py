"""CPU tests of the numpy restatement of mpf_getri and mpf_getdet (tests/getri_model.py).

The inverse model must keep LAPACK's own test ratio (dget03, threshold 30 of dtest.in) at the block sizes 4 and 256 on the shapes the GPU
tests use; the determinant model must equal exact integer arithmetic, stay finite where the plain product leaves fp64's range, and take
its sign from the pivots."""
from fractions import Fraction

import numpy as np
import pytest

import getri_model as M

SIZES = [1, 2, 7, 255, 256, 257, 600, 1031]
THRESH = 30.0   # LAPACK dtest.in


gen_matrix = M.gen_matrix


_factors = {}


def factors(n, kind):
    if (n, kind) not in _factors:
        A = gen_matrix(n, kind)
        _factors[(n, kind)] = (A,) + M.getrf(A)
    return _factors[(n, kind)]


CASES = [(n, "gen") for n in SIZES] + [(n, "svd") for n in SIZES if n > 2]


@pytest.mark.parametrize("nb", [4, 256])
@pytest.mark.parametrize("n,kind", CASES)
def test_model_inverse_ratio(n, kind, nb):
    A, LU, ipiv = factors(n, kind)
    X = M.getri_model(LU, ipiv, nb=nb)
    left, right = M.dget03_ratio(A, X, True), M.dget03_ratio(A, X, False)
    print(f"n={n} {kind} nb={nb}: ||I - X A|| ratio {left:.4g}, ||I - A X|| ratio {right:.4g}")
    assert left <= THRESH and right <= THRESH


def test_model_block_size_does_not_change_the_inverse_much():
    A, LU, ipiv = factors(257, "gen")
    X4, X256 = M.getri_model(LU, ipiv, nb=4), M.getri_model(LU, ipiv, nb=256)
    assert np.abs(X4 - X256).max() <= 1e-10 * np.abs(X256).max()


def test_model_scales_are_exact():
    n = 257
    A = gen_matrix(n, "gen")
    rng = np.random.default_rng(3)
    r = 2.0 ** rng.integers(-20, 21, size=n)
    c = 2.0 ** rng.integers(-20, 21, size=n)
    LU, ipiv = M.getrf(r[:, None] * A * c[None, :])
    Y = M.getri_model(LU, ipiv)
    X = M.getri_model(LU, ipiv, r=r, c=c)
    assert np.array_equal(X, c[:, None] * Y * r[None, :])
    assert M.dget03_ratio(A, X, True) <= THRESH and M.dget03_ratio(A, X, False) <= THRESH


def test_model_permutation_times_diagonal_is_exact():
    n = 600
    d = 2.0 ** (np.arange(n) % 41 - 20)
    for perm in (np.roll(np.arange(n), 1), np.arange(n)[::-1]):
        A = np.zeros((n, n))
        A[perm, np.arange(n)] = d            # A = P D
        LU, ipiv = M.getrf(A)
        want = np.zeros((n, n))
        want[np.arange(n), perm] = 1.0 / d   # D^-1 P^T
        assert np.array_equal(M.getri_model(LU, ipiv, nb=256), want)


def int_diag_case():
    """Integer diagonal whose product is exact in fp64's 53 bits (odd part 3^8 5^6 7^4 < 2^37) but far outside its range."""
    rng = np.random.default_rng(11)
    n = 700
    d = 2.0 ** rng.integers(0, 11, size=n)
    odd = [3] * 8 + [5] * 6 + [7] * 4
    pos = rng.choice(n, size=len(odd), replace=False)
    d[pos] *= np.array(odd, dtype=np.float64)
    d *= rng.choice([-1.0, 1.0], size=n)
    return d


def test_det_model_equals_exact_integer_arithmetic():
    d = int_diag_case()
    n = len(d)
    ipiv = np.arange(1, n + 1)
    mant, expo = M.getdet_model(d, ipiv)
    exact = Fraction(1)
    for v in d:
        exact *= Fraction(int(v))
    assert 0.5 <= abs(mant) < 1.0
    assert Fraction(mant) * Fraction(2) ** expo == exact
    # small case with interchanges: three swaps flip the sign
    d3 = np.array([3.0, -5.0, 7.0, 2.0])
    mant, expo = M.getdet_model(d3, [2, 3, 4, 4])
    assert Fraction(mant) * Fraction(2) ** expo == Fraction(-(3 * -5 * 7 * 2))


def test_det_model_stays_finite_outside_fp64_range():
    d = int_diag_case()
    n = len(d)
    with np.errstate(over="ignore", under="ignore"):
        assert np.isinf(np.linalg.det(np.diag(d)))
        assert np.linalg.det(np.diag(1.0 / d)) == 0.0
    for dd in (d, 1.0 / d):
        mant, expo = M.getdet_model(dd, np.arange(1, n + 1))
        assert np.isfinite(mant) and 0.5 <= abs(mant) < 1.0
        sign, logabs = M.slogdet_model(dd, np.arange(1, n + 1))
        s_np, l_np = np.linalg.slogdet(np.diag(dd))
        assert sign == s_np and abs(logabs - l_np) <= (n + 4) * 2.0 ** -52 * max(1.0, abs(l_np))


def test_det_model_sign_from_pivot_parity():
    rng = np.random.default_rng(5)
    for n in (5, 64, 257):
        A = rng.standard_normal((n, n))
        LU, ipiv = M.getrf(A)
        sign, logabs = M.slogdet_model(np.diag(LU), ipiv)
        s_np, l_np = np.linalg.slogdet(A)
        assert sign == s_np
        assert abs(logabs - l_np) <= 1e-10 * max(1.0, abs(l_np))


def test_det_model_special_values():
    assert M.getdet_model([], []) == (0.5, 1)
    assert M.getdet_model([2.0, 0.0, 3.0], [1, 2, 3]) == (0.0, 0)
    mant, expo = M.getdet_model([2.0, np.inf, 3.0], [1, 2, 3])
    assert np.isnan(mant) and expo == 0
    assert M.slogdet_model([2.0, 0.0], [1, 2]) == (0.0, -np.inf)
    # scales: det(A) = det(Dr A Dc) / (prod r prod c), an exact exponent shift
    d = np.array([3.0, 5.0, 0.75])
    r, c = np.array([2.0, 0.5, 8.0]), np.array([4.0, 4.0, 0.25])
    mant, expo = M.getdet_model(d, [1, 2, 3], r=r, c=c)
    m0, e0 = M.getdet_model(d, [1, 2, 3])
    assert mant == m0 and expo == e0 - int(np.log2(r).sum() + np.log2(c).sum())
