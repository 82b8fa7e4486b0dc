"""CPU checks of the batched LU's ground work (include/mpf_c.h: mpf_getrf_batched, mpf_getrs_batched): the library exports both entry
points, and the numpy restatement the GPU tests compare bits against (tests/batched_model.py) is itself right."""
import numpy as np
import pytest

import batched_model as M


def test_library_exports_the_batched_entry_points(mpf):
    mpf.build()
    L = mpf.load_library()
    for name in ("mpf_getrf_batched", "mpf_getrs_batched"):
        assert name in mpf.C_ABI_SYMBOLS
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes is not None
    assert hasattr(mpf.MPFContext, "getrf_batched") and hasattr(mpf.MPFContext, "getrs_batched")
    assert hasattr(mpf.MPFContext, "solve_batched") and hasattr(mpf.MPFContext, "colmajor_batch")


def test_layout_rule_of_the_python_side(mpf):
    """Which (batch, rows, cols) tensors go to the library as they stand: column-major matrices, padded or not; torch's row-major
    default and overlapping matrices are copied."""
    import torch
    lay = mpf.MPFContext._batch_layout
    assert lay(torch.empty(3, 5, 4).transpose(1, 2)) == (4, 20)                     # colmajor_batch's own layout
    assert lay(torch.empty(3, 4, 4)) is None                                         # row-major
    assert lay(torch.empty(1, 1, 1)) == (1, 1)
    buf = torch.empty(3 * (7 * 4 + 11))
    assert lay(torch.as_strided(buf, (3, 4, 4), (7 * 4 + 11, 1, 7))) == (7, 39)      # lda = n + 3, strideA = lda n + 11
    assert lay(torch.as_strided(buf, (3, 4, 4), (8, 1, 4))) is None                  # matrices overlap
    assert lay(torch.as_strided(buf, (1, 4, 4), (0, 1, 4))) == (4, 16)               # one matrix: its batch stride means nothing
    assert lay(torch.as_strided(buf, (3, 4, 1), (4, 1, 1))) == (4, 4)                # one column: ld = rows


@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("n", [1, 2, 5, 33])
def test_model_solves_the_system(n, trans):
    rng = np.random.default_rng(100 + n)
    A = rng.standard_normal((n, n)) + n * np.eye(n)            # well conditioned
    B = rng.standard_normal((n, 3))
    LU, ipiv, info = M.getrf_model(A)
    assert info == 0 and ipiv[n - 1] == n
    X = M.getrs_model(LU, ipiv, B, trans)
    op = A.T if trans else A
    assert np.abs(op @ X - B).max() <= 1e-12 * np.abs(B).max()
    # a vector goes in and comes out as a vector
    x = M.getrs_model(LU, ipiv, B[:, 0], trans)
    assert x.shape == (n,) and np.array_equal(x, X[:, 0])


def test_model_pivots_on_a_matrix_with_ties():
    """Worked by hand (LAPACK dgetf2: the FIRST maximum of a column wins).
    Column 0 = (2, -4, 4): rows 1 and 2 tie at 4, row 1 wins -> ipiv[0] = 2; multipliers -0.5 and -1.
    After the step the rest is [[2, 3], [2, 2]] (rows 1, 2): a tie at 2, the row in place wins -> ipiv[1] = 2; multiplier 1.
    The last pivot entry is n."""
    A = np.array([[2.0, 1.0, 1.0],
                  [-4.0, 2.0, 4.0],
                  [4.0, 0.0, -2.0]])
    LU, ipiv, info = M.getrf_model(A)
    assert ipiv.tolist() == [2, 2, 3] and info == 0
    want = np.array([[-4.0, 2.0, 4.0],
                     [-0.5, 2.0, 3.0],
                     [-1.0, 1.0, -1.0]])
    assert np.array_equal(LU, want)
    # a zero column: p = j, info names it, the division by zero is carried out
    Z = np.array([[1.0, 0.0], [0.5, 0.0]])
    LUz, ipz, infoz = M.getrf_model(Z)
    assert ipz.tolist() == [1, 2] and infoz == 2


@pytest.mark.parametrize("n", [2, 5, 9])
def test_transposed_interchanges_invert_the_plain_ones(n):
    """On a permutation matrix every operation is exact: solving with A, then multiplying back, returns B bit for bit, for both
    values of trans -- the interchange order of trans = 1 is the inverse of trans = 0's."""
    rng = np.random.default_rng(n)
    A = np.eye(n)[rng.permutation(n)]
    B = rng.integers(-9, 10, (n, 4)).astype(np.float64)
    LU, ipiv, info = M.getrf_model(A)
    assert info == 0 and np.array_equal(LU, np.eye(n))
    for trans in (False, True):
        X = M.getrs_model(LU, ipiv, B, trans)
        assert np.array_equal((A.T if trans else A) @ X, B), trans
    # the two orders undo each other on the factors alone
    Y = M.getrs_model(LU, ipiv, M.getrs_model(LU, ipiv, B, False), True)
    assert np.array_equal(Y, B)
