"""CPU tests of the batched inverse and determinant (include/mpf_c.h: mpf_getri_batched, mpf_getdet_batched): the exports, and the
numpy model the GPU tests compare bits with (tests/batched_inv_model.py)."""
import functools

import numpy as np
import pytest

import batched_inv_model as MI
import batched_model as M

SIZES = [1, 2, 3, 7, 8, 9, 16, 17, 31, 32, 33, 63, 64, 65, 100, 127, 128]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _factors(n, kind):
    """(A, LU, ipiv, 0) of a random matrix; "ints": the first of a fixed sequence of small-integer matrices that is not singular."""
    rng = np.random.default_rng(n * 7 + (kind == "ints"))
    while True:
        A = rng.integers(-3, 4, (n, n)).astype(np.float64) if kind == "ints" else rng.standard_normal((n, n))
        LU, ipiv, info = M.getrf_model(A)
        if info == 0:
            return A, LU, ipiv, info


def test_library_and_context_have_the_batched_inverse(mpf):
    mpf.build()
    L = mpf.load_library()
    for name in ("mpf_getri_batched", "mpf_getdet_batched"):
        assert name in mpf.C_ABI_SYMBOLS and hasattr(L, name), name
    for name in ("getri_batched", "getdet_batched", "inv_batched", "slogdet_batched"):
        assert callable(getattr(mpf.MPFContext, name, None)), name


@pytest.mark.parametrize("kind", ["normal", "ints"])
@pytest.mark.parametrize("n", SIZES)
def test_skipping_structural_zeros_changes_no_bit(n, kind):
    """The solve on an identity and the chain that starts every column at its one agree bit for bit, the signs of zeros included
    (small integers: many exact zeros among the factors and the results)."""
    _, LU, ipiv, info = _factors(n, kind)
    assert info == 0 and np.all(np.isfinite(LU)) and np.all(np.diag(LU) != 0.0)
    full, skip = MI.getri_model(LU, ipiv), MI.getri_model_skipping(LU, ipiv)
    assert np.array_equal(_bits(full), _bits(skip)), (n, kind)


def test_start_rows_are_where_the_identity_goes():
    _, LU, ipiv, _ = _factors(17, "normal")
    q = MI.start_rows(ipiv)
    P = M.getrs_model(np.eye(17), np.asarray(ipiv), np.eye(17))       # unit factors: the interchanges alone
    assert sorted(q.tolist()) == list(range(17))
    for k in range(17):
        assert P[q[k], k] == 1.0 and np.count_nonzero(P[:, k]) == 1


def test_model_inverse_is_accurate_on_the_end_to_end_inputs():
    """dget03 on both sides, LAPACK's dtest.in threshold 30 (as test_getri_cpu.py)."""
    A = np.random.default_rng(4848).standard_normal((64, 48, 48))      # test_gpu_batched.end_to_end_inputs()'s matrices
    worst = 0.0
    for b in range(A.shape[0]):
        LU, ipiv, info = M.getrf_model(A[b])
        assert info == 0
        X = MI.getri_model(LU, ipiv)
        worst = max(worst, MI.dget03_ratio(A[b], X, True), MI.dget03_ratio(A[b], X, False))
    print(f"model inverse, 64 matrices of order 48: worst dget03 ratio {worst:.3f}")
    assert worst <= 30.0


@pytest.mark.parametrize("n", [5, 128])
def test_model_inverse_is_accurate_at_the_ends(n):
    A, LU, ipiv, info = _factors(n, "normal")
    assert info == 0
    X = MI.getri_model_skipping(LU, ipiv)
    ratio = max(MI.dget03_ratio(A, X, True), MI.dget03_ratio(A, X, False))
    print(f"model inverse n={n}: dget03 ratio {ratio:.3f}")
    assert ratio <= 30.0


def test_determinant_model_is_one_chunk():
    """n <= 128 < 256: mpf_getdet's order has one chunk, and mant 2^expo is the determinant."""
    A, LU, ipiv, _ = _factors(9, "normal")
    mant, expo = MI.getdet_model(np.diag(LU), ipiv)
    assert 0.5 <= abs(mant) < 1.0
    assert abs(mant * 2.0 ** expo - np.linalg.det(A)) <= 1e-12 * abs(np.linalg.det(A))
    assert MI.getdet_model([2.0 ** -1000] * 128, np.arange(1, 129)) == (0.5, 128 * -1000 + 1)
