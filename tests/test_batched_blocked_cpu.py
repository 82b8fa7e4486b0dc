"""CPU tests of the blocked loop behind mpf_getrf_batched_blocked (tests/batched_blocked_model.py): for any panel width the blocked
right-looking LU gives the pivots, info and bits of the unblocked batched_model.getrf_model, fused and unfused -- the claim the
entry point's contract stands on (include/mpf_c.h).  No tolerance anywhere: bits, with NaN positions compared as positions."""
import functools

import numpy as np
import pytest

import batched_blocked_model as BM
import batched_model as M

SIZES = [1, 5, 33, 70, 129, 161]
WIDTHS = [8, 16, 32]
KINDS = ["random", "ints", "singular"]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same_with_nans(got, want):
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(np.where(nan, 0.0, got)), _bits(np.where(nan, 0.0, want)))


def _matrix(n, kind):
    rng = np.random.default_rng(7919 * n + KINDS.index(kind))
    A = rng.standard_normal((n, n))
    if kind == "ints":                      # many exact ties: the first maximum must win in every panel
        A = rng.integers(-3, 4, (n, n)).astype(np.float64)
    elif kind == "singular":                # a zero column: info, then Inf / NaN in everything behind it
        A[:, n // 2] = 0.0
    return np.asfortranarray(A)


def _gemm(oracle, fused):
    return (lambda Cm, L, U: oracle.dgemm_minus(Cm, L, U)) if fused else None


@functools.lru_cache(maxsize=None)
def _unblocked(n, kind, fused, oracle):
    return M.getrf_model(_matrix(n, kind), _gemm(oracle, fused))


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nb", WIDTHS)
@pytest.mark.parametrize("n", SIZES)
def test_blocked_equals_unblocked(oracle, n, nb, kind, fused):
    LU, ipiv, info = BM.getrf_blocked_model(_matrix(n, kind), nb, _gemm(oracle, fused))
    LU0, ipiv0, info0 = _unblocked(n, kind, fused, oracle)
    assert info == info0 and (info == n // 2 + 1 if kind == "singular" else info == 0)
    assert np.array_equal(ipiv, ipiv0)
    assert _same_with_nans(LU, LU0)
    if kind != "singular":
        assert not np.isnan(LU).any()


@pytest.mark.parametrize("fused", [False, True])
def test_a_width_that_is_no_power_of_two(oracle, fused):
    LU, ipiv, info = BM.getrf_blocked_model(_matrix(70, "random"), 7, _gemm(oracle, fused))
    LU0, ipiv0, info0 = _unblocked(70, "random", fused, oracle)
    assert info == info0 == 0 and np.array_equal(ipiv, ipiv0) and np.array_equal(_bits(LU), _bits(LU0))


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("nb", WIDTHS)
def test_a_dropped_term_at_a_seam_is_noticed(oracle, nb, fused):
    """The comparison can fail: the update behind the first panel without its last term (the one next to the seam)."""
    n = 70
    LU, _, _ = BM.getrf_blocked_model(_matrix(n, "random"), nb, _gemm(oracle, fused), drop=(0, nb - 1))
    LU0, _, _ = _unblocked(n, "random", fused, oracle)
    assert np.array_equal(_bits(LU[:nb]), _bits(LU0[:nb]))            # the first block row is final before the omission
    assert not np.array_equal(_bits(LU), _bits(LU0))
