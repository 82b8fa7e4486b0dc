"""The model behind tests/test_gpu_hgemm_exact.py, checked on the CPU: the operand rules of contract C6 as restated in
hgemm_exact_model.py (against the oracle's C1 where the two agree, against hand-worked values where they do not), the split
family's exact recovery, the worst-case accumulator bounds, and the model's own refusal of data that is not exact."""
import itertools

import numpy as np
import pytest

import hgemm_exact_model as M


def _f16(x):
    return np.asarray(x, dtype=np.float64).astype(np.float16)


def test_split_family_splits_back_exactly():
    """Every value hi + lo / 2048 of the split family: d2h_sat gives hi, d2h_lo gives lo, and the input itself is exact in fp64."""
    for hi, lo in itertools.product(M.SPLIT_HI, M.SPLIT_LO):
        if hi == 0 and lo != 0:
            continue
        x = np.array([hi + lo / 2048.0])
        assert (x[0] - hi) * 2048.0 == lo
        h = M.d2h_sat(x)
        assert h.dtype == np.float16 and float(h[0]) == hi, (hi, lo)
        assert float(M.d2h_lo(x, h)[0]) == lo, (hi, lo)
    x, hi, lo = M.split_values(np.random.default_rng(0), (300, 70))
    h = M.d2h_sat(x)
    assert np.array_equal(h.astype(np.float64), hi) and np.array_equal(M.d2h_lo(x, h).astype(np.float64), lo)
    assert set(np.unique(hi)) == set(float(v) for v in M.SPLIT_HI) and set(np.unique(lo)) == set(float(v) for v in M.SPLIT_LO)
    assert np.all(lo[hi == 0] == 0)


def test_plain_family_is_its_own_fp16_image():
    A, B, C = M.plain_family(50, 40, 30, 3, 1)
    assert A.shape == (50, 30) and B.shape == (30, 40) and C.shape == (53, 40)
    for v, lim in ((A, 3), (B, 3), (C, 64)):
        assert np.array_equal(v, np.round(v)) and np.abs(v).max() == lim
    assert np.array_equal(M.d2h_sat(A).astype(np.float64), A)


def test_worst_case_bounds_at_k_2048():
    """All operands at their extremes, K = 2048: the accumulators stay below 2^24 and the model accepts the case."""
    k = 2048
    assert 9 * k == 18432 < M.EXACT_LIMIT
    assert 49 * k == 100352 < M.EXACT_LIMIT and 42 * k == 86016 < M.EXACT_LIMIT
    A = np.full((2, k), 3.0)
    B = np.full((k, 2), -3.0)
    assert np.array_equal(M.product_terms(A, B, False), np.full((2, 2), -9.0 * k))
    A = np.full((2, k), 7.0 + 3.0 / 2048.0)
    B = np.full((k, 2), 7.0 + 3.0 / 2048.0)
    P = M.product_terms(A, B, True)
    assert np.array_equal(P, np.full((2, 2), 49.0 * k + 42.0 * k / 2048.0))
    # fp32 C: one rounding of S + X / 2048, one of the difference
    want = np.float32(np.float32(5.0) - np.float32(49.0 * k + 42.0 * k / 2048.0))
    assert np.array_equal(M.expected(np.full((3, 2), 5.0), A, B, True, True), np.array([[want] * 2] * 2 + [[5.0] * 2]))
    assert np.array_equal(M.expected(np.full((3, 2), 5.0), A, B, True, False),
                          np.array([[5.0 - (49.0 * k + 42.0)] * 2] * 2 + [[5.0] * 2]))


C1_FLUSH = float(np.float32(6.10352e-05))      # contract C1 flushes |xf| < 6.10352e-05f: an fp32 number six ulps ABOVE 2^-14


def test_d2h_sat_is_c1_from_the_flush_threshold_up(oracle):
    """C1's threshold constant is 2^-14 (1 + 6 * 2^-23) in fp32, so C1 flushes 2^-14 itself: the two rules agree from that constant
    up (every fp16 normal number but the smallest), and 2^-14 belongs to the other test."""
    rng = np.random.default_rng(3)
    x = rng.standard_normal(200000) * np.exp2(rng.integers(-13, 20, 200000))
    assert C1_FLUSH == 2.0 ** -14 * (1 + 6 * 2.0 ** -23)
    x = np.concatenate([x[np.abs(x) >= C1_FLUSH], [C1_FLUSH, -C1_FLUSH, 2.0 ** -14 * (1 + 2.0 ** -10), 65504.0, 65519.9, 65520.0, 1e6, -1e9, 1e300, 0.0,
                                                      1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -30]])
    assert np.array_equal(M.d2h_sat(x).view(np.uint16), oracle.double_to_fp16(x))


def test_d2h_sat_keeps_what_c1_flushes(oracle):
    rng = np.random.default_rng(4)
    j = rng.integers(1, 1024, 5000)
    x = j * 2.0 ** -24 * rng.choice([-1.0, 1.0], 5000)              # every fp16 subnormal magnitude is one of these
    got = M.d2h_sat(x)
    assert np.array_equal(got.astype(np.float64), x)                 # kept, exactly
    assert np.all(oracle.double_to_fp16(x) == 0)                     # C1: flushed to +0
    t = np.array([2.0 ** -14, -2.0 ** -14])                          # the smallest normal number: kept here, flushed by C1
    assert np.array_equal(M.d2h_sat(t).view(np.uint16), [0x0400, 0x8400]) and np.all(oracle.double_to_fp16(t) == 0)
    y = rng.uniform(2.0 ** -24, 2.0 ** -14 * (1 - 2.0 ** -11), 5000)          # between them: rounded to the 2^-24 grid, ties to even
    want = np.round(y * 2.0 ** 24) * 2.0 ** -24                      # (np.round is half-to-even)
    assert np.array_equal(M.d2h_sat(y).astype(np.float64), want)


@pytest.mark.parametrize("x,want", [
    (2.0 ** -24, 2.0 ** -24), (3 * 2.0 ** -20, 3 * 2.0 ** -20), (-5 * 2.0 ** -17, -5 * 2.0 ** -17), (2.0 ** -14, 2.0 ** -14),
    (2.0 ** -14 - 2.0 ** -24, 2.0 ** -14 - 2.0 ** -24), (2.0 ** -25, 0.0), (1.5 * 2.0 ** -24, 2 * 2.0 ** -24), (2.5 * 2.0 ** -24, 2 * 2.0 ** -24),
    (1.75 * 2.0 ** -24, 2 * 2.0 ** -24), (65504.0, 65504.0), (65519.9, 65504.0), (65520.0, 65504.0), (1e6, 65504.0), (-1e9, -65504.0),
    (np.inf, 65504.0), (-np.inf, -65504.0), (1e300, 65504.0)])
def test_d2h_sat_edge_values(x, want):
    assert float(M.d2h_sat(np.array([x]))[0]) == want


def test_d2h_sat_nan_stays_nan():
    assert np.isnan(M.d2h_sat(np.array([np.nan]))[0])


@pytest.mark.parametrize("x,want", [
    (65520.0, 32768.0),            # 65504 + 32768 / 2048 = 65520: the split still carries it exactly
    (65504.0, 0.0), (65519.9, None), (1e6, 0.0), (-1e9, 0.0), (np.inf, 0.0), (-np.inf, 0.0), (np.nan, 0.0),
    (1.75 * 2.0 ** -24, -2.0 ** -15), (5.0 + 3.0 / 2048.0, 3.0), (1.0 + 2.0 ** -11, 1.0)])
def test_d2h_lo_edge_values(x, want):
    xa = np.array([x])
    hi = M.d2h_sat(xa)
    lo = float(M.d2h_lo(xa, hi)[0])
    if want is None:               # 65519.9: (x - 65504) * 2048 = 32563.2 exactly in fp64 terms, rounded to fp16's grid of 16 there
        want = float(_f16(np.float32((x - 65504.0) * 2048.0)))
        assert want == 32560.0
    assert lo == want
    if x == 65520.0:
        assert float(hi[0]) + lo / 2048.0 == 65520.0


def test_expected_raises_on_data_that_is_not_exact():
    k = 2048
    C = np.zeros((2, 2))
    with pytest.raises(AssertionError, match="not exact"):           # 2048 * 97 * 97 = 19 269 632 >= 2^24
        M.expected(C, np.full((2, k), 97.0), np.full((k, 2), 97.0), False, False)
    # (96 = 3 * 32 passes although 2048 * 96 * 96 >= 2^24: every sum is a multiple of 1024, 18432 quanta)
    assert M.expected(C, np.full((2, k), 96.0), np.full((k, 2), 96.0), False, False)[0, 0] == -96.0 * 96.0 * k
    with pytest.raises(AssertionError, match="not exact"):           # S is fine (49 k), X = 2 * 7 * 1023 k is not
        M.expected(C, np.full((2, k), 7.0 + 1023.0 / 2048.0 / 256.0), np.full((k, 2), 7.0 + 1023.0 / 2048.0 / 256.0), True, False)
    with pytest.raises(AssertionError, match="not exact"):           # mixed magnitudes: 1 + 2^-24 j needs more than 24 bits
        M.expected(C, np.array([[1.0, 2.0 ** -24], [1.0, 1.0]]), np.array([[1.0, 1.0], [3.0, 1.0]]), False, False)
    # the same values in rows of their own are exact: the quantum is per row and column
    A = np.array([[2.0 ** -24, 3 * 2.0 ** -24], [1.0, 2.0]])
    B = np.array([[1.0, 2.0], [3.0, -1.0]])
    assert np.array_equal(M.expected(C, A, B, False, False), -(A @ B))


def test_expected_nan_and_saturation_rows():
    """A NaN operand makes exactly its row of C NaN; an Inf saturates to 65504 like any large number (contract C6)."""
    A, B, C = M.plain_family(6, 5, 8, 2, 7)
    A[2, 3] = np.nan
    A[4, 1] = np.inf
    B[1, :] = 1.0
    ref = A.copy()
    ref[2, 3] = 0.0
    ref[4, 1] = 65504.0
    want = C.copy()
    want[:6] -= ref @ B
    want[2, :] = np.nan
    for split in (False, True):
        got = M.expected(C, A, B, split, False)
        assert np.array_equal(got, want, equal_nan=True) and np.isnan(got).sum() == 5
