"""numpy model of the fp16 trailing update on operands for which fp32 accumulation is EXACT (test infrastructure, not a conftest).

C -= fp16(A) fp16(B) (contract C6) accumulates exact fp16 x fp16 products in fp32.  When every product is a multiple of one
quantum q and sum |a||b| < 2^24 q, every partial sum is exactly representable in fp32 WHATEVER the order: k order, MFMA shape,
ring depth and tile walk stop mattering, the expected result is one exact matrix product, and a test can compare every element
without a tolerance.  A dropped, repeated or misplaced k-step, row or column changes an integer.

The operand rules are restated here from contract C6 and the comments above d2h_sat / d2h_lo in trailing_f16.hip -- on purpose not
taken from the oracle, whose double_to_fp16 is contract C1 (the PANEL's conversion: it flushes |x| < 2^-14 to zero):

  d2h_sat : fp64 -> fp32 (round to nearest) -> clamp to +-65504 -> fp16 (round to nearest even); subnormals KEPT, NaN stays NaN,
            +-Inf saturates like any other large number;
  d2h_lo  : lo = fp16((x - hi) * 2048) through fp32, 0 when that is NaN or beyond +-65504 (saturated / non-finite hi).

Epilogues (hgemm_ring_kernel's, and its twins in the other kernels), S = sum hi_a hi_b, X = sum (hi_a lo_b + lo_a hi_b):

  fp64 C : C - (S + X / 2048)                  every operation exact here
  fp32 C : fl32(fl32(C) - fl32(S + X / 2048))  the product by 2^-11 is exact, so an fma contraction changes nothing
  plain  : X = 0: C - S, exact in both."""
import numpy as np

FP16_MAX = 65504.0
SPLIT_SCALE = 2048.0
EXACT_LIMIT = 2.0 ** 24          # integers (multiples of the quantum) an fp32 accumulator holds exactly

SPLIT_HI = (0, 5, -5, 6, -6, 7, -7)
SPLIT_LO = (-3, -2, -1, 0, 1, 2, 3)


# ---- operand rules (contract C6) -----------------------------------------------------------------------------------------------
def d2h_sat(x):
    """fp64 -> fp16 as the GEMM converts its operands; returns a float16 array."""
    with np.errstate(over="ignore", invalid="ignore"):
        xf = np.asarray(x, dtype=np.float64).astype(np.float32)
        xf = np.where(xf > np.float32(FP16_MAX), np.float32(FP16_MAX), xf)      # (comparisons with NaN are false: NaN stays)
        xf = np.where(xf < np.float32(-FP16_MAX), np.float32(-FP16_MAX), xf)
        return xf.astype(np.float16)


def d2h_lo(x, hi):
    """The correction term of the split mode for hi = d2h_sat(x); returns a float16 array."""
    with np.errstate(over="ignore", invalid="ignore"):
        r = (np.asarray(x, dtype=np.float64) - np.asarray(hi).astype(np.float64)) * SPLIT_SCALE
        r = np.where(np.isnan(r) | (r > FP16_MAX) | (r < -FP16_MAX), 0.0, r)
        return r.astype(np.float32).astype(np.float16)


# ---- operand families -----------------------------------------------------------------------------------------------------------
def plain_family(m, n, k, pad, seed):
    """A (m x k), B (k x n) integers in [-3, 3]; C (m + pad x n) integers in [-64, 64]."""
    rng = np.random.default_rng(seed)
    A = rng.integers(-3, 4, (m, k)).astype(np.float64)
    B = rng.integers(-3, 4, (k, n)).astype(np.float64)
    C = rng.integers(-64, 65, (m + pad, n)).astype(np.float64)
    return np.asfortranarray(A), np.asfortranarray(B), np.asfortranarray(C)


def split_values(rng, shape):
    """(x, hi, lo) with x = hi + lo / 2048, hi in {0, +-5, +-6, +-7}, lo in {-3 .. 3}, lo = 0 where hi = 0.  In [4, 8) the fp16
    ulp is 2^-8 and |lo| / 2048 <= 3 * 2^-11 is below half of it: the kernel's split gives back exactly (hi, lo)."""
    hi = rng.choice(np.array(SPLIT_HI, dtype=np.float64), size=shape)
    lo = rng.integers(-3, 4, shape).astype(np.float64)
    lo[hi == 0] = 0.0
    return hi + lo / SPLIT_SCALE, hi, lo


def split_family(m, n, k, pad, seed):
    rng = np.random.default_rng(seed)
    A = split_values(rng, (m, k))[0]
    B = split_values(rng, (k, n))[0]
    C = rng.integers(-64, 65, (m + pad, n)).astype(np.float64)
    return np.asfortranarray(A), np.asfortranarray(B), np.asfortranarray(C)


# ---- exactness --------------------------------------------------------------------------------------------------------------------
def _quantum(v, axis):
    """Per row (axis = 1) or column (axis = 0): the largest power of two that divides every finite non-zero entry (1 if none)."""
    a = np.abs(np.where(np.isfinite(v), v, 0.0))
    mant, ex = np.frexp(a)                                        # a = mant * 2^ex, mant in [0.5, 1): 53-bit integer * 2^(ex - 53)
    mi = (mant * 2.0 ** 53).astype(np.int64)
    tz = np.zeros(a.shape, dtype=np.int64)
    nz = mi != 0
    low = mi[nz] & -mi[nz]                                        # lowest set bit
    tz[nz] = np.round(np.log2(low.astype(np.float64))).astype(np.int64)
    e = np.where(nz, ex - 53 + tz, np.iinfo(np.int32).max)         # a is an odd integer * 2^e
    emin = e.min(axis=axis)
    return np.exp2(np.where(emin == np.iinfo(np.int32).max, 0, emin).astype(np.float64))


def _finite(v):
    return np.where(np.isfinite(v), v, 0.0)


def _assert_exact(terms, what):
    """terms: (A-side, B-side) pairs summed in ONE accumulator.  Every product of row i and column j is a multiple of
    q_ij = min over the pairs of q(row i) q(column j); the sum of their magnitudes must stay below 2^24 q_ij.  Returns
    (bound, q): the largest magnitude any partial sum can reach, and the quantum, per element."""
    bound, q = 0.0, None
    for a, b in terms:
        bound = bound + np.abs(_finite(a)) @ np.abs(_finite(b))
        qt = np.outer(_quantum(a, 1), _quantum(b, 0))
        q = qt if q is None else np.minimum(q, qt)
    worst = float(np.max(bound / q))
    assert worst < EXACT_LIMIT, f"{what}: partial sums reach {worst:.6g} quanta, not below 2^24: fp32 accumulation is not exact"
    return bound, q


def product_terms(A, B, split):
    """P = S + X / 2048 (X = 0 for plain operands) for the operands as the kernel converts them, exact in fp64; asserts before it
    returns that both fp32 accumulators (S; X) are exact in any order and that P itself is exact in fp64."""
    Ah, Bh = d2h_sat(A), d2h_sat(B)
    ah, bh = Ah.astype(np.float64), Bh.astype(np.float64)
    # d2h_sat leaves no Inf and d2h_lo neither Inf nor NaN: a NaN operand is all that is not finite, and it makes its row (A) or
    # column (B) of the product NaN -- NaN times anything, zero included.  Set by hand: a BLAS may skip zero operands.
    nan_rows, nan_cols = np.isnan(ah).any(axis=1), np.isnan(bh).any(axis=0)
    assert not (np.isinf(ah).any() or np.isinf(bh).any())
    ah, bh = _finite(ah), _finite(bh)
    bs, qs = _assert_exact([(ah, bh)], "S = sum hi_a hi_b")
    P = ah @ bh
    if split:
        al, bl = d2h_lo(A, Ah).astype(np.float64), d2h_lo(B, Bh).astype(np.float64)
        assert np.isfinite(al).all() and np.isfinite(bl).all()
        bx, qx = _assert_exact([(ah, bl), (al, bh)], "X = sum (hi_a lo_b + lo_a hi_b)")
        # S + X / 2048 in fp64: magnitudes below bs + bx / 2048 on the grid min(qs, qx / 2048)
        assert float(np.max((bs + bx / SPLIT_SCALE) / np.minimum(qs, qx / SPLIT_SCALE))) < 2.0 ** 53
        P = P + (ah @ bl + al @ bh) / SPLIT_SCALE
    P[nan_rows, :] = np.nan
    P[:, nan_cols] = np.nan
    return P


def apply_update(C, P, c32):
    """The epilogue on rows [0, P.shape[0]) of C (taller matrices keep their other rows)."""
    m = P.shape[0]
    out = np.array(C, dtype=np.float64, order="F")
    with np.errstate(invalid="ignore"):
        if c32:
            out[:m, :] = (out[:m, :].astype(np.float32) - P.astype(np.float32)).astype(np.float64)
        else:
            out[:m, :] = out[:m, :] - P
    return out


def expected(C, A, B, split, c32):
    """What the device must leave in C (m + pad rows; A is m x k): see the module docstring.  Raises AssertionError on operands
    for which the fp32 accumulation would not be exact -- such a case fails here, not on the device."""
    return apply_update(C, product_terms(A, B, split), c32)
