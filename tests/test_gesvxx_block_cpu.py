"""CPU checks of the model of the extra-precise expert solve (tests/gesvxx_block_model.py: what tests/test_gpu_gesvxx_block.py compares
the device with): the reciprocal pivot growth, the backward error's invariance under an exact row scaling, and the two-stage attempt
(plain refinement as a warm start, then the extra-precise loop with a fresh rule state) on N = 96 systems with modelled low-precision
factors."""
import math

import numpy as np
import pytest

import gerfsx_model as G
import gesvxx_block_model as XM

EPS = G.EPS


def wilkinson(n):
    """1 on the diagonal and in the last column, -1 below the diagonal: partial pivoting never interchanges and U's last column doubles
    from row to row."""
    W = np.eye(n) - np.tril(np.ones((n, n)), -1)
    W[:, -1] = 1.0
    return np.asfortranarray(W)


def test_rpvgrw_wilkinson_identity_and_skipped_column():
    W = wilkinson(40)
    LU, perm = XM.lu(W, pivot=False)
    assert np.array_equal(perm, np.arange(40)) and LU[39, 39] == 2.0 ** 39
    assert XM.rpvgrw(W, LU) == 2.0 ** -39
    LUp, permp = XM.lu(W, pivot=True)
    assert np.array_equal(permp, np.arange(40)) and np.array_equal(LUp, LU), "partial pivoting takes the diagonal (the first maximum)"
    I = np.eye(7)
    assert XM.rpvgrw(I, I) == 1.0
    assert XM.rpvgrw(4.0 * I, I) == 1.0, "the initial value 1 is the cap"
    # a column with umax = 0 is skipped: without it the quotient of column 2 (0.5 / 8) decides, with U[:, 3] = 0 column 3 (1 / 64) is out
    A = np.diag([1.0, 1.0, 0.5, 1.0])
    U = np.diag([1.0, 2.0, 8.0, 64.0])
    assert XM.rpvgrw(A, U) == 1.0 / 64
    U[3, 3] = 0.0
    assert XM.rpvgrw(A, U) == 0.5 / 8
    # scales: amax_j = max_i (|a_ij| r_i) c_j
    r, c = np.array([2.0, 1.0, 4.0, 0.5]), np.array([1.0, 0.25, 1.0, 2.0])
    U = np.diag([4.0, 4.0, 4.0, 4.0])
    assert XM.rpvgrw(A, U, r, c) == min(2.0 / 4, 0.25 / 4, 2.0 / 4, 1.0 / 4)
    An = A.copy()
    An[2, 1] = np.nan
    assert math.isnan(XM.rpvgrw(An, U))
    Un = U.copy()
    Un[0, 3] = np.nan
    assert math.isnan(XM.rpvgrw(A, Un))
    Ul = U.copy()
    Ul[3, 0] = np.nan                                     # L's part of the packed factors is not looked at
    assert XM.rpvgrw(A, Ul) == 0.5 / 4


@pytest.mark.parametrize("trans", [0, 1])
def test_berr_is_invariant_under_a_power_of_two_row_scaling(trans):
    """(A, b, x) and (Dr A, Dr b, x), Dr = 2^k: r and w scale by the same exact power of two row by row, the quotient is the same
    number.  For op(A) = A^T the rows of op(A) are A's columns: (A Dr)^T x = Dr b."""
    n, m = 60, 3
    rng = np.random.default_rng(11)
    A = G.rand(n, 5)
    B = rng.uniform(-1, 1, (n, m))
    Aop = np.ascontiguousarray(A.T if trans else A)
    X = np.linalg.solve(Aop, B) * (1 + 1e-9 * rng.uniform(-1, 1, (n, m)))
    k = rng.integers(-30, 31, n)
    be = XM.berr_model(Aop, B, X)
    be_s = XM.berr_model(np.ldexp(Aop, k[:, None]), np.ldexp(B, k[:, None]), X)
    assert np.all(be > 1e-12) and np.all(be < 1e-6)
    assert np.array_equal(be.view(np.uint64), be_s.view(np.uint64))
    Xn = X.copy()
    Xn[3, 1] = np.nan
    ben = XM.berr_model(Aop, B, Xn)
    assert math.isnan(ben[1]) and ben[0] == be[0] and ben[2] == be[2]


# The eight N = 96 systems of the design note: the suite's rand / ill generators, factors of A (1 + 2^-b E) for fp16-class
# (b = 11) and fp16x3-class (b = 22) factors, or fp64 factors of A itself (b = None); 4 right-hand sides.
# (name, matrix, b, cold corrections, plain steps of the warm start, corrections after it): the counts are THIS MODEL's output,
# regenerated with the model and asserted so that a change of the rules shows; they are not a statement about the device.
CASES = [
    ("fp16-class, diag-dominant", lambda: G.rand(96, 1), 11, [6, 6, 6, 6], [4, 4, 4, 4], [2, 2, 2, 3]),
    ("fp16-class, kappa 1e2", lambda: G.ill(96, 1e2, 2), 11, [7, 6, 7, 7], [4, 4, 4, 4], [3, 2, 3, 3]),
    ("fp16-class, kappa 1e3", lambda: G.ill(96, 1e3, 3), 11, [10, 10, 10, 10], [6, 6, 7, 6], [5, 5, 3, 4]),
    ("fp16x3-class, kappa 1e4", lambda: G.ill(96, 1e4, 4), 22, [4, 4, 4, 4], [2, 2, 3, 2], [2, 2, 2, 2]),
    ("fp64, diag-dominant", lambda: G.rand(96, 1), None, [1, 1, 1, 1], [0, 0, 0, 0], [1, 1, 1, 1]),
    ("fp64, kappa 1e6", lambda: G.ill(96, 1e6, 5), None, [1, 1, 1, 1], [3, 3, 3, 3], [1, 1, 1, 1]),
    ("fp64, kappa 1e10", lambda: G.ill(96, 1e10, 6), None, [2, 2, 2, 2], [2, 3, 3, 3], [2, 2, 2, 2]),
    ("fp64, kappa 1e13", lambda: G.ill(96, 1e13, 7), None, [4, 4, 4, 4], [3, 3, 3, 3], [4, 4, 4, 4]),
]


@pytest.mark.parametrize("name,make,bits,cold_n,plain_n,warm_n", CASES, ids=[c[0] for c in CASES])
def test_two_stage_attempt(name, make, bits, cold_n, plain_n, warm_n):
    """The warm start (plain steps on the cheap residual, then the extra-precise loop with a fresh rule state) ends every column CONV
    in both states with both bounds at the floor max(10, sqrt(N)) 2^-53, and the true error inside them; on low-precision factors it
    needs fewer pair-residual corrections than the cold loop, on fp64 factors the same number (the plain stage adds steps there and
    saves none: its stall rule has to end it)."""
    n, m = 96, 4
    A = make()
    B = np.random.default_rng(50).uniform(-1, 1, (n, m))
    solve, _ = XM.lu_solvers(*XM.perturbed_factors(A, bits, 9))
    cold = XM.cold_attempt(A, solve, B)
    warm = XM.two_stage_attempt(A, solve, B)
    got = ([c.corrections for c in cold["cols"]], warm["plain_steps"], [c.corrections for c in warm["cols"]])
    print(name, "cold", got[0], "plain", got[1], "then", got[2])
    floor = max(10.0, math.sqrt(n)) * EPS
    assert XM.stands(warm) and all(c.z_state == G.Z_CONV for c in warm["cols"])
    assert np.all(warm["err_norm"] == floor) and np.all(warm["err_comp"] == floor)
    Minv = np.linalg.inv(A)
    Xh, Xl = G.reference_pair(A, B, lambda V: Minv @ V)
    e_norm, e_comp = G.errors(warm["X"], Xh, Xl)
    assert np.all(e_norm <= warm["err_norm"]) and np.all(e_comp <= warm["err_comp"]), (e_norm / EPS, e_comp / EPS)
    assert got == (cold_n, plain_n, warm_n)
    if bits is not None:
        assert all(w < c for w, c in zip(got[2], got[0]))
    else:
        assert got[2] == got[0]


def test_all_or_nothing_fall_back():
    """kappa = 1e10 on fp16-class factors: the corrections do not contract, no column converges, the attempt does not stand and ALL
    columns go to the second set of factors; with fp64 factors alone the first attempt stands."""
    n, m = 96, 3
    A = G.ill(n, 1e10, 6)
    B = np.random.default_rng(51).uniform(-1, 1, (n, m))
    low, _ = XM.lu_solvers(*XM.perturbed_factors(A, 11, 9))
    f64, _ = XM.lu_solvers(*XM.perturbed_factors(A, None, 9))
    assert not XM.stands(XM.two_stage_attempt(A, low, B))
    out = XM.gesvxx_block_model(A, B, False, [low, f64])
    assert out["attempt"] == 1 and out["ret"] == 0 and np.all(out["berr"] <= 4 * EPS)
    alone = XM.gesvxx_block_model(A, B, False, [f64])
    assert alone["attempt"] == 0 and np.array_equal(alone["X"], out["X"])
    only_low = XM.gesvxx_block_model(A, B, False, [low])
    assert only_low["attempt"] == 0 and only_low["ret"] == 1, "the last attempt is returned whatever it says"
