"""GPU tests of mpf_getri and mpf_getdet (include/mpf_c.h): the inverse and the determinant from the factors.

The inverse is judged by LAPACK's own test ratio (dget03, both sides, threshold 30 of dtest.in) on sizes that sit on both sides of one
and two 256-seams and of the update kernel's 128-tile and ragged-edge paths, and bit for bit where the answer is exact: permutations
of power-of-two diagonals, bidiagonal factors, the scale vectors, two calls, two leading dimensions.  The determinant equals the numpy
restatement of its fixed order (tests/getri_model.py) bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest

import getri_model as M

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 7, 255, 256, 257, 600, 1031]
THRESH = 30.0    # LAPACK dtest.in
SENTINEL = -777.25


def padded(ctx, n, ld, fill=SENTINEL):
    """(base, view): a column-major ld x n device buffer filled with `fill` and its leading n x n view."""
    t = ctx.torch
    base = t.full((n, ld), fill, dtype=t.float64, device=ctx.device).t()
    return base, base[:n, :]


_cache = {}


def factored(ctx, n, kind, nb=256, pivot_search=1):
    """(A numpy, LU device, ipiv device) of a test matrix, computed once."""
    key = (n, kind, nb, pivot_search)
    if key not in _cache:
        A = ctx.to_numpy_f(ctx.matgen(n)) if kind == "matgen" else M.gen_matrix(n, kind)
        LU = ctx.from_numpy_f(A).clone()
        ipiv, info = ctx.factor(LU, nb, pivot_search=pivot_search)
        assert info == 0
        _cache[key] = (A, LU, ipiv)
    return _cache[key]


def inverse(ctx, LU, ipiv, ld, r=None, c=None):
    """getri with both leading dimensions = ld; returns (X numpy, the whole output buffer numpy)."""
    n = LU.shape[0]
    _, LUv = padded(ctx, n, ld, 0.0)
    LUv.copy_(LU)
    base, out = padded(ctx, n, ld)
    X, info = ctx.getri(LUv, ipiv, r=r, c=c, out=out)
    assert info == 0
    return ctx.to_numpy_f(X), ctx.to_numpy_f(base)


def check_ratio(A, X):
    left, right = M.dget03_ratio(A, X, True), M.dget03_ratio(A, X, False)
    print(f"n={A.shape[0]}: ||I - X A|| ratio {left:.4g}, ||I - A X|| ratio {right:.4g}")
    assert left <= THRESH and right <= THRESH


# ---- 1. ratio ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("n,kind", [(n, "gen") for n in SIZES] + [(n, "svd") for n in SIZES if n > 2])
def test_ratio(ctx, n, kind, pad):
    A, LU, ipiv = factored(ctx, n, kind)
    X, _ = inverse(ctx, LU, ipiv, n + pad)
    check_ratio(A, X)


def test_ratio_nb64(ctx):
    A, LU, ipiv = factored(ctx, 600, "gen", nb=64)
    check_ratio(A, inverse(ctx, LU, ipiv, 600)[0])


def test_ratio_default_pivot_rule_on_the_generators_matrix(ctx):
    A, LU, ipiv = factored(ctx, 1031, "matgen", pivot_search=0)
    check_ratio(A, inverse(ctx, LU, ipiv, 1031)[0])


# ---- 2. exact cases --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["shift", "reversal"])
def test_exact_permutation_times_diagonal(ctx, which):
    n = 600
    d = 2.0 ** (np.arange(n) % 41 - 20)
    perm = np.roll(np.arange(n), 1) if which == "shift" else np.arange(n)[::-1].copy()
    A = np.zeros((n, n))
    A[perm, np.arange(n)] = d              # A = P D: every interchange matters
    want = np.zeros((n, n))
    want[np.arange(n), perm] = 1.0 / d     # D^-1 P^T
    LU = ctx.from_numpy_f(A).clone()
    ipiv, info = ctx.factor(LU, 256, pivot_search=1)
    assert info == 0
    X, info = ctx.getri(LU, ipiv)
    assert info == 0
    assert np.array_equal(ctx.to_numpy_f(X), want)


@pytest.mark.parametrize("upper", [True, False])
def test_exact_bidiagonal(ctx, upper):
    n = 513
    A = np.eye(n) - (np.eye(n, k=1) if upper else np.eye(n, k=-1))
    want = np.triu(np.ones((n, n))) if upper else np.tril(np.ones((n, n)))
    LU = ctx.from_numpy_f(A).clone()
    ipiv, info = ctx.factor(LU, 256, pivot_search=1)
    assert info == 0
    X, info = ctx.getri(LU, ipiv)
    assert info == 0
    assert np.array_equal(ctx.to_numpy_f(X), want)


# ---- 3. scales -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [257, 600])
def test_scales_are_exact(ctx, n):
    A = M.gen_matrix(n, "gen")
    rng = np.random.default_rng(3 + n)
    r = 2.0 ** rng.integers(-20, 21, size=n)
    c = 2.0 ** rng.integers(-20, 21, size=n)
    LU = ctx.from_numpy_f(r[:, None] * A * c[None, :]).clone()
    ipiv, info = ctx.factor(LU, 256, pivot_search=1)
    assert info == 0
    t = ctx.torch
    dr, dc = t.from_numpy(r).to(ctx.device), t.from_numpy(c).to(ctx.device)
    Y = ctx.to_numpy_f(ctx.getri(LU, ipiv)[0])
    X = ctx.to_numpy_f(ctx.getri(LU, ipiv, r=dr, c=dc)[0])
    assert np.array_equal(X, c[:, None] * Y * r[None, :])
    assert np.array_equal(ctx.to_numpy_f(ctx.getri(LU, ipiv, r=dr)[0]), Y * r[None, :])
    assert np.array_equal(ctx.to_numpy_f(ctx.getri(LU, ipiv, c=dc)[0]), c[:, None] * Y)
    check_ratio(A, X)


# ---- 4. determinism and layout ------------------------------------------------------------------------------------------------------
def test_determinism_and_layout(ctx):
    n = 600
    A, LU, ipiv = factored(ctx, n, "gen")
    ip0 = ipiv.clone()
    got = {}
    for ld in (n, n + 3):
        # the buffers that reach the call, padding rows included, compared before and after it
        lu_base, LUv = padded(ctx, n, ld, 0.25)
        LUv.copy_(LU)
        lu_before = lu_base.clone()
        base, out = padded(ctx, n, ld)
        for rep in range(2):
            X, info = ctx.getri(LUv, ipiv, out=out)
            assert info == 0
            got[(ld, rep)] = ctx.to_numpy_f(X)
            assert ctx.torch.equal(lu_base, lu_before)        # d_LU is unchanged, its rows N .. ld - 1 too
            assert ctx.torch.equal(ipiv, ip0)                  # d_ipiv is unchanged
        whole = ctx.to_numpy_f(base)
        assert np.all(whole[n:, :] == SENTINEL)                # rows N .. ld - 1 of d_inv are not touched
    X1 = got[(n, 0)]
    assert np.array_equal(X1, got[(n, 1)])                     # two calls
    assert np.array_equal(X1, got[(n + 3, 0)])                 # ld = N and ld = N + 3
    # the leading dimensions of the factors and of the result are independent; the cached factors go in directly
    lu0 = LU.clone()
    _, LUv = padded(ctx, n, n + 5, 0.0)
    LUv.copy_(LU)
    assert np.array_equal(X1, ctx.to_numpy_f(ctx.getri(LUv, ipiv)[0]))
    assert np.array_equal(X1, ctx.to_numpy_f(ctx.getri(LU, ipiv)[0]))
    assert ctx.torch.equal(LU, lu0) and ctx.torch.equal(ipiv, ip0)


# ---- 5. singular factors, overlap ---------------------------------------------------------------------------------------------------
def test_singular_and_overlap(ctx, mpf):
    n = 600
    _, LU, ipiv = factored(ctx, n, "gen")
    S = LU.clone()
    S[300, 300] = 0.0
    S[450, 450] = 0.0
    base, out = padded(ctx, n, n + 3)
    _, info = ctx.getri(S, ipiv, out=out)
    assert info == 301
    assert np.all(ctx.to_numpy_f(base) == SENTINEL)
    with pytest.raises(mpf.MPFError, match="overlap"):
        ctx.getri(LU, ipiv, out=LU)
    big = ctx.colmajor(n, 2 * n)
    with pytest.raises(mpf.MPFError, match="overlap"):
        ctx.getri(big[:, :n], ipiv, out=big[:, n - 1:2 * n - 1])
    assert ctx.L.mpf_getri(ctx.h, None, n, None, 0, None, None, None, n) == 0   # N = 0: no work, not even the argument checks


# ---- 6. determinant -------------------------------------------------------------------------------------------------------------------
def diag_and_pivots(ctx, LU, ipiv):
    return np.diag(ctx.to_numpy_f(LU)).copy(), ipiv.cpu().numpy()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1031])
def test_det_equals_model(ctx, n):
    _, LU, ipiv = factored(ctx, n, "gen")
    d, ip = diag_and_pivots(ctx, LU, ipiv)
    got = ctx.getdet(LU, ipiv)
    assert got == M.getdet_model(d, ip)
    assert 0.5 <= abs(got[0]) < 1.0
    sign, logabs = ctx.slogdet(LU, ipiv)
    s_np, l_np = np.linalg.slogdet(M.gen_matrix(n, "gen"))
    assert sign == s_np and abs(logabs - l_np) <= 1e-9 * max(1.0, abs(l_np))
    # a padded leading dimension reads the same diagonal
    _, LUv = padded(ctx, n, n + 3, 0.0)
    LUv.copy_(LU)
    assert ctx.getdet(LUv, ipiv) == got


@pytest.mark.parametrize("power", [300, -300, "mixed"])
def test_det_outside_fp64_range(ctx, power):
    """Rows scaled by 2^+-300: all up, all down, or two rows in three up and the third down (the running product overflows at once)."""
    n = 257
    A = M.gen_matrix(n, "gen")
    if power == "mixed":
        A = A * (2.0 ** np.where(np.arange(n) % 3 == 2, -300.0, 300.0))[:, None]
    else:
        A = A * 2.0 ** power
    LU = ctx.from_numpy_f(A).clone()
    ipiv, info = ctx.factor(LU, 256, pivot_search=1)
    assert info == 0
    d, ip = diag_and_pivots(ctx, LU, ipiv)
    with np.errstate(over="ignore", under="ignore"):
        plain = np.prod(d)
    assert np.isinf(plain) or plain == 0.0             # the plain product leaves fp64's range
    mant, expo = ctx.getdet(LU, ipiv)
    assert (mant, expo) == M.getdet_model(d, ip)
    assert 0.5 <= abs(mant) < 1.0
    if power != "mixed":
        # the same matrix without the factor 2^power: the determinant moves by n * power binary places
        _, LU0, ipiv0 = factored(ctx, n, "gen")
        m0, e0 = ctx.getdet(LU0, ipiv0)
        assert (mant, expo) == (m0, e0 + n * power)
    else:
        sign, logabs = ctx.slogdet(LU, ipiv)
        s0, l0 = np.linalg.slogdet(M.gen_matrix(n, "gen"))
        shift = 300 * (n - 2 * (n // 3))               # 2 n / 3 rows up, n / 3 rows down
        assert sign == s0 and abs(logabs - (l0 + shift * math.log(2.0))) <= 1e-9 * abs(logabs)


def test_det_with_scales(ctx):
    n = 600
    A = M.gen_matrix(n, "gen")
    rng = np.random.default_rng(17)
    r = 2.0 ** rng.integers(-20, 21, size=n)
    c = 2.0 ** rng.integers(-20, 21, size=n)
    LU = ctx.from_numpy_f(r[:, None] * A * c[None, :]).clone()
    ipiv, info = ctx.factor(LU, 256, pivot_search=1)
    assert info == 0
    t = ctx.torch
    dr, dc = t.from_numpy(r).to(ctx.device), t.from_numpy(c).to(ctx.device)
    d, ip = diag_and_pivots(ctx, LU, ipiv)
    m0, e0 = M.getdet_model(d, ip)
    shift = int(np.log2(r).sum() + np.log2(c).sum())
    assert ctx.getdet(LU, ipiv) == (m0, e0)
    assert ctx.getdet(LU, ipiv, r=dr, c=dc) == (m0, e0 - shift) == M.getdet_model(d, ip, r=r, c=c)
    sign, logabs = ctx.slogdet(LU, ipiv, r=dr, c=dc)
    s_np, l_np = np.linalg.slogdet(A)
    assert sign == s_np and abs(logabs - l_np) <= 1e-9 * max(1.0, abs(l_np))


def test_slogdet_on_exact_factors(ctx):
    """Small-integer U and dyadic L with |l_ij| <= 1/2: every number of the elimination is exact, partial pivoting has one candidate
    per column, so numpy's LAPACK and this library both hold exactly these factors; numpy then sums N rounded logarithms."""
    n = 64
    rng = np.random.default_rng(23)
    L = np.tril(rng.integers(-1, 2, size=(n, n)) * 0.5, -1) + np.eye(n)
    U = np.triu(rng.integers(-3, 4, size=(n, n)).astype(np.float64), 1) + np.diag(rng.choice([-8., -6., -4., -3., -2., 2., 3., 4., 6., 8.], size=n))
    perm = rng.permutation(n)
    A = (L @ U)[perm, :]
    LU = ctx.from_numpy_f(A).clone()
    ipiv, info = ctx.factor(LU, 256, pivot_search=1)
    assert info == 0
    assert np.array_equal(ctx.to_numpy_f(LU), np.tril(L, -1) + U)      # the factors are exact
    sign, logabs = ctx.slogdet(LU, ipiv)
    s_np, l_np = np.linalg.slogdet(A)
    print(f"logabsdet {logabs!r} numpy {l_np!r}")
    assert sign == s_np
    assert abs(logabs - l_np) <= (n + 4) * 2.0 ** -52 * max(1.0, abs(l_np))


def test_det_zero_and_nonfinite_pivot(ctx):
    n = 600
    _, LU, ipiv = factored(ctx, n, "gen")
    S = LU.clone()
    S[300, 300] = 0.0
    assert ctx.getdet(S, ipiv) == (0.0, 0)
    assert ctx.slogdet(S, ipiv) == (0.0, -math.inf)
    S[17, 17] = math.inf
    mant, expo = ctx.getdet(S, ipiv)
    assert math.isnan(mant) and expo == 0
    m, e = C.c_double(0), C.c_int64(0)
    assert ctx.L.mpf_getdet(ctx.h, None, 1, None, 0, None, None, C.byref(m), C.byref(e)) == 0   # N = 0: the empty product
    assert (m.value, e.value) == (0.5, 1)


# ---- 7. inv ---------------------------------------------------------------------------------------------------------------------------
def test_inv(ctx, mpf):
    n = 257
    A, LU, ipiv = factored(ctx, n, "gen")
    dA = ctx.from_numpy_f(A)
    X = ctx.inv(dA, pivot_search=1)
    assert np.array_equal(ctx.to_numpy_f(X), ctx.to_numpy_f(ctx.getri(LU, ipiv)[0]))
    assert np.array_equal(ctx.to_numpy_f(dA), A)       # A is preserved
    check_ratio(A, ctx.to_numpy_f(ctx.inv(dA)))        # the default pivot rule
    Z = A.copy()
    Z[:, 5] = 0.0
    with pytest.raises(mpf.MPFError, match="singular"):
        ctx.inv(ctx.from_numpy_f(Z), pivot_search=1)
