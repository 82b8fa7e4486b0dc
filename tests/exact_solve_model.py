"""Exact-arithmetic test data for the large-matrix solve layer (tests/test_exact_solve_cpu.py, tests/test_gpu_exact_solve.py).

The solves take the factors as INPUT, so a test can hand them factors on which every evaluation order is exact:

    L = (I + N1)(I + N2)      Nk strictly lower, entries in {-1, 0, 1}, rows outside a subset Sk, columns inside it: Nk^2 = 0,
                              so L^-1 = (I - N2)(I - N1) is an integer matrix (two factors: N1 N2 != 0 keeps second-order paths alive)
    U = D V,  V = (I + M1)(I + M2) the same in the strict upper triangle,  D = diag(2^e), e in -2 .. 2
    ipiv      a random valid interchange sequence (no-ops and rows picked twice among it),  B integer in [-7, 7]

Every number a solve can form from these operands with +, -, *, fma and a division by a diagonal entry lies on a grid 2^-g: L, L^-1,
B and y = L^-1 P B are integers; U, 1 / u_ii, the blocks of U^-1 and x are multiples of 2^-2, a partly updated right-hand side
y - U x of 2^-4, and its product with an explicit inverse block of 2^-6 (g = 6; with B on the 2^-2 grid, as in refine_case, g = 8).
A multiple of 2^-g below 2^(53 - g) is a double, so NO operation rounds while the partial sums stay below that, whatever the order,
the blocking or the explicit inverses, and the result is the closed form
    x = (I - M2)(I - M1) D^-1 (I - N2)(I - N1) P b            (transposed: x = P^T (I - N1)^T (I - N2)^T D^-1 (I - M1)^T (I - M2)^T b)
which solve() evaluates in int64.  The generator bounds every partial sum by products of absolute values (|F^-1| (|rhs| + |F| |y|)
for a triangular stage F y = rhs, max |F^-1| |F| |F^-1| for the construction of explicit inverses), multiplies by 2^g and asserts the result
below LIMIT = 2^50, three bits under the 2^53 at which a double stops holding every integer: no test can run on data that might round.
The pieces are built with float64 BLAS products, exact under the same bounds (int64 matrix products are too slow at N = 1100).
"""
import functools

import numpy as np

LIMIT = 2.0 ** 50
MIN_FILL = 0.30


# ---- the interchanges ---------------------------------------------------------------------------------------------------------------
def make_ipiv(n, rng):
    """1-based, ipiv[i] >= i + 1: about a third no-ops, the others anywhere below; two far rows are picked twice when n allows."""
    ip = np.arange(1, n + 1, dtype=np.int64)
    for i in range(n):
        if rng.random() > 0.35:
            ip[i] = rng.integers(i, n) + 1
    if n >= 8:
        for t in (n - 1, n - 3):
            for i in rng.choice(n // 2, 2, replace=False):
                ip[i] = t + 1
    return ip.astype(np.int32)


def apply_p(ipiv, X):
    """P X: LAPACK's row interchanges, one after the other (a copy)."""
    X = np.array(X, copy=True)
    for i, p in enumerate(np.asarray(ipiv, dtype=np.int64) - 1):
        if p != i:
            X[[i, p]] = X[[p, i]]
    return X


def apply_pt(ipiv, X):
    """P^T X: the same interchanges in reverse order (a copy)."""
    X = np.array(X, copy=True)
    ip = np.asarray(ipiv, dtype=np.int64) - 1
    for i in range(len(ip) - 1, -1, -1):
        if ip[i] != i:
            X[[i, ip[i]]] = X[[ip[i], i]]
    return X


# ---- the factors -----------------------------------------------------------------------------------------------------------------------
def _nilpotent(n, rng, density):
    """Strictly lower, entries in {-1, 0, 1}, rows outside a random subset S and columns inside it (so the square is zero)."""
    S = rng.random(n) < 0.5
    N = rng.choice(np.array([-1.0, 1.0]), (n, n)) * (rng.random((n, n)) < density)
    N *= (~S)[:, None] & S[None, :]
    return np.tril(N, -1)


def blocks_hold_nonzeros(T):
    """Every 64 x 64 block that meets the strict lower triangle of T holds a nonzero there."""
    n = T.shape[0]
    strict = np.tril(np.ones((n, n), dtype=bool), -1)
    nz = strict & (T != 0)
    for i0 in range(0, n, 64):
        for j0 in range(0, i0 + 1, 64):
            if strict[i0:i0 + 64, j0:j0 + 64].any() and not nz[i0:i0 + 64, j0:j0 + 64].any():
                return False
    return True


def fill(T):
    """Nonzero share of the strict lower triangle (1 where there is none)."""
    n = T.shape[0]
    return 1.0 if n < 2 else float(np.count_nonzero(np.tril(T, -1))) / (n * (n - 1) / 2)


def _unit_lower(n, rng, density):
    """(F, F^-1, A1, A2): F = (I + A1)(I + A2), F^-1 = (I - A2)(I - A1); the subsets are drawn again until the fill conditions hold
    (family asserts them)."""
    I = np.eye(n)
    for _ in range(200):
        A1, A2 = _nilpotent(n, rng, density), _nilpotent(n, rng, density)
        F = (I + A1) @ (I + A2)
        if fill(F) >= MIN_FILL and blocks_hold_nonzeros(F):
            break
    return F, (I - A2) @ (I - A1), A1, A2


def grid_bits(B):
    """0 for an integer right-hand side, 2 for one on the 2^-2 grid; anything else is refused."""
    B = np.asarray(B, dtype=np.float64)
    if np.array_equal(B, np.rint(B)):
        return 0
    assert np.array_equal(4 * B, np.rint(4 * B)), "right-hand side off the 2^-2 grid"
    return 2


def _ab(F, v, t=False):
    """|F| v or |F|^T v (F = None: the identity)."""
    return v if F is None else np.abs(F.T if t else F) @ v


class Pieces:
    """The integer pieces of one family member.  L, Li = L^-1, V, Vi = V^-1: float64 arrays holding integers (None: the identity);
    d: the diagonal of U; parts = (N1, N2, M1, M2) of composite factors."""

    def __init__(self, n, ipiv, d, L=None, Li=None, V=None, Vi=None, parts=None):
        self.n, self.ipiv, self.d = n, ipiv, d
        self.L, self.Li, self.V, self.Vi, self.parts = L, Li, V, Vi, parts
        self.bounds = {}            # log2 of the asserted bounds and the fill, for the record

    def lu_packed(self):
        """LU as dgetrf packs it: the strict lower triangle of L under U = D V, column-major."""
        LU = np.diag(self.d) if self.V is None else self.d[:, None] * self.V
        if self.L is not None:
            LU = LU + np.tril(self.L, -1)
        return np.asfortranarray(LU)

    def abs_twin(self):
        """The same products on absolute values: what bounds the partial sums of m_times / times_m."""
        return Pieces(self.n, self.ipiv, self.d, None if self.L is None else np.abs(self.L), None, None if self.V is None else np.abs(self.V))

    def m_times(self, X):
        """M X, M = P^T L U."""
        Y = self.d[:, None] * (X if self.V is None else self.V @ X)
        return apply_pt(self.ipiv, Y if self.L is None else self.L @ Y)

    def times_m(self, X):
        """X M.  (X P^T = (P X^T)^T.)"""
        Y = apply_p(self.ipiv, X.T).T
        Y = (Y if self.L is None else Y @ self.L) * self.d[None, :]
        return Y if self.V is None else Y @ self.V

    def assert_solve_exact(self, B, trans):
        """The partial sums of op(A)^-1 B stay exact.  A triangular stage F y = rhs, however it is blocked, forms partial sums of
        rhs_i - sum_j F_ij y_j and of an explicit inverse block times such partly updated entries: all at most
        |F^-1| (|rhs| + |F| |y|) with the exact y, which stages() supplies.  Times 2^g <= LIMIT for both stages.
        Returns (log2 of the two bounds, the exact solution)."""
        B = np.asarray(B, dtype=np.float64).reshape(self.n, -1)
        g = 6 + grid_bits(B)
        d = self.d[:, None]
        L, Li, V, Vi = self.L, self.Li, self.V, self.Vi
        first, last = stages(self, B, trans)
        if not trans:                                                           # L y = P b, then D V x = y
            s1 = _ab(Li, np.abs(apply_p(self.ipiv, B)) + _ab(L, np.abs(first)))
            s2 = _ab(Vi, np.abs(first) / d + _ab(V, np.abs(last)))
        else:                                                                   # V^T D w = b, then L^T z = w (x = P^T z)
            s1 = _ab(Vi, np.abs(B) + _ab(V, d * np.abs(first), True), True) / d
            s2 = _ab(Li, np.abs(first) + _ab(L, np.abs(apply_p(self.ipiv, last)), True), True)
        b1, b2 = float(s1.max()) * 2.0 ** g, float(s2.max()) * 2.0 ** g
        assert b1 <= LIMIT and b2 <= LIMIT, (self.n, trans, np.log2(b1), np.log2(b2))
        return (float(np.log2(max(b1, 1.0))), float(np.log2(max(b2, 1.0)))), last


def _sub(F, X, t=False):
    """(I - F) X or (I - F)^T X in int64."""
    return X - (F.T if t else F).astype(np.int64) @ X


def stages(pieces, B, trans):
    """The closed form in int64 (B: n x nrhs, integer or on the 2^-2 grid): (the first triangular stage's result, the solution), both
    exact in float64.  trans = 0: y = L^-1 P b, x = U^-1 y; trans = 1: w = U^-T b, x = P^T L^-T w."""
    p = pieces
    B4 = np.rint(4 * B)
    assert np.array_equal(B4, 4 * B), "right-hand side off the 2^-2 grid"
    B4 = B4.astype(np.int64)
    s = np.rint(4.0 / p.d).astype(np.int64)[:, None]                            # 4 D^-1: 1 .. 16
    N1, N2, M1, M2 = p.parts if p.parts is not None else (None,) * 4
    if not trans:
        Y1 = apply_p(p.ipiv, B4)
        if N1 is not None:
            Y1 = _sub(N2, _sub(N1, Y1))
        Y2 = s * Y1
        if M1 is not None:
            Y2 = _sub(M2, _sub(M1, Y2))
        s1 = 4.0
    else:
        Y1 = s * (B4 if M1 is None else _sub(M1, _sub(M2, B4, True), True))
        Y2 = apply_pt(p.ipiv, Y1 if N1 is None else _sub(N1, _sub(N2, Y1, True), True))
        s1 = 16.0
    assert max(np.abs(Y1).max(initial=0), np.abs(Y2).max(initial=0)) < 2 ** 52
    return Y1.astype(np.float64) / s1, Y2.astype(np.float64) / 16.0


def solve(pieces, B, trans):
    """The closed-form solution of op(P^T L U) X = B, evaluated in int64; B a vector or n x nrhs."""
    B = np.asarray(B, dtype=np.float64)
    X = stages(pieces, B.reshape(pieces.n, -1), trans)[1]
    return X[:, 0] if B.ndim == 1 else X


@functools.lru_cache(maxsize=6)
def family(n, seed, density=1.0):
    """(LU packed column-major float64, ipiv int32, Pieces) of one member; rhs() below gives it right-hand sides."""
    rng = np.random.default_rng([n, seed, 20250])
    L, Li, N1, N2 = _unit_lower(n, rng, density)
    F, Fi, A1, A2 = _unit_lower(n, rng, density)
    V, Vi, M1, M2 = F.T.copy(), Fi.T.copy(), A2.T.copy(), A1.T.copy()          # F^T = (I + A2^T)(I + A1^T)
    d = 2.0 ** rng.integers(-2, 3, n)
    p = Pieces(n, make_ipiv(n, rng), d, L, Li, V, Vi, (N1, N2, M1, M2))
    I = np.eye(n)
    assert np.array_equal(L @ Li, I) and np.array_equal(V @ Vi, I)
    assert np.array_equal(L, (I + N1) @ (I + N2)) and np.array_equal(V, (I + M1) @ (I + M2)) and np.array_equal(Vi, (I - M2) @ (I - M1))
    for T in (L, V.T):
        assert fill(T) >= MIN_FILL and blocks_hold_nonzeros(T), (n, seed, fill(T))
    p.bounds["fill"] = (fill(L), fill(V.T))
    p.bounds["max"] = (float(np.abs(L).max()), float(np.abs(V).max()))
    # the construction of explicit inverses (64 x 64 by substitution, 256 x 256 from 64-block products): max |F^-1| |F| |F^-1| 2^6
    bi = max(float(_ab(Li, _ab(L, np.abs(Li))).max()), float((_ab(Vi, _ab(V, np.abs(Vi))) / d[None, :]).max())) * 64.0
    assert bi <= LIMIT, (n, np.log2(bi))
    p.bounds["inverses"] = float(np.log2(bi))
    LU = p.lu_packed()
    LU.setflags(write=False)
    return LU, p.ipiv, p


@functools.lru_cache(maxsize=8)
def rhs(pieces, nrhs, seed):
    """(B, X, Xt): integer right-hand sides in [-7, 7], n x nrhs, on which both solves with these factors are asserted exact, and
    the closed-form solutions of A X = B and A^T Xt = B."""
    B = np.random.default_rng([pieces.n, nrhs, seed, 7]).integers(-7, 8, (pieces.n, nrhs)).astype(np.float64)
    pieces.bounds["solve"], X = pieces.assert_solve_exact(B, 0)
    pieces.bounds["solve_t"], Xt = pieces.assert_solve_exact(B, 1)
    return B, X, Xt


def matrix(pieces):
    """A = P^T L U itself, exact (entries on the 2^-2 grid): against it the residual of the exact solution is exactly zero."""
    I = np.eye(pieces.n)
    assert float(pieces.abs_twin().m_times(I).max()) * 4.0 <= LIMIT
    return np.asfortranarray(pieces.m_times(I))


def assert_residual_exact(Aop, X, B):
    """Every partial sum of B - op(A) X is exact: op(A) and X on the 2^-2 grid, their products on 2^-4.  Returns log2 of the bound."""
    m = float((np.abs(B) + np.abs(Aop) @ np.abs(X)).max()) * 16.0
    assert m <= LIMIT, np.log2(m)
    return float(np.log2(max(m, 1.0)))


class RefineCase:
    pass


@functools.lru_cache(maxsize=4)
def refine_case(n, seed, trans=0, ncols=3, composite=True):
    """Data on which one refinement step is exact.  M = P^T L U (the composite factors of family(n, seed), or L = I, U = D),
    E integer in {-1, 0, 1} on rows outside T and columns inside T (E^2 = 0; full, not triangular), op(A) = op(M) (I + E),
    b = op(M) c with c integer.  Then, exactly and in any evaluation order,
        x0 = c,  r0 = -op(M) E c,  d = -E c,  x1 = c - E c,  r1 = 0."""
    rng = np.random.default_rng([n, seed, trans, 31337])
    if composite:
        LU, ipiv, p = family(n, seed)
    else:
        p = Pieces(n, make_ipiv(n, rng), 2.0 ** rng.integers(-2, 3, n))
        LU, ipiv = p.lu_packed(), p.ipiv
    T = rng.random(n) < 0.5
    E = rng.integers(-1, 2, (n, n)).astype(np.float64) * ((~T)[:, None] & T[None, :])
    C = rng.integers(-7, 8, (n, ncols)).astype(np.float64)
    IE = E.copy()
    IE[np.arange(n), np.arange(n)] += 1.0
    if not trans:
        A, bound = p.m_times(IE), p.abs_twin().m_times(np.abs(IE))              # M (I + E)
        mop = p.m_times
    else:
        A, bound = p.times_m(IE.T), p.abs_twin().times_m(np.abs(IE.T))          # (I + E)^T M:  A^T = M^T (I + E)
        mop = lambda X: p.times_m(X.T).T
    assert float(bound.max()) * 4.0 <= LIMIT                                    # the products that built A are exact
    del bound, IE
    EC = E @ C
    B, R0, X1 = mop(C), -mop(EC), C - EC
    Aop = A.T if trans else A
    q = RefineCase()
    q.bounds = {"residual": max(assert_residual_exact(Aop, C, B), assert_residual_exact(Aop, X1, B)),
                "solve_b": p.assert_solve_exact(B, trans)[0], "solve_r0": p.assert_solve_exact(R0, trans)[0]}
    assert np.array_equal(solve(p, B, trans), C) and np.array_equal(solve(p, R0, trans), -EC)
    assert np.array_equal(Aop @ C, B - R0) and not (B - Aop @ X1).any()
    q.n, q.trans, q.pieces, q.LU, q.ipiv = n, trans, p, LU, ipiv
    q.A, q.B, q.C, q.E, q.X1, q.R0 = np.asfortranarray(A), B, C, E, X1, R0
    # ||r0||^2 and ||b||^2 per column as exact integers (4 r0 and 4 b are integers): history[0] = sqrt(rr / bb)
    r4, b4 = np.rint(4 * R0).astype(np.int64), np.rint(4 * B).astype(np.int64)
    q.rr = [sum(int(v) * int(v) for v in r4[:, j]) for j in range(ncols)]
    q.bb = [sum(int(v) * int(v) for v in b4[:, j]) for j in range(ncols)]
    assert all(v > 0 for v in q.rr) and all(v > 0 for v in q.bb)
    return q


def history0_ok(h0, rr, bb, n):
    """|h0 - sqrt(rr / bb)| <= (n + 4) 2^-53 sqrt(rr / bb), judged in 60-digit decimals.  The margin is derived, not measured: a sum of
    n squares in any order carries a relative error of at most n 2^-53, which the square root halves; two such norms, their two
    square roots and the division add up to (n + 3) 2^-53 to first order."""
    from decimal import Decimal, getcontext
    getcontext().prec = 60
    ref = (Decimal(rr) / Decimal(bb)).sqrt()
    return abs(Decimal(float(h0)) - ref) <= ref * (n + 4) * Decimal(2) ** -53


# ---- plain integer substitution straight from (LU, ipiv): the second, independent reference of the CPU tests ---------------------------
def substitute(LU, ipiv, B, trans):
    """op(A)^-1 B by column-oriented substitution in int64, from the packed factors alone.  Needs what the family guarantees and what
    zeroing an entry keeps: L integer, diag(U) powers of two in 2^-2 .. 2^2, U / diag(U) integer, B on the 2^-2 grid."""
    LU = np.asarray(LU)
    n = LU.shape[0]
    d = np.diag(LU).copy()
    Vf, Lf = np.triu(LU, 1) / d[:, None], np.tril(LU, -1)
    s = np.rint(4.0 / d)
    assert np.array_equal(Vf, np.rint(Vf)) and np.array_equal(Lf, np.rint(Lf)) and np.array_equal(s, 4.0 / d)
    V, L, s = Vf.astype(np.int64), Lf.astype(np.int64), s.astype(np.int64)[:, None]
    B = np.asarray(B, dtype=np.float64)
    B4 = np.rint(4 * B.reshape(n, -1)).astype(np.int64)
    assert np.array_equal(B4, 4 * B.reshape(n, -1))
    if not trans:
        Y = apply_p(ipiv, B4)
        for j in range(n - 1):                              # L y = P b
            Y[j + 1:] -= L[j + 1:, j:j + 1] * Y[j:j + 1]
        Y *= s                                              # V x = D^-1 y
        for j in range(n - 1, 0, -1):
            Y[:j] -= V[:j, j:j + 1] * Y[j:j + 1]
    else:
        Y = B4.copy()
        for j in range(n - 1):                              # V^T t = b, w = D^-1 t
            Y[j + 1:] -= V[j, j + 1:, None] * Y[j:j + 1]
        Y *= s
        for j in range(n - 1, 0, -1):                       # L^T z = w
            Y[:j] -= L[j, :j, None] * Y[j:j + 1]
        Y = apply_pt(ipiv, Y)
    X = Y.astype(np.float64) / 16.0
    return X[:, 0] if B.ndim == 1 else X
