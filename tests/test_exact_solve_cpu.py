"""The exact-arithmetic family of the solve tests (tests/exact_solve_model.py) checked on the host alone: the generator's invariants,
that the family really is order-independent (a float64 model of blocked substitution with explicit inverses reproduces the closed
form bit for bit, at both block sizes, left- and right-looking, plain and transposed), and that the closed form is sensitive to every
entry next to a seam of the kernels, so that tests/test_gpu_exact_solve.py is known to bite."""
import numpy as np
import pytest

import exact_solve_model as M

SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 300, 513, 777, 1100]   # the GPU tests' shapes


def xmm(A, B):
    """A B for float64 arrays that hold integers (or multiples of 2^-2): int64 below N = 300, above it the float64 BLAS product, exact
    because the sums of absolute values stay below 2^50 (an int64 matrix product takes 10 s at N = 1100)."""
    if A.shape[0] <= 300:
        A4, B4 = np.rint(4 * A).astype(np.int64), np.rint(4 * B).astype(np.int64)
        assert np.array_equal(A4, 4 * A) and np.array_equal(B4, 4 * B)
        return (A4 @ B4).astype(np.float64) / 16.0
    assert float((np.abs(A) @ np.abs(B)).max()) * 16.0 <= M.LIMIT
    return A @ B


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_generator_invariants(n, seed):
    """L L^-1 = I and V V^-1 = I in integers, Nk^2 = 0, the packed LU is L under D V, the bounds and the fill conditions hold, ipiv
    is a valid interchange sequence, and the closed form equals plain integer substitution from (LU, ipiv) alone."""
    LU, ipiv, p = M.family(n, seed)
    I = np.eye(n)
    assert np.array_equal(xmm(p.L, p.Li), I) and np.array_equal(xmm(p.V, p.Vi), I)
    N1, N2, M1, M2 = p.parts
    for T in (N1, N2, M1, M2):
        assert not xmm(T, T).any() and np.abs(T).max(initial=0) <= 1 and np.array_equal(T, np.rint(T))
    assert not np.triu(N1).any() and not np.triu(N2).any() and not np.tril(M1).any() and not np.tril(M2).any()
    assert np.array_equal(p.L, xmm(I + N1, I + N2)) and np.array_equal(p.V, xmm(I + M1, I + M2))
    if n >= 64:
        assert xmm(N1, N2).any() and xmm(M1, M2).any()           # second-order paths are alive
    assert np.array_equal(np.tril(LU, -1), np.tril(p.L, -1)) and np.array_equal(np.triu(LU), p.d[:, None] * p.V)
    assert set(np.log2(p.d)) <= {-2.0, -1.0, 0.0, 1.0, 2.0} and LU.flags.f_contiguous
    assert ipiv.dtype == np.int32 and np.all(ipiv >= np.arange(1, n + 1)) and np.all(ipiv <= n)
    if n >= 8:
        assert np.any(ipiv == np.arange(1, n + 1)) and np.bincount(ipiv).max() >= 2   # no-ops, and a row picked twice
    assert min(p.bounds["fill"]) >= M.MIN_FILL and M.blocks_hold_nonzeros(p.L) and M.blocks_hold_nonzeros(p.V.T)
    assert p.bounds["inverses"] <= 50
    B, X, Xt = M.rhs(p, 5, seed)
    assert max(p.bounds["solve"] + p.bounds["solve_t"]) <= 50
    assert np.abs(B).max() <= 7 and np.array_equal(B, np.rint(B))
    assert np.array_equal(X, M.substitute(LU, ipiv, B, 0)) and np.array_equal(Xt, M.substitute(LU, ipiv, B, 1))
    assert np.array_equal(M.solve(p, B[:, 0], 0), X[:, 0]) and np.array_equal(M.solve(p, B, 1), Xt)
    # and it solves the system: A = P^T L U applied to the closed form gives B back, exactly
    A = M.matrix(p)
    M.assert_residual_exact(A, X, B)
    M.assert_residual_exact(A.T, Xt, B)
    assert np.array_equal(A @ X, B) and np.array_equal(A.T @ Xt, B)


# ---- a float64 model of blocked substitution with explicit inverses of the diagonal blocks ---------------------------------------------
def _invert(D, lower):
    """The explicit inverse of a triangular block by column-oriented substitution on the identity, in float64."""
    k = D.shape[0]
    X = np.eye(k)
    for j in (range(k) if lower else range(k - 1, -1, -1)):
        X[j] = X[j] / D[j, j]
        if lower:
            X[j + 1:] -= np.outer(D[j + 1:, j], X[j])
        else:
            X[:j] -= np.outer(D[:j, j], X[j])
    return X


def _blocked_tri(T, X, bs, lower, right):
    """T Y = X for triangular T, block by block (ascending for a lower T): the diagonal step is a product with the explicit inverse;
    right-looking takes each solved block out of all rows it still touches, left-looking gathers a block's updates before its step."""
    n = T.shape[0]
    X = X.copy()
    Y = np.zeros_like(X)
    starts = list(range(0, n, bs))
    for k in (starts if lower else starts[::-1]):
        e = min(k + bs, n)
        rest = slice(e, n) if lower else slice(0, k)
        if not right:
            X[k:e] -= T[k:e, slice(0, k) if lower else slice(e, n)] @ Y[slice(0, k) if lower else slice(e, n)]
        Y[k:e] = _invert(T[k:e, k:e], lower) @ X[k:e]
        if right:
            X[rest] -= T[rest, k:e] @ Y[k:e]
    return Y


def blocked_solve(LU, ipiv, B, trans, bs, right):
    n = LU.shape[0]
    L, U = np.tril(LU, -1) + np.eye(n), np.triu(LU)
    if not trans:
        return _blocked_tri(U, _blocked_tri(L, M.apply_p(ipiv, B), bs, True, right), bs, False, right)
    return M.apply_pt(ipiv, _blocked_tri(L.T, _blocked_tri(U.T, B, bs, True, right), bs, False, right))


@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("right", [False, True])
@pytest.mark.parametrize("bs", [64, 256])
@pytest.mark.parametrize("n", [1, 2, 65, 257, 513, 777, 1100])
def test_blocked_model_reproduces_the_closed_form(n, bs, right, trans):
    """Order independence, shown on the reference alone: float64 blocked substitution with explicit inverses, at block sizes 64 and
    256, left- and right-looking, plain and transposed, equals the int64 closed form exactly.  So does one refinement right-hand
    side (on the 2^-2 grid)."""
    LU, ipiv, p = M.family(n, 0)
    B, X, Xt = M.rhs(p, 5, 0)
    assert np.array_equal(blocked_solve(LU, ipiv, B, trans, bs, right), Xt if trans else X)
    if n in (65, 513):
        q = M.refine_case(n, 0, trans)
        assert np.array_equal(blocked_solve(LU, ipiv, q.B, trans, bs, right), q.C)
        assert np.array_equal(blocked_solve(LU, ipiv, q.R0, trans, bs, right), q.X1 - q.C)


# ---- sensitivity: the GPU test bites ---------------------------------------------------------------------------------------------------------
def _nearest_nonzero(T, s, lower):
    """The nonzero entry of T across seam s nearest to the corner (s, s - 1): lower: row >= s > column; upper: row < s <= column.
    None when that whole region of T is zero."""
    R = T[s:, :s] if lower else T[:s, s:].T                      # R[a, b]: a steps past the seam, column s - 1 - ... before it
    nz = np.argwhere(R != 0)
    if not len(nz):
        return None
    a, b = nz[np.argmin(nz[:, 0] + (s - 1 - nz[:, 1]))]
    return (s + a, b) if lower else (b, s + a)


@pytest.mark.parametrize("n", SIZES[1:])
def test_closed_form_is_sensitive_at_every_seam(n):
    """Zeroing one strictly-lower or one strictly-upper entry of LU next to a seam (every multiple of 32 -- the K chunks, the 64-row
    chunks and the 256 blocks --, the first column and the last row, where the w < 256 block and the column clamp end), or changing
    one ipiv entry, changes the exact answer of both solves: a kernel that drops such a term cannot pass the GPU test."""
    LU, ipiv, p = M.family(n, 0)
    B, X, Xt = M.rhs(p, 3, 0)
    want = (X, Xt)
    for s in sorted(set(range(32, n, 32)) | {1, n - 1}):
        for lower in (True, False):
            at = _nearest_nonzero(LU, s, lower)
            if at is None and s in (1, n - 1):                   # (the first column / last row of this member is empty: no term to drop)
                continue
            i, j = at
            P = LU.copy()
            P[i, j] = 0.0
            for trans in (0, 1):
                assert not np.array_equal(M.substitute(P, ipiv, B, trans), want[trans]), (s, lower, i, j, trans)
    # an interchange: a no-op becomes a swap with the last row, a swap becomes a no-op
    for i in (int(np.flatnonzero(ipiv[:-1] == np.arange(1, n))[0]) if np.any(ipiv[:-1] == np.arange(1, n)) else None,
              int(np.flatnonzero(ipiv != np.arange(1, n + 1))[0]) if np.any(ipiv != np.arange(1, n + 1)) else None):
        if i is None:
            continue
        ip = ipiv.copy()
        ip[i] = n if ip[i] == i + 1 else i + 1
        for trans in (0, 1):
            assert not np.array_equal(M.substitute(LU, ip, B, trans), want[trans]), (i, trans)


# ---- the refinement case ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("n,composite", [(65, True), (513, True), (1025, True), (4160, False)])
def test_refine_case_identities(n, composite, trans):
    """E^2 = 0 and E is full; op(A) = op(M)(I + E) and b = op(M) c in integers; x0 = c, d = -E c and r1 = 0 by integer substitution
    from (LU, ipiv); every bound holds; and the derived margin on history[0] accepts the true value but not one two margins away."""
    q = M.refine_case(n, 0, trans, composite=composite)
    E, C, X1, p = q.E, q.C, q.X1, q.pieces
    assert np.abs(E).max() == 1 and np.triu(E, 1).any() and np.tril(E, -1).any() and np.array_equal(E, np.rint(E))
    # rows outside T, columns inside T: a row and a column of the same index are never both occupied, so E^2 = 0
    assert not (np.abs(E).sum(axis=1).astype(bool) & np.abs(E).sum(axis=0).astype(bool)).any()
    mop = (lambda X: p.times_m(X.T).T) if trans else p.m_times   # op(M) X; exact on these operands (refine_case asserts the bounds)
    Aop = q.A.T if trans else q.A
    if n <= 1100:
        assert not xmm(E, E).any()
        Mop = mop(np.eye(n))
        assert np.array_equal(Mop, M.matrix(p).T if trans else M.matrix(p)) and np.array_equal(Aop, Mop + xmm(Mop, E))
    EC = (E.astype(np.int64) @ C.astype(np.int64)).astype(np.float64)
    assert EC.any() and np.array_equal(X1, C - EC)
    assert np.array_equal(q.B, mop(C)) and np.array_equal(q.R0, -mop(EC))
    assert np.array_equal(Aop @ C, q.B - q.R0) and np.array_equal(Aop @ X1, q.B)       # r0, and r1 = 0 (exact: bounds["residual"])
    assert np.array_equal(M.substitute(q.LU, q.ipiv, q.B, trans), q.C)
    assert np.array_equal(M.substitute(q.LU, q.ipiv, q.R0, trans), q.X1 - q.C)
    assert q.bounds["residual"] <= 50 and max(q.bounds["solve_b"] + q.bounds["solve_r0"]) <= 50
    for j in range(q.C.shape[1]):
        h = float(np.sqrt(q.rr[j] / q.bb[j]))
        assert abs(np.linalg.norm(q.R0[:, j]) / np.linalg.norm(q.B[:, j]) - h) <= 1e-12 * h
        assert M.history0_ok(h, q.rr[j], q.bb[j], n) and not M.history0_ok(h * (1 + 2 * (n + 4) * 2.0 ** -53), q.rr[j], q.bb[j], n)
