"""numpy restatement of mpf_getri's three stages (block size as a parameter) and of mpf_getdet's fixed order (include/mpf_c.h).

The inverse model follows the device algorithm stage by stage -- explicit inverses of the diagonal blocks, one rank-`nb` update per
block -- but not its summation order inside a product, so it is compared by LAPACK's dget03 ratio, not bit for bit.  The determinant
model multiplies numbers in [0.5, 1) and uses frexp only, both exact in any IEEE arithmetic: it gives the device's bits."""
import math

import numpy as np

CHUNK = 256   # mpf_getdet: consecutive diagonal entries per chunk


def gen_matrix(n, kind, seed=7):
    """The test matrices: "gen" = the generator's kind, integers(0, 100) / 10; "svd" = U diag(logspace(0, -8)) V^T."""
    rng = np.random.default_rng(seed + n)
    if kind == "gen":
        return rng.integers(0, 100, size=(n, n)).astype(np.float64) / 10.0
    U, _ = np.linalg.qr(rng.standard_normal((n, n)))
    V, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return U @ np.diag(np.logspace(0, -8, n)) @ V.T


def getrf(A):
    """LAPACK dgetf2 (partial pivoting, first maximum wins): returns (LU packed, ipiv 1-based int32)."""
    LU = np.array(A, dtype=np.float64, order="F")
    n = LU.shape[0]
    ipiv = np.arange(1, n + 1, dtype=np.int32)
    for j in range(n):
        p = j + int(np.argmax(np.abs(LU[j:, j])))
        ipiv[j] = p + 1
        if p != j:
            LU[[j, p], :] = LU[[p, j], :]
        if LU[j, j] != 0.0 and j + 1 < n:
            LU[j + 1:, j] /= LU[j, j]
            LU[j + 1:, j + 1:] -= np.outer(LU[j + 1:, j], LU[j, j + 1:])
    return LU, ipiv


def inv_upper(T):
    """Inverse of an upper triangular block by back substitution on the identity, row by row from the last."""
    n = T.shape[0]
    X = np.zeros((n, n))
    for i in range(n - 1, -1, -1):
        X[i, i] = 1.0 / T[i, i]
        if i + 1 < n:
            X[i, i + 1:] = -X[i, i] * (T[i, i + 1:] @ X[i + 1:, i + 1:])
    return X


def inv_unit_lower(T):
    """Inverse of a unit lower triangular block (the strict lower triangle of T is used, the diagonal reads as 1)."""
    n = T.shape[0]
    U = np.triu(T.T, 1) + np.eye(n)
    return inv_upper(U).T


def column_source(ipiv):
    """dgetri's interchanges (j = N - 2 .. 0: columns j and ipiv[j] - 1 change places) composed: column j of the result is column
    src[j] of inv(U) inv(L)."""
    n = len(ipiv)
    src = np.arange(n)
    for j in range(n - 2, -1, -1):
        p = int(ipiv[j]) - 1
        if p != j:
            src[j], src[p] = src[p], src[j]
    return src


def getri_model(LU, ipiv, nb=256, r=None, c=None):
    """inv(A) = Dc inv(A') Dr from the packed factors P A' = L U of A' = Dr A Dc."""
    LU = np.asarray(LU, dtype=np.float64)
    n = LU.shape[0]
    W = np.eye(n)
    nblk = (n + nb - 1) // nb
    # stage 1: inv(U) into the upper triangle, block rows from the last one up
    for k in range(nblk - 1, -1, -1):
        kb, ke = k * nb, min(n, k * nb + nb)
        W[kb:ke, kb:] = inv_upper(np.triu(LU[kb:ke, kb:ke])) @ W[kb:ke, kb:]
        W[:kb, kb:] -= LU[:kb, kb:ke] @ W[kb:ke, kb:]
    # stage 2: X L = inv(U), block columns from the last one down
    for j in range(nblk - 1, -1, -1):
        jb, je = j * nb, min(n, j * nb + nb)
        W[:, jb:je] = W[:, jb:je] @ inv_unit_lower(LU[jb:je, jb:je])
        W[:, :jb] -= W[:, jb:je] @ LU[jb:je, :jb]
    # stage 3: the column interchanges and the scales in one pass
    W = W[:, column_source(ipiv)]
    if c is not None:
        W = np.asarray(c)[:, None] * W
    if r is not None:
        W = W * np.asarray(r)[None, :]
    return W


def dget03_ratio(A, X, left=True):
    """LAPACK dget03: ||I - X A||_1 / (N ||A||_1 ||X||_1 2^-53)  (left = False: I - A X)."""
    n = A.shape[0]
    R = np.eye(n) - (X @ A if left else A @ X)
    an, xn = np.abs(A).sum(axis=0).max(), np.abs(X).sum(axis=0).max()
    return np.abs(R).sum(axis=0).max() / (n * an * xn * 2.0 ** -53)


def _step(p, e, m, em):
    p, k = math.frexp(p * m)
    return p, e + k + em


def getdet_model(diag, ipiv, r=None, c=None):
    """mpf_getdet's order on the diagonal of U: returns (mant, expo), det = mant 2^expo."""
    d = [float(v) for v in diag]
    n = len(d)
    if n == 0:
        return 0.5, 1
    if not all(math.isfinite(v) for v in d):
        return math.nan, 0
    if any(v == 0.0 for v in d):
        return 0.0, 0
    me = [math.frexp(v) for v in d]
    m = [v[0] for v in me]
    e = [v[1] for v in me]
    for s in (r, c):
        if s is not None:
            for i in range(n):
                e[i] -= math.frexp(float(s[i]))[1] - 1   # the exact exponent of a power of two
    P, E = 1.0, 0
    for c0 in range(0, n, CHUNK):
        p, ee = 1.0, 0
        for i in range(c0, min(n, c0 + CHUNK)):
            p, ee = _step(p, ee, m[i], e[i])
        P, E = _step(P, E, p, ee)
    flips = sum(1 for i in range(n) if int(ipiv[i]) != i + 1)
    return (-P if flips & 1 else P), E


def slogdet_model(diag, ipiv, r=None, c=None):
    mant, expo = getdet_model(diag, ipiv, r, c)
    if mant == 0.0:
        return 0.0, -math.inf
    if math.isnan(mant):
        return math.nan, math.nan
    return math.copysign(1.0, mant), math.log(abs(mant)) + expo * math.log(2.0)
