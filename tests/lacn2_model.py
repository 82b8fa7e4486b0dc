"""numpy restatement of LAPACK's dlacn2 / dgecon / dgeequb-with-powers-of-two (test infrastructure, not a conftest): the
reference the device's mpf_gecon and mpf_geequ are compared with."""
import numpy as np


def dlacn2(n, apply_b, apply_bt, itmax=5):
    """Hager / Higham 1-norm estimate of B from products x -> B x and x -> B^T x.  Returns (est, iterations)."""
    x = apply_b(np.full(n, 1.0 / n))
    if n == 1:
        return abs(x[0]), 1
    est = np.sum(np.abs(x))
    isgn = np.where(x >= 0, 1.0, -1.0)
    x = apply_bt(isgn.copy())
    j = int(np.argmax(np.abs(x)))
    it = 2
    while True:
        x = np.zeros(n)
        x[j] = 1.0
        x = apply_b(x)
        estold = est
        est = np.sum(np.abs(x))
        xs = np.where(x >= 0, 1.0, -1.0)
        if np.array_equal(xs, isgn) or est <= estold:
            break
        isgn = xs
        x = apply_bt(xs.copy())
        jlast = j
        j = int(np.argmax(np.abs(x)))
        if x[jlast] != abs(x[j]) and it < itmax:
            it += 1
            continue
        break
    i = np.arange(n, dtype=np.float64)
    x = apply_b(np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * (1.0 + i / (n - 1)))
    temp = 2.0 * (np.sum(np.abs(x)) / (3 * n))
    return (temp if temp > est else est), it


def _tri_solvers(LU):
    n = LU.shape[0]
    L = np.tril(LU, -1) + np.eye(n)
    U = np.triu(LU)
    try:
        from scipy.linalg import solve_triangular as st

        def lo(x, trans=False):
            return st(L, x, lower=True, unit_diagonal=True, trans=1 if trans else 0)

        def up(x, trans=False):
            return st(U, x, lower=False, trans=1 if trans else 0)
    except ImportError:
        def lo(x, trans=False):
            return np.linalg.solve(L.T if trans else L, x)

        def up(x, trans=False):
            return np.linalg.solve(U.T if trans else U, x)
    return lo, up


def gecon_ainvnm(LU, norm="1"):
    """dgecon's estimate of ||(L U)^-1|| ('1') or ||(L U)^-1||_inf ('I') from the packed factors (no P).  (ainvnm, iterations)"""
    lo, up = _tri_solvers(LU)

    def inv(x):       # (L U)^-1 x: L then U
        return up(lo(x))

    def inv_t(x):     # (L U)^-T x: U^T then L^T
        return lo(up(x, True), True)
    one = norm in ("1", "O")
    return dlacn2(LU.shape[0], inv if one else inv_t, inv_t if one else inv)


def gecon(LU, anorm, norm="1"):
    """LAPACK dgecon on packed factors: rcond = (1 / ainvnm) / anorm, 0 for anorm == 0 or a zero diagonal entry of U."""
    if anorm == 0 or np.any(np.diag(LU) == 0):
        return 0.0
    ainvnm, _ = gecon_ainvnm(LU, norm)
    return (1.0 / ainvnm) / anorm if ainvnm != 0 and np.isfinite(ainvnm) else 0.0


def pow2_inv(m):
    """2^-floor(log2 m) for m > 0, exponent clamped to [-1022, 1022] (mpf_geequ's factors)."""
    e = np.frexp(m)[1].astype(np.int64) - 1
    return np.ldexp(1.0, -np.clip(e, -1022, 1022))


def geequ(A):
    """mpf_geequ's restatement: (r, c, rowcnd, colcnd, amax, info)."""
    n = A.shape[0]
    small = np.finfo(np.float64).tiny
    big = 1.0 / small
    rm = np.abs(A).max(axis=1)
    amax = rm.max()
    if np.any(rm == 0):
        return None, None, 0.0, 0.0, amax, int(np.argmax(rm == 0)) + 1
    r = pow2_inv(rm)
    rowcnd = max(rm.min(), small) / min(rm.max(), big)
    cm = (np.abs(A) * r[:, None]).max(axis=0)
    if np.any(cm == 0):
        return r, None, rowcnd, 0.0, amax, n + int(np.argmax(cm == 0)) + 1
    c = pow2_inv(cm)
    colcnd = max(cm.min(), small) / min(cm.max(), big)
    return r, c, rowcnd, colcnd, amax, 0
