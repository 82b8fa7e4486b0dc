"""numpy restatement of mpf_lange_batched, mpf_gecon_batched, mpf_residual_batched and mpf_gerfs_batched for ONE matrix of the batch
(include/mpf_c.h) -- test infrastructure.  Every chain is batched_model.getrs_model; the tree sum is stated once, here.

The shared rules:
  tree sum   every sum over a row or column index: the terms padded to 128 with +0, then v = v[:64] + v[64:], v[:32] + v[32:], ...
             down to one element, + rounded once per step.
  maxima     np.max: order-free, a NaN among the terms gives NaN.
  fusion     every product is rounded before it is added or subtracted (numpy never fuses).
  constants  mpf_gerfs's: eps = 2^-53, safmin = DBL_MIN, nz = n + 1, safe1 = nz safmin, safe2 = safe1 / eps.
Neither norm is LAPACK's estimate: both are formed exactly from the rows or columns of the inverse that the chains leave."""
import numpy as np

import batched_model as M

EPS = 2.0 ** -53
SAFMIN = np.finfo(np.float64).tiny
TREE = 128


def tree_sum(v, axis=0):
    """The halving tree over `axis` (length <= 128) of an array of non-negative terms."""
    v = np.moveaxis(np.asarray(v, dtype=np.float64), axis, 0)
    assert v.shape[0] <= TREE
    pad = np.zeros((TREE,) + v.shape[1:])
    pad[:v.shape[0]] = v
    with np.errstate(all="ignore"):
        while pad.shape[0] > 1:
            h = pad.shape[0] // 2
            pad = pad[:h] + pad[h:]
    return pad[0]


def _max(v):
    with np.errstate(all="ignore"):
        return np.max(v)          # NaN when one is present


def lange_model(A, norm="1"):
    A = np.abs(np.asarray(A, dtype=np.float64))
    if norm in ("1", "O"):
        return _max(tree_sum(A, axis=0))
    if norm == "I":
        return _max(tree_sum(A, axis=1))
    assert norm == "M"
    return _max(A)


def gecon_model(LU, anorm, norm="1"):
    """(rcond, ainvnm) from the packed factors, no P.  '1': the columns the trans = 0 chains leave for e_k; 'I': the vectors the
    trans = 1 chains leave for e_i (the rows of the same inverse, rounded their own way)."""
    LU = np.asarray(LU, dtype=np.float64)
    n = LU.shape[0]
    if np.any(np.diag(LU) == 0):                     # before any arithmetic
        return 0.0, np.inf
    nop = np.arange(1, n + 1, dtype=np.int32)
    X = M.getrs_model(LU, nop, np.eye(n), trans=(norm == "I"))     # column k: the chain from e_k
    assert norm in ("1", "O", "I")
    ainvnm = _max(tree_sum(np.abs(X), axis=0))
    if anorm == 0 or ainvnm == 0 or not np.isfinite(ainvnm):
        return 0.0, ainvnm
    with np.errstate(all="ignore"):
        return (1.0 / ainvnm) / anorm, ainvnm


def residual_model(A, X, B, trans=False):
    """(R, W): r_i from b_i, op(A)_ij x_j subtracted for j ascending; w_i from |b_i|, |op(A)_ij| |x_j| added.  X, B: (n, k) or (n,)."""
    A = np.asarray(A, dtype=np.float64)
    Aop = A.T if trans else A
    n = A.shape[0]
    Xm = np.asarray(X, dtype=np.float64).reshape(n, -1)
    R = np.array(B, dtype=np.float64, copy=True).reshape(n, -1)
    W = np.abs(R)
    with np.errstate(all="ignore"):
        for j in range(n):
            R = R - np.outer(Aop[:, j], Xm[j])
            W = W + np.outer(np.abs(Aop[:, j]), np.abs(Xm[j]))
    return R.reshape(np.shape(B)), W.reshape(np.shape(B))


def backward_error(r, w, n):
    safe1 = (n + 1) * SAFMIN
    safe2 = safe1 / EPS
    with np.errstate(all="ignore"):
        big = w > safe2
        q = np.where(big, np.abs(r) / np.where(big, w, 1.0), (np.abs(r) + safe1) / (w + safe1))
    return _max(q)


def gerfs_column(A, LU, ipiv, b, x, trans=False, itmax=0, want_ferr=True, inv_rows=None):
    """One column: (x, ferr, berr, iters, stop) with stop one of "berr <= eps", "not halved", "itmax", "nan".
    inv_rows: |Y| with Y[i] = getrs_model(1 - trans) of e_i (shared by the columns of a matrix)."""
    n = A.shape[0]
    itmax = 5 if itmax <= 0 else min(itmax, 31)
    nz = n + 1
    safe1 = nz * SAFMIN
    safe2 = safe1 / EPS
    x = np.array(x, dtype=np.float64, copy=True)
    lst, its, count = 3.0, 0, 1
    while True:
        r, w = residual_model(A, x, b, trans)
        be = backward_error(r, w, n)
        if np.isnan(be):
            stop = "nan"
        elif not be > EPS:
            stop = "berr <= eps"
        elif not 2.0 * be <= lst:
            stop = "not halved"
        elif not count <= itmax:
            stop = "itmax"
        else:
            with np.errstate(all="ignore"):
                x = x + M.getrs_model(LU, ipiv, r, trans=trans)
            lst, its = be, count
            count += 1
            continue
        break
    ferr = None
    if want_ferr:
        with np.errstate(all="ignore"):
            g = np.abs(r) + (nz * EPS) * w
            g = np.where(w > safe2, g, g + safe1)
            if inv_rows is None:
                inv_rows = inverse_rows(LU, ipiv, trans)
            f = tree_sum(inv_rows * g[None, :], axis=1)            # f_i = tree_k |y_k| g_k
            num, xmax = _max(f), _max(np.abs(x))
            ferr = num / xmax if xmax != 0 else num
    return x, ferr, be, its, stop


def inverse_rows(LU, ipiv, trans=False):
    """|Y|, Y[i, k] = y_k of the chain getrs_model(1 - trans) leaves for e_i, interchanges included: (op(A)^-1)_ik."""
    n = LU.shape[0]
    return np.abs(M.getrs_model(LU, ipiv, np.eye(n), trans=not trans)).T.copy()


def gerfs_model(A, LU, ipiv, B, X, trans=False, itmax=0, want_ferr=True):
    """(X, ferr, berr, iters, stops) for B, X of shape (n, nrhs); every column by gerfs_column."""
    n = A.shape[0]
    B = np.asarray(B, dtype=np.float64).reshape(n, -1)
    X = np.array(X, dtype=np.float64, copy=True).reshape(n, -1)
    Y = inverse_rows(LU, ipiv, trans) if want_ferr else None
    nrhs = B.shape[1]
    ferr, berr, its, stops = np.zeros(nrhs), np.zeros(nrhs), np.zeros(nrhs, dtype=np.int32), []
    for c in range(nrhs):
        X[:, c], fe, berr[c], its[c], st = gerfs_column(A, LU, ipiv, B[:, c], X[:, c], trans, itmax, want_ferr, Y)
        if want_ferr:
            ferr[c] = fe
        stops.append(st)
    return X, (ferr if want_ferr else None), berr, its, stops
