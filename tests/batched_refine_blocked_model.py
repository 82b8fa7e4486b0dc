"""numpy restatement of mpf_lange_batched_blocked, mpf_gecon_batched_blocked, mpf_residual_batched_blocked and
mpf_gerfs_batched_blocked for ONE matrix of the batch (include/mpf_c.h) -- test infrastructure.  It is batched_refine_model's
functions with the tree padded to 1024 instead of 128: the residual, the backward error and the chains are that module's, unchanged.

  tree sum   the terms padded to 1024 with +0, then v = v[:512] + v[512:], v[:256] + v[256:], ... down to one element.  Every term
             is >= +0, so for n <= 128 this is batched_refine_model.tree_sum bit for bit (tests/test_batched_refine_blocked_cpu.py).

family(n, ks) is the input family of the GPU tests: batched_refine_model's stale factors plus ONE EXACT COLUMN, B[:, -1] = column j of
op(A) with X0[:, -1] = e_j, so that r = 0 exactly, berr = 0 and no correction is made -- the stale family alone no longer reaches
"berr <= eps" above n of about 200."""
import numpy as np

import batched_model as M
import batched_refine_model as R

EPS, SAFMIN = R.EPS, R.SAFMIN
TREE = 1024

residual_model = R.residual_model
backward_error = R.backward_error
_max = R._max


def tree_sum(v, axis=0, pad_to=TREE):
    """The halving tree over `axis` (length <= pad_to, a power of two) of an array of non-negative terms."""
    v = np.moveaxis(np.asarray(v, dtype=np.float64), axis, 0)
    assert v.shape[0] <= pad_to and pad_to & (pad_to - 1) == 0
    pad = np.zeros((pad_to,) + v.shape[1:])
    pad[:v.shape[0]] = v
    with np.errstate(all="ignore"):
        while pad.shape[0] > 1:
            h = pad.shape[0] // 2
            pad = pad[:h] + pad[h:]
    return pad[0]


def lange_model(A, norm="1"):
    A = np.abs(np.asarray(A, dtype=np.float64))
    if norm in ("1", "O"):
        return _max(tree_sum(A, axis=0))
    if norm == "I":
        return _max(tree_sum(A, axis=1))
    assert norm == "M"
    return _max(A)


def rcond_of(ainvnm, anorm):
    """rcond from the two norms: 0, never NaN, for anorm 0 and for an ainvnm that is 0 or not finite."""
    if anorm == 0 or ainvnm == 0 or not np.isfinite(ainvnm):
        return 0.0
    with np.errstate(all="ignore"):
        return (1.0 / ainvnm) / anorm


def ainvnm_of(X):
    """max over the chains (columns of X) of the tree over the row index."""
    return _max(tree_sum(np.abs(X), axis=0))


def gecon_model(LU, anorm, norm="1"):
    """(rcond, ainvnm) from the packed factors, no P (batched_refine_model.gecon_model with the larger tree)."""
    LU = np.asarray(LU, dtype=np.float64)
    n = LU.shape[0]
    assert norm in ("1", "O", "I")
    if np.any(np.diag(LU) == 0):                     # before any arithmetic
        return 0.0, np.inf
    nop = np.arange(1, n + 1, dtype=np.int32)
    ainvnm = ainvnm_of(M.getrs_model(LU, nop, np.eye(n), trans=(norm == "I")))
    return rcond_of(ainvnm, anorm), ainvnm


def rule(be, lst, count, itmax):
    """One decision of the refinement rule: None to go on (x <- x + dx), else the stop reason."""
    if np.isnan(be):
        return "nan"
    if not be > EPS:
        return "berr <= eps"
    if not 2.0 * be <= lst:
        return "not halved"
    if not count <= itmax:
        return "itmax"
    return None


def ferr_of(r, w, x, inv_rows):
    """ferr of one column from its last r and w: g, f_i = tree_k |y_k| g_k, max_i f_i / max_i |x_i|."""
    n = r.shape[0]
    nz = n + 1
    safe1 = nz * SAFMIN
    safe2 = safe1 / EPS
    with np.errstate(all="ignore"):
        g = np.abs(r) + (nz * EPS) * w
        g = np.where(w > safe2, g, g + safe1)
        f = tree_sum(inv_rows * g[None, :], axis=1)
        num, xmax = _max(f), _max(np.abs(x))
        return num / xmax if xmax != 0 else num


def gerfs_column(A, LU, ipiv, b, x, trans=False, itmax=0, want_ferr=True, inv_rows=None):
    """One column: (x, ferr, berr, iters, stop), batched_refine_model.gerfs_column with the larger tree."""
    n = A.shape[0]
    itmax = 5 if itmax <= 0 else min(itmax, 31)
    x = np.array(x, dtype=np.float64, copy=True)
    lst, its, count = 3.0, 0, 1
    while True:
        r, w = residual_model(A, x, b, trans)
        be = backward_error(r, w, n)
        stop = rule(be, lst, count, itmax)
        if stop is not None:
            break
        with np.errstate(all="ignore"):
            x = x + M.getrs_model(LU, ipiv, r, trans=trans)
        lst, its = be, count
        count += 1
    ferr = None
    if want_ferr:
        if inv_rows is None:
            inv_rows = R.inverse_rows(LU, ipiv, trans)
        ferr = ferr_of(r, w, x, inv_rows)
    return x, ferr, be, its, stop


def gerfs_model(A, LU, ipiv, B, X, trans=False, itmax=0, want_ferr=True, inv_rows=None):
    """(X, ferr, berr, iters, stops) for B, X of shape (n, nrhs); every column by gerfs_column.  inv_rows: |Y| as
    batched_refine_model.inverse_rows returns it (computed here when None and ferr is wanted)."""
    n = A.shape[0]
    B = np.asarray(B, dtype=np.float64).reshape(n, -1)
    X = np.array(X, dtype=np.float64, copy=True).reshape(n, -1)
    if want_ferr and inv_rows is None:
        inv_rows = R.inverse_rows(LU, ipiv, trans)
    nrhs = B.shape[1]
    ferr, berr, its, stops = np.zeros(nrhs), np.zeros(nrhs), np.zeros(nrhs, dtype=np.int32), []
    for c in range(nrhs):
        X[:, c], fe, berr[c], its[c], st = gerfs_column(A, LU, ipiv, B[:, c], X[:, c], trans, itmax, want_ferr, inv_rows)
        if want_ferr:
            ferr[c] = fe
        stops.append(st)
    return X, (ferr if want_ferr else None), berr, its, stops


# ---- the input family of the tests ---------------------------------------------------------------------------------------------------
KS = [None, 40, 20, 12, 8, 4, 2]
NRHS = 5


def family(n, ks=KS, nrhs=NRHS):
    """(A, Af, B): len(ks) matrices A, the matrices Af = A + 2^-k E whose factors the refinement gets, and nrhs right-hand sides --
    batched_refine_model's stale-factor family, seeds 7000 + n.  The caller overwrites the last column with exact_column()."""
    rng = np.random.default_rng(7000 + n)
    nb = len(ks)
    A = rng.standard_normal((nb, n, n))
    E = rng.standard_normal((nb, n, n))
    B = rng.standard_normal((nb, n, nrhs))
    Af = np.stack([A[s] if k is None else A[s] + 2.0 ** -k * E[s] for s, k in enumerate(ks)])
    return A, Af, B


def exact_column(A, trans):
    """(b, x0) with op(A) x0 = b exactly: x0 = e_j and b = column j of op(A), j = n // 2.  r = 0, berr = 0, no correction."""
    n = A.shape[0]
    j = n // 2
    x0 = np.zeros(n)
    x0[j] = 1.0
    return (A[j, :] if trans else A[:, j]).copy(), x0
