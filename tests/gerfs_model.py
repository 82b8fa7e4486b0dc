"""numpy restatement of LAPACK's dgerfs (test infrastructure, not a conftest): the reference mpf_gerfs is compared with.

The constants are LAPACK's: eps = dlamch('E') = 2^-53 (the relative machine epsilon, half of numpy's finfo.eps), safmin = DBL_MIN,
nz = N + 1, safe1 = nz safmin, safe2 = safe1 / eps.  With them the model reproduces the ferr of LAPACK's dgesvx to a ratio of
1.000 +- 0.001 for N >= 63 (checked once against scipy; nothing here needs scipy)."""
import numpy as np

from lacn2_model import dlacn2

EPS = 2.0 ** -53
SAFMIN = np.finfo(np.float64).tiny


def backward_error(r, w, n):
    """dgerfs's componentwise backward error per column from r and w (n x k each; a NaN is kept)."""
    safe1 = (n + 1) * SAFMIN
    safe2 = safe1 / EPS
    big = w > safe2
    q = np.where(big, np.abs(r) / np.where(big, w, 1.0), (np.abs(r) + safe1) / (w + safe1))
    return np.max(q, axis=0)          # np.max returns NaN when one is present


def gerfs_model(A, solve, solve_t, B, X, trans=False, itmax=0):
    """dgerfs, every column by its own rules.  solve(V) = op(A)^-1 V and solve_t(V) = op(A)^-T V with whatever factors are under
    test, for a vector or the columns of a matrix (op(A) = A^T when trans).  The columns still refining share each residual and each
    correction as one matrix product; dlacn2 runs column by column.
    Returns (X, ferr, berr, iterations, lacn2_iterations); X is a refined copy."""
    n = A.shape[0]
    Aop = A.T if trans else A
    absA = np.abs(Aop)
    itmax = 5 if itmax <= 0 else min(itmax, 31)
    nz = n + 1
    safe1 = nz * SAFMIN
    safe2 = safe1 / EPS
    X = np.array(X, dtype=np.float64, order="F", copy=True)
    nrhs = X.shape[1]
    ferr, berr = np.zeros(nrhs), np.zeros(nrhs)
    its, lits = np.zeros(nrhs, dtype=int), np.zeros(nrhs, dtype=int)
    lstres = np.full(nrhs, 3.0)
    active = np.ones(nrhs, dtype=bool)
    count = 1
    while True:
        # r = b - op(A) x and w = |b| + |op(A)| |x| (a stopped column's x no longer changes: its r and w stay its last ones)
        R = B - Aop @ X
        W = np.abs(B) + absA @ np.abs(X)
        be = backward_error(R, W, n)
        berr[active] = be[active]
        with np.errstate(invalid="ignore"):
            go = active & (be > EPS) & (2.0 * be <= lstres) & (count <= itmax)      # (false for a NaN: the column stops)
        active = go
        if not go.any():
            break
        X[:, go] += solve(R[:, go])
        lstres[go] = be[go]
        its[go] = count
        count += 1
    T = np.abs(R) + nz * EPS * W
    W = np.where(W > safe2, T, T + safe1)
    for j in range(nrhs):
        w = W[:, j]
        # dlacn2 on (op(A)^-1 diag(w))^T: KASE 1 is v -> w .* (op(A)^-T v), KASE 2 is v -> op(A)^-1 (w .* v)
        est, lits[j] = dlacn2(n, lambda v: w * solve_t(v), lambda v: solve(w * v))
        xmax = np.max(np.abs(X[:, j]))
        ferr[j] = est / xmax if xmax != 0 else est
    return X, ferr, berr, its, lits
