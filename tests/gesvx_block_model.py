"""numpy restatement of steps 5 .. 7 of mpf_gesvx_block on given factors and scales (test infrastructure, not a conftest): blocked
refinement by mpf_solve_ir_block's per-column rules, the all-or-nothing fall-back, and dgerfs's bounds (tests/gerfs_model.py) of the
ORIGINAL system, all with the equilibrated factors as the preconditioner

    op(A)^-1 v ~ post * F^-1 (pre * v),    op(A)^-T v ~ pre * F^-T (post * v)        (F = the factored op(Dr A Dc), P included)

trans = 0: pre = Dr, post = Dc; trans = 1: pre = Dc, post = Dr; None stands for no scaling.  Every scale is an exact power of two, so
the residual and the weights of the original system are the equilibrated ones times a power of two per row: berr is the same number in
both systems, bit for bit (tests/test_gesvx_block_cpu.py)."""
import numpy as np

import gerfs_model as G

EPS = G.EPS
LD = np.longdouble


def _col(s, v):
    return v if s is None else (s[:, None] * v if v.ndim == 2 else s * v)


def scaled_solvers(f_solve, f_solve_t, pre=None, post=None):
    """(solve, solve_t) of the original system from those of the factored, equilibrated one (vectors or the columns of a matrix)."""
    def solve(v):
        return _col(post, f_solve(_col(pre, v)))

    def solve_t(v):
        return _col(pre, f_solve_t(_col(post, v)))
    return solve, solve_t


def refine_model(A, solve, B, trans=False, max_iter=10, tol=1e-12):
    """mpf_solve_ir_block's rules, column by column: x0 = solve(b); r = b - op(A) x; stop at ||r|| / ||b|| <= tol (||b|| = 0 reads 1),
    at max_iter (clamped to 31), on a NaN, or when two steps in a row gained less than a factor 0.7.  A stopped column is frozen.
    Returns (X, stats): stats a list of dicts (iterations, converged, stalled, rel_residual, history)."""
    max_iter = min(max_iter, 31)
    Aop = A.T if trans else A
    nrhs = B.shape[1]
    nb2 = np.linalg.norm(B, axis=0)
    nb2[nb2 == 0] = 1.0
    X = np.array(solve(B), dtype=np.float64, order="F")
    st = [dict(iterations=0, converged=0, stalled=0, rel_residual=0.0, history=[]) for _ in range(nrhs)]
    active = np.ones(nrhs, dtype=bool)
    it = 0
    while True:
        R = B - Aop @ X
        rel = np.linalg.norm(R, axis=0) / nb2
        go = np.zeros(nrhs, dtype=bool)
        for j in np.flatnonzero(active):
            s = st[j]
            s["rel_residual"] = rel[j]
            s["history"].append(rel[j])
            s["iterations"] = it
            h = s["history"]
            if rel[j] <= tol:
                s["converged"] = 1
            elif it >= max_iter or rel[j] != rel[j]:
                pass
            elif it >= 2 and h[it] > 0.7 * h[it - 1] and h[it - 1] > 0.7 * h[it - 2]:
                s["stalled"] = 1
            else:
                go[j] = True
        active = go
        if not go.any():
            return X, st
        X[:, go] += solve(R[:, go])
        it += 1


def worst_column(st):
    """The attempt's summary: the column with the largest final rel_residual (a NaN counts as largest, the first one wins)."""
    w = 0
    for j in range(1, len(st)):
        a, b = st[j]["rel_residual"], st[w]["rel_residual"]
        if b == b and (a != a or a > b):
            w = j
    return w


def gesvx_block_model(A, B, trans, attempts, max_iter=10, tol=1e-12, itmax=0, bounds=True):
    """Steps 5 .. 7.  attempts: [(solve, solve_t)] of the original system (scaled_solvers), the low-precision factors first when there
    are two.  Step 5 refines all columns on the first; step 6: if ANY column did not converge and there is a second, all columns are
    solved and refined again on it; step 7: dgerfs on the factors that produced the answer.
    Returns dict(X, ferr, berr, attempt, ir, iterations, lacn2_iterations, ret): attempt = index of the factors used, ret = 0 / 1."""
    for k, (solve, solve_t) in enumerate(attempts):
        X, ir = refine_model(A, solve, B, trans, max_iter, tol)
        if ir[worst_column(ir)]["converged"]:
            break
    out = dict(X=X, ferr=None, berr=None, attempt=k, ir=ir, iterations=None, lacn2_iterations=None,
               ret=0 if all(s["converged"] for s in ir) else 1)
    if bounds:
        out["X"], out["ferr"], out["berr"], out["iterations"], out["lacn2_iterations"] = G.gerfs_model(A, solve, solve_t, B, X, trans, itmax)
    return out


def exact_quantities(Aop, inv, B, X, X0):
    """What the bound assertions need for the returned X (n x k) of op(A) X = B, with inv = op(A)^-1 to working precision and X0 a
    solution to working precision:  (berr_exact, err, lo, hi) per column,
        r_ld = b - op(A) x in longdouble, w2 = |b| + |op(A)| |x|, berr_exact = dgerfs's ratio from r_ld and w2,
        err = max|x - x_ref| / max|x|, x_ref = X0 refined once with a longdouble residual,
        lo = max_i (|inv| (nz eps w2))_i / max|x|,  hi = max_i (|inv| (|r_ld| + 2 nz eps w2))_i / max|x|."""
    n = Aop.shape[0]
    nz = n + 1
    safe1 = nz * G.SAFMIN
    safe2 = safe1 / EPS
    Al = Aop.astype(LD)
    r_ld = B.astype(LD) - Al @ X.astype(LD)
    r0 = (B.astype(LD) - Al @ X0.astype(LD)).astype(np.float64)
    x_ref = X0 + inv @ r0
    w2 = np.abs(B) + np.abs(Aop) @ np.abs(X)
    big = w2 > safe2
    q = np.where(big, np.abs(r_ld) / np.where(big, w2, 1.0).astype(LD), (np.abs(r_ld) + safe1) / (w2.astype(LD) + safe1))
    berr_exact = q.max(axis=0).astype(np.float64)
    xmax = np.abs(X).max(axis=0)
    xmax = np.where(xmax == 0, 1.0, xmax)
    err = np.abs(X - x_ref).max(axis=0) / xmax
    absinv = np.abs(inv)
    lo = (absinv @ (nz * EPS * w2)).max(axis=0) / xmax
    hi = (absinv @ (np.abs(r_ld).astype(np.float64) + 2 * nz * EPS * w2)).max(axis=0) / xmax
    return berr_exact, err, lo, hi
