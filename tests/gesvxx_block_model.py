"""numpy restatement of the extra-precise expert solve (include/mpf_c.h: mpf_gerpvgrw, mpf_gerfsx_scaled's berr, mpf_gesvxx_block's
attempt) on given factors (test infrastructure, not a conftest):

    rpvgrw             LAPACK dla_gerpvgrw on A, the factors of Dr A Dc and the two scale vectors
    berr_model         dgerfs's componentwise backward error from an exactly rounded residual (gerfsx_model.exact_residual) and
                       w = |b| + |op(A)| |x| in longdouble: the reference mpf_gerfsx_scaled's berr is compared with
    two_stage_attempt  stage (a) mpf_solve_ir_block's rules on the plain fp64 residual (gesvx_block_model.refine_model), then stage (b)
                       mpf_gerfsx's loop with a fresh rule state (gerfsx_model.gerfsx_model) on that X; cold_attempt is stage (b) alone
                       from x0 = solve(b)
    gesvxx_block_model the attempts in sequence: the first whose columns ALL end stage (b) converged stands, the last one is returned
                       whatever it says

and the factors the CPU tests drive them with: an LU with partial pivoting or none, in numpy, of A or of a perturbed copy
A (1 + 2^-b E) that stands for fp16-class (b = 11) and fp16x3-class (b = 22) factors."""
import numpy as np

import gerfs_model as GF
import gerfsx_model as G
import gesvx_block_model as GB

EPS = G.EPS
LD = np.longdouble


def lu(A, pivot=True):
    """(LU packed as LAPACK packs it, perm) with P A = L U, rows perm of A: partial pivoting, or none (perm = identity)."""
    LU = np.array(A, dtype=np.float64, order="F")
    n = LU.shape[0]
    perm = np.arange(n)
    for k in range(n - 1):
        if pivot:
            p = k + int(np.argmax(np.abs(LU[k:, k])))
            if p != k:
                LU[[k, p]] = LU[[p, k]]
                perm[[k, p]] = perm[[p, k]]
        LU[k + 1:, k] /= LU[k, k]
        LU[k + 1:, k + 1:] -= np.outer(LU[k + 1:, k], LU[k, k + 1:])
    return LU, perm


def lu_solvers(LU, perm):
    """(solve, solve_t): A^-1 V and A^-T V from the packed factors of P A = L U, as products with the explicit (L U)^-1."""
    n = LU.shape[0]
    M = np.linalg.inv((np.tril(LU, -1) + np.eye(n)) @ np.triu(LU))

    def solve(v):
        return M @ v[perm]

    def solve_t(v):
        out = np.empty_like(v)
        out[perm] = M.T @ v
        return out
    return solve, solve_t


def perturbed_factors(A, bits, seed):
    """Factors of A (1 + 2^-bits E), E uniform in (-1, 1) per element: what low-precision factors look like to refinement (bits = 11:
    fp16-class, 22: fp16x3-class; None: fp64 factors of A itself)."""
    if bits is None:
        return lu(A)
    E = np.random.default_rng(seed).uniform(-1, 1, A.shape)
    return lu(A * (1.0 + 2.0 ** -bits * E))


def rpvgrw(A, LU, r=None, c=None):
    """dla_gerpvgrw: min(1, min over the columns j with umax_j != 0 of amax_j / umax_j), amax_j = max_i (|a_ij| r_i) c_j, umax_j =
    max_{i <= j} |u_ij|; a NaN in a column's A or U part makes the result NaN."""
    n = A.shape[0]
    S = np.abs(A)
    if r is not None:
        S = S * r[:, None]
    if c is not None:
        S = S * c[None, :]
    out = 1.0
    U = np.abs(np.triu(LU))
    for j in range(n):
        amax, umax = S[:, j].max(), U[:j + 1, j].max()          # (np.max returns NaN when one is present)
        if np.isnan(amax) or np.isnan(umax):
            return float("nan")
        if umax != 0:
            out = min(out, float(amax / umax))
    return out


def berr_model(Aop, B, X):
    """dgerfs's componentwise backward error per column of op(A) X = B for the given X: r rounded once from the exact residual, w =
    |b| + |op(A)| |x| and the quotient in longdouble, rounded to fp64 at the end; safe1 / safe2 as mpf_gerfs.  A NaN is kept."""
    n = Aop.shape[0]
    safe1 = LD((n + 1) * GF.SAFMIN)
    safe2 = safe1 / LD(EPS)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.abs(G.exact_residual(Aop, X, B)).astype(LD)
        w = np.abs(B).astype(LD) + np.abs(Aop).astype(LD) @ np.abs(X).astype(LD)
        big = w > safe2
        q = np.where(big, r / np.where(big, w, LD(1)), (r + safe1) / (w + safe1))
    return np.max(q, axis=0).astype(np.float64)


def cold_attempt(Aop, solve, B, ithresh=0):
    """Stage (b) alone from x0 = solve(b): what mpf_gerfsx does after mpf_getrs.  dict(X, err_norm, err_comp, cols, plain_steps = 0)."""
    X, en, ec, cols = G.gerfsx_model(Aop, solve, B, solve(B), ithresh)
    return dict(X=X, err_norm=en, err_comp=ec, cols=cols, ir=None, plain_steps=[0] * B.shape[1])


def two_stage_attempt(A, solve, B, trans=False, max_iter=10, tol=1e-12, ithresh=0):
    """One attempt of mpf_gesvxx_block: (a) refine_model on the plain residual (its converged flags decide nothing), (b) gerfsx_model
    with a fresh rule state on that X.  dict(X, err_norm, err_comp, cols, ir, plain_steps): plain_steps = the corrections of stage (a)
    per column, cols[j].corrections those of stage (b)."""
    Aop = np.ascontiguousarray(A.T if trans else A)
    Xa, ir = GB.refine_model(A, solve, B, trans, max_iter, tol)
    X, en, ec, cols = G.gerfsx_model(Aop, solve, B, Xa, ithresh)
    return dict(X=X, err_norm=en, err_comp=ec, cols=cols, ir=ir, plain_steps=[s["iterations"] for s in ir])


def stands(attempt):
    return all(c.x_state == G.X_CONV for c in attempt["cols"])


def gesvxx_block_model(A, B, trans, solvers, max_iter=10, tol=1e-12, ithresh=0, want_berr=True):
    """The attempts of mpf_gesvxx_block on `solvers` = [solve of the original system per set of factors], the low-precision ones first
    when there are two: the first attempt that stands is returned, else the last.  Adds attempt (index), ret (0 / 1) and berr."""
    for k, solve in enumerate(solvers):
        out = two_stage_attempt(A, solve, B, trans, max_iter, tol, ithresh)
        if stands(out):
            break
    out["attempt"] = k
    out["ret"] = 0 if stands(out) else 1
    out["berr"] = berr_model(np.ascontiguousarray(A.T if trans else A), B, out["X"]) if want_berr else None
    return out
