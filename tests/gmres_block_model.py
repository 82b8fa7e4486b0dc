"""numpy model of mpf_solve_gmres_ir_block (include/mpf_c.h), column by column: GMRES-IR after Carson & Higham with the low-precision
factors as the preconditioner M^-1 and classical Gram-Schmidt applied twice (CGS2).  The rules are those of csrc/solve_rules.h
(GmresCol); the device differs from this model in its summation orders only.

M^-1 is a callable (N x k matrix -> N x k matrix) or a pair (LU, ipiv) of packed factors with LAPACK's 1-based pivots, applied by
explicit triangular solves (lu_solver).  gmres_ir_model records what each inner step saw (h, hn) and decided, so that
tests/gmres_rules_driver.cpp can be fed the same Hessenberg columns."""
import numpy as np


def ill(n, kappa, seed):
    """tests/test_gpu_gesvx_block.py's _ill: singular values 1 .. 1 / kappa between two random orthogonal factors."""
    rng = np.random.default_rng(seed)
    U, _ = np.linalg.qr(rng.standard_normal((n, n)))
    V, _ = np.linalg.qr(rng.standard_normal((n, n)))
    s = np.logspace(0, -np.log10(kappa), n)
    return np.asfortranarray((U * s) @ V.T)


def getrf(A):
    """LAPACK dgetf2 in fp64 (partial pivoting, first largest): (packed LU, 1-based ipiv)."""
    LU = np.array(A, dtype=np.float64, order="F")
    n = LU.shape[0]
    ipiv = np.zeros(n, dtype=np.int32)
    for k in range(n):
        p = k + int(np.argmax(np.abs(LU[k:, k])))
        ipiv[k] = p + 1
        if p != k:
            LU[[k, p], :] = LU[[p, k], :]
        if LU[k, k] != 0:
            LU[k + 1:, k] /= LU[k, k]
        LU[k + 1:, k + 1:] -= np.outer(LU[k + 1:, k], LU[k, k + 1:])
    return LU, ipiv


def lu_solver(LU, ipiv, trans):
    """v -> op(A)^-1 v from packed factors P A = L U by explicit substitution (v: N x k)."""
    LU = np.asarray(LU, dtype=np.float64)
    n = LU.shape[0]
    perm = np.arange(n)
    for i in range(n):
        p = int(ipiv[i]) - 1
        perm[[i, p]] = perm[[p, i]]

    try:   # LAPACK's dtrtrs where scipy is there (the same substitutions, much faster at N = 300)
        from scipy.linalg import solve_triangular as tri
    except ImportError:
        tri = None

    def solve(V):
        V = np.array(V, dtype=np.float64)
        if tri is not None and not trans:
            return tri(LU, tri(LU, V[perm], lower=True, unit_diagonal=True), lower=False)
        if tri is not None:
            out = np.empty_like(V)
            out[perm] = tri(LU, tri(LU, V, lower=False, trans=1), lower=True, unit_diagonal=True, trans=1)
            return out
        if not trans:
            Y = V[perm]
            for i in range(n):                       # L y = P v
                Y[i] -= LU[i, :i] @ Y[:i]
            for i in range(n - 1, -1, -1):           # U x = y
                Y[i] = (Y[i] - LU[i, i + 1:] @ Y[i + 1:]) / LU[i, i]
            return Y
        Y = V.copy()
        for i in range(n):                           # U^T w = v
            Y[i] = (Y[i] - LU[:i, i] @ Y[:i]) / LU[i, i]
        for i in range(n - 1, -1, -1):               # L^T z = w
            Y[i] -= LU[i + 1:, i] @ Y[i + 1:]
        out = np.empty_like(Y)
        out[perm] = Y                                # x = P^T z
        return out
    return solve


def clamp(max_outer, restart):
    """mpf_solve_gmres_ir's clamps."""
    if restart < 1:
        restart = 30
    restart = min(restart, 100)
    return min(max(max_outer, 1), 31), restart


def gmres_ir_column(opA, solve, b, max_outer, restart, tol):
    """One column.  Returns (x, stats); stats["cycles"]: per outer step that ran an inner loop a dict rel, beta, steps = [(h, hn)],
    k (the inner steps taken) and y."""
    max_outer, m = clamp(max_outer, restart)
    n = b.shape[0]
    col = lambda v: solve(v.reshape(n, 1)).reshape(n)
    nb2 = float(np.linalg.norm(b))
    if nb2 == 0:
        nb2 = 1.0
    x = col(b)
    st = {"converged": 0, "outer_iterations": 0, "inner_iterations": 0, "rel_residual": 0.0, "history": [], "cycles": [], "budget_expired": 0}
    outer = 0
    while True:
        r = b - opA @ x
        rel = float(np.linalg.norm(r)) / nb2
        st["history"].append(rel)
        st["outer_iterations"] = outer
        st["rel_residual"] = rel
        if rel <= tol:
            st["converged"] = 1
            break
        if outer >= max_outer or rel != rel:
            break
        z = col(r)
        beta = float(np.linalg.norm(z))
        cyc = {"rel": rel, "beta": beta, "steps": [], "k": 0, "y": []}
        st["cycles"].append(cyc)
        if beta == 0 or beta != beta:
            break
        V = np.zeros((n, m + 1))
        V[:, 0] = z * (1.0 / beta)
        H = np.zeros((m + 1, m))
        cs, sn, g = np.zeros(m), np.zeros(m), np.zeros(m + 1)
        g[0] = beta
        inner_tol = max(1e-14, min(1e-2, 0.1 * tol / rel))
        k = 0
        while k < m:
            w = col(opA @ V[:, k])
            h = V[:, :k + 1].T @ w
            w = w - V[:, :k + 1] @ h
            h2 = V[:, :k + 1].T @ w
            w = w - V[:, :k + 1] @ h2
            hn = float(np.sqrt(w @ w))
            H[:k + 1, k] = h + h2
            H[k + 1, k] = hn
            cyc["steps"].append(((h + h2).tolist(), hn))
            if hn > 0:
                V[:, k + 1] = w * (1.0 / hn)
            for i in range(k):
                t = cs[i] * H[i, k] + sn[i] * H[i + 1, k]
                H[i + 1, k] = -sn[i] * H[i, k] + cs[i] * H[i + 1, k]
                H[i, k] = t
            a, b2 = H[k, k], H[k + 1, k]
            den = float(np.hypot(a, b2))
            cs[k] = a / den if den > 0 else 1.0
            sn[k] = b2 / den if den > 0 else 0.0
            H[k, k] = den
            H[k + 1, k] = 0
            g[k + 1] = -sn[k] * g[k]
            g[k] = cs[k] * g[k]
            st["inner_iterations"] += 1
            k += 1
            if abs(g[k]) <= inner_tol * beta or hn == 0:
                break
        y = np.zeros(k)
        with np.errstate(all="ignore"):
            for i in range(k - 1, -1, -1):
                s2 = g[i]
                for j in range(i + 1, k):
                    s2 -= H[i, j] * y[j]
                y[i] = s2 / H[i, i]
            for i in range(k):
                x = x + y[i] * V[:, i]
        cyc["k"] = k
        cyc["y"] = y.tolist()
        outer += 1
    return x, st


def gmres_ir_model(A, M, B, trans=False, max_outer=10, restart=30, tol=1e-12):
    """All columns of B (N x nrhs), each on its own: (X, [stats])."""
    A = np.asarray(A, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    if B.ndim == 1:
        B = B.reshape(-1, 1)
    opA = A.T if trans else A
    solve = M if callable(M) else lu_solver(M[0], M[1], trans)
    X = np.zeros(B.shape, order="F")
    stats = []
    for j in range(B.shape[1]):
        X[:, j], st = gmres_ir_column(opA, solve, B[:, j], max_outer, restart, tol)
        stats.append(st)
    return X, stats


def classical_ir_converges(A, M, B, trans=False, max_iter=10, tol=1e-12):
    """Plain refinement's verdict per column (stop rule ||r|| <= tol ||b|| only): the fixture's guard."""
    opA = (np.asarray(A).T if trans else np.asarray(A))
    solve = M if callable(M) else lu_solver(M[0], M[1], trans)
    X = solve(B)
    nb = np.linalg.norm(B, axis=0)
    nb[nb == 0] = 1
    for _ in range(max_iter + 1):
        R = B - opA @ X
        rel = np.linalg.norm(R, axis=0) / nb
        if np.all(rel <= tol):
            break
        X = X + solve(R)
    return rel <= tol


def fixture(n, kappa, nrhs, trans, zero_col=None):
    """The issue's fixture: A = ill(n, kappa, 7); the "low-precision" matrix A16 = fp16(A) in fp64 (its fp64 factors are the
    preconditioner); B = op(A) X with X uniform in [-1, 1) from default_rng(1) and one zero column (the last but one, or column 0
    when there is only one... none then)."""
    A = ill(n, kappa, 7)
    A16 = np.asfortranarray(A.astype(np.float16).astype(np.float64))
    X = np.random.default_rng(1).uniform(-1, 1, (n, nrhs))
    B = np.asfortranarray((A.T if trans else A) @ X)
    if zero_col is None:
        zero_col = nrhs - 2 if nrhs >= 2 else None
    if zero_col is not None:
        B[:, zero_col] = 0
    return A, A16, B, zero_col
