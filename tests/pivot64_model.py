"""numpy restatement of the fp64 pivot search (include/mpf_c.h: mpf_dgetf2_piv, mpf_opts.pivot_search = 1) -- test infrastructure.

panel_piv: LAPACK dgetf2 column by column -- idamax (first maximum), the swap, the division, one UNFUSED rank-1 update.  Per element
that is mpf_dgetf2_npv's arithmetic (contract C3), so its bits are those of the no-pivot panel on the pre-permuted rows.
factor_piv: the panel loop of mpf_factor_dev (MPF.cu:100-242) around it with plain numpy for TRSM and GEMM: whole-matrix factors
are good to a tolerance only (another summation order than the device's kernels)."""
import numpy as np


def panel_piv(P, ipiv_offset=0, rank1=None):
    """In place on the (rows, cols) array P.  Returns (ipiv int32[min(rows, cols)] = pivot row + 1 + ipiv_offset, info).
    rank1(C, l, u): another in-place C -= l u (l a column, u a row, views of P) -- the tests pass the oracle's one-FMA update
    for the fused form; None is the unfused numpy one."""
    rows, cols = P.shape
    kmax = min(rows, cols)
    ipiv = np.zeros(kmax, dtype=np.int32)
    info = 0
    with np.errstate(all="ignore"):
        for j in range(kmax):
            col = np.abs(P[j:, j])
            col = np.where(np.isnan(col), 0.0, col)       # a NaN never beats a number; an all-NaN rest keeps p = j
            p = j + int(np.argmax(col))                   # first maximum
            ipiv[j] = p + 1 + ipiv_offset
            if p != j:
                P[[j, p], :] = P[[p, j], :]
            if P[j, j] == 0.0 and info == 0:
                info = j + 1
            l = P[j + 1:, j] / P[j, j]
            P[j + 1:, j] = l
            if rank1 is None:
                P[j + 1:, j + 1:] -= np.outer(l, P[j, j + 1:])   # product and difference rounded separately
            elif j + 1 < rows and j + 1 < cols:
                rank1(P[j + 1:, j + 1:], P[j + 1:, j:j + 1], P[j:j + 1, j + 1:])
    return ipiv, info


def permute_rows(P, ipiv, ipiv_offset=0):
    """The panel with its rows pre-permuted by panel_piv's pivots (a copy)."""
    Q = P.copy(order="F")
    for j, pv in enumerate(ipiv):
        p = int(pv) - 1 - ipiv_offset
        if p != j:
            Q[[j, p], :] = Q[[p, j], :]
    return Q


def factor_piv(A, nb):
    """The loop of mpf_factor_dev with pivot_search = 1 on a copy of A.  Returns (LU, ipiv): ipiv is pre-initialised to the identity
    and the entry of a 1 x 1 tail stays untouched (MPF.cu:104)."""
    A = np.array(A, dtype=np.float64, order="F")
    n = A.shape[0]
    ipiv = np.arange(1, n + 1, dtype=np.int32)
    for k in range(0, n, nb):
        pc, pr = min(nb, n - k), n - k
        if pr <= 1:
            break
        P = A[k:, k:k + pc]
        pv, _ = panel_piv(P, ipiv_offset=k)
        ipiv[k:k + pc] = pv
        for j, g in enumerate(pv):                          # interchange of the columns left and right of the panel
            p, r = int(g) - 1, k + j
            if p != r:
                A[[r, p], :k] = A[[p, r], :k]
                A[[r, p], k + pc:] = A[[p, r], k + pc:]
        if k + pc < n:
            L11 = np.tril(A[k:k + pc, k:k + pc], -1) + np.eye(pc)
            A[k:k + pc, k + pc:] = np.linalg.solve(L11, A[k:k + pc, k + pc:])
            A[k + pc:, k + pc:] -= A[k + pc:, k:k + pc] @ A[k:k + pc, k + pc:]
    return A, ipiv


def plu_residual(A, LU, ipiv):
    """||P A - L U||_F / ||A||_F for 1-based sequential pivots."""
    n = A.shape[0]
    PA = np.array(A, dtype=np.float64)
    for j, g in enumerate(ipiv):
        p = int(g) - 1
        if p != j:
            PA[[j, p], :] = PA[[p, j], :]
    L = np.tril(LU, -1) + np.eye(n)
    U = np.triu(LU)
    return float(np.linalg.norm(PA - L @ U) / np.linalg.norm(A))
