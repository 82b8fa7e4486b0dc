"""numpy restatement of tournament pivoting (include/mpf_c.h: mpf_dgetf2_tp, mpf_opts.pivot_search = 2) -- test infrastructure.

select:     LAPACK's partial pivoting (first maximum among the CURRENT positions, interchange, unfused elimination) on a private copy
            of a stack of <= 256 rows: the rows it takes, in order.
tournament: the winners of one 32-column sub-panel: select on every group of 256 active rows, then on the stacked lists of eight
            groups at a time (the rows' values as they were on entry), until one list is left.
panel_tp:   the panel by sub-panels of 32 columns: tournament, the winners as sequential LAPACK interchanges, the sub-panel without
            pivoting (one UNFUSED update per element and k: contract C3), the U row-block and the update right of it.
factor_tp:  the panel loop of mpf_factor_dev around it with plain numpy for TRSM and GEMM (good to a tolerance only)."""
import numpy as np

from pivot64_model import permute_rows, plu_residual  # noqa: F401  (re-exported: the tests take them from here)

IB = 32       # sub-panel width (DV_IB)
GROUP = 256   # rows of a level-0 group, and the tallest stack of a merge
FAN = 8       # lists merged at a time (FAN * IB = GROUP)


def select(S):
    """Ordered list of min(m, w) positions (rows of S as given) of the (m, w) stack S: the rows LAPACK's dgetf2 would take, in
    order, on a private copy.  S is not changed."""
    X = np.array(S, dtype=np.float64)
    m, w = X.shape
    perm = list(range(m))                                       # perm[i]: the row of S that stands at position i now
    out = []
    with np.errstate(all="ignore"):
        for s in range(min(m, w)):
            key = np.abs(X[perm[s:], s])
            key = np.where(np.isnan(key), 0.0, key)            # a NaN counts as 0
            i = s + int(np.argmax(key))                        # first maximum; all keys 0: position s itself
            perm[s], perm[i] = perm[i], perm[s]                # the interchange
            p, rest = perm[s], perm[s + 1:]
            out.append(p)
            mult = X[rest, s] / X[p, s]
            X[rest, s + 1:] = X[rest, s + 1:] - np.outer(mult, X[p, s + 1:])   # product and difference rounded separately
    return out


def tournament(V, row0=0):
    """The winners (row indices, row0 + position in V) of the (m, w) array V of active rows, m >= w, in ranking order."""
    m, w = V.shape
    lists = []
    for g0 in range(0, m, GROUP):
        lists.append([g0 + p for p in select(V[g0:g0 + GROUP])])
    while len(lists) > 1:
        merged = []
        for i in range(0, len(lists), FAN):
            stack = [r for lst in lists[i:i + FAN] for r in lst]
            merged.append([stack[p] for p in select(V[stack])])
        lists = merged
    return [row0 + r for r in lists[0]]


def panel_tp(P, ipiv_offset=0, rank1=None):
    """In place on the (rows, cols) array P.  Returns (ipiv int32[min(rows, cols)] = pivot row + 1 + ipiv_offset, info).
    rank1(C, l, u): another in-place C -= l u for the FACTORIZATION (the fused form); the selection is unfused whatever it is."""
    rows, cols = P.shape
    kmax = min(rows, cols)
    ipiv = np.zeros(kmax, dtype=np.int32)
    info = 0
    with np.errstate(all="ignore"):
        for j0 in range(0, kmax, IB):
            w = min(IB, kmax - j0)
            q = tournament(P[j0:, j0:j0 + w], j0)
            where = {}                                          # original row -> where it stands now (identity if absent)
            who = {}                                            # row -> the original row that stands there
            for s in range(w):
                p = where.get(q[s], q[s])
                ipiv[j0 + s] = p + 1 + ipiv_offset
                r = j0 + s
                if p != r:
                    P[[r, p], :] = P[[p, r], :]
                    a, b = who.get(r, r), who.get(p, p)
                    who[r], who[p] = b, a
                    where[a], where[b] = p, r
            for j in range(j0, j0 + w):                         # no pivoting: the rows that won are in place
                if P[j, j] == 0.0 and info == 0:
                    info = j + 1
                l = P[j + 1:, j] / P[j, j]
                P[j + 1:, j] = l
                if rank1 is None:
                    P[j + 1:, j + 1:] -= np.outer(l, P[j, j + 1:])
                elif j + 1 < rows and j + 1 < cols:
                    rank1(P[j + 1:, j + 1:], P[j + 1:, j:j + 1], P[j:j + 1, j + 1:])
    return ipiv, info


def factor_tp(A, nb):
    """The loop of mpf_factor_dev with pivot_search = 2 on a copy of A.  Returns (LU, ipiv) like pivot64_model.factor_piv."""
    A = np.array(A, dtype=np.float64, order="F")
    n = A.shape[0]
    ipiv = np.arange(1, n + 1, dtype=np.int32)
    for k in range(0, n, nb):
        pc, pr = min(nb, n - k), n - k
        if pr <= 1:
            break
        pv, _ = panel_tp(A[k:, k:k + pc], ipiv_offset=k)
        ipiv[k:k + pc] = pv
        for j, g in enumerate(pv):                              # interchange of the columns left and right of the panel
            p, r = int(g) - 1, k + j
            if p != r:
                A[[r, p], :k] = A[[p, r], :k]
                A[[r, p], k + pc:] = A[[p, r], k + pc:]
        if k + pc < n:
            L11 = np.tril(A[k:k + pc, k:k + pc], -1) + np.eye(pc)
            A[k:k + pc, k + pc:] = np.linalg.solve(L11, A[k:k + pc, k + pc:])
            A[k + pc:, k + pc:] -= A[k + pc:, k:k + pc] @ A[k:k + pc, k + pc:]
    return A, ipiv
