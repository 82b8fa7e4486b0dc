"""numpy restatement of the blocked loop of mpf_getrf_batched_blocked for ONE matrix (include/mpf_c.h; csrc/batched_blocked.hip) -- test
infrastructure.

Per panel step: the panel by pivot64_model.panel_piv (mpf_dgetf2_piv's rule), the panel's interchanges on the columns left and right of
it, the U row block by forward substitution with k ascending, the trailing matrix by one K = nb update with k ascending.  `gemm` is the
in-place C -= L U whose chain per element is c = fma(-l_k, u_k, c), k ascending (the oracle's dgemm_minus, contract C5) for the fused
form; None is the unfused form, a rounded product and a rounded difference per k.  Every element sees the updates of the unblocked
batched_model.getrf_model in the same order, so the two agree bit for bit for any panel width; tests/test_batched_blocked_cpu.py checks
that, and that dropping one term at a panel seam does not go unnoticed."""
import numpy as np

import pivot64_model as P64


def _minus(Cm, L, U, gemm):
    """Cm -= L U in place, k ascending, one update per k."""
    if Cm.size == 0:
        return
    if gemm is not None:
        gemm(Cm, L, U)
        return
    for k in range(L.shape[1]):
        Cm -= np.outer(L[:, k], U[k, :])          # product and difference rounded separately


def getrf_blocked_model(A, nb, gemm=None, drop=None):
    """(LU, ipiv 1-based int32[n], info) of a copy of the n x n matrix A, by panels of nb columns.
    drop = (j0, k): the trailing update of the panel step that starts at column j0 leaves out its term k (a deliberately wrong loop)."""
    LU = np.array(A, dtype=np.float64, order="F", copy=True)
    n = LU.shape[0]
    ipiv = np.zeros(n, dtype=np.int32)
    info = 0
    with np.errstate(all="ignore"):
        for j0 in range(0, n, nb):
            jc = min(nb, n - j0)
            j1 = j0 + jc
            pv, inf = P64.panel_piv(LU[j0:, j0:j1], ipiv_offset=j0, rank1=gemm)
            ipiv[j0:j1] = pv
            if inf and not info:
                info = j0 + inf
            for j, g in enumerate(pv):                 # the interchanges, in order, on the columns outside the panel
                p, r = int(g) - 1, j0 + j
                if p != r:
                    LU[[r, p], :j0] = LU[[p, r], :j0]
                    LU[[r, p], j1:] = LU[[p, r], j1:]
            if j1 == n:
                break
            for k in range(jc - 1):                    # U row block: y_i -= l_ik y_k, k ascending
                _minus(LU[j0 + k + 1:j1, j1:], LU[j0 + k + 1:j1, j0 + k:j0 + k + 1], LU[j0 + k:j0 + k + 1, j1:], gemm)
            Lb, Ub, Cb = LU[j1:, j0:j1], LU[j0:j1, j1:], LU[j1:, j1:]
            if drop is not None and drop[0] == j0:
                keep = [k for k in range(jc) if k != drop[1]]
                _minus(Cb, np.asfortranarray(Lb[:, keep]), np.asfortranarray(Ub[keep, :]), gemm)
            else:
                _minus(Cb, Lb, Ub, gemm)
    return LU, ipiv, info
