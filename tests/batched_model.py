"""numpy restatement of mpf_getrf_batched and mpf_getrs_batched for ONE matrix of the batch (include/mpf_c.h) -- test infrastructure.

getrf_model: the factorization is mpf_dgetf2_piv's on an n x n panel, so the model is pivot64_model.panel_piv as it stands (for
fused = 1 the caller passes the oracle's one-FMA update as rank1).
getrs_model: dgetrs's chains, column-oriented -- every element sees the same operations in the same order as in the row-oriented
statement of the header; numpy rounds the product, then the difference (always unfused)."""
import numpy as np

import pivot64_model as P64


def getrf_model(A, rank1=None):
    """(LU, ipiv 1-based int32[n], info) of a copy of the n x n matrix A."""
    LU = np.array(A, dtype=np.float64, order="F", copy=True)
    ipiv, info = P64.panel_piv(LU, 0, rank1)
    return LU, ipiv, info


def _swap(X, j, p):
    if p != j:
        X[[j, p], :] = X[[p, j], :]


def getrs_model(LU, ipiv, B, trans=False):
    """X = A^-1 B (trans False) or A^-T B from the factors; B is (n, nrhs) or (n,).  Returns a new array of B's shape."""
    n = LU.shape[0]
    X = np.array(B, dtype=np.float64, copy=True).reshape(n, -1)
    with np.errstate(all="ignore"):
        if not trans:
            for j in range(n):
                _swap(X, j, int(ipiv[j]) - 1)
            for j in range(n):                              # L: b_i -= l_ij b_j
                X[j + 1:] -= np.outer(LU[j + 1:, j], X[j])
            for j in range(n - 1, -1, -1):                  # U: b_j /= u_jj, then b_i -= u_ij b_j
                X[j] = X[j] / LU[j, j]
                X[:j] -= np.outer(LU[:j, j], X[j])
        else:
            for j in range(n):                              # U^T: b_j /= u_jj, then b_i -= u_ji b_j
                X[j] = X[j] / LU[j, j]
                X[j + 1:] -= np.outer(LU[j, j + 1:], X[j])
            for j in range(n - 1, -1, -1):                  # L^T: b_i -= l_ji b_j
                X[:j] -= np.outer(LU[j, :j], X[j])
            for j in range(n - 1, -1, -1):
                _swap(X, j, int(ipiv[j]) - 1)
    return X.reshape(np.shape(B))
