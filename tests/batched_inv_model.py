"""numpy restatement of mpf_getri_batched and mpf_getdet_batched for ONE matrix of the batch (include/mpf_c.h) -- test infrastructure.

getri_model: the contract itself -- mpf_getrs_batched(trans = 0) on an identity, batched_model.getrs_model as it stands.
getri_model_skipping: a second, independent statement of the same chain, column by column and element by element, that never forms
the identity and skips what a kernel may skip: column k starts as e_q, the forward steps j < q are not carried out, rows above q are
never touched before the backward sweep.  The two agree bit for bit for finite factors (+0 - (+-0) = +0), the signs of zeros included.
getdet_model: mpf_getdet's order, re-exported from getri_model.py (n <= 128 is one chunk of it)."""
import numpy as np

import batched_model as M
from getri_model import dget03_ratio, getdet_model  # noqa: F401  (re-exported)


def getri_model(LU, ipiv):
    """inv(A) from the packed factors: the solve's chains on the identity."""
    n = LU.shape[0]
    return M.getrs_model(LU, ipiv, np.eye(n))


def start_rows(ipiv):
    """q[k]: the position row k reaches under the interchanges j = 0 .. n-1 (rows j and ipiv[j] - 1 change places)."""
    n = len(ipiv)
    q = np.arange(n)
    for j in range(n):
        p = int(ipiv[j]) - 1
        for k in range(n):
            if q[k] == j:
                q[k] = p
            elif q[k] == p:
                q[k] = j
    return q


def getri_model_skipping(LU, ipiv):
    """The same inverse as the header states it per element: the forward sweep one column at a time from the column's one downwards
    (nothing is computed on a structural zero), the backward sweep row-oriented (x_i -= u_ij x_j for j descending, then x_i /= u_ii;
    batched_model states it column-oriented).  The product is rounded, then the difference."""
    LU = np.asarray(LU, dtype=np.float64)
    n = LU.shape[0]
    q = start_rows(ipiv)
    X = np.zeros((n, n))
    with np.errstate(all="ignore"):
        for k in range(n):
            x = X[:, k]
            x[q[k]] = 1.0
            for j in range(q[k], n - 1):                   # L: x_i -= l_ij x_j, rows below j only
                t = LU[j + 1:, j] * x[j]
                x[j + 1:] = x[j + 1:] - t
        for i in range(n - 1, -1, -1):                     # U: row i of X for all columns at once
            for j in range(n - 1, i, -1):
                t = LU[i, j] * X[j]
                X[i] = X[i] - t
            X[i] = X[i] / LU[i, i]
    return X
