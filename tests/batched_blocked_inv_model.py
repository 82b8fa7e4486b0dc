"""numpy restatement of mpf_getri_batched_blocked and mpf_getdet_batched_blocked for ONE matrix of the batch (include/mpf_c.h;
csrc/batched_blocked.hip: bb_getri_kernel, bb_getdet_kernel) -- test infrastructure.

getri_blocked_model: the algorithm as built.  inv(A) = inv(U) inv(L) P, so column k of the result is column q(k) of inv(L) taken
through the backward sweep; the interchanges are one composed map and no arithmetic.  The columns of inv(L) are taken in ascending q
in tiles of `ct`; a tile starts as columns q0 .. q0 + ct - 1 of the identity, its forward sweep starts at the block of `bs` rows that
holds q0 (rows above stay +0), every block is solved and its steps are then applied, in order, to the rows beyond it; the backward
sweep runs over all blocks; the tile is stored at columns k(q).  The product is rounded, then the difference.  The contract
(batched_inv_model.getri_model, the solve's chains on an identity) is met bit for bit for any ct and bs.
drop = (sweep, j): leave out step j's terms for the rows beyond its block in sweep "L" or "U" -- what a kernel that loses a term at a
block seam would compute; the tests check that the answer changes.

getdet_chunked_model: bb_getdet_kernel's structure -- (m_i, e_i) = frexp(u_ii) for every entry first, one chain per chunk of 256 with
the exponent in 32 bits, then the combining chain."""
import math

import numpy as np

CHUNK = 256


def clean_pivots(ipiv, n):
    """0-based pivots; an entry outside 1 .. n reads as "no interchange"."""
    p = np.asarray(ipiv, dtype=np.int64)[:n] - 1
    j = np.arange(n)
    return np.where((p < 0) | (p >= n), j, p)


def column_map(ipiv, n):
    """k[q]: the column of the result that starts as e_q, i.e. the row that stands at position q after the interchanges."""
    p = clean_pivots(ipiv, n)
    pos = np.arange(n)                                   # pos[t]: where row t stands
    for j in range(n):
        pj = p[j]
        pos = np.where(pos == j, pj, np.where(pos == pj, j, pos))
    k = np.empty(n, dtype=np.int64)
    k[pos] = np.arange(n)
    return k


def getri_blocked_model(LU, ipiv, ct=16, bs=32, drop=None):
    LU = np.asarray(LU, dtype=np.float64)
    n = LU.shape[0]
    k = column_map(ipiv, n)
    nblk = (n + bs - 1) // bs
    X = np.full((n, n), np.nan)
    with np.errstate(all="ignore"):
        for q0 in range(0, n, ct):
            w = min(ct, n - q0)
            x = np.zeros((n, w))
            x[q0 + np.arange(w), np.arange(w)] = 1.0
            for kb in range(q0 // bs, nblk):             # L: x_i -= l_ij x_j, j ascending; the blocks above q0 meet zeros only
                r0, r1 = kb * bs, min(n, kb * bs + bs)
                for j in range(r0, r1):
                    x[j + 1:r1] -= np.outer(LU[j + 1:r1, j], x[j])
                for j in range(r0, r1):
                    if drop != ("L", j):
                        x[r1:] -= np.outer(LU[r1:, j], x[j])
            for kb in range(nblk - 1, -1, -1):           # U: x_j /= u_jj, then x_i -= u_ij x_j, j descending; nothing is skipped
                r0, r1 = kb * bs, min(n, kb * bs + bs)
                for j in range(r1 - 1, r0 - 1, -1):
                    x[j] = x[j] / LU[j, j]
                    x[r0:j] -= np.outer(LU[r0:j, j], x[j])
                for j in range(r1 - 1, r0 - 1, -1):
                    if drop != ("U", j):
                        x[:r0] -= np.outer(LU[:r0, j], x[j])
            X[:, k[q0:q0 + w]] = x
    return X


def getdet_chunked_model(diag, ipiv):
    """(mant, expo) as bb_getdet_kernel forms them; expo is checked to fit 32 bits at every step."""
    d = np.asarray(diag, dtype=np.float64)
    n = len(d)
    if n == 0:
        return 0.5, 1
    m, e = np.frexp(d)
    bad = not bool(np.all(np.abs(d) <= np.finfo(np.float64).max))
    zero = bool(np.any(d == 0.0))
    flips = int(np.count_nonzero(np.asarray(ipiv)[:n] != np.arange(1, n + 1))) & 1

    def step(p, ee, mi, ei):
        p, kk = math.frexp(p * mi)
        ee = ee + kk + int(ei)
        assert -2 ** 31 <= ee < 2 ** 31
        return p, ee

    parts = []
    for c0 in range(0, n, CHUNK):
        p, ee = 1.0, 0
        for i in range(c0, min(n, c0 + CHUNK)):
            p, ee = step(p, ee, float(m[i]), e[i])
        parts.append((p, ee))
    P, E = 1.0, 0
    for p, ee in parts:
        P, E = step(P, E, p, ee)
    if flips:
        P = -P
    if bad:
        return math.nan, 0
    if zero:
        return 0.0, 0
    return P, E
