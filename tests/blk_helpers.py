"""Helpers shared by the GPU tests of the solve layer (test_gpu_getrs, _gerfs, _gerfsx, _gmres_block, _gesvx_block, _expert): the test
matrices, device copies with a padded leading dimension, the factors, bit comparisons, and host solves with the device's factors."""
import numpy as np


def rand(n, seed, dominant=2.0):
    """Uniform (-1, 1) entries, `dominant` added to the diagonal (0.5 at n = 1; None: the diagonal as drawn), column-major."""
    A = np.random.default_rng(seed).uniform(-1, 1, (n, n))
    if dominant is not None:
        A[np.arange(n), np.arange(n)] += dominant if n > 1 else 0.5
    return np.asfortranarray(A)


def ill(n, kappa, seed):
    """Singular values spread evenly in the exponent over 1 .. 1 / kappa between two random orthogonal matrices."""
    rng = np.random.default_rng(seed)
    U, _ = np.linalg.qr(rng.standard_normal((n, n)))
    V, _ = np.linalg.qr(rng.standard_normal((n, n)))
    s = np.logspace(0, -np.log10(kappa), n)
    return np.asfortranarray((U * s) @ V.T)


def factor(ctx, A_np, ld=None, nb=128, trailing=0, check=True):
    """(device copy of A, its factors stored with leading dimension ld, ipiv, info); info == 0 is asserted unless check=False."""
    n = A_np.shape[0]
    dA = ctx.from_numpy_f(A_np)
    W = ctx.colmajor(ld or n, n)[:n]
    W.copy_(dA)
    ipiv, info = ctx.factor(W, nb, trailing=trailing)
    ctx.synchronize()
    assert info == 0 or not check
    return dA, W, ipiv, info


def dev(ctx, M_np, ld=None, fill=7.5):
    """Column-major device copy of M with leading dimension ld (rows beyond N hold `fill`): (the N-row view, the whole buffer)."""
    import torch
    n, m = M_np.shape
    buf = ctx.colmajor(ld or n, m)
    buf.fill_(fill)
    v = buf[:n]
    v.copy_(torch.from_numpy(np.ascontiguousarray(M_np)))
    return v, buf


def ld(t):
    """Leading dimension of a column-major device matrix."""
    return t.stride(1) if t.shape[1] > 1 else max(t.shape[0], 1)


def bits(a):
    """The uint64 bit patterns of an array (or of a tensor's host copy), C-contiguous."""
    if hasattr(a, "cpu"):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a).view(np.uint64)


def tensor_bits(t):
    """The uint64 bit patterns of a device tensor in its own layout."""
    return t.cpu().numpy().view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def host_solvers(LU, ipiv, trans):
    """(solve, solve_t) = (op(A)^-1 V, op(A)^-T V) on the host with the DEVICE's factors P A = L U, as products with the explicit
    (L U)^-1: a model's solves are then one matrix product each."""
    n = LU.shape[0]
    perm = np.arange(n)
    for i, p in enumerate(np.asarray(ipiv, dtype=np.int64) - 1):
        perm[[i, p]] = perm[[p, i]]
    M = np.linalg.inv((np.tril(LU, -1) + np.eye(n)) @ np.triu(LU))

    def inv(v):
        return M @ v[perm]

    def inv_t(v):
        out = np.empty_like(v)
        out[perm] = M.T @ v
        return out
    return (inv_t, inv) if trans else (inv, inv_t)
