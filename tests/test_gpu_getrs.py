"""GPU tests of the blocked multi-right-hand-side solve (include/mpf_c.h: mpf_getrs, mpf_solve_ir_block)."""
import ctypes as C

import numpy as np
import pytest

import blk_helpers as H

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
IRS = ("iterations", "converged", "rel_residual", "stalled")


def _kappa(A):
    return np.linalg.norm(A, 1) * np.linalg.norm(np.linalg.inv(A), 1)


def _st(s):
    return tuple(getattr(s, f) for f in IRS) + tuple(s.history[:s.iterations + 1])


@pytest.mark.parametrize("n", [1, 2, 63, 255, 256, 257, 777, 1024, 4096])
@pytest.mark.parametrize("trans", [0, 1])
def test_getrs_accuracy(ctx, n, trans):
    """getrs of fp64 factors is within 10 N kappa eps of numpy for every column; rows beyond N of B stay untouched."""
    import torch
    ld = 800 if n == 777 else n
    A = H.rand(n, 300 + n)
    dA, W, ipiv, info = H.factor(ctx, A, ld=ld)
    assert info == 0
    kappa = _kappa(A)
    Aop = A.T if trans else A
    for nrhs in (1, 2, 15, 16, 17, 64, 65, 200):
        B_np = np.random.default_rng(nrhs).uniform(-1, 1, (n, nrhs))
        buf = ctx.colmajor(ld, nrhs)
        buf.fill_(7.5)
        B = buf[:n]
        B.copy_(torch.from_numpy(B_np))
        X = ctx.getrs(W, ipiv, B, trans=trans, overwrite=True)
        ctx.synchronize()
        assert X.data_ptr() == B.data_ptr()
        X_ref = np.linalg.solve(Aop, B_np)
        err = np.abs(X.cpu().numpy() - X_ref).max(axis=0) / np.abs(X_ref).max(axis=0)
        assert err.max() <= 10 * n * kappa * EPS, (nrhs, err.max(), kappa)
        if ld > n:
            assert bool((buf[n:] == 7.5).all()), "padding rows of B were written"


@pytest.mark.parametrize("trans", [0, 1])
def test_getrs_group_seam(ctx, trans):
    """513 right-hand sides are two groups (512 + 1 columns): the columns at the tile seam (31, 32) and at the group seam (511, 512)
    have the bits of the same column solved alone, and with ldb = N + 3 the rows beyond N of B stay untouched."""
    import torch
    n, nrhs, ldb = 64, 513, 67
    dA, W, ipiv, _ = H.factor(ctx, H.rand(n, 17), nb=32)
    B_np = np.random.default_rng(8).uniform(-1, 1, (n, nrhs))
    B, buf = H.dev(ctx, B_np, ldb)
    X = ctx.getrs(W, ipiv, B, trans=trans, overwrite=True)
    ctx.synchronize()
    assert X.data_ptr() == B.data_ptr()
    assert bool((buf[n:] == 7.5).all()), "padding rows of B were written"
    for j in (0, 31, 32, 511, 512):
        bj = torch.from_numpy(B_np[:, j:j + 1].copy()).to(ctx.device)
        x1 = ctx.getrs(W, ipiv, bj, trans=trans)
        assert np.array_equal(H.tensor_bits(x1)[:, 0], H.tensor_bits(X)[:, j]), j


def test_getrs_keeps_b(ctx):
    """Without overwrite, getrs returns a new X and leaves B as it was."""
    import torch
    n = 300
    A = H.rand(n, 5)
    dA, W, ipiv, _ = H.factor(ctx, A, check=False)
    B = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, (n, 3))).to(ctx.device)
    B0 = B.clone()
    X = ctx.getrs(W, ipiv, B)
    ctx.synchronize()
    assert torch.equal(B, B0) and X.data_ptr() != B.data_ptr()
    assert np.allclose(X.cpu().numpy(), np.linalg.solve(A, B0.cpu().numpy()), rtol=0, atol=1e-10)


@pytest.mark.parametrize("trans", [0, 1])
def test_getrs_agrees_with_column_solves(ctx, trans):
    """N = 8192, 64 columns: getrs agrees with solve_ir_nrhs / solve_ir_trans at max_iter = 0 within 10 N kappa eps."""
    import torch
    n, nrhs = 8192, 64
    A = H.rand(n, 77, dominant=float(n) ** 0.5)
    dA, W, ipiv, info = H.factor(ctx, A, nb=256)
    assert info == 0
    B = torch.from_numpy(np.random.default_rng(2).uniform(-1, 1, (n, nrhs))).to(ctx.device).t().contiguous().t()
    X = ctx.getrs(W, ipiv, B, trans=trans).cpu().numpy()
    if trans:
        X0, _ = ctx.solve_ir_trans(dA, W, ipiv, B, max_iter=0)
    else:
        X0, _ = ctx.solve_ir_nrhs(dA, W, ipiv, B, max_iter=0)
    X0 = X0.cpu().numpy()
    kappa = ctx.cond(dA, W)
    err = np.abs(X - X0).max(axis=0) / np.abs(X0).max(axis=0)
    assert err.max() <= 10 * n * kappa * EPS, (err.max(), kappa)


@pytest.mark.parametrize("trans", [0, 1])
def test_column_independence(ctx, trans):
    """A column's bits do not depend on the other columns, on nrhs or on its position; two calls give the same bits.
    For getrs and for solve_ir_block (X and every stats field but ms_total)."""
    import torch
    n, nrhs = 1000, 37
    A = H.rand(n, 11)
    dA, W16, ipiv16, _ = H.factor(ctx, A, trailing=1, check=False)
    B = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (n, nrhs)) * np.logspace(-3, 3, nrhs)).to(ctx.device)
    B = B.t().contiguous().t()
    perm = np.random.default_rng(4).permutation(nrhs)
    Bp = B[:, torch.from_numpy(perm).to(ctx.device)].t().contiguous().t()
    X = ctx.getrs(W16, ipiv16, B, trans=trans)
    Xr = ctx.getrs(W16, ipiv16, B, trans=trans)
    Xp = ctx.getrs(W16, ipiv16, Bp, trans=trans)
    assert np.array_equal(H.tensor_bits(X), H.tensor_bits(Xr))
    Y, S = ctx.solve_ir_block(dA, W16, ipiv16, B, trans=trans, max_iter=10, tol=1e-12)
    Yr, Sr = ctx.solve_ir_block(dA, W16, ipiv16, B, trans=trans, max_iter=10, tol=1e-12)
    Yp, Sp = ctx.solve_ir_block(dA, W16, ipiv16, Bp, trans=trans, max_iter=10, tol=1e-12)
    assert np.array_equal(H.tensor_bits(Y), H.tensor_bits(Yr))
    assert [_st(s) for s in S] == [_st(s) for s in Sr]
    assert all(s.ms_total == S[0].ms_total for s in S)
    where = {int(j): i for i, j in enumerate(perm)}
    for j in (0, 16, 36):
        bj = B[:, j:j + 1].contiguous()
        x1 = ctx.getrs(W16, ipiv16, bj, trans=trans)
        assert np.array_equal(H.tensor_bits(x1)[:, 0], H.tensor_bits(X)[:, j]), j
        assert np.array_equal(H.tensor_bits(Xp)[:, where[j]], H.tensor_bits(X)[:, j]), j
        y1, s1 = ctx.solve_ir_block(dA, W16, ipiv16, bj, trans=trans, max_iter=10, tol=1e-12)
        assert np.array_equal(H.tensor_bits(y1)[:, 0], H.tensor_bits(Y)[:, j]), j
        assert np.array_equal(H.tensor_bits(Yp)[:, where[j]], H.tensor_bits(Y)[:, j]), j
        assert _st(s1[0]) == _st(S[j]) == _st(Sp[where[j]]), j


@pytest.mark.parametrize("trans", [0, 1])
def test_block_refinement_fp16(ctx, trans):
    """fp16 factors of a diagonally dominant N = 4096 matrix, 40 columns scaled 1e-6 .. 1e6 and one zero column: every column
    converges to 1e-12, the numpy residual is <= 1e-11 ||b||, iteration counts are within 1 of the per-column solve's."""
    import torch
    n, nrhs = 4096, 40
    A = H.rand(n, 21, dominant=float(n) ** 0.5)
    dA, W, ipiv, info = H.factor(ctx, A, nb=256, trailing=1)
    assert info == 0
    B_np = np.random.default_rng(5).uniform(-1, 1, (n, nrhs)) * np.logspace(-6, 6, nrhs)
    B_np[:, 7] = 0.0
    B = torch.from_numpy(B_np).to(ctx.device).t().contiguous().t()
    X, S = ctx.solve_ir_block(dA, W, ipiv, B, trans=trans, max_iter=10, tol=1e-12)
    if trans:
        X0, S0 = ctx.solve_ir_trans(dA, W, ipiv, B, max_iter=10, tol=1e-12)
    else:
        X0, S0 = ctx.solve_ir_nrhs(dA, W, ipiv, B, max_iter=10, tol=1e-12)
    Xn = X.cpu().numpy()
    Aop = A.T if trans else A
    for j in range(nrhs):
        assert S[j].converged == 1 and S[j].rel_residual <= 1e-12, (j, list(S[j].history)[:S[j].iterations + 1])
        r = np.linalg.norm(B_np[:, j] - Aop @ Xn[:, j])
        assert r <= 1e-11 * max(np.linalg.norm(B_np[:, j]), np.finfo(float).tiny), (j, r)
        assert abs(S[j].iterations - S0[j].iterations) <= 1, (j, S[j].iterations, S0[j].iterations)
    assert not Xn[:, 7].any() and S[7].converged == 1


def _stopped_as_ir_core(s, max_iter):
    h = s.history[s.iterations]
    return s.stalled == 1 or s.iterations == max_iter or h != h


@pytest.mark.parametrize("trans", [0, 1])
def test_block_refinement_ill_conditioned(ctx, trans):
    """kappa ~ 1e9 on fp16 factors: no column converges in either path, every column stops by ir_core's rules, and its history
    is finite up to the stop wherever the per-column solve's is."""
    import torch
    n, nrhs, mi = 1024, 8, 10
    A = H.ill(n, 1e9, 31)
    dA, W, ipiv, _ = H.factor(ctx, A, nb=256, trailing=1, check=False)
    B = torch.from_numpy(np.random.default_rng(6).uniform(-1, 1, (n, nrhs))).to(ctx.device).t().contiguous().t()
    X, S = ctx.solve_ir_block(dA, W, ipiv, B, trans=trans, max_iter=mi, tol=1e-12)
    if trans:
        _, S0 = ctx.solve_ir_trans(dA, W, ipiv, B, max_iter=mi, tol=1e-12)
    else:
        _, S0 = ctx.solve_ir_nrhs(dA, W, ipiv, B, max_iter=mi, tol=1e-12)
    for j in range(nrhs):
        assert S[j].converged == 0 and S0[j].converged == 0, j
        assert _stopped_as_ir_core(S[j], mi), (j, S[j].iterations, S[j].stalled)
        h, h0 = np.array(S[j].history[:S[j].iterations + 1]), np.array(S0[j].history[:S0[j].iterations + 1])
        k = min(len(h), len(h0))
        assert np.all(np.isfinite(h[:k]) | ~np.isfinite(h0[:k])), (j, h, h0)


def test_arguments(ctx, mpf):
    """nrhs = 0 -> 0; N <= 0, ldb / ldx / ldlu < N -> -1 with the error set; a bad ipiv entry -> -1."""
    import torch
    n = 64
    A = H.rand(n, 9)
    dA, W, ipiv, _ = H.factor(ctx, A, check=False)
    B = ctx.from_numpy_f(np.ones((n, 2)))
    X = ctx.colmajor(n, 2)
    L, h = ctx.L, ctx.h
    p = lambda t: C.c_void_p(t.data_ptr())
    ctx._bind()
    st = (mpf.MpfIrStats * 2)()
    assert L.mpf_getrs(h, 0, p(W), n, p(ipiv), n, 0, p(B), n) == 0
    assert L.mpf_solve_ir_block(h, 0, p(dA), n, p(W), n, p(ipiv), n, 0, p(B), n, p(X), n, 3, 1e-12, st) == 0
    for args in ((0, p(W), n, p(ipiv), 0, 2, p(B), n), (0, p(W), n, p(ipiv), -3, 2, p(B), n),
                 (0, p(W), n, p(ipiv), n, 2, p(B), n - 1), (0, p(W), n - 1, p(ipiv), n, 2, p(B), n),
                 (2, p(W), n, p(ipiv), n, 2, p(B), n)):
        assert L.mpf_getrs(h, *args) == -1, args
        assert L.mpf_last_error(h).decode()
    assert L.mpf_solve_ir_block(h, 0, p(dA), n, p(W), n, p(ipiv), n, 2, p(B), n, p(X), n - 1, 3, 1e-12, st) == -1
    assert L.mpf_solve_ir_block(h, 1, p(dA), n, p(W), n - 1, p(ipiv), n, 2, p(B), n, p(X), n, 3, 1e-12, st) == -1
    bad = ipiv.clone()
    bad[5] = n + 7
    assert L.mpf_getrs(h, 0, p(W), n, p(bad), n, 2, p(B), n) == -1
    assert "ipiv" in L.mpf_last_error(h).decode()
    assert L.mpf_solve_ir_block(h, 0, p(dA), n, p(W), n, p(bad), n, 2, p(B), n, p(X), n, 3, 1e-12, st) == -1
    torch.cuda.synchronize()
