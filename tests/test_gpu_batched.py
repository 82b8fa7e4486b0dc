"""GPU tests of the batched LU (include/mpf_c.h: mpf_getrf_batched, mpf_getrs_batched; csrc/batched.hip).

Sizes: 1, 2, 3 (almost nothing below the pivot), 7 / 8 / 9, 16 / 17, 31 / 32 / 33 (the seams of the wave form's widths 8, 16, 32 and its
crossover to the workgroup form), 63 / 64 / 65 (the workgroup form's 64- and 128-row thread layouts; the solve's one and two rows per
lane), 100, 127, 128 (the largest).  Odd n with packed matrices takes the 8-byte loads, even n the 16-byte ones.

Bit checks need no tolerance: the model of the factorization is tests/pivot64_model.py (for fused = 1 with the oracle's one-FMA
update, as tests/test_gpu_pivot64.py does), the model of the solve tests/batched_model.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import batched_model as M

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 7, 8, 9, 16, 17, 31, 32, 33, 63, 64, 65, 100, 127, 128]
KINDS = ["normal", "ints", "tiny", "last_row", "sorted"]


def _bits(a):
    if hasattr(a, "cpu"):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a).view(np.uint64)


def _same_with_nans(got, want):
    """Equal bits where `want` is a number, NaN where it is NaN (a NaN's sign and payload are not part of the contract)."""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(np.where(nan, 0.0, got)), _bits(np.where(nan, 0.0, want)))


def _matrix(n, kind, seed=0):
    rng = np.random.default_rng(n * 1009 + 13 * seed + KINDS.index(kind))
    A = rng.standard_normal((n, n))
    if kind == "ints":                    # many exact ties: the first maximum must win
        A = rng.integers(-3, 4, (n, n)).astype(np.float64)
    elif kind == "tiny":                  # far below fp16's range
        A *= 2.0 ** -40
    elif kind == "sorted":                # rows in pivot order already: no interchange at all
        A = _permuted(A)
    elif kind == "last_row":              # every column takes its pivot from the LAST row: the row that moves there carries 1000 in the next column
        A[n - 1, :] = 100.0
        for j in range(n - 1):
            A[j, j + 1] = 1000.0
    return np.asfortranarray(A)


def _permuted(A):
    import pivot64_model as P64
    piv, _ = P64.panel_piv(np.asfortranarray(A.copy()))
    return P64.permute_rows(np.asfortranarray(A), piv)


def _rank1(oracle, fused):
    return (lambda Cm, l, u: oracle.dgemm_minus(Cm, l, u)) if fused else None


@functools.lru_cache(maxsize=None)
def _model(n, kind, fused, oracle, seed=0):
    """(LU, ipiv, info) of the model on _matrix(n, kind, seed): computed once, shared, read-only."""
    LU, ipiv, info = M.getrf_model(_matrix(n, kind, seed), _rank1(oracle, fused))
    LU.setflags(write=False)
    ipiv.setflags(write=False)
    return LU, ipiv, info


def _dev_batch(ctx, mats):
    """Packed column-major device batch of the equally shaped numpy matrices."""
    import torch
    mats = np.stack([np.asarray(m) for m in mats])
    T = ctx.colmajor_batch(*mats.shape)
    T.copy_(torch.from_numpy(np.ascontiguousarray(mats)))
    return T


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_getrf_against_the_model(ctx, oracle, n, fused):
    """One call sees all five kinds of matrix, one per batch slot."""
    A = _dev_batch(ctx, [_matrix(n, k) for k in KINDS])
    LU, ipiv, info = ctx.getrf_batched(A, fused=fused)
    assert LU.shape == (5, n, n) and ipiv.shape == (5, n) and info.shape == (5,)
    got, piv = LU.cpu().numpy(), ipiv.cpu().numpy()
    assert info.cpu().numpy().tolist() == [0] * 5
    for b, kind in enumerate(KINDS):
        LU_m, piv_m, info_m = _model(n, kind, fused, oracle)
        assert info_m == 0
        if kind == "sorted" and not fused:
            assert np.array_equal(piv_m, np.arange(1, n + 1))
        if kind == "last_row" and not fused:
            assert np.all(piv_m == n)
        assert np.array_equal(piv[b], piv_m), (n, kind, fused)
        assert np.array_equal(_bits(got[b]), _bits(LU_m)), (n, kind, fused)
        assert piv[b][n - 1] == n
    # the input was left alone, and an in-place call gives the same
    assert np.array_equal(_bits(A[0]), _bits(_matrix(n, KINDS[0])))
    LU2, ipiv2, _ = ctx.getrf_batched(A, fused=fused, overwrite=True)
    assert LU2.data_ptr() == A.data_ptr()
    assert np.array_equal(_bits(LU2), _bits(got)) and np.array_equal(ipiv2.cpu().numpy(), piv)


@pytest.mark.parametrize("n", [5, 32, 33, 128])
def test_getrf_against_the_panel_operator(ctx, n):
    mats = [_matrix(n, "normal", seed=s) for s in (1, 2, 3)]
    for fused in (False, True):
        LU, ipiv, info = ctx.getrf_batched(_dev_batch(ctx, mats), fused=fused)
        for b, A in enumerate(mats):
            dP = ctx.from_numpy_f(A)
            piv1, info1 = ctx.dgetf2_piv(dP, fused=fused)
            assert info1 == 0 and int(info[b]) == 0
            assert np.array_equal(ipiv[b].cpu().numpy(), piv1.cpu().numpy()), (n, fused, b)
            assert np.array_equal(_bits(LU[b]), _bits(dP)), (n, fused, b)


@pytest.mark.parametrize("n", [4, 40, 128])
def test_singular_matrix_in_the_batch(ctx, oracle, n):
    mats = [_matrix(n, "normal", seed=s).copy() for s in (4, 5, 6)]
    mats[1][:, n // 2] = 0.0
    LU, ipiv, info = ctx.getrf_batched(_dev_batch(ctx, mats))
    assert info.cpu().numpy().tolist() == [0, n // 2 + 1, 0]
    dP = ctx.from_numpy_f(mats[1])
    piv1, info1 = ctx.dgetf2_piv(dP)
    assert info1 == n // 2 + 1
    assert np.array_equal(ipiv[1].cpu().numpy(), piv1.cpu().numpy())
    assert _same_with_nans(LU[1].cpu().numpy(), dP.cpu().numpy())
    for b, s in ((0, 4), (2, 6)):
        LU_m, piv_m, _ = _model(n, "normal", False, oracle, seed=s)
        assert np.array_equal(ipiv[b].cpu().numpy(), piv_m) and np.array_equal(_bits(LU[b]), _bits(LU_m))


@pytest.mark.parametrize("n", [6, 40])
def test_nan_never_becomes_the_pivot(ctx, n):
    one = _matrix(n, "normal", seed=7).copy()
    one[3, 0] = np.nan                        # below the diagonal in column 0
    col = _matrix(n, "normal", seed=8).copy()
    col[:, 2] = np.nan                        # an all-NaN column: p = j, and everything after it is NaN
    LU, ipiv, info = ctx.getrf_batched(_dev_batch(ctx, [one, col]))
    piv = ipiv.cpu().numpy()
    for b, A in enumerate((one, col)):
        LU_m, piv_m, info_m = M.getrf_model(A)
        assert np.array_equal(piv[b], piv_m), (n, b)
        assert _same_with_nans(LU[b].cpu().numpy(), LU_m), (n, b)
        assert int(info[b]) == info_m == 0
    assert piv[0][0] != 4 and not np.isnan(LU[0].cpu().numpy()[0, 0])
    assert np.array_equal(piv[1][2:], np.arange(3, n + 1))


@pytest.mark.parametrize("n", [7, 32, 33, 128])
def test_layout_padding_is_not_touched(ctx, n):
    import torch
    batch, lda, sp = 3, n + 3, n + 2
    sa = lda * n + 11
    mats = [_matrix(n, "normal", seed=s) for s in (9, 10, 11)]
    want_LU, want_piv, _ = ctx.getrf_batched(_dev_batch(ctx, mats))
    buf = torch.full((batch * sa,), -7.25, dtype=torch.float64, device=ctx.device)
    pbuf = torch.full((batch * sp,), -7, dtype=torch.int32, device=ctx.device)
    A = torch.as_strided(buf, (batch, n, n), (sa, 1, lda))
    P = torch.as_strided(pbuf, (batch, n), (sp, 1))
    A.copy_(torch.from_numpy(np.stack(mats)))
    LU, ipiv, info = ctx.getrf_batched(A, overwrite=True, ipiv=P)
    assert LU.data_ptr() == buf.data_ptr() and ipiv.data_ptr() == pbuf.data_ptr()
    assert np.array_equal(_bits(LU), _bits(want_LU)) and np.array_equal(ipiv.cpu().numpy(), want_piv.cpu().numpy())
    assert info.cpu().numpy().tolist() == [0, 0, 0]
    pad = torch.ones_like(buf, dtype=torch.bool)
    torch.as_strided(pad, (batch, n, n), (sa, 1, lda)).fill_(False)
    assert int(pad.sum()) == batch * sa - batch * n * n and bool((buf[pad] == -7.25).all())
    ppad = torch.ones_like(pbuf, dtype=torch.bool)
    torch.as_strided(ppad, (batch, n), (sp, 1)).fill_(False)
    assert bool((pbuf[ppad] == -7).all())


@pytest.mark.parametrize("n,batches", [(8, (1, 2, 1000)), (33, (1, 2, 1025)), (128, (1, 2, 257))])
def test_batch_independence_and_grid_tails(ctx, n, batches):
    """Device against device: a matrix of a long batch equals the same matrix factored alone; the matrix, pivots and info word right
    behind the batch, in the same allocations, are not touched."""
    import torch
    for batch in batches:
        rng = np.random.default_rng(n * 31 + batch)
        src = _dev_batch(ctx, rng.standard_normal((batch + 1, n, n)))
        W = src.clone(memory_format=torch.preserve_format)
        assert W.stride() == src.stride()
        pbuf = torch.full((batch + 1, n), -7, dtype=torch.int32, device=ctx.device)
        ibuf = torch.full((batch + 1,), -7, dtype=torch.int32, device=ctx.device)
        LU, ipiv, info = ctx.getrf_batched(W[:batch], overwrite=True, ipiv=pbuf[:batch], info=ibuf[:batch])
        assert LU.data_ptr() == W.data_ptr()
        assert np.array_equal(_bits(W[batch]), _bits(src[batch])), (n, batch)
        assert bool((pbuf[batch] == -7).all()) and int(ibuf[batch]) == -7
        assert bool((ibuf[:batch] == 0).all())
        for b in sorted({0, batch // 2, batch - 1}):
            LU1, ipiv1, info1 = ctx.getrf_batched(src[b:b + 1])
            assert np.array_equal(_bits(LU[b]), _bits(LU1[0])), (n, batch, b)
            assert np.array_equal(ipiv[b].cpu().numpy(), ipiv1[0].cpu().numpy()), (n, batch, b)
            assert int(ipiv[b][n - 1]) == n


def test_batch_longer_than_one_launch(ctx, mpf):
    """n = 1 makes a batch past the launch chunk (2^22 matrices) cheap: LU = A, every pivot is 1, info names the zeros; the solve
    divides."""
    import torch
    batch = (1 << 22) + 3
    a = np.random.default_rng(22).uniform(1.0, 2.0, batch)
    a[-1] = 0.0
    A = torch.from_numpy(a).to(ctx.device).view(batch, 1, 1)
    LU, ipiv, info = ctx.getrf_batched(A)
    assert np.array_equal(_bits(LU.reshape(-1)), _bits(a))
    assert bool((ipiv == 1).all())
    inf = info.cpu().numpy()
    assert inf[-1] == 1 and not inf[:-1].any()
    rhs = np.random.default_rng(23).uniform(1.0, 2.0, batch)
    X = ctx.getrs_batched(LU, ipiv, torch.from_numpy(rhs).to(ctx.device).view(batch, 1, 1))
    with np.errstate(divide="ignore"):
        assert np.array_equal(_bits(X.reshape(-1)), _bits(rhs / a))


@functools.lru_cache(maxsize=None)
def _factors(n, batch=4):
    out = []
    for s in range(batch):
        LU, ipiv, info = M.getrf_model(_matrix(n, "normal", seed=20 + s))
        assert info == 0
        out.append((LU, ipiv))
    return out


@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("n", [1, 2, 9, 32, 33, 64, 65, 128])
def test_getrs_against_the_model(ctx, n, trans):
    import torch
    batch = 4
    fac = _factors(n)
    LU = _dev_batch(ctx, [f[0] for f in fac])
    ipiv = torch.from_numpy(np.stack([f[1] for f in fac])).to(ctx.device)
    for nrhs in (1, 3, 40):
        B = np.random.default_rng(n * 100 + nrhs).standard_normal((batch, n, nrhs))
        want = np.stack([M.getrs_model(fac[b][0], fac[b][1], B[b], trans) for b in range(batch)])
        buf = ctx.colmajor_batch(batch, n + 1, nrhs)        # ldb = n + 1: one sentinel row under every matrix
        buf.fill_(-7.25)
        Bd = buf[:, :n, :]
        Bd.copy_(torch.from_numpy(B))
        X = ctx.getrs_batched(LU, ipiv, Bd, trans=trans, overwrite=True)
        assert X.data_ptr() == buf.data_ptr()
        assert np.array_equal(_bits(X), _bits(want)), (n, nrhs, trans)
        assert bool((buf[:, n, :] == -7.25).all()), (n, nrhs, trans)
        # out of place: B stays, the result is the same
        Bd.copy_(torch.from_numpy(B))
        X2 = ctx.getrs_batched(LU, ipiv, Bd, trans=trans)
        assert np.array_equal(_bits(Bd), _bits(B)) and np.array_equal(_bits(X2), _bits(want))
        if nrhs == 40:                                      # columns do not read each other
            X1 = ctx.getrs_batched(LU, ipiv, torch.from_numpy(np.ascontiguousarray(B[:, :, 2:3])).to(ctx.device), trans=trans)
            assert np.array_equal(_bits(X1[:, :, 0]), _bits(want[:, :, 2])), (n, trans)
        if nrhs == 1:                                       # a (batch, n) tensor is one right-hand side per matrix
            xv = ctx.getrs_batched(LU, ipiv, torch.from_numpy(np.ascontiguousarray(B[:, :, 0])).to(ctx.device), trans=trans)
            assert xv.shape == (batch, n) and np.array_equal(_bits(xv), _bits(want[:, :, 0]))


def end_to_end_inputs():
    """The fixed inputs of test_solve_batched_end_to_end (64 systems of order 48, two right-hand sides each)."""
    rng = np.random.default_rng(4848)
    return rng.standard_normal((64, 48, 48)), rng.standard_normal((64, 48, 2))


def end_to_end_error(A, X, B, trans):
    """max over the batch and the columns of ||op(A) x - b||_inf / (||A||_inf ||x||_inf), the residual in extended precision."""
    worst = 0.0
    for b in range(A.shape[0]):
        op = (A[b].T if trans else A[b]).astype(np.longdouble)
        R = np.abs(op @ X[b].astype(np.longdouble) - B[b].astype(np.longdouble)).max(axis=0)
        anorm = np.abs(A[b]).sum(axis=1).max()
        worst = max(worst, float((R / (anorm * np.abs(X[b]).max(axis=0))).max()))
    return worst


@pytest.mark.parametrize("trans", [False, True])
def test_solve_batched_end_to_end(ctx, trans):
    """From torch's row-major default (the copy path).  Bound: n eps of a backward-stable solve, n = 48, eps = 2^-52; the numpy model
    of the same chains gives 1.83e-16 (trans = 0) and 2.32e-16 (trans = 1) on these inputs, the bound is 1.07e-14."""
    import torch
    A, B = end_to_end_inputs()
    dA, dB = torch.from_numpy(A).to(ctx.device), torch.from_numpy(B).to(ctx.device)
    assert dA.is_contiguous() and dA.stride() == (48 * 48, 48, 1)
    X = ctx.solve_batched(dA, dB, trans=trans)
    assert X.shape == (64, 48, 2)
    err = end_to_end_error(A, X.cpu().numpy(), B, trans)
    print(f"solve_batched trans={int(trans)}: max backward error {err:.3e}")
    assert err <= 48 * 2.0 ** -52
    assert np.array_equal(_bits(dA), _bits(A)) and np.array_equal(_bits(dB), _bits(B))


def test_solve_batched_names_the_singular_matrix(ctx, mpf):
    import torch
    A, B = end_to_end_inputs()
    A = A.copy()
    A[5][:, 7] = 0.0
    with pytest.raises(mpf.MPFError) as ei:
        ctx.solve_batched(torch.from_numpy(A).to(ctx.device), torch.from_numpy(B).to(ctx.device))
    assert "matrix 5" in str(ei.value) and "zero pivot 8" in str(ei.value)


def test_argument_checks(ctx, mpf):
    import torch
    L, h = ctx.L, ctx.h
    n, batch = 4, 3
    A = ctx.colmajor_batch(batch, n, n)
    A.copy_(torch.eye(n, dtype=torch.float64, device=ctx.device).expand(batch, n, n))
    keep = A.clone(memory_format=torch.preserve_format)
    ipiv = torch.zeros((batch, n), dtype=torch.int32, device=ctx.device)
    B = ctx.colmajor_batch(batch, n, 2)
    B.fill_(1.0)
    pa, pp, pb, null = C.c_void_p(A.data_ptr()), C.c_void_p(ipiv.data_ptr()), C.c_void_p(B.data_ptr()), C.c_void_p(0)

    def err():
        return L.mpf_last_error(h).decode()

    assert L.mpf_getrf_batched(h, pa, 129, 129 * 129, 129, 1, pp, 129, null, 0) == -1 and "mpf_factor_dev" in err()
    assert L.mpf_getrf_batched(h, pa, n - 1, n * n, n, batch, pp, n, null, 0) == -1 and "leading dimension" in err()
    assert L.mpf_getrf_batched(h, pa, n, n * n - 1, n, batch, pp, n, null, 0) == -1 and "stride" in err()
    assert L.mpf_getrf_batched(h, pa, n, n * n, n, batch, pp, n - 1, null, 0) == -1 and "ipiv" in err()
    assert L.mpf_getrf_batched(h, pa, n, n * n, -1, batch, pp, n, null, 0) == -1
    assert L.mpf_getrf_batched(h, null, n, n * n, n, batch, pp, n, null, 0) == -1 and "null" in err()
    assert L.mpf_getrf_batched(h, pa, n, n * n, n, 0, pp, n, null, 0) == 0
    assert L.mpf_getrf_batched(h, pa, n, n * n, 0, batch, pp, n, null, 0) == 0
    assert L.mpf_getrf_batched(h, pa, n, 0, n, 1, pp, 0, null, 0) == 0              # one matrix: the strides mean nothing
    assert L.mpf_getrs_batched(h, 0, pa, 129, 129 * 129, 129, 1, pp, 129, 1, pb, 129, 129) == -1 and "mpf_factor_dev" in err()
    assert L.mpf_getrs_batched(h, 0, pa, n, n * n, n, batch, pp, n, 2, pb, n - 1, 2 * n) == -1 and "leading dimension" in err()
    assert L.mpf_getrs_batched(h, 0, pa, n, n * n, n, batch, pp, n, 2, pb, n, 2 * n - 1) == -1 and "stride" in err()
    assert L.mpf_getrs_batched(h, 2, pa, n, n * n, n, batch, pp, n, 2, pb, n, 2 * n) == -1 and "trans" in err()
    assert L.mpf_getrs_batched(h, 0, pa, n, n * n, n, batch, pp, n, 0, pb, n, 2 * n) == 0
    assert L.mpf_getrs_batched(h, 0, pa, n, n * n, n, 0, pp, n, 2, pb, n, 2 * n) == 0
    ctx.synchronize()
    # only the one-matrix call above did any work: identity in, identity out, the other matrices and B as they were
    assert np.array_equal(_bits(A), _bits(keep)) and bool((B == 1.0).all())
    assert ipiv.cpu().numpy().tolist() == [[1, 2, 3, 4], [0] * 4, [0] * 4]
    # the Python side: an input that would be copied cannot be overwritten; n > 128 is the library's error
    with pytest.raises(mpf.MPFError):
        ctx.getrf_batched(torch.zeros((2, 4, 4), dtype=torch.float64, device=ctx.device), overwrite=True)
    with pytest.raises(mpf.MPFError) as ei:
        ctx.getrf_batched(ctx.colmajor_batch(1, 129, 129))
    assert "mpf_factor_dev" in str(ei.value)
