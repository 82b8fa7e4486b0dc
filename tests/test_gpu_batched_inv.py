"""GPU tests of the batched inverse and determinant (include/mpf_c.h: mpf_getri_batched, mpf_getdet_batched; csrc/batched.hip).

Sizes are test_gpu_batched.py's seams: 7 / 8 / 9, 16 / 17, 31 / 32 / 33 (the wave form's widths and its crossover to the workgroup form),
63 / 64 / 65 (one and two rows per lane, 256 and 1024 threads), 100 (columns that do not fill the last group of four), 127, 128.

Bit checks need no tolerance.  The factors come from the numpy model of the factorization (tests/batched_model.py) and are uploaded,
so a failure points at the inverse; the model of the inverse is the solve's model on an identity (tests/batched_inv_model.py), the
model of the determinant tests/getri_model.py."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import batched_inv_model as MI
import batched_model as M

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 7, 8, 9, 16, 17, 31, 32, 33, 63, 64, 65, 100, 127, 128]
KINDS = ["normal", "ints", "tiny", "last_row", "sorted"]          # test_gpu_batched.py's; "ints" may be singular and is not used here
INV_KINDS = ["normal", "tiny", "last_row", "sorted"]
FILL = -7.25


def _bits(a):
    if hasattr(a, "cpu"):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a).view(np.uint64)


def _matrix(n, kind, seed=0):
    rng = np.random.default_rng(n * 1009 + 13 * seed + KINDS.index(kind))
    A = rng.standard_normal((n, n))
    if kind == "tiny":                    # far below fp16's range
        A *= 2.0 ** -40
    elif kind == "sorted":                # rows in pivot order already: no interchange at all
        import pivot64_model as P64
        piv, _ = P64.panel_piv(np.asfortranarray(A.copy()))
        A = P64.permute_rows(np.asfortranarray(A), piv)
    elif kind == "last_row":              # every column takes its pivot from the LAST row
        A[n - 1, :] = 100.0
        for j in range(n - 1):
            A[j, j + 1] = 1000.0
    return np.asfortranarray(A)


def _dev_batch(ctx, mats):
    """Packed column-major device batch of the equally shaped numpy matrices."""
    import torch
    mats = np.stack([np.asarray(m) for m in mats])
    T = ctx.colmajor_batch(*mats.shape)
    T.copy_(torch.from_numpy(np.ascontiguousarray(mats)))
    return T


@functools.lru_cache(maxsize=None)
def _model(n, kind, seed=0):
    """(LU, ipiv, inverse) of the model on _matrix(n, kind, seed): computed once, shared, read-only."""
    LU, ipiv, info = M.getrf_model(_matrix(n, kind, seed))
    assert info == 0 and np.all(np.diag(LU) != 0.0) and np.all(np.isfinite(LU)), (n, kind, seed)
    X = MI.getri_model(LU, ipiv)
    for a in (LU, ipiv, X):
        a.setflags(write=False)
    return LU, ipiv, X


def _upload(ctx, facs):
    import torch
    LU = _dev_batch(ctx, [f[0] for f in facs])
    ipiv = torch.from_numpy(np.stack([f[1] for f in facs])).to(ctx.device)
    return LU, ipiv


def _out_with_sentinel_rows(ctx, batch, n):
    """(buffer, view): a (batch, n, n) view with ldinv = n + 1 into a buffer filled with FILL -- one sentinel row under every matrix."""
    buf = ctx.colmajor_batch(batch, n + 1, n)
    buf.fill_(FILL)
    return buf, buf[:, :n, :]


@pytest.mark.parametrize("n", SIZES)
def test_inverse_against_the_model(ctx, n):
    import torch
    facs = [_model(n, k) for k in INV_KINDS]
    LU, ipiv = _upload(ctx, facs)
    keep_LU, keep_piv = LU.clone(memory_format=torch.preserve_format), ipiv.clone()
    buf, out = _out_with_sentinel_rows(ctx, len(facs), n)
    info = torch.full((len(facs),), -7, dtype=torch.int32, device=ctx.device)
    X, info2 = ctx.getri_batched(LU, ipiv, out=out, info=info)
    assert X.data_ptr() == buf.data_ptr() and info2.data_ptr() == info.data_ptr()
    assert info.cpu().numpy().tolist() == [0] * len(facs)
    got = X.cpu().numpy()
    for b, kind in enumerate(INV_KINDS):
        if kind == "sorted":
            assert np.array_equal(facs[b][1], np.arange(1, n + 1))
        assert np.array_equal(_bits(got[b]), _bits(facs[b][2])), (n, kind)
    assert bool((buf[:, n, :] == FILL).all())
    assert np.array_equal(_bits(LU), _bits(keep_LU)) and bool((ipiv == keep_piv).all())
    # without out / info: new tensors, the same bits
    X2, info3 = ctx.getri_batched(LU, ipiv)
    assert np.array_equal(_bits(X2), _bits(got)) and not bool(info3.any())


@pytest.mark.parametrize("n", [5, 32, 33, 64, 65, 128])
def test_inverse_against_the_solve_on_an_identity(ctx, n):
    import torch
    LU, ipiv = _upload(ctx, [_model(n, k) for k in INV_KINDS])
    eye = ctx.colmajor_batch(len(INV_KINDS), n, n)
    eye.copy_(torch.eye(n, dtype=torch.float64, device=ctx.device).expand(len(INV_KINDS), n, n))
    want = ctx.getrs_batched(LU, ipiv, eye, overwrite=True)
    X, _ = ctx.getri_batched(LU, ipiv)
    assert np.array_equal(_bits(X), _bits(want)), n


@pytest.mark.parametrize("n", [4, 40, 128])
def test_singular_matrices_are_reported_and_left_alone(ctx, n):
    import torch
    facs = [_model(n, "normal", seed=s) for s in range(1, 6)]
    zero_at = {0: 0, 2: n // 2, 4: n - 1}
    mats = [f[0].copy() for f in facs]
    for b, i in zero_at.items():
        mats[b][i, i] = 0.0
    LU = _dev_batch(ctx, mats)
    ipiv = torch.from_numpy(np.stack([f[1] for f in facs])).to(ctx.device)
    want_info = [zero_at[b] + 1 if b in zero_at else 0 for b in range(5)]
    for with_info in (True, False):
        buf, out = _out_with_sentinel_rows(ctx, 5, n)
        info = torch.full((5,), -7, dtype=torch.int32, device=ctx.device)
        lay = ctx._batch_layout(out)
        rc = ctx.L.mpf_getri_batched(ctx.h, C.c_void_p(LU.data_ptr()), n, n * n, n, 5, C.c_void_p(ipiv.data_ptr()), n,
                                     C.c_void_p(out.data_ptr()), lay[0], lay[1], C.c_void_p(info.data_ptr() if with_info else 0))
        assert rc == 0
        ctx.synchronize()
        assert info.cpu().numpy().tolist() == (want_info if with_info else [-7] * 5)
        for b in range(5):
            if b in zero_at:
                assert bool((buf[b] == FILL).all()), (n, b, with_info)
            else:
                assert np.array_equal(_bits(out[b]), _bits(facs[b][2])), (n, b, with_info)
        assert bool((buf[:, n, :] == FILL).all())


@pytest.mark.parametrize("n", [6, 40])
def test_nan_in_one_matrix_stays_there(ctx, n):
    import torch
    facs = [_model(n, "normal", seed=s) for s in (7, 8, 9)]
    mats = [f[0].copy() for f in facs]
    mats[1][3, 1] = np.nan
    mats[1][1, 4] = np.inf
    piv = np.stack([f[1] for f in facs]).copy()
    piv[1][2] = 1000                                   # out of range: reads as "no interchange", every access stays in range
    LU = _dev_batch(ctx, mats)
    X, info = ctx.getri_batched(LU, torch.from_numpy(piv).to(ctx.device))
    ctx.synchronize()
    for b in (0, 2):
        assert np.array_equal(_bits(X[b]), _bits(facs[b][2])), (n, b)
        assert int(info[b]) == 0


@pytest.mark.parametrize("n", [7, 32, 33, 128])
def test_padded_layouts_give_the_same_bits(ctx, n):
    import torch
    batch, ldlu, sp, ldinv = 3, n + 3, n + 2, n + 1
    slu, sinv = ldlu * n + 11, ldinv * n + 5
    facs = [_model(n, "normal", seed=s) for s in (10, 11, 12)]
    lubuf = torch.full((batch * slu,), 3.5, dtype=torch.float64, device=ctx.device)
    pbuf = torch.full((batch * sp,), -7, dtype=torch.int32, device=ctx.device)
    ibuf = torch.full((batch * sinv,), FILL, dtype=torch.float64, device=ctx.device)
    LU = torch.as_strided(lubuf, (batch, n, n), (slu, 1, ldlu))
    P = torch.as_strided(pbuf, (batch, n), (sp, 1))
    out = torch.as_strided(ibuf, (batch, n, n), (sinv, 1, ldinv))
    LU.copy_(torch.from_numpy(np.stack([f[0] for f in facs])))
    P.copy_(torch.from_numpy(np.stack([f[1] for f in facs])))
    keep_lu, keep_p = lubuf.clone(), pbuf.clone()
    X, info = ctx.getri_batched(LU, P, out=out)
    assert X.data_ptr() == ibuf.data_ptr()
    for b in range(batch):
        assert np.array_equal(_bits(X[b]), _bits(facs[b][2])), (n, b)
    assert info.cpu().numpy().tolist() == [0] * batch
    pad = torch.ones_like(ibuf, dtype=torch.bool)
    torch.as_strided(pad, (batch, n, n), (sinv, 1, ldinv)).fill_(False)
    assert int(pad.sum()) == batch * sinv - batch * n * n and bool((ibuf[pad] == FILL).all())
    assert np.array_equal(_bits(lubuf), _bits(keep_lu)) and bool((pbuf == keep_p).all())
    # the determinant reads the same padded factors
    mant, expo = ctx.getdet_batched(LU, P)
    for b in range(batch):
        assert (float(mant[b]), int(expo[b])) == MI.getdet_model(np.diag(facs[b][0]), facs[b][1]), (n, b)


@pytest.mark.parametrize("n,batches", [(8, (1, 2, 1000)), (33, (1, 2, 1025)), (128, (1, 2, 257))])
def test_batch_independence_and_grid_tails(ctx, n, batches):
    """Device against device (the factors are the device's own): a matrix of a long batch equals the same matrix inverted alone; the
    slot, the info word and the determinant behind the batch, in the same allocations, are not touched."""
    import torch
    for batch in batches:
        rng = np.random.default_rng(n * 37 + batch)
        LU, ipiv, finfo = ctx.getrf_batched(_dev_batch(ctx, rng.standard_normal((batch, n, n))))
        assert not bool(finfo.any())
        buf = ctx.colmajor_batch(batch + 1, n, n)
        buf.fill_(FILL)
        ibuf = torch.full((batch + 1,), -7, dtype=torch.int32, device=ctx.device)
        X, info = ctx.getri_batched(LU, ipiv, out=buf[:batch], info=ibuf[:batch])
        assert X.data_ptr() == buf.data_ptr()
        assert bool((buf[batch] == FILL).all()) and int(ibuf[batch]) == -7, (n, batch)
        assert not bool(ibuf[:batch].any())
        mant, expo = ctx.getdet_batched(LU, ipiv)
        for b in sorted({0, batch // 2, batch - 1}):
            X1, _ = ctx.getri_batched(LU[b:b + 1], ipiv[b:b + 1])
            assert np.array_equal(_bits(X[b]), _bits(X1[0])), (n, batch, b)
            m1, e1 = ctx.getdet_batched(LU[b:b + 1], ipiv[b:b + 1])
            assert np.array_equal(_bits(mant[b:b + 1]), _bits(m1)) and int(expo[b]) == int(e1[0]), (n, batch, b)


def test_batch_longer_than_one_launch(ctx):
    """n = 1 makes a batch past the launch chunk (2^22 matrices) cheap: inv = 1 / a, det = a; the one zero is reported and its slot
    untouched."""
    import torch
    batch = (1 << 22) + 3
    a = np.random.default_rng(24).uniform(1.0, 2.0, batch) * np.exp2(np.random.default_rng(25).integers(-30, 30, batch))
    a[-1] = 0.0
    LU = torch.from_numpy(a).to(ctx.device).view(batch, 1, 1)
    ipiv = torch.ones((batch, 1), dtype=torch.int32, device=ctx.device)
    out = torch.full((batch, 1, 1), FILL, dtype=torch.float64, device=ctx.device)
    X, info = ctx.getri_batched(LU, ipiv, out=out)
    want = np.full(batch, FILL)
    want[:-1] = 1.0 / a[:-1]
    assert np.array_equal(_bits(X.reshape(-1)), _bits(want))
    inf = info.cpu().numpy()
    assert inf[-1] == 1 and not inf[:-1].any()
    mant, expo = ctx.getdet_batched(LU, ipiv)
    m, e = np.frexp(a[:-1])
    assert np.array_equal(_bits(mant[:-1]), _bits(m)) and np.array_equal(expo[:-1].cpu().numpy(), e.astype(np.int32))
    assert float(mant[-1]) == 0.0 and int(expo[-1]) == 0


@pytest.mark.parametrize("n", SIZES)
def test_getdet_against_the_model(ctx, n):
    facs = [_model(n, k) for k in INV_KINDS]
    LU, ipiv = _upload(ctx, facs)
    mant, expo = ctx.getdet_batched(LU, ipiv)
    import torch
    assert mant.dtype == torch.float64 and expo.dtype == torch.int32 and mant.shape == expo.shape == (len(facs),)
    for b, kind in enumerate(INV_KINDS):
        wm, we = MI.getdet_model(np.diag(facs[b][0]), facs[b][1])
        assert _bits(np.float64(float(mant[b]))) == _bits(np.float64(wm)) and int(expo[b]) == we, (n, kind)
        flips = int(np.count_nonzero(facs[b][1] != np.arange(1, n + 1)))
        if kind == "sorted":
            assert flips == 0
        if kind == "last_row" and n > 1:
            assert flips == n - 1


def test_getdet_special_cases(ctx):
    import torch
    # a zero and a non-finite entry on the diagonal, at a thread-per-matrix size and a wave-per-matrix size
    for n in (6, 40):
        facs = [_model(n, "normal", seed=s) for s in (13, 14, 15, 16)]
        mats = [f[0].copy() for f in facs]
        mats[0][n // 2, n // 2] = 0.0
        mats[1][n - 1, n - 1] = np.inf
        mats[2][0, 0] = 0.0
        mats[2][1, 1] = np.nan                         # non-finite wins over zero
        LU = _dev_batch(ctx, mats)
        ipiv = torch.from_numpy(np.stack([f[1] for f in facs])).to(ctx.device)
        mant, expo = ctx.getdet_batched(LU, ipiv)
        m, e = mant.cpu().numpy(), expo.cpu().numpy()
        assert m[0] == 0.0 and e[0] == 0
        assert np.isnan(m[1]) and e[1] == 0 and np.isnan(m[2]) and e[2] == 0
        assert (float(m[3]), int(e[3])) == MI.getdet_model(np.diag(facs[3][0]), facs[3][1])
    # the exponent is carried, not overflowed: det = 2^-128000 and 2^127000
    for n, s in ((128, -1000), (127, 1000)):
        LU = _dev_batch(ctx, [np.eye(n) * 2.0 ** s])
        ipiv = torch.arange(1, n + 1, dtype=torch.int32, device=ctx.device).view(1, n)
        mant, expo = ctx.getdet_batched(LU, ipiv)
        assert (float(mant[0]), int(expo[0])) == (0.5, n * s + 1) == MI.getdet_model([2.0 ** s] * n, np.arange(1, n + 1))


@pytest.mark.parametrize("n", [5, 33, 128])
def test_getdet_against_the_single_matrix_entry_point(ctx, n):
    import torch
    facs = [_model(n, k) for k in ("normal", "last_row")]
    LU, ipiv = _upload(ctx, facs)
    mant, expo = ctx.getdet_batched(LU, ipiv)
    for b, f in enumerate(facs):
        m1, e1 = ctx.getdet(ctx.from_numpy_f(f[0].copy()), torch.from_numpy(f[1].copy()).to(ctx.device))
        assert _bits(np.float64(float(mant[b]))) == _bits(np.float64(m1)) and int(expo[b]) == e1, (n, b)


def test_inv_batched_end_to_end(ctx, mpf):
    """From torch's row-major default (the copy path).  dget03 on both sides against LAPACK's dtest.in threshold 30; the numpy model
    gives at most 0.63 on random normal matrices up to n = 128."""
    import torch
    from test_gpu_batched import end_to_end_inputs
    A, _ = end_to_end_inputs()
    dA = torch.from_numpy(A).to(ctx.device)
    assert dA.is_contiguous() and dA.stride() == (48 * 48, 48, 1)
    X = ctx.inv_batched(dA)
    assert X.shape == (64, 48, 48)
    Xh = X.cpu().numpy()
    worst = max(max(MI.dget03_ratio(A[b], Xh[b], True), MI.dget03_ratio(A[b], Xh[b], False)) for b in range(64))
    print(f"inv_batched: worst dget03 ratio {worst:.3f}")
    assert worst <= 30.0
    assert np.array_equal(_bits(dA), _bits(A))
    B = A.copy()
    B[5][:, 7] = 0.0
    with pytest.raises(mpf.MPFError) as ei:
        ctx.inv_batched(torch.from_numpy(B).to(ctx.device))
    assert "matrix 5" in str(ei.value) and "zero pivot 8" in str(ei.value)


def test_slogdet_batched_against_mant_and_expo(ctx):
    """|logabsdet - (log|mant| + expo ln 2)| <= 8 * 2^-53 * max(0.7, |expo| ln 2): one rounding of the sum plus a few ulps between the
    device's and numpy's logarithm (|log|mant|| <= ln 2 < 0.7).  Absolute, because the two terms can cancel."""
    import torch
    ln2 = math.log(2.0)
    for n in (8, 40, 128):
        mats = [_model(n, k)[0].copy() for k in INV_KINDS] + [np.eye(n) * 2.0 ** -1000, np.eye(n)]
        mats[-1][n // 2, n // 2] = 0.0
        pivs = [_model(n, k)[1] for k in INV_KINDS] + [np.arange(1, n + 1, dtype=np.int32)] * 2
        LU = _dev_batch(ctx, mats)
        ipiv = torch.from_numpy(np.stack(pivs)).to(ctx.device)
        mant, expo = ctx.getdet_batched(LU, ipiv)
        sign, logabs = ctx.slogdet_batched(LU, ipiv)
        assert sign.is_cuda and logabs.is_cuda and sign.shape == logabs.shape == (len(mats),)
        m, e, s, la = mant.cpu().numpy(), expo.cpu().numpy().astype(np.float64), sign.cpu().numpy(), logabs.cpu().numpy()
        assert s[-1] == 0.0 and la[-1] == -np.inf
        for b in range(len(mats) - 1):
            want = np.log(abs(m[b])) + e[b] * ln2
            err, bound = abs(la[b] - want), 8 * 2.0 ** -53 * max(0.7, abs(e[b]) * ln2)
            print(f"slogdet n={n} slot {b}: expo {int(e[b])} |diff| {err:.3e} bound {bound:.3e}")
            assert s[b] == np.sign(m[b]) and err <= bound, (n, b)
    # from the matrices themselves: a copy is factored first; a non-finite determinant is NaN
    A = np.stack([_matrix(9, "normal"), _matrix(9, "last_row")])
    sign, logabs = ctx.slogdet_batched(torch.from_numpy(A).to(ctx.device))
    s0, l0 = np.linalg.slogdet(A)
    assert np.array_equal(sign.cpu().numpy(), s0) and np.allclose(logabs.cpu().numpy(), l0, rtol=1e-12, atol=1e-12)
    LU, ipiv = _upload(ctx, [_model(9, "normal")])
    LU[0, 4, 4] = float("nan")
    sign, logabs = ctx.slogdet_batched(LU, ipiv)
    assert math.isnan(float(sign[0])) and math.isnan(float(logabs[0]))


def test_argument_checks(ctx, mpf):
    import torch
    L, h = ctx.L, ctx.h
    n, batch = 4, 3
    LU = ctx.colmajor_batch(batch, n, n)
    LU.copy_(torch.eye(n, dtype=torch.float64, device=ctx.device).expand(batch, n, n))
    ipiv = torch.arange(1, n + 1, dtype=torch.int32, device=ctx.device).repeat(batch, 1).contiguous()
    out = ctx.colmajor_batch(batch, n, n)
    out.fill_(FILL)
    info = torch.full((batch,), -7, dtype=torch.int32, device=ctx.device)
    mant = torch.full((batch,), FILL, dtype=torch.float64, device=ctx.device)
    expo = torch.full((batch,), -7, dtype=torch.int32, device=ctx.device)
    keep = LU.clone(memory_format=torch.preserve_format)
    pl, pp, po, pi, pm, pe = (C.c_void_p(t.data_ptr()) for t in (LU, ipiv, out, info, mant, expo))
    null = C.c_void_p(0)

    def err():
        return L.mpf_last_error(h).decode()

    nn = n * n
    assert L.mpf_getri_batched(h, pl, 129, 129 * 129, 129, 1, pp, 129, po, 129, 129 * 129, pi) == -1 and "mpf_factor_dev" in err()
    assert L.mpf_getri_batched(h, pl, n - 1, nn, n, batch, pp, n, po, n, nn, pi) == -1 and "leading dimension" in err()
    assert L.mpf_getri_batched(h, pl, n, nn, n, batch, pp, n, po, n - 1, nn, pi) == -1 and "leading dimension" in err()
    assert L.mpf_getri_batched(h, pl, n, nn - 1, n, batch, pp, n, po, n, nn, pi) == -1 and "stride" in err()
    assert L.mpf_getri_batched(h, pl, n, nn, n, batch, pp, n, po, n, nn - 1, pi) == -1 and "stride" in err()
    assert L.mpf_getri_batched(h, pl, n, nn, n, batch, pp, n - 1, po, n, nn, pi) == -1 and "ipiv" in err()
    assert L.mpf_getri_batched(h, pl, n, nn, -1, batch, pp, n, po, n, nn, pi) == -1
    for args in ((null, pp, po), (pl, null, po), (pl, pp, null)):
        assert L.mpf_getri_batched(h, args[0], n, nn, n, batch, args[1], n, args[2], n, nn, pi) == -1 and "null" in err()
    # overlap: the result over the factors, and a result that starts inside the last matrix of the factors
    assert L.mpf_getri_batched(h, pl, n, nn, n, batch, pp, n, pl, n, nn, pi) == -1 and "overlaps" in err()
    inside = C.c_void_p(LU.data_ptr() + 8 * (batch * nn - 1))
    assert L.mpf_getri_batched(h, pl, n, nn, n, batch, pp, n, inside, n, nn, pi) == -1 and "overlaps" in err()
    assert L.mpf_getri_batched(h, pl, n, nn, n, 0, pp, n, po, n, nn, pi) == 0
    assert L.mpf_getri_batched(h, pl, n, nn, 0, batch, pp, n, po, n, nn, pi) == 0
    assert L.mpf_getdet_batched(h, pl, 129, 129 * 129, 129, 1, pp, 129, pm, pe) == -1 and "mpf_factor_dev" in err()
    assert L.mpf_getdet_batched(h, pl, n - 1, nn, n, batch, pp, n, pm, pe) == -1 and "leading dimension" in err()
    assert L.mpf_getdet_batched(h, pl, n, nn - 1, n, batch, pp, n, pm, pe) == -1 and "stride" in err()
    assert L.mpf_getdet_batched(h, pl, n, nn, n, batch, pp, n - 1, pm, pe) == -1 and "ipiv" in err()
    for args in ((null, pp, pm, pe), (pl, null, pm, pe), (pl, pp, null, pe), (pl, pp, pm, null)):
        assert L.mpf_getdet_batched(h, args[0], n, nn, n, batch, args[1], n, args[2], args[3]) == -1 and "null" in err()
    assert L.mpf_getdet_batched(h, pl, n, nn, n, 0, pp, n, pm, pe) == 0
    assert L.mpf_getdet_batched(h, pl, n, nn, 0, batch, pp, n, pm, pe) == 0
    ctx.synchronize()
    # nothing was written by any of these calls
    assert bool((out == FILL).all()) and bool((info == -7).all()) and bool((mant == FILL).all()) and bool((expo == -7).all())
    assert np.array_equal(_bits(LU), _bits(keep))
    # one matrix: the strides mean nothing
    assert L.mpf_getri_batched(h, pl, n, 0, n, 1, pp, 0, po, n, 0, pi) == 0
    assert L.mpf_getdet_batched(h, pl, n, 0, n, 1, pp, 0, pm, pe) == 0
    ctx.synchronize()
    assert bool((out[0] == torch.eye(n, dtype=torch.float64, device=ctx.device)).all()) and bool((out[1:] == FILL).all())
    assert info.cpu().numpy().tolist() == [0, -7, -7]
    assert mant.cpu().numpy().tolist() == [0.5, FILL, FILL] and expo.cpu().numpy().tolist() == [1, -7, -7]
    # the Python side: out must hold column-major matrices; n > 128 is the library's error
    with pytest.raises(mpf.MPFError):
        ctx.getri_batched(LU, ipiv, out=torch.zeros((batch, n, n), dtype=torch.float64, device=ctx.device))
    with pytest.raises(mpf.MPFError) as ei:
        ctx.getri_batched(ctx.colmajor_batch(1, 129, 129), torch.ones((1, 129), dtype=torch.int32, device=ctx.device))
    assert "mpf_factor_dev" in str(ei.value)
