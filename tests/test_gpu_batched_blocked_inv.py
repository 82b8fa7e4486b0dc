"""GPU tests of the blocked batched inverse and determinant (include/mpf_c.h: mpf_getri_batched_blocked,
mpf_getdet_batched_blocked; csrc/batched_blocked.hip).

Every comparison is on bits and has no tolerance, except dget03 and slogdet in the two end-to-end tests.  The yardsticks are the numpy
models (tests/batched_inv_model.py: the solve's chains on an identity; tests/getri_model.py: getdet_model), the n <= 128 entry points,
and for the large sizes the device's own getrs_batched_blocked on an identity.  SMALL: with option batched_blocked_min_n = 0 every n
runs the new kernels -- both sides of every 32-row block and 64-lane wave seam, and matrices smaller than one block.  NATURAL: default
options."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import batched_blocked_inv_model as BI
import batched_inv_model as MI
from test_gpu_batched_inv import FILL, INV_KINDS, _bits, _dev_batch, _model, _upload

pytestmark = pytest.mark.gpu

SMALL = [1, 2, 7, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128]
NATURAL = [129, 130, 161, 256, 257]
LARGE = [511, 513, 1023, 1024]
TILES = [8, 16]
CHUNK = 1 << 15           # BB_MAX_LAUNCH of csrc/mpf_internal.h


@pytest.fixture(scope="module")
def bctx(mpf):
    """Every n through the blocked kernels; the tests set batched_blocked_inv_ct as they go."""
    c = mpf.MPFContext(0, options={"batched_blocked_min_n": 0})
    yield c
    c.close()


def _sentinel_out(c, batch, n):
    buf = c.colmajor_batch(batch, n + 1, n)
    buf.fill_(FILL)
    return buf, buf[:, :n, :]


# ---- the inverse -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SMALL)
def test_small_against_the_model_and_getri_batched(bctx, ctx, n):
    import torch
    facs = [_model(n, k) for k in INV_KINDS]
    LU, ipiv = _upload(bctx, facs)
    keep_LU, keep_piv = LU.clone(memory_format=torch.preserve_format), ipiv.clone()
    small, _ = ctx.getri_batched(LU, ipiv)
    for ct in [0] + TILES:
        bctx.set_option("batched_blocked_inv_ct", ct)
        buf, out = _sentinel_out(bctx, len(facs), n)
        info = torch.full((len(facs),), -7, dtype=torch.int32, device=bctx.device)
        X, info2 = bctx.getri_batched_blocked(LU, ipiv, out=out, info=info)
        assert X.data_ptr() == buf.data_ptr() and info2.data_ptr() == info.data_ptr()
        assert info.cpu().numpy().tolist() == [0] * len(facs)
        got = X.cpu().numpy()
        for b, kind in enumerate(INV_KINDS):
            assert np.array_equal(_bits(got[b]), _bits(facs[b][2])), (n, kind, ct)
        assert np.array_equal(_bits(got), _bits(small)), (n, ct)
        assert bool((buf[:, n, :] == FILL).all())
    bctx.set_option("batched_blocked_inv_ct", 0)
    assert np.array_equal(_bits(LU), _bits(keep_LU)) and bool((ipiv == keep_piv).all())


@functools.lru_cache(maxsize=None)
def _crafted(n):
    """Factors passed straight in: L with -0.0 and exact zeros, pivots by reversal, from the last row, and with entries out of
    range.  (LU, ipiv, the contract's inverse with the out-of-range entries read as "no interchange")."""
    rng = np.random.default_rng(500 + n)
    out = []
    j = np.arange(n)
    for kind in ("reversal", "last_row", "out_of_range"):
        LU = rng.uniform(-1.0, 1.0, (n, n))
        LU[j, j] = rng.uniform(1.0, 2.0, n) * rng.choice([-1.0, 1.0], n)
        low = np.tril_indices(n, -1)
        sel = rng.random(len(low[0]))
        LU[low[0][sel < 0.15], low[1][sel < 0.15]] = 0.0
        LU[low[0][sel > 0.85], low[1][sel > 0.85]] = -0.0
        if kind == "reversal":
            p = np.where(j < n // 2, n - 1 - j, j)
        elif kind == "last_row":
            p = np.full(n, n - 1)
        else:
            p = j + rng.integers(0, n - j)
            bad = np.array([-6, -1, n, n + 1, 999])
            at = rng.integers(0, n, size=min(n, 5))
            p[at] = bad[:len(at)]
        ipiv = (p + 1).astype(np.int32)
        want = MI.getri_model(LU, (BI.clean_pivots(ipiv, n) + 1).astype(np.int32))
        for a in (LU, ipiv, want):
            a.setflags(write=False)
        out.append((LU, ipiv, want))
    return out


@pytest.mark.parametrize("n", [2, 33, 64, 97, 128])
def test_small_crafted_factors(bctx, n):
    facs = _crafted(n)
    LU, ipiv = _upload(bctx, facs)
    for ct in TILES:
        bctx.set_option("batched_blocked_inv_ct", ct)
        X, info = bctx.getri_batched_blocked(LU, ipiv)
        assert not bool(info.any())
        for b, f in enumerate(facs):
            assert np.array_equal(_bits(X[b]), _bits(f[2])), (n, b, ct)
    bctx.set_option("batched_blocked_inv_ct", 0)


@pytest.mark.parametrize("n", NATURAL)
def test_natural_path_against_the_model(ctx, n):
    facs = [_model(n, k) for k in INV_KINDS]
    LU, ipiv = _upload(ctx, facs)
    X, info = ctx.getri_batched_blocked(LU, ipiv)
    assert not bool(info.any())
    for b, kind in enumerate(INV_KINDS):
        assert np.array_equal(_bits(X[b]), _bits(facs[b][2])), (n, kind)


@pytest.mark.parametrize("n", LARGE)
def test_large_against_the_solve_on_an_identity(ctx, n):
    import torch
    rng = np.random.default_rng(n)
    LU, ipiv, finfo = ctx.getrf_batched_blocked(_dev_batch(ctx, rng.standard_normal((3, n, n))))
    assert not bool(finfo.any())
    eye = ctx.colmajor_batch(3, n, n)
    eye.copy_(torch.eye(n, dtype=torch.float64, device=ctx.device).expand(3, n, n))
    want = ctx.getrs_batched_blocked(LU, ipiv, eye, overwrite=True)
    X, info = ctx.getri_batched_blocked(LU, ipiv)
    assert not bool(info.any())
    assert np.array_equal(_bits(X), _bits(want)), n


def test_small_n_is_forwarded_by_default(ctx):
    facs = [_model(65, k) for k in INV_KINDS]
    LU, ipiv = _upload(ctx, facs)
    X, info = ctx.getri_batched_blocked(LU, ipiv)
    for b in range(len(facs)):
        assert np.array_equal(_bits(X[b]), _bits(facs[b][2]))
    mant, expo = ctx.getdet_batched_blocked(LU, ipiv)
    for b, f in enumerate(facs):
        assert (float(mant[b]), int(expo[b])) == MI.getdet_model(np.diag(f[0]), f[1])


@pytest.mark.parametrize("n", [33, 161])
def test_singular_matrices_are_reported_and_left_alone(bctx, n):
    import torch
    zero_at = {0: 0, 2: 31, 3: 32, 5: n - 1}
    facs = [_model(n, "normal", seed=s) for s in range(1, 7)]
    mats = [f[0].copy() for f in facs]
    for b, i in zero_at.items():
        mats[b][i, i] = 0.0
    mats[3][n - 1, n - 1] = 0.0                                    # (a second zero behind the first: the first is reported)
    batch = len(mats)
    LU = _dev_batch(bctx, mats)
    ipiv = torch.from_numpy(np.stack([f[1] for f in facs])).to(bctx.device)
    want_info = [zero_at[b] + 1 if b in zero_at else 0 for b in range(batch)]
    for with_info in (True, False):
        buf, out = _sentinel_out(bctx, batch, n)
        info = torch.full((batch,), -7, dtype=torch.int32, device=bctx.device)
        lay = bctx._batch_layout(out)
        bctx._bind()                                               # (the direct call below runs on the stream of the fills above)
        rc = bctx.L.mpf_getri_batched_blocked(bctx.h, C.c_void_p(LU.data_ptr()), n, n * n, n, batch, C.c_void_p(ipiv.data_ptr()), n,
                                              C.c_void_p(out.data_ptr()), lay[0], lay[1],
                                              C.c_void_p(info.data_ptr() if with_info else 0))
        assert rc == 0
        bctx.synchronize()
        assert info.cpu().numpy().tolist() == (want_info if with_info else [-7] * batch)
        for b in range(batch):
            if b in zero_at:
                assert bool((buf[b] == FILL).all()), (n, b, with_info)
            else:
                assert np.array_equal(_bits(out[b]), _bits(facs[b][2])), (n, b, with_info)
        assert bool((buf[:, n, :] == FILL).all())


@pytest.mark.parametrize("n", [40, 161])
def test_nan_in_one_matrix_stays_there(bctx, n):
    import torch
    facs = [_model(n, "normal", seed=s) for s in (7, 8, 9)]
    mats = [f[0].copy() for f in facs]
    mats[1][3, 1] = np.nan
    mats[1][1, 4] = np.inf
    mats[1][n - 1, n - 1] = np.nan
    piv = np.stack([f[1] for f in facs]).copy()
    piv[1][2] = 1000
    piv[1][n - 1] = -3
    LU = _dev_batch(bctx, mats)
    buf = bctx.colmajor_batch(4, n, n)
    buf.fill_(FILL)
    X, info = bctx.getri_batched_blocked(LU, torch.from_numpy(piv).to(bctx.device), out=buf[:3])
    bctx.synchronize()
    for b in (0, 2):
        assert np.array_equal(_bits(X[b]), _bits(facs[b][2])), (n, b)
        assert int(info[b]) == 0
    assert bool((buf[3] == FILL).all())


@pytest.mark.parametrize("n", [33, 161])
def test_padded_layouts_give_the_same_bits(bctx, n):
    import torch
    batch, ldlu, sp, ldinv = 3, n + 3, n + 2, n + 1
    slu, sinv = ldlu * n + 11, ldinv * n + 5
    facs = [_model(n, "normal", seed=s) for s in (10, 11, 12)]
    lubuf = torch.full((batch * slu,), 3.5, dtype=torch.float64, device=bctx.device)
    pbuf = torch.full((batch * sp,), -7, dtype=torch.int32, device=bctx.device)
    ibuf = torch.full((batch * sinv,), FILL, dtype=torch.float64, device=bctx.device)
    LU = torch.as_strided(lubuf, (batch, n, n), (slu, 1, ldlu))
    P = torch.as_strided(pbuf, (batch, n), (sp, 1))
    out = torch.as_strided(ibuf, (batch, n, n), (sinv, 1, ldinv))
    LU.copy_(torch.from_numpy(np.stack([f[0] for f in facs])))
    P.copy_(torch.from_numpy(np.stack([f[1] for f in facs])))
    keep_lu, keep_p = lubuf.clone(), pbuf.clone()
    X, info = bctx.getri_batched_blocked(LU, P, out=out)
    assert X.data_ptr() == ibuf.data_ptr()
    for b in range(batch):
        assert np.array_equal(_bits(X[b]), _bits(facs[b][2])), (n, b)
    assert info.cpu().numpy().tolist() == [0] * batch
    pad = torch.ones_like(ibuf, dtype=torch.bool)
    torch.as_strided(pad, (batch, n, n), (sinv, 1, ldinv)).fill_(False)
    assert int(pad.sum()) == batch * sinv - batch * n * n and bool((ibuf[pad] == FILL).all())
    assert np.array_equal(_bits(lubuf), _bits(keep_lu)) and bool((pbuf == keep_p).all())
    mant, expo = bctx.getdet_batched_blocked(LU, P)
    for b in range(batch):
        assert (float(mant[b]), int(expo[b])) == MI.getdet_model(np.diag(facs[b][0]), facs[b][1]), (n, b)


@pytest.mark.parametrize("n,batches", [(33, (1, 2, 261)), (161, (1, 2, 67))])
def test_position_and_batch_change_nothing(bctx, n, batches):
    """The same matrix first, in the middle and last, at batch sizes that leave grid tails; the slot, the info word and the
    determinant behind the batch are not touched."""
    import torch
    one = _model(n, "normal", seed=20)
    X1, _ = bctx.getri_batched_blocked(*_upload(bctx, [one]))
    assert np.array_equal(_bits(X1[0]), _bits(one[2]))
    for batch in batches:
        others = [_model(n, "normal", seed=21 + (b % 3)) for b in range(batch)]
        where = sorted({0, batch // 2, batch - 1})
        for b in where:
            others[b] = one
        LU, ipiv = _upload(bctx, others)
        buf = bctx.colmajor_batch(batch + 1, n, n)
        buf.fill_(FILL)
        ibuf = torch.full((batch + 1,), -7, dtype=torch.int32, device=bctx.device)
        X, info = bctx.getri_batched_blocked(LU, ipiv, out=buf[:batch], info=ibuf[:batch])
        assert bool((buf[batch] == FILL).all()) and int(ibuf[batch]) == -7 and not bool(ibuf[:batch].any())
        for b in where:
            assert np.array_equal(_bits(X[b]), _bits(X1[0])), (n, batch, b)
        assert np.array_equal(_bits(X[batch - 1 if batch < 3 else 1]), _bits(others[batch - 1 if batch < 3 else 1][2]))


def test_batch_longer_than_one_launch(bctx):
    """Order 2 makes a batch past the launch chunk cheap: upper triangular factors [[a, c], [0, d]] with one interchange."""
    import torch
    batch = CHUNK + 3
    rng = np.random.default_rng(31)
    mats = np.zeros((batch, 2, 2))
    mats[:, 0, 0] = rng.uniform(1.0, 2.0, batch)
    mats[:, 1, 1] = rng.uniform(1.0, 2.0, batch)
    mats[:, 0, 1] = rng.uniform(-1.0, 1.0, batch)
    mats[:, 1, 0] = rng.uniform(-1.0, 1.0, batch)
    mats[-2, 1, 1] = 0.0
    LU = _dev_batch(bctx, mats)
    piv = np.tile(np.array([2, 2], dtype=np.int32), (batch, 1))
    ipiv = torch.from_numpy(piv).to(bctx.device)
    out = bctx.colmajor_batch(batch, 2, 2)
    out.fill_(FILL)
    X, info = bctx.getri_batched_blocked(LU, ipiv, out=out)
    inf = info.cpu().numpy()
    assert inf[-2] == 2 and np.count_nonzero(inf) == 1
    got = X.cpu().numpy()
    assert np.all(got[-2] == FILL)
    for b in (0, 1, CHUNK - 1, CHUNK, CHUNK + 2):
        assert np.array_equal(_bits(got[b]), _bits(MI.getri_model(mats[b], piv[b]))), b
    mant, expo = bctx.getdet_batched_blocked(LU, ipiv)
    for b in (0, CHUNK - 1, CHUNK, CHUNK + 2):
        assert (float(mant[b]), int(expo[b])) == MI.getdet_model(np.diag(mats[b]), piv[b]), b
    assert float(mant[-2]) == 0.0 and int(expo[-2]) == 0


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
    ri, det = L.mpf_getri_batched_blocked, L.mpf_getdet_batched_blocked

    def err():
        return L.mpf_last_error(h).decode()

    nn = n * n
    assert ri(h, pl, 1025, 1025 * 1025, 1025, 1, pp, 1025, po, 1025, 1025 * 1025, pi) == -1
    assert "mpf_factor_dev" in err() and "mpf_getri" in err()
    assert ri(h, pl, n - 1, nn, n, batch, pp, n, po, n, nn, pi) == -1 and "leading dimension" in err()
    assert ri(h, pl, n, nn, n, batch, pp, n, po, n - 1, nn, pi) == -1 and "leading dimension" in err()
    assert ri(h, pl, n, nn - 1, n, batch, pp, n, po, n, nn, pi) == -1 and "stride" in err()
    assert ri(h, pl, n, nn, n, batch, pp, n, po, n, nn - 1, pi) == -1 and "stride" in err()
    assert ri(h, pl, n, nn, n, batch, pp, n - 1, po, n, nn, pi) == -1 and "ipiv" in err()
    assert ri(h, pl, n, nn, -1, batch, pp, n, po, n, nn, pi) == -1
    assert ri(h, pl, n, nn, n, -1, pp, n, po, n, nn, pi) == -1
    for args in ((null, pp, po), (pl, null, po), (pl, pp, null)):
        assert ri(h, args[0], n, nn, n, batch, args[1], n, args[2], n, nn, pi) == -1 and "null" in err()
    # overlap: the result over the factors, and a result that starts inside the last matrix of the factors
    assert ri(h, pl, n, nn, n, batch, pp, n, pl, n, nn, pi) == -1 and "overlaps" in err() and "out of place" in err()
    inside = C.c_void_p(LU.data_ptr() + 8 * (batch * nn - 1))
    assert ri(h, pl, n, nn, n, batch, pp, n, inside, n, nn, pi) == -1 and "overlaps" in err()
    assert ri(h, pl, n, nn, n, 0, pp, n, po, n, nn, pi) == 0
    assert ri(h, pl, n, nn, 0, batch, pp, n, po, n, nn, pi) == 0
    assert det(h, pl, 1025, 1025 * 1025, 1025, 1, pp, 1025, pm, pe) == -1 and "mpf_factor_dev" in err() and "mpf_getdet" in err()
    assert det(h, pl, n - 1, nn, n, batch, pp, n, pm, pe) == -1 and "leading dimension" in err()
    assert det(h, pl, n, nn - 1, n, batch, pp, n, pm, pe) == -1 and "stride" in err()
    assert det(h, pl, n, nn, n, batch, pp, n - 1, pm, pe) == -1 and "ipiv" in err()
    for args in ((null, pp, pm, pe), (pl, null, pm, pe), (pl, pp, null, pe), (pl, pp, pm, null)):
        assert det(h, args[0], n, nn, n, batch, args[1], n, args[2], args[3]) == -1 and "null" in err()
    assert det(h, pl, n, nn, n, 0, pp, n, pm, pe) == 0
    assert det(h, pl, n, nn, 0, batch, pp, n, pm, pe) == 0
    ctx.synchronize()
    # nothing was written by any of these calls
    assert bool((out == FILL).all()) and bool((info == -7).all()) and bool((mant == FILL).all()) and bool((expo == -7).all())
    assert np.array_equal(_bits(LU), _bits(keep))
    with pytest.raises(mpf.MPFError):
        ctx.getri_batched_blocked(LU, ipiv, out=torch.zeros((batch, n, n), dtype=torch.float64, device=ctx.device))
    assert "batched_blocked_inv_ct" in mpf.option_names()


# ---- the determinant ---------------------------------------------------------------------------------------------------------------------
def _diag_batch(c, diags):
    """Factors that hold the given diagonals and a sentinel everywhere else (the determinant reads the diagonal only)."""
    n = len(diags[0])
    T = c.colmajor_batch(len(diags), n, n)
    T.fill_(float("nan"))
    import torch
    idx = torch.arange(n, device=c.device)
    T[:, idx, idx] = torch.from_numpy(np.stack(diags)).to(c.device)
    return T


@pytest.mark.parametrize("n", [1, 128, 255, 256, 257, 511, 512, 513, 1024])
def test_getdet_against_the_model_and_the_other_entry_points(bctx, ctx, n):
    import torch
    rng = np.random.default_rng(900 + n)
    base = rng.uniform(1.0, 2.0, n) * rng.choice([-1.0, 1.0], n)
    with_zero, with_inf, with_nan = base.copy(), base.copy(), base.copy()
    with_zero[n // 2] = 0.0
    with_inf[n - 1] = np.inf
    with_nan[0] = 0.0
    with_nan[n // 3] = np.nan                                      # non-finite wins over zero
    diags = [base, base * 2.0 ** rng.integers(-40, 40, n), np.full(n, 1e300), np.full(n, 1e-300), with_zero, with_inf, with_nan, base]
    odd = np.arange(1, n + 1, dtype=np.int32)
    odd[0] = n                                                     # one interchange (none when n == 1)
    even = odd.copy()
    if n > 2:
        even[1] = n                                                # two
    pivs = [np.arange(1, n + 1, dtype=np.int32), odd, even, odd, odd, even, odd, even]
    LU = _diag_batch(bctx, diags)
    ipiv = torch.from_numpy(np.stack(pivs)).to(bctx.device)
    mant, expo = bctx.getdet_batched_blocked(LU, ipiv)
    assert mant.dtype == torch.float64 and expo.dtype == torch.int32 and mant.shape == expo.shape == (len(diags),)
    m, e = mant.cpu().numpy(), expo.cpu().numpy()
    for b in range(len(diags)):
        wm, we = MI.getdet_model(diags[b], pivs[b])
        if math.isnan(wm):
            assert math.isnan(m[b]) and e[b] == 0, (n, b)
        else:
            assert _bits(np.float64(m[b])) == _bits(np.float64(wm)) and int(e[b]) == we, (n, b)
    assert m[4] == 0.0 and e[4] == 0 and np.isnan(m[5]) and np.isnan(m[6])
    if n > 2:                                                      # slots 0 and 7: the same diagonal, none and two interchanges
        assert _bits(np.float64(m[7])) == _bits(np.float64(m[0])) and e[7] == e[0]
    for b in (1, 2, 3):                                            # mpf_getdet on each matrix
        m1, e1 = ctx.getdet(ctx.from_numpy_f(np.diag(diags[b])), ipiv[b].contiguous())
        assert _bits(np.float64(m1)) == _bits(np.float64(m[b])) and e1 == int(e[b]), (n, b)
    if n <= 128:
        m2, e2 = ctx.getdet_batched(LU, ipiv)
        assert np.array_equal(_bits(m2.cpu().numpy()[:4]), _bits(m[:4])) and np.array_equal(e2.cpu().numpy(), e)


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
def test_inv_batched_blocked_end_to_end(ctx, mpf):
    """From torch's row-major default (the copy path).  dget03 on both sides against LAPACK's dtest.in threshold 30."""
    import torch
    rng = np.random.default_rng(300)
    n = 300
    A = rng.standard_normal((8, n, n)) + 4.0 * np.eye(n)
    dA = torch.from_numpy(A).to(ctx.device)
    assert dA.is_contiguous() and dA.stride() == (n * n, n, 1)
    X = ctx.inv_batched_blocked(dA)
    assert X.shape == (8, n, n)
    Xh = X.cpu().numpy()
    worst = max(max(MI.dget03_ratio(A[b], Xh[b], True), MI.dget03_ratio(A[b], Xh[b], False)) for b in range(8))
    print(f"inv_batched_blocked: worst dget03 ratio {worst:.3f}")
    assert worst <= 30.0
    assert np.array_equal(_bits(dA), _bits(A))
    B = A.copy()
    B[5][:, 7] = 0.0
    with pytest.raises(mpf.MPFError) as ei:
        ctx.inv_batched_blocked(torch.from_numpy(B).to(ctx.device))
    assert "inv_batched_blocked" in str(ei.value) and "matrix 5" in str(ei.value) and "zero pivot 8" in str(ei.value)


def test_slogdet_batched_blocked(ctx):
    """|logabsdet - (log|mant| + expo ln 2)| <= 8 * 2^-53 * max(0.7, |expo| ln 2), test_slogdet_batched_against_mant_and_expo's
    bound (in terms of expo, so it carries over to n <= 1024), and numpy's slogdet from the matrices themselves."""
    import torch
    ln2 = math.log(2.0)
    n = 300
    rng = np.random.default_rng(301)
    diags = [rng.uniform(1.0, 2.0, n) * rng.choice([-1.0, 1.0], n), np.full(n, 2.0 ** -1000), np.full(n, 1e300), np.ones(n)]
    diags[-1][n // 2] = 0.0
    LU = _diag_batch(ctx, diags)
    ipiv = torch.arange(1, n + 1, dtype=torch.int32, device=ctx.device).repeat(len(diags), 1).contiguous()
    mant, expo = ctx.getdet_batched_blocked(LU, ipiv)
    sign, logabs = ctx.slogdet_batched_blocked(LU, ipiv)
    assert sign.is_cuda and logabs.is_cuda and sign.shape == logabs.shape == (len(diags),)
    m, e, s, la = mant.cpu().numpy(), expo.cpu().numpy().astype(np.float64), sign.cpu().numpy(), logabs.cpu().numpy()
    assert s[-1] == 0.0 and la[-1] == -np.inf
    for b in range(len(diags) - 1):
        want = np.log(abs(m[b])) + e[b] * ln2
        err, bound = abs(la[b] - want), 8 * 2.0 ** -53 * max(0.7, abs(e[b]) * ln2)
        print(f"slogdet_batched_blocked slot {b}: expo {int(e[b])} |diff| {err:.3e} bound {bound:.3e}")
        assert s[b] == np.sign(m[b]) and err <= bound, b
    A = rng.standard_normal((3, n, n))
    sign, logabs = ctx.slogdet_batched_blocked(torch.from_numpy(A).to(ctx.device))
    s0, l0 = np.linalg.slogdet(A)
    assert np.array_equal(sign.cpu().numpy(), s0) and np.allclose(logabs.cpu().numpy(), l0, rtol=1e-12, atol=1e-12)
