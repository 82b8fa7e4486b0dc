"""GPU tests of the blocked batched LU (include/mpf_c.h: mpf_getrf_batched_blocked, mpf_getrs_batched_blocked;
csrc/batched_blocked.hip).

Every comparison is on bits (NaN positions as positions); there is no tolerance.  The yardsticks are the numpy models
(tests/batched_model.py, tests/pivot64_model.py; for fused = 1 with the oracle's one-FMA update), the n <= 128 entry points, and for the
large sizes the device's own mpf_dgetf2_piv.  SMALL: with option batched_blocked_min_n = 0 every n runs the blocked kernels -- a shape on
either side of every panel width (8, 16, 32) and of every 16-wide MFMA tile, and matrices smaller than one panel and one tile.  NATURAL:
default options, one past a panel and one past a tile, odd and even n (8- and 16-byte aligned columns)."""
import ctypes as C
import functools

import numpy as np
import pytest

import batched_model as M
import test_gpu_batched as TB
from test_gpu_batched import KINDS, _bits, _dev_batch, _matrix, _same_with_nans

pytestmark = pytest.mark.gpu

SMALL = [1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 65]
NATURAL = [129, 130, 160, 161, 255, 256, 257]
LARGE = [511, 512, 513, 1023, 1024]
WIDTHS = [8, 16, 32]
CHUNK = 1 << 15           # BB_MAX_LAUNCH of csrc/mpf_internal.h


@pytest.fixture(scope="module")
def bctx(mpf):
    """Every n through the blocked kernels; the tests set batched_blocked_nb as they go."""
    c = mpf.MPFContext(0, options={"batched_blocked_min_n": 0})
    yield c
    c.close()


@pytest.fixture(scope="module")
def nctx(mpf):
    """Default path choice; the tests set batched_blocked_nb as they go (the session's context keeps its defaults)."""
    c = mpf.MPFContext(0)
    yield c
    c.close()


def _check_against_models(got, oracle, n, fused, who):
    LU, ipiv, info = got
    assert LU.shape == (5, n, n) and ipiv.shape == (5, n) and info.shape == (5,)
    assert info.cpu().numpy().tolist() == [0] * 5, who
    lu, piv = LU.cpu().numpy(), ipiv.cpu().numpy()
    for b, kind in enumerate(KINDS):
        LU_m, piv_m, info_m = TB._model(n, kind, fused, oracle)
        assert info_m == 0
        assert np.array_equal(piv[b], piv_m), (who, n, kind, fused)
        assert np.array_equal(_bits(lu[b]), _bits(LU_m)), (who, n, kind, fused)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("nb", WIDTHS)
@pytest.mark.parametrize("n", SMALL)
def test_getrf_smallest_shapes(bctx, ctx, oracle, n, nb, fused):
    bctx.set_option("batched_blocked_nb", nb)
    A = _dev_batch(bctx, [_matrix(n, k) for k in KINDS])
    got = bctx.getrf_batched_blocked(A, fused=fused)
    _check_against_models(got, oracle, n, fused, f"nb={nb}")
    LU0, ipiv0, _ = ctx.getrf_batched(A, fused=fused)               # the n <= 128 sibling
    assert np.array_equal(_bits(got[0]), _bits(LU0)) and np.array_equal(got[1].cpu().numpy(), ipiv0.cpu().numpy())
    assert np.array_equal(_bits(A[0]), _bits(_matrix(n, KINDS[0])))  # the input was left alone


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("n", NATURAL)
def test_getrf_natural_path(ctx, nctx, oracle, n, fused):
    A = _dev_batch(ctx, [_matrix(n, k) for k in KINDS])
    got = ctx.getrf_batched_blocked(A, fused=fused)
    _check_against_models(got, oracle, n, fused, "auto")
    for nb in WIDTHS:                                               # the panel width changes no bit
        nctx.set_option("batched_blocked_nb", nb)
        LU, ipiv, info = nctx.getrf_batched_blocked(A, fused=fused)
        assert np.array_equal(_bits(LU), _bits(got[0])) and np.array_equal(ipiv.cpu().numpy(), got[1].cpu().numpy()), (n, nb, fused)
        assert not info.cpu().numpy().any()
    nctx.set_option("batched_blocked_nb", 0)


def test_small_n_is_forwarded_by_default(ctx, oracle):
    """n = 65 < batched_blocked_min_n = 129: the one-workgroup kernels take it, and the bits are the model's either way."""
    assert ctx.get_option("batched_blocked_min_n") == 129 and ctx.get_option("batched_blocked_nb") == 0
    A = _dev_batch(ctx, [_matrix(65, k) for k in KINDS])
    _check_against_models(ctx.getrf_batched_blocked(A), oracle, 65, False, "forwarded")


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("n", LARGE)
def test_getrf_large_against_the_panel_operator(ctx, n, fused):
    """The device's mpf_dgetf2_piv on the whole matrix is the yardstick here (the numpy model is slow at this size)."""
    import torch
    rng = np.random.default_rng(n + 5)
    mats = rng.standard_normal((3, n, n))
    LU, ipiv, info = ctx.getrf_batched_blocked(_dev_batch(ctx, mats), fused=fused)
    assert not info.cpu().numpy().any()
    for b in range(3):
        dP = ctx.from_numpy_f(mats[b])
        piv1, info1 = ctx.dgetf2_piv(dP, fused=fused)
        assert info1 == 0
        assert bool(torch.equal(ipiv[b], piv1.to(ipiv.dtype))), (n, fused, b)
        assert np.array_equal(_bits(LU[b]), _bits(dP)), (n, fused, b)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("n", [49, 161])
def test_fused_update_on_the_valu_kernel(mpf, bctx, n, fused):
    """Probe library: the VALU instantiation of the fused update is the MFMA kernel's cross-check."""
    pc = mpf.MPFContext(0, probe=True, options={"batched_blocked_min_n": 0, "batched_blocked_valu": 1})
    try:
        bctx.set_option("batched_blocked_nb", 0)
        mats = [_matrix(n, k, seed=3) for k in KINDS]
        LU, ipiv, _ = bctx.getrf_batched_blocked(_dev_batch(bctx, mats), fused=fused)
        LU1, ipiv1, _ = pc.getrf_batched_blocked(_dev_batch(pc, mats), fused=fused)
        assert np.array_equal(_bits(LU), _bits(LU1)) and np.array_equal(ipiv.cpu().numpy(), ipiv1.cpu().numpy())
    finally:
        pc.close()


# ---- independence ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [33, 161])
def test_position_batch_and_padding_change_nothing(bctx, n):
    """The same matrix at the first and the last position, alone, and in a padded layout whose padding rows and gaps keep their
    sentinel; overwrite=True works in place."""
    import torch
    bctx.set_option("batched_blocked_nb", 0)
    rng = np.random.default_rng(n)
    one = rng.standard_normal((n, n))
    mats = [one] + [rng.standard_normal((n, n)) for _ in range(3)] + [one]
    batch = len(mats)
    LU1, piv1, _ = bctx.getrf_batched_blocked(_dev_batch(bctx, [one]))
    LU, piv, info = bctx.getrf_batched_blocked(_dev_batch(bctx, mats))
    for b in (0, batch - 1):
        assert np.array_equal(_bits(LU[b]), _bits(LU1[0])) and np.array_equal(piv[b].cpu().numpy(), piv1[0].cpu().numpy())
    lda, sp = n + 3, n + 2
    sa = lda * n + 11
    buf = torch.full((batch * sa,), -7.25, dtype=torch.float64, device=bctx.device)
    pbuf = torch.full((batch * sp,), -7, dtype=torch.int32, device=bctx.device)
    A = torch.as_strided(buf, (batch, n, n), (sa, 1, lda))
    P = torch.as_strided(pbuf, (batch, n), (sp, 1))
    A.copy_(torch.from_numpy(np.stack(mats)))
    LU2, piv2, info2 = bctx.getrf_batched_blocked(A, overwrite=True, ipiv=P)
    assert LU2.data_ptr() == buf.data_ptr() and piv2.data_ptr() == pbuf.data_ptr()
    assert np.array_equal(_bits(LU2), _bits(LU)) and np.array_equal(piv2.cpu().numpy(), piv.cpu().numpy())
    assert not info2.cpu().numpy().any()
    pad = torch.ones_like(buf, dtype=torch.bool)
    torch.as_strided(pad, (batch, n, n), (sa, 1, lda)).fill_(False)
    assert int(pad.sum()) == batch * sa - batch * n * n and bool((buf[pad] == -7.25).all())
    ppad = torch.ones_like(pbuf, dtype=torch.bool)
    torch.as_strided(ppad, (batch, n), (sp, 1)).fill_(False)
    assert bool((pbuf[ppad] == -7).all())


def test_batch_longer_than_one_launch(bctx):
    """n = 1 makes a batch past the launch chunk cheap: LU = A, every pivot is 1, info names the zeros; the solve divides."""
    import torch
    batch = CHUNK + 3
    a = np.random.default_rng(22).uniform(1.0, 2.0, batch)
    a[-1] = 0.0
    A = torch.from_numpy(a).to(bctx.device).view(batch, 1, 1)
    LU, ipiv, info = bctx.getrf_batched_blocked(A)
    assert np.array_equal(_bits(LU.reshape(-1)), _bits(a))
    assert bool((ipiv == 1).all())
    inf = info.cpu().numpy()
    assert inf[-1] == 1 and not inf[:-1].any()
    rhs = np.random.default_rng(23).uniform(1.0, 2.0, batch)
    X = bctx.getrs_batched_blocked(LU, ipiv, torch.from_numpy(rhs).to(bctx.device).view(batch, 1, 1))
    with np.errstate(divide="ignore"):
        assert np.array_equal(_bits(X.reshape(-1)), _bits(rhs / a))


# ---- special values: once at a forced-small n, once at n = 161 ---------------------------------------------------------------------------
def _special(n):
    rng = np.random.default_rng(1000 + n)
    out = {}
    for name in ("plain0", "singular", "plain1", "nan_below", "nan_column", "inf_below_panel"):
        out[name] = rng.standard_normal((n, n))
    out["singular"][:, n // 2] = 0.0
    out["nan_below"][3, 0] = np.nan                 # below the diagonal in column 0
    out["nan_column"][:, 2] = np.nan                # an all-NaN column: p = j, and everything after it is NaN
    out["inf_below_panel"][min(32, n - 1), n - 2] = np.inf   # the first row below a 32-wide panel, in a column right of it
    return out


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("n", [40, 161])
def test_special_values(bctx, ctx, oracle, n, fused):
    sp = _special(n)
    names = list(sp)
    for nb in (WIDTHS if n == 40 else [0]):
        bctx.set_option("batched_blocked_nb", nb)
        LU, ipiv, info = bctx.getrf_batched_blocked(_dev_batch(bctx, [sp[k] for k in names]), fused=fused)
        lu, piv, inf = LU.cpu().numpy(), ipiv.cpu().numpy(), info.cpu().numpy()
        for b, name in enumerate(names):
            LU_m, piv_m, info_m = M.getrf_model(sp[name], TB._rank1(oracle, fused))
            assert np.array_equal(piv[b], piv_m), (n, nb, name)
            assert _same_with_nans(lu[b], LU_m), (n, nb, name)
            assert int(inf[b]) == info_m, (n, nb, name)
            if name.startswith("plain"):                    # the neighbours of the special matrices are ordinary
                assert info_m == 0 and not np.isnan(lu[b]).any()
        assert inf[names.index("singular")] == n // 2 + 1
        b = names.index("nan_below")
        assert piv[b][0] != 4 and not np.isnan(lu[b][0, 0])
        assert np.array_equal(piv[names.index("nan_column")][2:], np.arange(3, n + 1))
        assert np.isinf(lu[names.index("inf_below_panel")]).any() or np.isnan(lu[names.index("inf_below_panel")]).any()
    # the singular matrix as mpf_dgetf2_piv leaves it
    dP = ctx.from_numpy_f(sp["singular"])
    piv1, info1 = ctx.dgetf2_piv(dP, fused=fused)
    b = names.index("singular")
    assert info1 == inf[b] and np.array_equal(piv1.cpu().numpy(), piv[b]) and _same_with_nans(lu[b], dP.cpu().numpy())
    bctx.set_option("batched_blocked_nb", 0)


# ---- solve ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _solve_inputs(n, batch=3):
    rng = np.random.default_rng(31 * n + 1)
    return rng.standard_normal((batch, n, n)), rng.standard_normal((batch, n, 33))


@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("n", SMALL + NATURAL + [513])
def test_getrs_against_the_model(bctx, ctx, n, trans):
    """On the factors the device produced.  nrhs = 1, 3 take the one-column tile, 8 and 33 the eight-column tile (33: a ragged last tile)."""
    import torch
    bctx.set_option("batched_blocked_nb", 0)
    A, Ball = _solve_inputs(n)
    batch = A.shape[0]
    LU, ipiv, info = bctx.getrf_batched_blocked(_dev_batch(bctx, A))
    assert not info.cpu().numpy().any()
    lu, piv = np.stack([bctx.to_numpy_f(LU[b]) for b in range(batch)]), ipiv.cpu().numpy()
    want33 = None
    for nrhs in ((2,) if n == 513 else (1, 3, 8, 33)):
        B = Ball[:, :, :nrhs]
        want = np.stack([M.getrs_model(lu[b], piv[b], B[b], trans) for b in range(batch)])
        buf = bctx.colmajor_batch(batch, n + 1, nrhs)       # ldb = n + 1: one sentinel row under every matrix
        buf.fill_(-7.25)
        Bd = buf[:, :n, :]
        Bd.copy_(torch.from_numpy(np.ascontiguousarray(B)))
        X = bctx.getrs_batched_blocked(LU, ipiv, Bd, trans=trans, overwrite=True)
        assert X.data_ptr() == buf.data_ptr()
        assert np.array_equal(_bits(X), _bits(want)), (n, nrhs, trans)
        assert bool((buf[:, n, :] == -7.25).all()), (n, nrhs, trans)
        if n <= 128:                                        # the n <= 128 sibling, on the same factors
            X0 = ctx.getrs_batched(LU, ipiv, torch.from_numpy(np.ascontiguousarray(B)).to(ctx.device), trans=trans)
            assert np.array_equal(_bits(X0), _bits(want)), (n, nrhs, trans)
        if nrhs == 33:
            want33 = want
    if want33 is not None:                                  # a column solved alone equals the same column solved among 33
        X1 = bctx.getrs_batched_blocked(LU, ipiv, torch.from_numpy(np.ascontiguousarray(Ball[:, :, 20:21])).to(bctx.device), trans=trans)
        assert np.array_equal(_bits(X1[:, :, 0]), _bits(want33[:, :, 20])), (n, trans)
        xv = bctx.getrs_batched_blocked(LU, ipiv, torch.from_numpy(np.ascontiguousarray(Ball[:, :, 0])).to(bctx.device), trans=trans)
        assert xv.shape == (batch, n) and np.array_equal(_bits(xv), _bits(want33[:, :, 0]))


@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("n", [40, 161])
def test_exact_small_integer_systems(bctx, n, trans):
    """A = L U with l_ij in {-1/2, 0, 1/2}, u_jj = +-2^k (k = 1, 2, 3), small integers above the diagonal: every |l_ij u_jj| < |u_jj|, so
    partial pivoting interchanges nothing, every intermediate of the elimination and of both triangular solves is a dyadic number of
    a few bits, and the integer solution comes back exactly."""
    import torch
    bctx.set_option("batched_blocked_nb", 0)
    rng = np.random.default_rng(n)
    batch = 3
    L = np.tril(rng.integers(-1, 2, (batch, n, n)) * 0.5, -1) + np.eye(n)
    U = np.triu(rng.integers(-2, 3, (batch, n, n)).astype(np.float64), 1)
    d = rng.choice([-1.0, 1.0], (batch, n)) * 2.0 ** rng.integers(1, 4, (batch, n))
    U[:, np.arange(n), np.arange(n)] = d
    A = L @ U
    X = rng.integers(-4, 5, (batch, n, 5)).astype(np.float64)
    B = (np.swapaxes(A, 1, 2) if trans else A) @ X
    assert np.abs(A).max() < 2.0 ** 20 and np.abs(B).max() < 2.0 ** 30      # exact products and sums
    got = bctx.solve_batched_blocked(torch.from_numpy(A).to(bctx.device), torch.from_numpy(B).to(bctx.device), trans=trans)
    assert np.array_equal(got.cpu().numpy(), X)
    LU, ipiv, _ = bctx.getrf_batched_blocked(torch.from_numpy(A).to(bctx.device))
    assert np.array_equal(ipiv.cpu().numpy(), np.tile(np.arange(1, n + 1, dtype=np.int32), (batch, 1)))
    assert np.array_equal(LU.cpu().numpy(), np.tril(L, -1) + U)


# ---- arguments and the Python layer ----------------------------------------------------------------------------------------------------
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

    rf, rs = L.mpf_getrf_batched_blocked, L.mpf_getrs_batched_blocked
    assert rf(h, pa, 1025, 1025 * 1025, 1025, 1, pp, 1025, null, 0) == -1 and "mpf_factor_dev" in err()
    assert rf(h, pa, n - 1, n * n, n, batch, pp, n, null, 0) == -1 and "leading dimension" in err()
    assert rf(h, pa, n, n * n - 1, n, batch, pp, n, null, 0) == -1 and "stride" in err()
    assert rf(h, pa, n, n * n, n, batch, pp, n - 1, null, 0) == -1 and "ipiv" in err()
    assert rf(h, pa, n, n * n, -1, batch, pp, n, null, 0) == -1
    assert rf(h, pa, n, n * n, n, -1, pp, n, null, 0) == -1
    assert rf(h, null, n, n * n, n, batch, pp, n, null, 0) == -1 and "null" in err()
    assert rf(h, pa, n, n * n, n, batch, null, n, null, 0) == -1 and "null" in err()
    assert rf(h, pa, n, n * n, n, 0, pp, n, null, 0) == 0
    assert rf(h, pa, n, n * n, 0, batch, pp, n, null, 0) == 0
    assert rs(h, 0, pa, 1025, 1025 * 1025, 1025, 1, pp, 1025, 1, pb, 1025, 1025) == -1 and "mpf_factor_dev" in err()
    assert rs(h, 0, pa, n, n * n, n, batch, pp, n, 2, pb, n - 1, 2 * n) == -1 and "leading dimension" in err()
    assert rs(h, 0, pa, n, n * n, n, batch, pp, n, 2, pb, n, 2 * n - 1) == -1 and "stride" in err()
    assert rs(h, 2, pa, n, n * n, n, batch, pp, n, 2, pb, n, 2 * n) == -1 and "trans" in err()
    assert rs(h, 0, pa, n, n * n, n, batch, pp, n, -1, pb, n, 2 * n) == -1
    assert rs(h, 0, pa, n, n * n, n, batch, pp, n, 2, null, n, 2 * n) == -1 and "null" in err()
    assert rs(h, 0, pa, n, n * n, n, batch, pp, n, 0, pb, n, 2 * n) == 0
    assert rs(h, 0, pa, n, n * n, n, 0, pp, n, 2, pb, n, 2 * n) == 0
    assert rs(h, 0, pa, n, n * n, 0, batch, pp, n, 2, pb, n, 2 * n) == 0
    ctx.synchronize()
    # the zero sizes wrote nothing
    assert np.array_equal(_bits(A), _bits(keep)) and bool((B == 1.0).all()) and not ipiv.cpu().numpy().any()
    names = mpf.option_names()
    assert "batched_blocked_min_n" in names and "batched_blocked_nb" in names
    # the n <= 128 entry points keep their limit
    assert L.mpf_getrf_batched(h, pa, 129, 129 * 129, 129, 1, pp, 129, null, 0) == -1 and "mpf_factor_dev" in err()


def test_python_layer(ctx, mpf):
    import torch
    n = 130
    rng = np.random.default_rng(130)
    A, B = rng.standard_normal((4, n, n)), rng.standard_normal((4, n, 2))
    dA, dB = torch.from_numpy(A).to(ctx.device), torch.from_numpy(B).to(ctx.device)
    assert dA.is_contiguous()                                  # torch's row-major default: copied, the input stays
    LU, ipiv, info = ctx.getrf_batched_blocked(dA)
    assert LU.data_ptr() != dA.data_ptr() and np.array_equal(_bits(dA), _bits(A))
    LU_m, piv_m, _ = M.getrf_model(A[1])
    assert np.array_equal(ipiv[1].cpu().numpy(), piv_m) and np.array_equal(_bits(LU[1]), _bits(LU_m))
    X = ctx.solve_batched_blocked(dA, dB)
    assert np.array_equal(_bits(X[1]), _bits(M.getrs_model(LU_m, piv_m, B[1])))
    with pytest.raises(mpf.MPFError):
        ctx.getrf_batched_blocked(dA, overwrite=True)
    with pytest.raises(mpf.MPFError) as ei:
        ctx.getrf_batched_blocked(ctx.colmajor_batch(1, 1025, 1025))
    assert "mpf_factor_dev" in str(ei.value)
    A[2][:, 7] = 0.0
    with pytest.raises(mpf.MPFError) as ei:
        ctx.solve_batched_blocked(torch.from_numpy(A).to(ctx.device), dB)
    assert "matrix 2" in str(ei.value) and "zero pivot 8" in str(ei.value)
