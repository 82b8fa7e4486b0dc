"""GPU tests of the extra-precise refinement (include/mpf_c.h: mpf_residual_x, mpf_gerfsx) against tests/gerfsx_model.py: the
residual against an exactly rounded one (math.fsum over the exact products) and, on grid data, against an int64 product; the refined
solution against a reference kept as an unevaluated pair of doubles; corrections and states against the model driven by the device's
own factors.  EPS = 2^-53 throughout.

The residual's bound, per element, is the pair accumulation's own error bound with a factor 4 of slack:
    |r - r_exact| <= 2^-52 |r_exact| + 4 (N + 1) 2^-106 S,   S = |b| + sum_k |a_k| |x_k|
(the model's largest ratio to it is 0.019; one fp64 chain misses it by 10^2 .. 10^12)."""
import ctypes as C

import numpy as np
import pytest

import blk_helpers as H
import gerfsx_model as G

pytestmark = pytest.mark.gpu
EPS = G.EPS
FILL = 7.5


def _resx(ctx, dA, lda, X_np, B_np, trans, pad):
    """mpf_residual_x through the C ABI on buffers with `pad` extra rows of FILL: (R, whether every padding row kept FILL)."""
    n, m = B_np.shape
    ld = n + pad
    X, Xbuf = H.dev(ctx, X_np, ld)
    B, Bbuf = H.dev(ctx, B_np, ld)
    R, Rbuf = H.dev(ctx, np.full((n, m), FILL), ld)
    ctx._bind()
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = ctx.L.mpf_residual_x(ctx.h, int(trans), p(dA), lda, n, m, p(X), ld, p(B), ld, p(R), ld)
    assert rc == 0, ctx.L.mpf_last_error(ctx.h)
    kept = all(bool((b[n:] == FILL).all()) for b in (Xbuf, Bbuf, Rbuf))
    same = np.array_equal(X.cpu().numpy(), X_np) and np.array_equal(B.cpu().numpy(), B_np)
    return R.cpu().numpy(), kept and same


def _gerfsx(ctx, dA, W, ipiv, B, X, trans, ithresh=0):
    """mpf_gerfsx through the C ABI, in place on X: (rc, err_norm, err_comp, stats)."""
    import importlib
    mpf = importlib.import_module("mixed-precision_lu_factorization_amd")
    n, m = B.shape
    ctx._bind()
    p = lambda t: C.c_void_p(t.data_ptr())
    en, ec = np.zeros(max(m, 1)), np.zeros(max(m, 1))
    st = (mpf.MpfGerfsxStats * max(m, 1))()
    dp = C.POINTER(C.c_double)
    rc = ctx.L.mpf_gerfsx(ctx.h, int(trans), p(dA), H.ld(dA), p(W), H.ld(W), p(ipiv), n, m, p(B), H.ld(B), p(X), H.ld(X), int(ithresh),
                          en.ctypes.data_as(dp), ec.ctypes.data_as(dp), st)
    assert rc >= 0, ctx.L.mpf_last_error(ctx.h)
    return rc, en[:m], ec[:m], list(st)[:m]


def _key(X_np, en, ec, st, j):
    s = st[j]
    return (H.bits(X_np[:, j]).tolist(), H.bits(en[j:j + 1])[0], H.bits(ec[j:j + 1])[0], s.iterations, s.x_state, s.z_state, s.solves,
            H.bits(np.array([s.final_dx_x, s.final_dz_z, s.dxratmax, s.dzratmax])).tolist())


# ---- the residual ---------------------------------------------------------------------------------------------------------------
NRHS = (1, 33, 70)      # one column, the 32-column tile seam, the seam of the two tiles of one launch


@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 31, 65, 257, 300])
def test_residual_full_mantissa(ctx, n, trans):
    """Full-mantissa data, X once the fp64 solution (a heavily cancelling residual) and once random, nrhs = 1, 33, 70 (the reference
    is computed once for 70 columns: a column's bits do not depend on its neighbours), every leading dimension padded."""
    rng = np.random.default_rng(100 * n + trans)
    A = G.rand(n, 40 + n)
    Aop = np.ascontiguousarray(A.T if trans else A)
    B = rng.uniform(-1, 1, (n, max(NRHS)))
    dA, Abuf = H.dev(ctx, A, n + 5)
    for kind, X in (("solution", np.linalg.solve(Aop, B)), ("random", rng.uniform(-1, 1, B.shape))):
        Rx = G.exact_residual(Aop, X, B)
        S = np.abs(B) + np.abs(Aop) @ np.abs(X)
        bound = 2.0 ** -52 * np.abs(Rx) + 4 * (n + 1) * 2.0 ** -106 * S
        for m in NRHS:
            R, untouched = _resx(ctx, dA, n + 5, X[:, :m], B[:, :m], trans, pad=3)
            err = np.abs(R - Rx[:, :m])
            print(n, trans, kind, m, "largest error / bound", (err / bound[:, :m]).max())
            assert np.all(err <= bound[:, :m]), (kind, m, (err / bound[:, :m]).max())
            assert untouched, "padding rows or inputs were written"
    assert bool((Abuf[n:] == FILL).all())


@pytest.mark.parametrize("trans", [0, 1])
def test_residual_partial_seam_exact(ctx, trans):
    """N = 4100 (two partials of 4096 columns of op(A)): A on a 2^-20 grid, X on a 2^-30 grid, B = numpy's fp64 A X.  Every product is
    exact and everything lies on a 2^-50 grid, so the exact residual is an int64 product on the host and any correct pair
    accumulation returns it exactly."""
    n, m = 4100, 4
    rng = np.random.default_rng(77)
    Ai, Xi = rng.integers(-2 ** 20, 2 ** 20, (n, n)), rng.integers(-2 ** 30, 2 ** 30, (n, m))
    Aopi = np.ascontiguousarray(Ai.T if trans else Ai)
    A, X = Ai * 2.0 ** -20, Xi * 2.0 ** -30
    B = (A.T if trans else A) @ X
    assert np.abs(B).max() < 2.0 ** 12
    Bi = (B * 2.0 ** 50).astype(np.int64)
    assert np.array_equal(Bi * 2.0 ** -50, B), "B is not on the 2^-50 grid"
    Ri = Bi - Aopi @ Xi                                   # |terms| <= 4100 x 2^50 + 2^62 < 2^63
    assert np.abs(Ri).max() < 2 ** 53
    Rx = Ri * 2.0 ** -50
    dA, _ = H.dev(ctx, A)
    R, untouched = _resx(ctx, dA, n, X, B, trans, pad=1)
    print("non-zero entries", np.count_nonzero(Rx), "of", Rx.size, "wrong", np.count_nonzero(R != Rx))
    assert np.count_nonzero(Rx) > 0.5 * Rx.size
    assert np.array_equal(R, Rx) and untouched


# ---- bits -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide(ctx):
    """N = 64 with 513 columns (one more than a group of 512) scaled 1e-3 .. 1e3, fp64 factors, both op(A): the residual of getrs's X
    and gerfsx's results for all columns, once.  Shared and left unchanged."""
    import torch
    n, m = 64, 513
    A = G.rand(n, 8)
    dA, W, ipiv, _ = H.factor(ctx, A, nb=32)
    B = torch.from_numpy(np.random.default_rng(9).uniform(-1, 1, (n, m)) * np.logspace(-3, 3, m)).to(ctx.device).t().contiguous().t()
    out = {}
    for trans in (0, 1):
        X0 = ctx.getrs(W, ipiv, B, trans=trans)
        R = ctx.residual_x(dA, X0, B, trans=trans).cpu().numpy()
        X, en, ec, st = ctx.gerfsx(dA, W, ipiv, B, X0, trans=trans)
        out[trans] = (X0, R, (X.cpu().numpy(), en, ec, st))
    return dA, W, ipiv, B, out


@pytest.mark.parametrize("trans", [0, 1])
def test_column_independence(ctx, wide, trans):
    """A column's residual and its gerfsx results (x, both bounds, the stats but ms_total) have the same bits among 513 columns
    (across the group seam), alone, at another position among 37 others, and in a second call."""
    import torch
    dA, W, ipiv, B, out = wide
    X0, R, full = out[trans]
    assert all(s.ms_total == full[3][0].ms_total for s in full[3])
    X2, en2, ec2, st2 = ctx.gerfsx(dA, W, ipiv, B, X0, trans=trans)
    again = (X2.cpu().numpy(), en2, ec2, st2)
    assert np.array_equal(H.bits(ctx.residual_x(dA, X0, B, trans=trans).cpu().numpy()), H.bits(R))
    for j in range(B.shape[1]):
        assert _key(*again, j) == _key(*full, j), j
    pick = np.random.default_rng(4).permutation(513)[:37]
    pick[:4] = (512, 0, 31, 32)
    idx = torch.from_numpy(pick).to(ctx.device)
    Bp, Xp0 = B[:, idx].t().contiguous().t(), X0[:, idx].t().contiguous().t()
    assert np.array_equal(H.bits(ctx.residual_x(dA, Xp0, Bp, trans=trans).cpu().numpy()), H.bits(R[:, pick]))
    Xp, enp, ecp, stp = ctx.gerfsx(dA, W, ipiv, Bp, Xp0, trans=trans)
    permd = (Xp.cpu().numpy(), enp, ecp, stp)
    for i, j in enumerate(pick):
        assert _key(*permd, i) == _key(*full, int(j)), j
    for j in (0, 32, 512):
        bj, xj = B[:, j:j + 1].contiguous(), X0[:, j:j + 1].contiguous()
        assert np.array_equal(H.bits(ctx.residual_x(dA, xj, bj, trans=trans).cpu().numpy()[:, 0]), H.bits(R[:, j])), j
        Xa, ena, eca, sta = ctx.gerfsx(dA, W, ipiv, bj, xj, trans=trans)
        assert _key(Xa.cpu().numpy(), ena, eca, sta, 0) == _key(*full, j), j
        assert np.array_equal(xj.cpu().numpy(), X0[:, j:j + 1].cpu().numpy()), "overwrite=False changed X"


# ---- mpf_gerfsx -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("kappa,seed", [(1e2, 1), (1e6, 2), (1e10, 3)])
def test_fp64_factors(ctx, kappa, seed, trans):
    """ill(257, kappa), 33 columns, X on entry from getrs: every column converges, the error against the pair-of-doubles reference
    is within 4 x 2^-53 and within the bounds.  For kappa = 1e10 the X of solve_ir_block at tol = 1e-14 is more than 100 x 2^-53 off
    (the model's plain fp64 residual: 6e8 x 2^-53): that is what the feature is for."""
    n, m = 257, 33
    A = G.ill(n, kappa, seed)
    Aop = np.ascontiguousarray(A.T if trans else A)
    B_np = np.random.default_rng(seed).uniform(-1, 1, (n, m))
    Minv = np.linalg.inv(Aop)
    Xh, Xl = G.reference_pair(Aop, B_np, lambda V: Minv @ V)
    dA, W, ipiv, _ = H.factor(ctx, A)
    B, _ = H.dev(ctx, B_np)
    X = ctx.getrs(W, ipiv, B, trans=trans)
    rc, en, ec, st = _gerfsx(ctx, dA, W, ipiv, B, X, trans)
    e_norm, e_comp = G.errors(X.cpu().numpy(), Xh, Xl)
    zc = np.array([s.z_state == G.Z_CONV for s in st])
    print(kappa, trans, "norm/eps", e_norm.max() / EPS, "comp/eps", e_comp.max() / EPS, "corrections", sorted({s.iterations for s in st}),
          "z converged", int(zc.sum()), "err_norm/eps", en.max() / EPS, "err_comp/eps", ec[zc].max() / EPS if zc.any() else None)
    assert rc == 0 and all(s.x_state == G.X_CONV for s in st)
    assert np.all(e_norm <= 4 * EPS) and np.all(e_norm <= en)
    assert np.all(e_comp[zc] <= 4 * EPS) and np.all(e_comp[zc] <= ec[zc])
    assert all(s.solves == s.iterations + 1 and s.ms_total == st[0].ms_total for s in st)
    if kappa == 1e10:
        Xir, _ = ctx.solve_ir_block(dA, W, ipiv, B, trans=trans, tol=1e-14)
        plain = G.errors(Xir.cpu().numpy(), Xh, Xl)[0]
        print("solve_ir_block norm/eps", plain.min() / EPS, plain.max() / EPS)
        assert np.all(plain > 100 * EPS)


@pytest.fixture(scope="module")
def lowp(ctx):
    """The suite's diagonally dominant rand(300) on fp16 factors, 5 columns: the device's factors on the host, the reference."""
    n, m = 300, 5
    A = G.rand(n, 11)
    B_np = np.random.default_rng(3).uniform(-1, 1, (n, m))
    dA, W, ipiv, _ = H.factor(ctx, A, trailing=1)
    B, _ = H.dev(ctx, B_np)
    LU, ip = ctx.to_numpy_f(W), ipiv.cpu().numpy()
    ref = {}
    for trans in (0, 1):
        Aop = np.ascontiguousarray(A.T if trans else A)
        Minv = np.linalg.inv(Aop)
        ref[trans] = (Aop, G.reference_pair(Aop, B_np, lambda V: Minv @ V), H.host_solvers(LU, ip, trans)[0])
    return dA, W, ipiv, B, B_np, ref


@pytest.mark.parametrize("ithresh", [0, 31])
@pytest.mark.parametrize("trans", [0, 1])
def test_fp16_factors(ctx, lowp, trans, ithresh):
    """fp16 factors converge within LAPACK's 10 iterations and within 31, to the same normwise 4 x 2^-53 (measured 0.42 .. 0.67);
    corrections and states agree with the model driven by the device's own factors, within one correction (another summation order
    in the solves may decide one step differently).  The componentwise error is printed, not asserted: a correction through fp16
    factors is accurate normwise only, to about a third of its own size here, so a component a hundred times below max |x| is
    left 1 .. 25 x 2^-53 off even where z_state ends CONV (measured; the model takes the same decisions); err_comp means what it says on factors
    that solve accurately per component, which test_fp64_factors asserts."""
    dA, W, ipiv, B, B_np, ref = lowp
    Aop, (Xh, Xl), solve = ref[trans]
    X = ctx.getrs(W, ipiv, B, trans=trans)
    X0 = X.cpu().numpy()
    rc, en, ec, st = _gerfsx(ctx, dA, W, ipiv, B, X, trans, ithresh)
    Xm, en_m, ec_m, cols = G.gerfsx_model(Aop, solve, B_np, X0, ithresh)
    e_norm, e_comp = G.errors(X.cpu().numpy(), Xh, Xl)
    print(trans, ithresh, "norm/eps", e_norm / EPS, "comp/eps", e_comp / EPS, "model comp/eps", G.errors(Xm, Xh, Xl)[1] / EPS, "corrections", [s.iterations for s in st], "model",
          [c.corrections for c in cols], "states", [(s.x_state, s.z_state) for s in st], "model", [(c.x_state, c.z_state) for c in cols])
    assert rc == 0 and all(s.x_state == G.X_CONV for s in st)
    assert np.all(e_norm <= 4 * EPS) and np.all(e_norm <= en)
    assert np.all(G.errors(Xm, Xh, Xl)[0] <= 4 * EPS)
    for s, c in zip(st, cols):
        assert abs(s.iterations - c.corrections) <= 1 and (s.x_state, s.z_state) == (c.x_state, c.z_state)


@pytest.mark.parametrize("trans", [0, 1])
def test_stops_without_convergence(ctx, trans):
    """ill(257, 1e10) on fp16 factors: the corrections do not contract.  Return value 1, NOPROG, X finite, and err_norm is not below
    the true error."""
    n, m = 257, 3
    A = G.ill(n, 1e10, 3)
    Aop = np.ascontiguousarray(A.T if trans else A)
    B_np = np.random.default_rng(5).uniform(-1, 1, (n, m))
    Minv = np.linalg.inv(Aop)
    Xh, Xl = G.reference_pair(Aop, B_np, lambda V: Minv @ V)
    dA, W, ipiv, _ = H.factor(ctx, A, trailing=1)
    B, _ = H.dev(ctx, B_np)
    X = ctx.getrs(W, ipiv, B, trans=trans)
    rc, en, ec, st = _gerfsx(ctx, dA, W, ipiv, B, X, trans)
    X_np = X.cpu().numpy()
    e_norm = np.abs((X_np - Xh) - Xl).max(axis=0) / np.abs(X_np).max(axis=0)     # relative to the returned x, as the bound is
    print(trans, "error", e_norm, "err_norm", en, "states", [(s.x_state, s.z_state, s.iterations) for s in st])
    assert rc == 1 and all(s.x_state == G.X_NOPROG for s in st)
    assert np.isfinite(X_np).all() and np.all(en >= e_norm)


# ---- edges ----------------------------------------------------------------------------------------------------------------------
def test_edges(ctx):
    """A zero right-hand side (x = 0: converged at once, both bounds at the floor); a NaN in B stops that column only (x_state 3,
    +Inf bounds) and leaves its neighbours' bits alone; N = 1."""
    n, m = 65, 35
    A = G.rand(n, 2)
    dA, W, ipiv, _ = H.factor(ctx, A, nb=32)
    B_np = np.random.default_rng(6).uniform(-1, 1, (n, m))
    B_np[:, 4] = 0.0
    for trans in (0, 1):
        B, _ = H.dev(ctx, B_np)
        X0 = ctx.getrs(W, ipiv, B, trans=trans)
        X, en, ec, st = ctx.gerfsx(dA, W, ipiv, B, X0, trans=trans)
        X_np = X.cpu().numpy()
        lbnd = 10 * EPS
        assert not X_np[:, 4].any() and (st[4].x_state, st[4].z_state, st[4].iterations) == (G.X_CONV, G.Z_CONV, 0)
        assert st[4].final_dx_x == 0.0 and en[4] == lbnd and ec[4] == lbnd
        Bn_np = B_np.copy()
        Bn_np[7, 33] = np.nan
        Bn, _ = H.dev(ctx, Bn_np)
        Xn0 = X0.clone()
        Xn0[:, 33] = ctx.getrs(W, ipiv, Bn[:, 33:34].contiguous(), trans=trans)[:, 0]
        rc, enn, ecn, stn = _gerfsx(ctx, dA, W, ipiv, Bn, Xn0, trans)
        assert rc == 1 and stn[33].x_state == G.X_NAN and enn[33] == np.inf and ecn[33] == np.inf
        Xn_np = Xn0.cpu().numpy()
        for j in range(m):
            if j != 33:
                assert _key(Xn_np, enn, ecn, stn, j) == _key(X_np, en, ec, st, j), j
    A1 = np.array([[0.75]])
    dA1, W1, ipiv1, _ = H.factor(ctx, A1, nb=32)
    b1, _ = H.dev(ctx, np.array([[1.0, -3.0, 1e-5]]))
    for trans in (0, 1):
        X, en, ec, st = ctx.gerfsx(dA1, W1, ipiv1, b1, ctx.getrs(W1, ipiv1, b1, trans=trans), trans=trans)
        want = np.array([[1.0, -3.0, 1e-5]]) / 0.75           # (a correction at 2^-53 or below is not applied: x may stay one ulp off)
        assert np.all(np.abs(X.cpu().numpy() - want) <= 4 * EPS * np.abs(want))
        assert all(s.x_state == G.X_CONV and s.z_state == G.Z_CONV for s in st) and np.all(en == 10 * EPS) and np.all(ec == 10 * EPS)
        r = ctx.residual_x(dA1, X, b1, trans=trans).cpu().numpy()
        assert np.array_equal(r, G.exact_residual(A1, X.cpu().numpy(), np.array([[1.0, -3.0, 1e-5]])))


def test_arguments(ctx, mpf):
    """nrhs = 0 -> 0 and nothing written; bad trans, N <= 0, a leading dimension < N, a null pointer -> -1 with the error set."""
    import torch
    n, ld = 64, 80
    A = G.rand(n, 9)
    dA, W, ipiv, _ = H.factor(ctx, A)
    B, Bbuf = H.dev(ctx, np.ones((n, 2)), ld)
    X, Xbuf = H.dev(ctx, np.linalg.solve(A, np.ones((n, 2))), ld)
    R, Rbuf = H.dev(ctx, np.full((n, 2), FILL), ld)
    L, h = ctx.L, ctx.h
    p = lambda t: C.c_void_p(t.data_ptr())
    null = C.c_void_p(0)
    ctx._bind()
    st = (mpf.MpfGerfsxStats * 2)()
    en, ec = (C.c_double * 2)(), (C.c_double * 2)()
    good = [0, p(dA), n, p(W), n, p(ipiv), n, 2, p(B), ld, p(X), ld, 0, en, ec, st]
    assert L.mpf_gerfsx(h, *good) == 0
    assert en[0] == 10 * EPS and st[0].x_state == G.X_CONV and st[0].ms_total > 0
    a = list(good)
    a[13], a[14], a[15] = en, ec, None                    # stats are optional
    assert L.mpf_gerfsx(h, *a) == 0
    assert bool((Xbuf[n:] == FILL).all()) and bool((Bbuf[n:] == FILL).all()), "padding rows were written"
    a = list(good)
    a[7] = 0
    before = X.clone()
    assert L.mpf_gerfsx(h, *a) == 0 and torch.equal(X, before)
    bad = {0: 2, 6: 0, 2: n - 1, 4: n - 1, 9: n - 1, 11: n - 1, 1: null, 3: null, 5: null, 8: null, 10: null, 13: None, 14: None}
    for pos, val in list(bad.items()) + [(6, -3), (0, -1), (7, -1)]:
        a = list(good)
        a[pos] = val
        assert L.mpf_gerfsx(h, *a) == -1, (pos, val)
        assert "gerfsx" in L.mpf_last_error(h).decode(), (pos, val)
    wrong = ipiv.clone()
    wrong[5] = n + 7
    a = list(good)
    a[5] = p(wrong)
    assert L.mpf_gerfsx(h, *a) == -1 and "ipiv" in L.mpf_last_error(h).decode()
    good = [0, p(dA), n, n, 2, p(X), ld, p(B), ld, p(R), ld]
    assert L.mpf_residual_x(h, *good) == 0 and bool((Rbuf[n:] == FILL).all()) and not bool((R == FILL).any())
    a = list(good)
    a[4] = 0
    R.fill_(FILL)
    assert L.mpf_residual_x(h, *a) == 0 and bool((R == FILL).all())
    for pos, val in [(0, 2), (0, -1), (3, 0), (4, -1), (2, n - 1), (6, n - 1), (8, n - 1), (10, n - 1), (1, null), (5, null), (7, null), (9, null)]:
        a = list(good)
        a[pos] = val
        assert L.mpf_residual_x(h, *a) == -1, (pos, val)
        assert "residual_x" in L.mpf_last_error(h).decode(), (pos, val)
    torch.cuda.synchronize()
