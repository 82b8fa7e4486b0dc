"""GPU tests of the extra-precise expert solve (include/mpf_c.h: mpf_gerpvgrw, mpf_gerfsx_scaled, mpf_gesvxx_block) against
tests/gesvxx_block_model.py and tests/gerfsx_model.py, nb = 128 throughout, EPS = 2^-53.

Shapes: N in {1, 33, 257, 300} (one row; fewer rows than a tile is wide; one row past the 256-row block; a 256-row pad with N no
multiple of 256), nrhs in {1, 33} (one column; the 32-column tile seam) and 513 once per property that a seam can break (the 512-column
group).

The backward error is compared with the model's (an exactly rounded residual, w and the quotient in longdouble) within
    (N + 2) 2^-53 berr + 8 (N + 1) 2^-106:
w is a sum of N + 1 non-negative terms on fp64 MFMA (gamma_{N+1} in any order), r has the pair residual's error of include/mpf_c.h
(2^-53 |r| + 4 (N + 1) 2^-106 w, the bound tests/test_gpu_gerfsx.py asserts, doubled), the quotient is one more rounding.
Accuracy is judged against a solution kept as an unevaluated pair of doubles (gerfsx_model.reference_pair on exact factors).

Right-hand sides of the scaled systems.  The rule's normwise measure max|d| / max|x| is taken on the caller's x = post .* y (y: the
solution of the equilibrated system, post = Dc, or Dr for A^T).  The blocked solves multiply by inverted 256 x 256 diagonal blocks and
are stable normwise in y, not per component: a correction carries an error of about kappa 2^-53 max|d_y| in EVERY component, and
the component j of x sees it times post_j.  Where x's large components are those with a large post_j -- a solution that follows the
column scaling, which is what a change of units of the unknowns produces -- that error stays kappa 2^-53 of max|d| and the loop
contracts to 2^-53.  Where a solution of uniform size meets column scales spread over 2^60, the same error is up to post_j max|y| /
max|x| ~ 2^60 times larger relative to max|x|, the corrections stop shrinking at some 10 x 2^-53 and the decisions are taken on
rounding noise (measured on the device: NOPROG after 3 .. 4 corrections, errors 3 .. 16 x 2^-53).  A comparison of
states with a host model, or an error at the floor, is defined for the first class only, so _natural_rhs builds B = op(A) (post .* Y)
with Y uniform."""
import ctypes as C
import math

import numpy as np
import pytest

import blk_helpers as H
import gerfsx_model as G
import gesvx_block_model as GB
import gesvxx_block_model as XM

pytestmark = pytest.mark.gpu
EPS = G.EPS
NB = 128
FILL = 7.5


def _floor(n):
    return max(10.0, math.sqrt(n)) * EPS


def _berr_close(berr, model, n):
    return np.all(np.abs(berr - model) <= (n + 2) * EPS * model + 8 * (n + 1) * 2.0 ** -106)


def _xkey(X_np, en, ec, be, st, j):
    s = st[j]
    return (H.bits(X_np[:, j]).tolist(), H.bits(en[j:j + 1])[0], H.bits(ec[j:j + 1])[0], None if be is None else H.bits(be[j:j + 1])[0],
            s.iterations, s.x_state, s.z_state, s.solves, H.bits(np.array([s.final_dx_x, s.final_dz_z, s.dxratmax, s.dzratmax])).tolist())


def _irkey(ir, j):
    s = ir[j]
    return (s.iterations, s.converged, s.stalled, H.bits(np.array([s.rel_residual]))[0])


def _pow2_scaled(n, seed, lo=-30, hi=30, dominant=None):
    """(A = Dk S Dl, S, k, l): the diagonally dominant S with its rows and columns scaled by 2^k_i and 2^l_j, k and l in [lo, hi]."""
    rng = np.random.default_rng(seed)
    S = H.rand(n, seed + 1, dominant=float(n) ** 0.5 if dominant is None else dominant)
    k, l = rng.integers(lo, hi + 1, n), rng.integers(lo, hi + 1, n)
    return np.asfortranarray(np.ldexp(S, k[:, None] + l[None, :])), S, k, l


def _natural_rhs(Aop, post, m, seed):
    """B = op(A) (post .* Y), Y uniform in (-1, 1) times 1e-3 .. 1e3 per column: a solution that follows the column scaling `post`."""
    Y = np.random.default_rng(seed).uniform(-1, 1, (Aop.shape[0], m)) * np.logspace(-3, 3, m)
    return np.asfortranarray(Aop @ (post[:, None] * Y))


def _raw(ctx, mpf, dA, n, nrhs, B, ldb, X, ldx, work, ipiv, trans=0, equilibrate=1, try_fp16=1, kappa_max=0.0, max_iter=10, tol=1e-12,
         ithresh=0, berr=True, rpvgrw=True):
    """The C entry point itself: (return value, err_norm, err_comp, berr, rpvgrw, stats, ir, xr)."""
    p = lambda t: C.c_void_p(t.data_ptr())
    ctx._bind()
    k = max(nrhs, 1)
    en, ec, be = np.zeros(k), np.zeros(k), np.zeros(k)
    dp = C.POINTER(C.c_double)
    pg = C.c_double(-1.0)
    st, ir, xr = mpf.MpfGesvxStats(), (mpf.MpfIrStats * k)(), (mpf.MpfGerfsxStats * k)()
    rc = ctx.L.mpf_gesvxx_block(ctx.h, p(dA), dA.stride(1) if dA.shape[1] > 1 else n, n, NB, p(work), p(ipiv), nrhs, p(B), ldb, p(X), ldx,
                                trans, equilibrate, try_fp16, kappa_max, max_iter, tol, ithresh, None, None,
                                en.ctypes.data_as(dp), ec.ctypes.data_as(dp),
                                be.ctypes.data_as(dp) if berr else None, C.byref(pg) if rpvgrw else None, C.byref(st), ir, xr)
    return rc, en[:nrhs], ec[:nrhs], be[:nrhs], pg.value, st, list(ir)[:nrhs], list(xr)[:nrhs]


# ---- mpf_gerpvgrw ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 33, 257])
def test_rpvgrw_equals_the_formula(ctx, n):
    """A random matrix without a dominant diagonal (the factors grow: the value lies below 1 for N > 1), device factors with a padded
    leading dimension; without scales against the factors of A, with power-of-two scales against those of Dr A Dc (every product is
    exact, so the numpy formula has one value whatever its order)."""
    rng = np.random.default_rng(n)
    A = H.rand(n, 20 + n, dominant=None)
    dA, W, _, _ = H.factor(ctx, A, ld=n + 5, nb=NB)
    got = ctx.gerpvgrw(dA, W)
    want = XM.rpvgrw(A, ctx.to_numpy_f(W))
    print(n, "rpvgrw", got, want)
    assert got == want and 0 < got <= 1 and (n == 1 or got < 1)
    k, l = rng.integers(-20, 21, n), rng.integers(-20, 21, n)
    r, c = np.ldexp(1.0, k), np.ldexp(1.0, l)
    S = np.asfortranarray(np.ldexp(A, k[:, None] + l[None, :]))
    _, Ws, _, _ = H.factor(ctx, S, ld=n + 5, nb=NB)
    LUs = ctx.to_numpy_f(Ws)
    import torch
    dr, dc = torch.from_numpy(r).to(ctx.device), torch.from_numpy(c).to(ctx.device)
    for rr, cc, dr_, dc_ in ((r, c, dr, dc), (r, None, dr, None), (None, c, None, dc)):
        # (one scale alone does not match these factors: the formula is what is compared, not its meaning)
        assert ctx.gerpvgrw(dA, Ws, dr_, dc_) == XM.rpvgrw(A, LUs, rr, cc)
    assert ctx.gerpvgrw(dA, Ws, dr, dc) == XM.rpvgrw(S, LUs), "scaling by powers of two is exact"
    assert ctx.gerpvgrw(dA, Ws, dr, dc) == ctx.gerpvgrw(ctx.from_numpy_f(S), Ws)


def test_rpvgrw_wilkinson_and_nan(ctx):
    """The N = 40 Wilkinson matrix with true partial pivoting (pivot_search = 1: no interchange, U's last column doubles row by row):
    exactly 2^-39.  The identity: 1.  A zero column of U is skipped.  A NaN in A or in U's part: NaN; in L's part: ignored."""
    n = 40
    Wk = np.eye(n) - np.tril(np.ones((n, n)), -1)
    Wk[:, -1] = 1.0
    dA = ctx.from_numpy_f(Wk)
    W = dA.clone()
    ipiv, info = ctx.factor(W, NB, pivot_search=1)
    ctx.synchronize()
    assert info == 0 and np.array_equal(ipiv.cpu().numpy(), np.arange(1, n + 1))
    assert ctx.gerpvgrw(dA, W) == 2.0 ** -39
    I = ctx.from_numpy_f(np.eye(7))
    assert ctx.gerpvgrw(I, I) == 1.0
    A = ctx.from_numpy_f(np.diag([1.0, 1.0, 0.5, 1.0]))
    U = np.diag([1.0, 2.0, 8.0, 64.0])
    assert ctx.gerpvgrw(A, ctx.from_numpy_f(U)) == 1.0 / 64
    U[3, 3] = 0.0
    assert ctx.gerpvgrw(A, ctx.from_numpy_f(U)) == 0.5 / 8
    An = Wk.copy()
    An[17, 5] = np.nan
    assert math.isnan(ctx.gerpvgrw(ctx.from_numpy_f(An), W))
    LU = ctx.to_numpy_f(W)
    Un = LU.copy()
    Un[3, 30] = np.nan
    assert math.isnan(ctx.gerpvgrw(dA, ctx.from_numpy_f(Un)))
    Ln = LU.copy()
    Ln[30, 3] = np.nan
    assert ctx.gerpvgrw(dA, ctx.from_numpy_f(Ln)) == 2.0 ** -39
    L, h = ctx.L, ctx.h
    p = lambda t: C.c_void_p(t.data_ptr())
    out = C.c_double(0)
    for a in ([None, n, p(W), n, n, None, None, C.byref(out)], [p(dA), n, None, n, n, None, None, C.byref(out)],
              [p(dA), n, p(W), n, n, None, None, None], [p(dA), n - 1, p(W), n, n, None, None, C.byref(out)],
              [p(dA), n, p(W), n - 1, n, None, None, C.byref(out)], [p(dA), n, p(W), n, 0, None, None, C.byref(out)]):
        assert L.mpf_gerpvgrw(h, *a) == -1 and "gerpvgrw" in L.mpf_last_error(h).decode()


# ---- mpf_gerfsx_scaled -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fp16_300(ctx):
    """rand(300) on fp16 factors with 33 columns scaled 1e-3 .. 1e3 and getrs's X for both op(A): shared, left unchanged."""
    n, m = 300, 33
    A = G.rand(n, 11)
    B_np = np.random.default_rng(3).uniform(-1, 1, (n, m)) * np.logspace(-3, 3, m)
    dA, W, ipiv, _ = H.factor(ctx, A, nb=NB, trailing=1)
    B, _ = H.dev(ctx, B_np)
    X0 = {t: ctx.getrs(W, ipiv, B, trans=t) for t in (0, 1)}
    return A, B_np, dA, W, ipiv, B, X0


@pytest.mark.parametrize("trans", [0, 1])
def test_gerfsx_scaled_without_scales_is_gerfsx(ctx, fp16_300, trans):
    """NULL scales and NULL berr: mpf_gerfsx's bits in X, both bounds and the stats; asking for berr changes none of them."""
    A, B_np, dA, W, ipiv, B, X0 = fp16_300
    X1, en1, ec1, st1 = ctx.gerfsx(dA, W, ipiv, B, X0[trans], trans=trans)
    X2, en2, ec2, be2, st2 = ctx.gerfsx_scaled(dA, W, ipiv, B, X0[trans], trans=trans, want_berr=False)
    X3, en3, ec3, be3, st3 = ctx.gerfsx_scaled(dA, W, ipiv, B, X0[trans], trans=trans)
    assert be2 is None and all(s.x_state == G.X_CONV for s in st1)
    for j in range(B.shape[1]):
        k1 = _xkey(X1.cpu().numpy(), en1, ec1, None, st1, j)
        assert _xkey(X2.cpu().numpy(), en2, ec2, None, st2, j) == k1, j
        assert _xkey(X3.cpu().numpy(), en3, ec3, None, st3, j) == k1, j


@pytest.mark.parametrize("ithresh", [1, 0])
@pytest.mark.parametrize("trans", [0, 1])
def test_berr_against_the_model(ctx, fp16_300, trans, ithresh):
    """berr of the returned X against the model's, for an X one correction away from getrs's on fp16 factors (ithresh = 1: an error of
    some 1e-7, far above the residual's rounding level (N + 1) 2^-53: the relative part of the bound) and for the converged one (at or
    below that level, where dgerfs too stops refining: the absolute part matters)."""
    A, B_np, dA, W, ipiv, B, X0 = fp16_300
    n = A.shape[0]
    X, en, ec, be, st = ctx.gerfsx_scaled(dA, W, ipiv, B, X0[trans], trans=trans, ithresh=ithresh)
    model = XM.berr_model(np.ascontiguousarray(A.T if trans else A), B_np, X.cpu().numpy())
    print(trans, ithresh, "berr/eps", be.min() / EPS, be.max() / EPS, "largest |berr - model| / bound",
          (np.abs(be - model) / ((n + 2) * EPS * model + 8 * (n + 1) * 2.0 ** -106)).max())
    assert _berr_close(be, model, n)
    assert np.all(be > 0) and (np.all(be <= (n + 1) * EPS) if ithresh == 0 else np.all(be > (n + 1) * EPS))


@pytest.mark.parametrize("trans", [0, 1])
def test_gerfsx_scaled_on_equilibrated_factors(ctx, trans):
    """The suite's badly scaled matrix (rows over 1e-20 .. 1e20, columns over 1e3 .. 1e-3), N = 257: fp64 factors of Dr A Dc with
    mpf_geequ's scales.  Every column converges; states and corrections equal the model driven by the device's factors and the same
    x0, within one correction (another summation order in the solves may decide one step differently, as in tests/test_gpu_gerfsx.py);
    berr against the model."""
    import torch
    n, m = 257, 5
    rng = np.random.default_rng(4)
    A = np.asfortranarray(rng.uniform(-1, 1, (n, n)) * np.logspace(-20, 20, n)[:, None] * np.logspace(3, -3, n)[None, :])
    Aop = np.ascontiguousarray(A.T if trans else A)
    dA = ctx.from_numpy_f(A)
    dr, dc, _, _, _, info = ctx.geequ(dA)
    assert info == 0
    r, c = dr.cpu().numpy(), dc.cpu().numpy()
    B_np = _natural_rhs(Aop, r if trans else c, m, 5)
    S = np.asfortranarray((A * r[:, None]) * c[None, :])
    _, W, ipiv, _ = H.factor(ctx, S, nb=NB)
    fs, fst = H.host_solvers(ctx.to_numpy_f(W), ipiv.cpu().numpy(), trans)
    solve, _ = GB.scaled_solvers(fs, fst, c if trans else r, r if trans else c)
    X0_np = np.asfortranarray(solve(B_np))
    B, _ = H.dev(ctx, B_np)
    X0, _ = H.dev(ctx, X0_np)
    X, en, ec, be, st = ctx.gerfsx_scaled(dA, W, ipiv, B, X0, trans=trans, r=dr, c=dc)
    Xm, en_m, ec_m, cols = G.gerfsx_model(Aop, solve, B_np, X0_np)
    print(trans, "corrections", [s.iterations for s in st], "model", [q.corrections for q in cols], "states", [(s.x_state, s.z_state) for s in st],
          "model", [(q.x_state, q.z_state) for q in cols], "berr/eps", be / EPS)
    assert all(s.x_state == G.X_CONV for s in st) and np.all(en == _floor(n))
    for s, q in zip(st, cols):
        assert abs(s.iterations - q.corrections) <= 1 and (s.x_state, s.z_state) == (q.x_state, q.z_state)
    assert _berr_close(be, XM.berr_model(Aop, B_np, X.cpu().numpy()), n)
    assert torch.equal(X0, torch.from_numpy(X0_np).to(ctx.device)), "overwrite=False changed X"


# ---- the driver: composition ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("n,nrhs", [(1, 1), (33, 33), (257, 1), (300, 33), (300, 513)])
def test_composition_without_scaling(ctx, mpf, n, nrhs, trans):
    """equilibrate = 0, try_fp16 = 0: X, both bounds, berr and the per-column stats are the bits of ctx.factor + solve_ir_block +
    gerfsx_scaled(no scales); d_work and ipiv are ctx.factor's; rpvgrw is mpf_gerpvgrw's of them; the rows beyond N of B and X keep
    their sentinel; without berr and rpvgrw the rest is unchanged."""
    import torch
    A = H.rand(n, 40 + n)
    B_np = np.random.default_rng(nrhs).uniform(-1, 1, (n, nrhs)) * np.logspace(-3, 3, nrhs)
    ld = n + 3
    dA = ctx.from_numpy_f(A)
    W = dA.clone()
    ipiv_ref, info = ctx.factor(W, NB)
    assert info == 0
    B, Bbuf = H.dev(ctx, B_np, ld)
    X1, ist = ctx.solve_ir_block(dA, W, ipiv_ref, B, trans=trans)
    X2, en_ref, ec_ref, be_ref, xst = ctx.gerfsx_scaled(dA, W, ipiv_ref, B, X1, trans=trans)
    X, Xbuf = H.dev(ctx, np.zeros((n, nrhs)), ld)
    work, ipiv = ctx.colmajor(n, n), torch.zeros(n, dtype=torch.int32, device=ctx.device)
    rc, en, ec, be, pg, st, ir, xr = _raw(ctx, mpf, dA, n, nrhs, B, ld, X, ld, work, ipiv, trans=trans, equilibrate=0, try_fp16=0)
    assert rc == 0 and st.path == 2 and st.equed == 0 and st.skipped_by_rcond == 0
    assert torch.equal(work, W) and torch.equal(ipiv, ipiv_ref)
    X_np, X2_np = X.cpu().numpy(), X2.cpu().numpy().reshape(n, nrhs)
    for j in range(nrhs):
        assert _xkey(X_np, en, ec, be, xr, j) == _xkey(X2_np, en_ref, ec_ref, be_ref, xst, j), j
        assert _irkey(ir, j) == _irkey(ist, j) and ir[j].ms_total == ir[0].ms_total and xr[j].ms_total == xr[0].ms_total, j
    worst = max(range(nrhs), key=lambda j: ir[j].rel_residual)
    assert st.ir_final.rel_residual == ir[worst].rel_residual and st.ms_ir >= xr[0].ms_total > 0
    assert pg == ctx.gerpvgrw(dA, W) and 0 < pg <= 1
    assert bool((Xbuf[n:] == FILL).all()) and bool((Bbuf[n:] == FILL).all()), "padding rows were written"
    rc, en2, ec2, _, pg2, _, _, xr2 = _raw(ctx, mpf, dA, n, nrhs, B, ld, X, ld, work, ipiv, trans=trans, equilibrate=0, try_fp16=0,
                                           berr=False, rpvgrw=False)
    assert rc == 0 and pg2 == -1.0, "rpvgrw NULL: nothing is written"
    for j in range(nrhs):
        assert _xkey(X.cpu().numpy(), en2, ec2, None, xr2, j) == _xkey(X2_np, en_ref, ec_ref, None, xst, j), j
    Xw = ctx.gesvxx_block(dA, B[:, 0].contiguous() if nrhs == 1 else B, nb=NB, trans=trans, equilibrate=0, try_fp16=0)[0]
    assert Xw.dim() == (1 if nrhs == 1 else 2) and H.same(Xw.view(n, nrhs), X2_np)


@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("n,nrhs", [(33, 33), (257, 33)])
def test_composition_with_scaling(ctx, n, nrhs, trans):
    """equilibrate = 2, try_fp16 = 0 on a matrix scaled by 2^+-30 per row and column: the driver equals mpf_gesvx_block without its
    bounds stage (stage (a) with the scales: the same code) followed by mpf_gerfsx_scaled with the driver's d_r / d_c on the factors in
    its d_work, bit for bit."""
    import torch
    A, _, k, l = _pow2_scaled(n, 70 + n)
    B_np = _natural_rhs(np.ascontiguousarray(A.T if trans else A), np.ldexp(1.0, -(k if trans else l)), nrhs, n + trans)
    dA, B = ctx.from_numpy_f(A), ctx.from_numpy_f(B_np)
    kw = dict(nb=NB, trans=trans, equilibrate=2, try_fp16=0, want_scales=True)
    X, en, ec, be, pg, st, ir, xr, work, ipiv, r, c = ctx.gesvxx_block(dA, B, **kw)
    Xa, _, _, sta, ira, _, worka, ipiva, ra, ca = ctx.gesvx_block(dA, B, bounds=False, **kw)
    assert st.equed == 3 and sta.equed == 3 and st.path == sta.path == 2
    assert torch.equal(work, worka) and torch.equal(ipiv, ipiva) and torch.equal(r, ra) and torch.equal(c, ca)
    Xb, en_b, ec_b, be_b, xst = ctx.gerfsx_scaled(dA, work, ipiv, B, Xa, trans=trans, r=r, c=c)
    for j in range(nrhs):
        assert _xkey(X.cpu().numpy(), en, ec, be, xr, j) == _xkey(Xb.cpu().numpy(), en_b, ec_b, be_b, xst, j), j
        assert _irkey(ir, j) == _irkey(ira, j), j
    assert all(s.x_state == G.X_CONV for s in xr) and np.all(en == _floor(n))
    assert pg == ctx.gerpvgrw(dA, work, r, c) and 0 < pg <= 1


# ---- the driver: decisions -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,try_fp16,path", [("dominant", 300, 1, 1), ("ill", 257, 1, 2), ("dominant", 300, 0, 2), ("ill", 257, 0, 2)])
def test_same_decisions_and_factors_as_gesvx_block(ctx, kind, n, try_fp16, path):
    """Inputs on which both drivers take the same path: a diagonally dominant matrix (fp16 factors stand), kappa = 1e10 (the rcond gate
    sends both to fp64), and try_fp16 = 0.  Everything that depends on A alone is equal bit for bit, and rpvgrw is mpf_gerpvgrw on
    the driver's own outputs."""
    import torch
    nrhs = 33
    A = H.rand(n, 5, dominant=float(n) ** 0.5) if kind == "dominant" else H.ill(n, 1e10, 3)
    B_np = np.asfortranarray(A @ np.random.default_rng(8).uniform(-1, 1, (n, nrhs)))
    dA, B = ctx.from_numpy_f(A), ctx.from_numpy_f(B_np)
    kw = dict(nb=NB, try_fp16=try_fp16, want_scales=True)
    X, en, ec, be, pg, s, ir, xr, W, ip, r, c = ctx.gesvxx_block(dA, B, **kw)
    _, _, _, s1, ir1, _, W1, ip1, r1, c1 = ctx.gesvx_block(dA, B, bounds=False, **kw)
    print(kind, try_fp16, "path", s.path, s1.path, "equed", s.equed, "rcond", s.rcond, "rcond_lowp", s.rcond_lowp, "skipped", s.skipped_by_rcond,
          "rpvgrw", pg, "plain steps", sorted({q.iterations for q in ir}), "corrections", sorted({q.iterations for q in xr}))
    assert s.path == path and s1.path == path
    for f in ("path", "info", "equed", "skipped_by_rcond", "rcond_lowp", "rcond", "anorm", "rowcnd", "colcnd", "amax", "kappa_max"):
        assert getattr(s, f) == getattr(s1, f), f
    assert torch.equal(W, W1) and torch.equal(ip, ip1)
    assert torch.equal(r, r1) and torch.equal(c, c1), "mpf_geequ's factors, applied or not"
    assert [_irkey(ir, j) for j in range(nrhs)] == [_irkey(ir1, j) for j in range(nrhs)], "stage (a) is mpf_gesvx_block's step 5"
    assert all(q.x_state == G.X_CONV for q in xr)
    assert pg == ctx.gerpvgrw(dA, W, r if s.equed & 1 else None, c if s.equed & 2 else None) and 0 < pg <= 1


# ---- the driver: accuracy ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trans", [0, 1])
def test_accuracy_fp16_factors(ctx, trans):
    """Diagonally dominant N = 300 on fp16 factors: path 1, every column CONV, the true normwise error within err_norm, and err_norm at
    the floor max(10, sqrt(N)) 2^-53 (what the CPU model returns for this class of input: tests/test_gesvxx_block_cpu.py)."""
    n, m = 300, 5
    A = H.rand(n, 5, dominant=float(n) ** 0.5)
    Aop = np.ascontiguousarray(A.T if trans else A)
    B_np = np.random.default_rng(21).uniform(-1, 1, (n, m))
    Minv = np.linalg.inv(Aop)
    Xh, Xl = G.reference_pair(Aop, B_np, lambda V: Minv @ V)
    X, en, ec, be, pg, st, ir, xr, _, _ = ctx.gesvxx_block(ctx.from_numpy_f(A), ctx.from_numpy_f(B_np), nb=NB, trans=trans, try_fp16=1)
    e_norm, _ = G.errors(X.cpu().numpy(), Xh, Xl)
    print(trans, "path", st.path, "norm/eps", e_norm / EPS, "err_norm/eps", en / EPS, "plain steps", [q.iterations for q in ir],
          "corrections", [q.iterations for q in xr], "berr/eps", be / EPS, "rpvgrw", pg)
    assert st.path == 1 and all(q.x_state == G.X_CONV for q in xr)
    assert np.all(e_norm <= en) and np.all(en == _floor(n))
    assert _berr_close(be, XM.berr_model(Aop, B_np, X.cpu().numpy()), n)


@pytest.mark.parametrize("trans", [0, 1])
def test_accuracy_badly_scaled(ctx, trans):
    """N = 257 with rows and columns scaled by 2^+-30, equilibrate = 1: the reference comes from the exactly equilibrated matrix
    (A^-1 = Dl^-1 S^-1 Dk^-1 with powers of two), the solution follows the column scaling (_natural_rhs).  The true normwise error of
    the caller's X is within err_norm, which is at the floor."""
    n, m = 257, 5
    A, S, k, l = _pow2_scaled(n, 31)
    Ainv = np.ldexp(np.linalg.inv(S), -l[:, None] - k[None, :])
    Aop, Minv = (np.ascontiguousarray(A.T), np.ascontiguousarray(Ainv.T)) if trans else (A, Ainv)
    B_np = _natural_rhs(Aop, np.ldexp(1.0, -(k if trans else l)), m, 22)
    Xh, Xl = G.reference_pair(Aop, B_np, lambda V: Minv @ V)
    X, en, ec, be, pg, st, ir, xr, _, _ = ctx.gesvxx_block(ctx.from_numpy_f(A), ctx.from_numpy_f(B_np), nb=NB, trans=trans, equilibrate=1)
    e_norm, _ = G.errors(X.cpu().numpy(), Xh, Xl)
    print(trans, "path", st.path, "equed", st.equed, "norm/eps", e_norm / EPS, "err_norm/eps", en / EPS, "plain steps", [q.iterations for q in ir],
          "corrections", [q.iterations for q in xr], "berr/eps", be / EPS, "rpvgrw", pg)
    assert st.equed == 3 and all(q.x_state == G.X_CONV for q in xr)
    assert np.all(e_norm <= en) and np.all(en == _floor(n))
    assert _berr_close(be, XM.berr_model(Aop, B_np, X.cpu().numpy()), n)


@pytest.fixture(scope="module")
def ill10():
    """ill(257, 1e10) with 5 columns and its pair-of-doubles reference, for both op(A): computed once, left unchanged."""
    n, m = 257, 5
    A = G.ill(n, 1e10, 3)
    B_np = np.random.default_rng(3).uniform(-1, 1, (n, m))
    ref = {}
    for trans in (0, 1):
        Aop = np.ascontiguousarray(A.T if trans else A)
        Minv = np.linalg.inv(Aop)
        ref[trans] = G.reference_pair(Aop, B_np, lambda V: Minv @ V)
    return A, B_np, ref


@pytest.mark.parametrize("trans", [0, 1])
def test_past_the_fp64_residual_floor(ctx, ill10, trans):
    """kappa = 1e10 on fp64 factors: the error is within err_norm, and mpf_gesvx_block's answer to the same system with the same
    arguments is at least 1e6 times further from the exact solution, column by column (README: 3.6e8 x 2^-53 against 1)."""
    A, B_np, ref = ill10
    Xh, Xl = ref[trans]
    dA, B = ctx.from_numpy_f(A), ctx.from_numpy_f(B_np)
    kw = dict(nb=NB, trans=trans, try_fp16=0, tol=1e-14)
    X, en, ec, be, pg, st, ir, xr, _, _ = ctx.gesvxx_block(dA, B, **kw)
    Xp = ctx.gesvx_block(dA, B, bounds=False, **kw)[0]
    e_norm, plain = G.errors(X.cpu().numpy(), Xh, Xl)[0], G.errors(Xp.cpu().numpy(), Xh, Xl)[0]
    print(trans, "norm/eps", e_norm / EPS, "err_norm/eps", en / EPS, "gesvx_block norm/eps", plain / EPS, "plain steps", [q.iterations for q in ir],
          "corrections", [q.iterations for q in xr])
    assert st.path == 2 and all(q.x_state == G.X_CONV for q in xr)
    assert np.all(e_norm <= en)
    assert np.all(plain >= 1e6 * e_norm)


@pytest.mark.parametrize("trans", [0, 1])
def test_fall_back_to_fp64(ctx, ill10, trans):
    """kappa = 1e10 with try_fp16 = 1 and kappa_max = 1e300, so that the gate lets the fp16 factors through: their corrections do not
    contract (NOPROG, README), the attempt does not stand and ALL columns go to fp64 factors: path 2, every column CONV, the error
    within err_norm."""
    A, B_np, ref = ill10
    Xh, Xl = ref[trans]
    X, en, ec, be, pg, st, ir, xr, _, _ = ctx.gesvxx_block(ctx.from_numpy_f(A), ctx.from_numpy_f(B_np), nb=NB, trans=trans, try_fp16=1,
                                                            kappa_max=1e300)
    e_norm = G.errors(X.cpu().numpy(), Xh, Xl)[0]
    print(trans, "path", st.path, "skipped", st.skipped_by_rcond, "1/rcond_lowp", 1 / st.rcond_lowp if st.rcond_lowp else None,
          "lowp worst", st.ir_lowp.rel_residual, "norm/eps", e_norm / EPS, "err_norm/eps", en / EPS)
    assert st.skipped_by_rcond == 0 and st.ir_lowp.rel_residual > 0, "the low-precision attempt ran"
    assert st.path == 2 and all(q.x_state == G.X_CONV for q in xr)
    assert np.all(e_norm <= en)


# ---- the driver: column independence -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trans", [0, 1])
def test_column_independence(ctx, trans):
    """N = 33, fp16 factors of a matrix scaled by powers of two (equed includes rows), 513 columns scaled 1e-3 .. 1e3: column j has the
    same X, bounds, berr and stats (but the times) among 513 (across the 512-column group seam), among 33 at another position, alone
    and in a second call -- within the same path, which is asserted first."""
    n, m = 33, 513
    A, _, _, _ = _pow2_scaled(n, 12, -20, 20)
    rng = np.random.default_rng(13)
    B_np = np.asfortranarray((A.T if trans else A) @ (rng.uniform(-1, 1, (n, m)) * np.logspace(-3, 3, m)))
    dA = ctx.from_numpy_f(A)
    run = lambda Bn: ctx.gesvxx_block(dA, ctx.from_numpy_f(np.asfortranarray(Bn)), nb=NB, trans=trans, try_fp16=1)
    key = lambda res, j: _xkey(res[0].cpu().numpy().reshape(n, -1), res[1], res[2], res[3], res[7], j) + _irkey(res[6], j)
    full, again = run(B_np), run(B_np)
    print("path", full[5].path, "equed", full[5].equed, "rpvgrw", full[4])
    assert full[5].equed & 1 and full[5].path == again[5].path
    keys = [key(full, j) for j in range(m)]
    assert [key(again, j) for j in range(m)] == keys and full[4] == again[4]
    pick = rng.permutation(m)[:33]
    pick[:4] = (512, 0, 31, 32)
    some = run(B_np[:, pick])
    assert some[5].path == full[5].path
    for i, j in enumerate(pick):
        assert key(some, i) == keys[int(j)], j
    for j in (0, 32, 512):
        alone = run(B_np[:, j:j + 1])
        assert alone[5].path == full[5].path and key(alone, 0) == keys[j], j


# ---- arguments -----------------------------------------------------------------------------------------------------------------------------
def test_arguments(ctx, mpf):
    """nrhs = 0 -> 0 with d_work untouched; bad trans, equilibrate, try_fp16 or a leading dimension < N -> -1 with the error set; a null
    pointer, err_norm and err_comp included -> -1; berr, rpvgrw and the stats are optional."""
    import torch
    n, ld = 64, 80
    A = H.rand(n, 9)
    dA = ctx.from_numpy_f(A)
    B, Bbuf = H.dev(ctx, np.ones((n, 2)), ld)
    X, Xbuf = H.dev(ctx, np.zeros((n, 2)), ld)
    work = ctx.colmajor(n, n)
    work.fill_(3.25)
    ipiv = torch.zeros(n, dtype=torch.int32, device=ctx.device)
    L, h = ctx.L, ctx.h
    p = lambda t: C.c_void_p(t.data_ptr())
    ctx._bind()
    en, ec, be = (C.c_double * 2)(), (C.c_double * 2)(), (C.c_double * 2)()
    pg = C.c_double(0)
    st, ir, xr = mpf.MpfGesvxStats(), (mpf.MpfIrStats * 2)(), (mpf.MpfGerfsxStats * 2)()
    good = [p(dA), n, n, NB, p(work), p(ipiv), 2, p(B), ld, p(X), ld, 0, 1, 1, 0.0, 10, 1e-12, 0, None, None, en, ec, be, C.byref(pg),
            C.byref(st), ir, xr]
    a = list(good)
    a[6] = 0
    assert L.mpf_gesvxx_block(h, *a) == 0
    torch.cuda.synchronize()
    assert bool((work == 3.25).all()), "nrhs = 0 does no work"
    null = C.c_void_p(0)
    bad = [(11, 2), (11, -1), (12, 3), (12, -1), (13, 3), (13, -1), (1, n - 1), (8, n - 1), (10, n - 1), (2, 0), (6, -1),
           (20, None), (21, None), (0, null), (4, null), (5, null), (7, null), (9, null)]
    for pos, val in bad:
        a = list(good)
        a[pos] = val
        assert L.mpf_gesvxx_block(h, *a) == -1, (pos, val)
        assert "gesvxx_block" in L.mpf_last_error(h).decode(), (pos, val)
    assert bool((work == 3.25).all())
    assert L.mpf_gesvxx_block(h, *good) == 0
    assert st.path in (1, 2) and en[0] == 10 * EPS and 0 <= be[0] <= (n + 1) * EPS and 0 < pg.value <= 1 and xr[1].x_state == G.X_CONV
    assert bool((Xbuf[n:] == FILL).all()) and bool((Bbuf[n:] == FILL).all()), "padding rows were written"
    want = np.linalg.solve(A, np.ones((n, 2)))
    assert np.abs(X.cpu().numpy() - want).max() <= 4 * EPS * np.abs(want).max() * np.linalg.cond(A, np.inf)
    a = list(good)
    a[22], a[23], a[24], a[25], a[26] = None, None, None, None, None
    before = X.clone()
    assert L.mpf_gesvxx_block(h, *a) == 0 and torch.equal(X, before)
    torch.cuda.synchronize()
