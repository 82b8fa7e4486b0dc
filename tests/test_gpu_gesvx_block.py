"""GPU tests of the expert driver for many right-hand sides (include/mpf_c.h: mpf_gesvx_block), nb = 128 throughout.

Shapes: N in {1, 33, 300} (one tile row block; fewer rows than a tile is wide; a 256-row pad with N no multiple of 256) and nrhs in
{1, 33, 513} (one column; the 32-column tile seam; the 512-column group seam, at N = 300 only).  B and X of the composition test have
ld = N + 3 with a sentinel in the rows beyond N.

Bounds asserted against extended precision (test 6; tests/test_gpu_gerfs.py justifies the brackets and margins), with op(A)^-1 built
from the exactly equilibrated matrix, nz = N + 1, eps = 2^-53:
    max|x - x_ref| / max|x| <= ferr;  |berr - berr_exact| <= 2 nz eps;  lo / 3 <= ferr <= 1.01 hi (1.1 hi on fp16 factors).
Agreement with mpf_gesvx (test 3): both answers converged, i.e. the device's fp64 residual is <= tol ||b||; recomputed in longdouble it
may exceed that by the fp64 residual's own rounding error, so the assertion is
    ||b - op(A) x||_2 <= tol ||b||_2 + nz eps || |b| + |op(A)| |x| ||_2."""
import ctypes as C

import numpy as np
import pytest

import blk_helpers as H
import gesvx_block_model as GB
import lacn2_model as M

pytestmark = pytest.mark.gpu
EPS = GB.EPS
LD = np.longdouble
NB = 128


def _badly_scaled(n, seed):
    """Rows scaled over 1e-20 .. 1e20 and columns over 1e3 .. 1e-3 (test_gpu_expert.py's equilibration matrix)."""
    rng = np.random.default_rng(seed)
    return np.asfortranarray(rng.uniform(-1, 1, (n, n)) * np.logspace(-20, 20, n)[:, None] * np.logspace(3, -3, n)[None, :])


def _rhs_of(A, trans, X):
    """B = op(A) X.  On a badly row-scaled matrix a B drawn at random has rows where |op(A)| |x| exceeds |b| by the ratio of the row
    scales, the fp64 residual there is eps times that, and the 2-norm stop rule ||r|| <= tol ||b|| cannot be met on ANY factors;
    a B that is a product has |b| of the size of |op(A)| |x| row by row."""
    return np.asfortranarray((A.T if trans else A) @ X)


def _raw(ctx, mpf, dA, n, nrhs, B, ldb, X, ldx, work, ipiv, trans=0, equilibrate=1, try_fp16=1, kappa_max=0.0, max_iter=10, tol=1e-12,
         itmax=0, bounds=True):
    """The C entry point itself: (return value, ferr, berr, stats, ir, rfs)."""
    p = lambda t: C.c_void_p(t.data_ptr())
    ctx._bind()
    k = max(nrhs, 1)
    ferr, berr = np.zeros(k), np.zeros(k)
    dp = C.POINTER(C.c_double)
    st, ir, rfs = mpf.MpfGesvxStats(), (mpf.MpfIrStats * k)(), (mpf.MpfGerfsStats * k)()
    rc = ctx.L.mpf_gesvx_block(ctx.h, p(dA), dA.stride(1) if dA.shape[1] > 1 else n, n, NB, p(work), p(ipiv), nrhs, p(B), ldb, p(X), ldx,
                               trans, equilibrate, try_fp16, kappa_max, max_iter, tol, itmax, None, None,
                               ferr.ctypes.data_as(dp) if bounds else None, berr.ctypes.data_as(dp) if bounds else None, C.byref(st), ir, rfs)
    return rc, ferr[:nrhs], berr[:nrhs], st, list(ir)[:nrhs], list(rfs)[:nrhs]


def _key(X, ferr, berr, ir, rfs, j):
    return (H.bits(X[:, j]).tolist(), H.bits(ferr[j:j + 1])[0], H.bits(berr[j:j + 1])[0], ir[j].iterations, ir[j].converged,
            rfs[j].iterations, rfs[j].lacn2_iterations)


# ---- 1. composition without scaling ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("n,nrhs", [(1, 1), (33, 1), (33, 33), (300, 1), (300, 33), (300, 513)])
def test_composition_is_factor_then_solve_ir_block_then_gerfs(ctx, mpf, n, nrhs, trans):
    """equilibrate = 0, try_fp16 = 0: X, ferr, berr and the per-column counts are the bits of ctx.factor + solve_ir_block + gerfs, d_work
    and ipiv are ctx.factor's; bounds=False returns solve_ir_block's X untouched; the rows beyond N of B and X keep their sentinel."""
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
    X2, ferr_ref, berr_ref, rst = ctx.gerfs(dA, W, ipiv_ref, B, X1, trans=trans)
    X, Xbuf = H.dev(ctx, np.zeros((n, nrhs)), ld)
    work, ipiv = ctx.colmajor(n, n), torch.zeros(n, dtype=torch.int32, device=ctx.device)
    rc, ferr, berr, st, ir, rfs = _raw(ctx, mpf, dA, n, nrhs, B, ld, X, ld, work, ipiv, trans=trans, equilibrate=0, try_fp16=0)
    assert rc == 0 and st.path == 2 and st.equed == 0 and st.skipped_by_rcond == 0
    assert torch.equal(work, W) and torch.equal(ipiv, ipiv_ref)
    assert H.same(X, X2.view(n, nrhs)) and H.same(ferr, ferr_ref) and H.same(berr, berr_ref)
    for j in range(nrhs):
        assert (ir[j].iterations, ir[j].converged, ir[j].stalled) == (ist[j].iterations, ist[j].converged, ist[j].stalled), j
        assert ir[j].rel_residual == ist[j].rel_residual and ir[j].ms_total == ir[0].ms_total, j
        assert (rfs[j].iterations, rfs[j].lacn2_iterations, rfs[j].solves) == (rst[j].iterations, rst[j].lacn2_iterations, rst[j].solves), j
    worst = max(range(nrhs), key=lambda j: ir[j].rel_residual)
    assert st.ir_final.rel_residual == ir[worst].rel_residual and st.ms_ir >= rfs[0].ms_total > 0
    assert bool((Xbuf[n:] == 7.5).all()) and bool((Bbuf[n:] == 7.5).all()), "padding rows were written"
    rc, _, _, st, ir, _ = _raw(ctx, mpf, dA, n, nrhs, B, ld, X, ld, work, ipiv, trans=trans, equilibrate=0, try_fp16=0, bounds=False)
    assert rc == 0 and H.same(X, X1.view(n, nrhs)), "without the bounds stage X is solve_ir_block's"
    Xw, fe, be, _, _, rs, _, _ = ctx.gesvx_block(dA, B[:, 0].contiguous() if nrhs == 1 else B, nb=NB, trans=trans, equilibrate=0, try_fp16=0,
                                                 bounds=False)
    assert fe is None and be is None and rs is None and Xw.dim() == (1 if nrhs == 1 else 2) and H.same(Xw.view(n, nrhs), X1.view(n, nrhs))


# ---- 2. row-scaling invariance: the scaled loads and stores ----------------------------------------------------------------------------
@pytest.mark.parametrize("try_fp16", [0, 1])
@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("n,nrhs", [(33, 33), (300, 33)])
def test_row_scaling_invariance(ctx, n, nrhs, trans, try_fp16):
    """A = Dr^-1 A0 with Dr = 2^k, k in [-20, 20], equilibrate = 2 for both: r(A) = Dr r(A0) exactly, so both calls factor the same bits.
    trans = 0 with B = Dr^-1 B0: factors, ipiv, X, berr, ferr equal bit for bit.  trans = 1 with B unchanged: X == Dr X0 bit for bit and
    berr is equal (ferr is not compared: max|x| moves).
    The refinement's stop rule ||r||_2 / ||b||_2 <= tol is NOT invariant under a row scaling (for trans = 0 the two calls weigh the
    rows differently), so the comparison needs stop decisions that are clear of tol: with the diagonal raised by sqrt(N) (kappa of a
    few) x0 on fp64 factors has a residual of some 1e-16 and fp16 factors gain 3 to 4 digits per step (1e-4, 1e-7, 1e-11, 1e-14), a
    factor 10 or more away from tol = 1e-12 on either side.  The per-column iteration counts are asserted equal first."""
    import torch
    rng = np.random.default_rng(7 * n + trans)
    A0 = H.rand(n, 60 + n, dominant=float(n) ** 0.5)
    k = rng.integers(-20, 21, n)
    A = np.asfortranarray(np.ldexp(A0, -k[:, None]))
    B0 = rng.uniform(-1, 1, (n, nrhs)) * np.logspace(-3, 3, nrhs)
    Bs = B0 if trans else np.ldexp(B0, -k[:, None])
    kw = dict(nb=NB, trans=trans, equilibrate=2, try_fp16=try_fp16, itmax=10, want_scales=True)
    X0, ferr0, berr0, st0, ir0, rfs0, W0, ip0, r0, c0 = ctx.gesvx_block(ctx.from_numpy_f(A0), ctx.from_numpy_f(B0), **kw)
    X, ferr, berr, st, ir, rfs, W, ip, r, c = ctx.gesvx_block(ctx.from_numpy_f(A), ctx.from_numpy_f(Bs), **kw)
    print("path", st0.path, st.path, "equed", st0.equed, st.equed, "ir iterations", [s.iterations for s in ir0], [s.iterations for s in ir],
          "gerfs iterations", [s.iterations for s in rfs0], [s.iterations for s in rfs])
    hist = lambda q: [(min(s.history[i] for s in q if s.iterations >= i), max(s.history[i] for s in q if s.iterations >= i))
                      for i in range(max(s.iterations for s in q) + 1)]
    print("rel_residual (min, max) per step", hist(ir0), hist(ir))
    assert st.equed == 3 and st0.equed == 3 and st.path == st0.path
    assert [s.iterations for s in ir] == [s.iterations for s in ir0], "a stop decision fell on tol: the comparison below needs the same steps"
    assert np.array_equal(r.cpu().numpy(), np.ldexp(r0.cpu().numpy(), k)), "r(A) = Dr r(A0)"
    assert torch.equal(c, c0) and torch.equal(W, W0) and torch.equal(ip, ip0)
    assert st.rcond == st0.rcond and st.rcond_lowp == st0.rcond_lowp and st.anorm == st0.anorm
    assert H.same(berr, berr0)
    if trans:
        assert H.same(X, np.ldexp(X0.cpu().numpy(), k[:, None]))
    else:
        assert H.same(X, X0) and H.same(ferr, ferr0)


# ---- 3. agreement with mpf_gesvx -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("try_fp16", [0, 1])
@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("kind", ["scaled", "dominant"])
def test_same_decisions_and_factors_as_gesvx(ctx, kind, trans, try_fp16):
    import torch
    n, tol = 300, 1e-12
    A = _badly_scaled(n, 4) if kind == "scaled" else H.rand(n, 5, dominant=float(n) ** 0.5)
    b_np = (A.T if trans else A) @ np.random.default_rng(8).uniform(-1, 1, n)     # (see _rhs_of: a b the stop rule can reach)
    dA, b = ctx.from_numpy_f(A), torch.from_numpy(b_np).to(ctx.device)
    x1, s1, W1, ip1 = ctx.gesvx(dA, b, nb=NB, trans=trans, try_fp16=try_fp16, tol=tol)
    x, _, _, s, ir, _, W, ip = ctx.gesvx_block(dA, b, nb=NB, trans=trans, try_fp16=try_fp16, tol=tol, bounds=False)
    assert x.dim() == 1
    print(kind, "path", s.path, "equed", s.equed, "rcond", s.rcond, "rcond_lowp", s.rcond_lowp, "skipped", s.skipped_by_rcond)
    for f in ("equed", "skipped_by_rcond", "rcond_lowp", "anorm", "rowcnd", "colcnd", "amax", "kappa_max"):
        assert getattr(s, f) == getattr(s1, f), f
    assert s.path == s1.path and s.rcond == s1.rcond and s.info == s1.info
    assert torch.equal(W, W1) and torch.equal(ip, ip1)
    assert s1.ir_final.converged == 1 and all(q.converged == 1 for q in ir)
    Aop = (A.T if trans else A).astype(LD)
    for xh in (x1.cpu().numpy(), x.cpu().numpy()):
        res = np.linalg.norm((b_np.astype(LD) - Aop @ xh.astype(LD)).astype(np.float64))
        slack = (n + 1) * EPS * np.linalg.norm(np.abs(b_np) + np.abs(Aop.astype(np.float64)) @ np.abs(xh))
        assert res <= tol * np.linalg.norm(b_np) + slack, (res, tol * np.linalg.norm(b_np), slack)


# ---- 4. column independence ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trans", [0, 1])
def test_column_independence(ctx, trans):
    """N = 300, fp16 factors of a row-scaled matrix: column j of a 33-column call has the same X, ferr, berr and counts alone, at another
    position and in a second call -- within the same path, which is asserted first."""
    import torch
    n, nrhs = 300, 33
    rng = np.random.default_rng(12)
    A = np.asfortranarray(np.ldexp(H.rand(n, 13, dominant=float(n) ** 0.5), rng.integers(-20, 21, n)[:, None]))
    B_np = _rhs_of(A, trans, rng.uniform(-1, 1, (n, nrhs)) * np.logspace(-3, 3, nrhs))
    dA = ctx.from_numpy_f(A)
    kw = dict(nb=NB, trans=trans, try_fp16=1, itmax=10)
    perm = rng.permutation(nrhs)
    run = lambda Bn: ctx.gesvx_block(dA, ctx.from_numpy_f(np.asfortranarray(Bn)), **kw)
    full, again, permd = run(B_np), run(B_np), run(B_np[:, perm])
    print("path", full[3].path, "equed", full[3].equed)
    assert full[3].path == again[3].path == permd[3].path and full[3].equed & 1
    pick = lambda res: (res[0].cpu().numpy(), res[1], res[2], res[4], res[5])
    where = {int(j): i for i, j in enumerate(perm)}
    for j in range(nrhs):
        assert _key(*pick(full), j) == _key(*pick(again), j), j
        assert _key(*pick(full), j) == _key(*pick(permd), where[j]), j
    assert torch.equal(full[6], again[6]) and torch.equal(full[7], again[7])
    for j in (0, 16, 32):
        alone = run(B_np[:, j:j + 1])
        assert alone[3].path == full[3].path
        assert _key(*pick(alone), 0) == _key(*pick(full), j), j


# ---- 5. paths ------------------------------------------------------------------------------------------------------------------------
def test_ill_conditioned_goes_to_fp64_without_refining(ctx, mpf):
    import torch
    n, nrhs = 300, 33
    A = H.ill(n, 1e8, 7)
    B_np = _rhs_of(A, 0, np.random.default_rng(7).uniform(-1, 1, (n, nrhs)))     # (a random B has ||x|| ~ kappa ||b|| / ||A||: no 1e-12)
    dA, (B, _), (X, _) = ctx.from_numpy_f(A), H.dev(ctx, B_np), H.dev(ctx, np.zeros((n, nrhs)))
    work, ipiv = ctx.colmajor(n, n), torch.zeros(n, dtype=torch.int32, device=ctx.device)
    rc, ferr, berr, st, ir, rfs = _raw(ctx, mpf, dA, n, nrhs, B, n, X, n, work, ipiv, try_fp16=1)
    print("rcond_lowp", st.rcond_lowp, "rcond", st.rcond, "ferr max", ferr.max(), "berr/eps", berr.max() / EPS)
    assert st.skipped_by_rcond == 1 and st.path == 2 and rc == 0 and st.ir_lowp.iterations == 0
    assert all(s.converged == 1 for s in ir) and np.all(ferr > 0) and np.all(berr < 1e-12)


@pytest.mark.parametrize("kappa", [3e2, 3e3])
def test_fallback_rule(ctx, mpf, kappa):
    """1 / rcond under kappa_max and max_iter = 1 on fp16 factors.  Only what the rule says: when some column of the low-precision attempt
    did not converge the call is on path 2 (all columns solved again on fp64 factors); on path 1 every column converged."""
    import torch
    n, nrhs = 300, 33
    A = H.ill(n, kappa, 8)
    B_np = np.random.default_rng(9).uniform(-1, 1, (n, nrhs))
    dA, (B, _), (X, _) = ctx.from_numpy_f(A), H.dev(ctx, B_np), H.dev(ctx, np.zeros((n, nrhs)))
    work, ipiv = ctx.colmajor(n, n), torch.zeros(n, dtype=torch.int32, device=ctx.device)
    rc, ferr, berr, st, ir, rfs = _raw(ctx, mpf, dA, n, nrhs, B, n, X, n, work, ipiv, try_fp16=1, kappa_max=1e7, max_iter=1)
    print("kappa", kappa, "1/rcond_lowp", 1 / st.rcond_lowp, "lowp worst", st.ir_lowp.rel_residual, st.ir_lowp.converged, "path", st.path, "rc", rc)
    assert st.skipped_by_rcond == 0 and 1 / st.rcond_lowp <= 1e7
    assert st.ir_lowp.rel_residual > 0, "the low-precision attempt ran"
    if st.ir_lowp.converged == 0:
        assert st.path == 2
    if st.path == 1:
        assert all(s.converged == 1 for s in ir) and rc == 0
    assert rc == (0 if all(s.converged == 1 for s in ir) else 1)
    assert st.ir_final.rel_residual == max(s.rel_residual for s in ir)


# ---- 6. quality against extended precision -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("try_fp16", [0, 1])
@pytest.mark.parametrize("trans", [0, 1])
def test_bounds_of_the_original_system(ctx, trans, try_fp16):
    n, nrhs = 300, 33
    A = _badly_scaled(n, 4)
    B_np = _rhs_of(A, trans, np.random.default_rng(10).uniform(-1, 1, (n, nrhs)) * np.logspace(-3, 3, nrhs))
    X, ferr, berr, st, ir, rfs, _, _ = ctx.gesvx_block(ctx.from_numpy_f(A), ctx.from_numpy_f(B_np), nb=NB, trans=trans, try_fp16=try_fp16, itmax=10)
    X = X.cpu().numpy()
    # op(A)^-1 from the exactly equilibrated matrix: A = Dr^-1 S Dc^-1 with powers of two
    r, c, _, _, _, info = M.geequ(A)
    S = (A * r[:, None]) * c[None, :]
    Sinv = np.linalg.inv(S)
    inv = c[:, None] * Sinv * r[None, :]
    Aop, inv = (np.ascontiguousarray(A.T), np.ascontiguousarray(inv.T)) if trans else (A, inv)
    berr_exact, err, lo, hi = GB.exact_quantities(Aop, inv, B_np, X, inv @ B_np)
    margin = 1.1 if st.path == 1 else 1.01
    print("path", st.path, "equed", st.equed, "berr/eps", berr.max() / EPS, "|berr - exact| / (nz eps)", (np.abs(berr - berr_exact) / ((n + 1) * EPS)).max(),
          "err/ferr", (err / ferr).max(), "ferr/lo", (ferr / lo).min(), "ferr/hi", (ferr / hi).max(), "iterations", [s.iterations for s in rfs])
    assert st.equed == 3 and all(s.converged == 1 for s in ir)
    assert np.all(err <= ferr), (err, ferr)
    assert np.all(np.abs(berr - berr_exact) <= 2 * (n + 1) * EPS), (berr, berr_exact)
    assert np.all(lo / 3 <= ferr) and np.all(ferr <= margin * hi), (lo, ferr, hi)


# ---- 7. arguments ----------------------------------------------------------------------------------------------------------------------
def test_arguments(ctx, mpf):
    """nrhs = 0 -> 0 with d_work untouched; bad trans, equilibrate, try_fp16 or a leading dimension < N -> -1 with the error set; ferr
    without berr -> -1; a null pointer -> -1."""
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
    fe, be = (C.c_double * 2)(), (C.c_double * 2)()
    st, ir, rfs = mpf.MpfGesvxStats(), (mpf.MpfIrStats * 2)(), (mpf.MpfGerfsStats * 2)()
    good = [p(dA), n, n, NB, p(work), p(ipiv), 2, p(B), ld, p(X), ld, 0, 1, 1, 0.0, 10, 1e-12, 0, None, None, fe, be, C.byref(st), ir, rfs]
    a = list(good)
    a[6] = 0
    assert L.mpf_gesvx_block(h, *a) == 0
    torch.cuda.synchronize()
    assert bool((work == 3.25).all()), "nrhs = 0 does no work"
    null = C.c_void_p(0)
    bad = [(11, 2), (11, -1), (12, 3), (12, -1), (13, 3), (13, -1), (1, n - 1), (8, n - 1), (10, n - 1), (2, 0), (6, -1),
           (20, None), (21, None), (0, null), (4, null), (5, null), (7, null), (9, null)]
    for pos, val in bad:
        a = list(good)
        a[pos] = val
        assert L.mpf_gesvx_block(h, *a) == -1, (pos, val)
        assert "gesvx_block" in L.mpf_last_error(h).decode(), (pos, val)
    assert bool((work == 3.25).all())
    assert L.mpf_gesvx_block(h, *good) == 0
    assert st.path in (1, 2) and 0 < fe[0] < 1e-10 and 0 <= be[0] < 1e-12
    assert bool((Xbuf[n:] == 7.5).all()) and bool((Bbuf[n:] == 7.5).all()), "padding rows were written"
    assert np.abs(X.cpu().numpy() - np.linalg.solve(A, np.ones((n, 2)))).max() < 1e-12
    torch.cuda.synchronize()
