"""Exact-arithmetic GPU tests of the large-matrix solve layer: mpf_getrs, mpf_solve_ir / _nrhs / _trans, mpf_solve_ir_block and
mpf_solve_ir_dist on crafted factors (tests/exact_solve_model.py) on which every evaluation order is exact, compared with the int64
closed form by np.array_equal -- no tolerance, no factorization, every element.  tests/test_exact_solve_cpu.py shows on the host that
the data is order-independent and that the closed form changes when one term next to a kernel seam is dropped, so a mismatch here
is a kernel or driver bug.  The one toleranced figure is history[0], a quotient of two norms, within its derived (n + 4) 2^-53.

What each test reaches:
  test_getrs_exact           blk_load / blk_store (gather, scatter), blk_gemm_kernel in its four triangular roles, the 64 x 64 and
                             256 x 256 inverses (trsv_invert_blocks_kernel, trsv_inv256_level_kernel), the 32-column tiles and the 512-column groups
  test_vector_solve_exact    trsv_step_kernel<UPPER> (near / diag roles), trsv_t_step_kernel, gather_rows / scatter_rows, and at max_iter = 0
                             residual_kernel / residual_reduce_kernel and col_part_kernel / part_finish_kernel on an exactly zero residual
  test_refinement_exact      the same plus blk_gemm_kernel as the residual GEMM, blk_res_reduce_kernel, blk_masked_axpy_kernel, the
                             512-column chunks (N = 513, 1025) and the 4096-wide chunks (N = 4160) of the residuals
  test_dist_solve_exact      the 64-block trsv_lower / upper_step_kernel and launch_residual_rect (their only user)
"""
import numpy as np
import pytest

import blk_helpers as H
import exact_solve_model as M

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 300, 513, 777, 1100]
NRHS = (1, 31, 32, 33, 65)       # the 32-column tile seam; 513 (the 512-column group seam) at N = 64 and 257 only
PAD = 7.5


def _lds(n):
    """(ldlu, ldb): padded at N = 777, packed elsewhere."""
    return (800, 803) if n == 777 else (n, n)


def _factors(ctx, LU, ipiv, ldlu):
    import torch
    W, _ = H.dev(ctx, np.array(LU), ldlu, fill=PAD)           # (a copy: the family's LU is read-only)
    return W, torch.from_numpy(ipiv.copy()).to(ctx.device)


def _vec(ctx, v):
    import torch
    return torch.from_numpy(np.ascontiguousarray(v)).to(ctx.device)


def _getrs_both_ways(ctx, W, dip, B_np, X_np, trans, ldb):
    """getrs in place (rows beyond N of B untouched) and into a new X (B untouched altogether): both equal the closed form."""
    import torch
    n = B_np.shape[0]
    B, buf = H.dev(ctx, B_np, ldb, fill=PAD)
    X = ctx.getrs(W, dip, B, trans=trans, overwrite=True)
    ctx.synchronize()
    assert X.data_ptr() == B.data_ptr()
    assert np.array_equal(X.cpu().numpy(), X_np), _first_wrong(X.cpu().numpy(), X_np)
    assert bool((buf[n:] == PAD).all()), "padding rows of B were written"
    B, buf = H.dev(ctx, B_np, ldb, fill=PAD)
    before = buf.clone()
    X = ctx.getrs(W, dip, B, trans=trans)
    ctx.synchronize()
    assert X.data_ptr() != B.data_ptr() and torch.equal(buf, before), "B (or its padding rows) was written"
    assert np.array_equal(X.cpu().numpy(), X_np), _first_wrong(X.cpu().numpy(), X_np)


def _first_wrong(got, want):
    """(count, first wrong (row, column), got, want) for the assertion message: the position names the seam."""
    bad = np.argwhere(np.atleast_2d(got.T).T != np.atleast_2d(want.T).T)
    if not len(bad):
        return None
    i, j = bad[np.lexsort((bad[:, 0], bad[:, 1]))][0]
    return len(bad), (int(i), int(j)), float(np.atleast_2d(got.T).T[i, j]), float(np.atleast_2d(want.T).T[i, j])


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("trans", [0, 1])
def test_getrs_exact(ctx, n, seed, trans):
    """mpf_getrs equals the closed form for 1, 31, 32, 33, 65 (and at N = 64, 257: 513) right-hand sides; N = 777 with ldlu = 800 and
    ldb = 803; the padding rows of B are untouched with overwrite and without."""
    LU, ipiv, p = M.family(n, seed)
    ldlu, ldb = _lds(n)
    W, dip = _factors(ctx, LU, ipiv, ldlu)
    counts = NRHS + ((513,) if n in (64, 257) else ())
    B, X, Xt = M.rhs(p, max(counts), seed)
    want = Xt if trans else X
    for nrhs in counts:
        _getrs_both_ways(ctx, W, dip, np.ascontiguousarray(B[:, :nrhs]), want[:, :nrhs], trans, ldb)


def _check_zero_iter(st, what):
    assert st.iterations == 0 and st.converged == 1 and st.history[0] == 0.0 and st.rel_residual == 0.0, (what, st.iterations, st.history[0])


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("trans", [0, 1])
def test_vector_solve_exact(ctx, n, seed, trans):
    """The single-vector path at max_iter = 0, 1 and 3 right-hand sides: mpf_solve_ir and mpf_solve_ir_nrhs (trans = 0),
    mpf_solve_ir_trans (trans = 1) equal the closed form; no bounded wait gave up (the call returns 0: the wrapper raises on -4);
    and against A = P^T L U itself the residual of that exact solution is exactly zero, so history[0] == 0."""
    LU, ipiv, p = M.family(n, seed)
    W, dip = _factors(ctx, LU, ipiv, _lds(n)[0])
    A = M.matrix(p)
    B, X, Xt = M.rhs(p, 3, seed)
    want = Xt if trans else X
    M.assert_residual_exact(A.T if trans else A, want, B)
    dA = ctx.from_numpy_f(A)
    dB, _ = H.dev(ctx, B, _lds(n)[1], fill=PAD)
    b0 = _vec(ctx, B[:, 0])
    if trans:
        x, st = ctx.solve_ir_trans(dA, W, dip, b0, max_iter=0)
        Xd, sts = ctx.solve_ir_trans(dA, W, dip, dB, max_iter=0)
    else:
        x, st = ctx.solve_ir(dA, W, dip, b0, max_iter=0)
        Xd, sts = ctx.solve_ir_nrhs(dA, W, dip, dB, max_iter=0)
    assert np.array_equal(x.cpu().numpy(), want[:, 0]), _first_wrong(x.cpu().numpy(), want[:, 0])
    assert np.array_equal(Xd.cpu().numpy(), want), _first_wrong(Xd.cpu().numpy(), want)
    _check_zero_iter(st, "vector")
    for j, s in enumerate(sts):
        _check_zero_iter(s, j)


def _check_refined(q, x, st, j, what):
    """One exact refinement step: x == c - E c, one iteration, converged, history[1] == 0, history[0] within its derived margin."""
    x = x.cpu().numpy()
    assert np.array_equal(x, q.X1[:, j]), (what, j, _first_wrong(x, q.X1[:, j]))
    assert st.iterations == 1 and st.converged == 1 and st.history[1] == 0.0 and st.rel_residual == 0.0, \
        (what, j, st.iterations, st.converged, list(st.history[:4]))
    print(what, j, "history[0] =", repr(st.history[0]), "exact =", repr(float(np.sqrt(q.rr[j] / q.bb[j]))))
    assert M.history0_ok(st.history[0], q.rr[j], q.bb[j], q.n), (what, j, st.history[0], float(np.sqrt(q.rr[j] / q.bb[j])))


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("n,composite", [(65, True), (513, True), (1025, True), (4160, False)])
@pytest.mark.parametrize("trans", [0, 1])
def test_refinement_exact(ctx, n, composite, seed, trans):
    """max_iter = 3, tol = 1e-12 on op(A) = op(M)(I + E), b = op(M) c: through mpf_solve_ir / _nrhs (trans = 0), mpf_solve_ir_trans
    (trans = 1) and mpf_solve_ir_block, x == c - E c, iterations == 1, converged, history[1] == 0.0, and history[0] equals
    ||M E c|| / ||b|| from the integers within (n + 4) 2^-53.  N = 513 and 1025 cross the 512-column chunks of the residuals, N = 4160
    (lda = 4163, L = I, U = D) is the smallest size past their 4096-wide chunks.  x1 - c = -E c is the solve of the first residual:
    a residual kernel that mis-sums one chunk changes x1."""
    q = M.refine_case(n, seed, trans, composite=composite)
    W, dip = _factors(ctx, q.LU, q.ipiv, n)
    dA, _ = H.dev(ctx, q.A, 4163 if n == 4160 else n, fill=PAD)
    dB = ctx.from_numpy_f(q.B)
    b0 = _vec(ctx, q.B[:, 0])
    kw = dict(max_iter=3, tol=1e-12)
    if trans:
        x, st = ctx.solve_ir_trans(dA, W, dip, b0, **kw)
        Xd, sts = ctx.solve_ir_trans(dA, W, dip, dB, **kw)
    else:
        x, st = ctx.solve_ir(dA, W, dip, b0, **kw)
        Xd, sts = ctx.solve_ir_nrhs(dA, W, dip, dB, **kw)
    Xb, stb = ctx.solve_ir_block(dA, W, dip, dB, trans=trans, **kw)
    _check_refined(q, x, st, 0, "vector")
    for j in range(q.C.shape[1]):
        _check_refined(q, Xd[:, j], sts[j], j, "columns")
        _check_refined(q, Xb[:, j], stb[j], j, "block")


@pytest.mark.parametrize("nb", [64, 128, 256])
@pytest.mark.parametrize("n", [65, 300, 777])
def test_dist_solve_exact(ctx, mpf, n, nb):
    """mpf_solve_ir_dist on one rank (the only user of the 64-block step kernels and of launch_residual_rect): at max_iter = 0 the
    closed form and an exactly zero residual, and the exact refinement step; two seeds each."""
    one = mpf.MpfDist(rank=0, world=1)
    for seed in (0, 1):
        LU, ipiv, p = M.family(n, seed)
        W, dip = _factors(ctx, LU, ipiv, n)
        A = M.matrix(p)
        B, X, _ = M.rhs(p, 1, seed)
        M.assert_residual_exact(A, X, B)
        x, st = ctx.solve_ir_dist(ctx.from_numpy_f(A), W, dip, _vec(ctx, B[:, 0]), n, nb, one, max_iter=0)
        assert np.array_equal(x.cpu().numpy(), X[:, 0]), (seed, _first_wrong(x.cpu().numpy(), X[:, 0]))
        _check_zero_iter(st, seed)
        q = M.refine_case(n, seed, 0)
        x, st = ctx.solve_ir_dist(ctx.from_numpy_f(q.A), W, dip, _vec(ctx, q.B[:, 0]), n, nb, one, max_iter=3, tol=1e-12)
        _check_refined(q, x, st, 0, "dist seed %d" % seed)


@pytest.mark.parametrize("n", [65, 300, 777])
def test_dist_solve_refuses_nb_96(ctx, mpf, n):
    """The distributed solve walks 64-row steps from every panel start: nb = 96 is refused with the documented error as soon as a
    second panel exists (N = 300, 777).  At N = 65 the one panel starts at row 0, nothing is misaligned, and the answer is exact."""
    one = mpf.MpfDist(rank=0, world=1)
    LU, ipiv, p = M.family(n, 0)
    W, dip = _factors(ctx, LU, ipiv, n)
    A = M.matrix(p)
    B, X, _ = M.rhs(p, 1, 0)
    if n > 96:
        with pytest.raises(mpf.MPFError, match="multiple of 64"):
            ctx.solve_ir_dist(ctx.from_numpy_f(A), W, dip, _vec(ctx, B[:, 0]), n, 96, one, max_iter=0)
    else:
        x, st = ctx.solve_ir_dist(ctx.from_numpy_f(A), W, dip, _vec(ctx, B[:, 0]), n, 96, one, max_iter=0)
        assert np.array_equal(x.cpu().numpy(), X[:, 0])
        _check_zero_iter(st, n)


def test_interleaved_factor_sets_stay_exact(ctx):
    """getrs on two exact factor sets of different N in turn on the shared context: the grow-only inverse buffers (sized for the
    larger N, offsets by the current one) and the step counters are reused, and both answers stay exact, plain and transposed."""
    sets = []
    for n, seed in ((777, 0), (300, 1)):
        LU, ipiv, p = M.family(n, seed)
        W, dip = _factors(ctx, LU, ipiv, _lds(n)[0])
        sets.append((n, W, dip, M.rhs(p, 33, seed)))
    for turn in range(2):
        for n, W, dip, (B, X, Xt) in sets + sets[::-1]:
            for trans, want in ((turn, Xt if turn else X), (1 - turn, X if turn else Xt)):
                dB, buf = H.dev(ctx, B, _lds(n)[1], fill=PAD)
                got = ctx.getrs(W, dip, dB, trans=trans, overwrite=True).cpu().numpy()
                assert np.array_equal(got, want), (n, trans, turn, _first_wrong(got, want))
                assert bool((buf[n:] == PAD).all())
