"""GPU tests of the expert driver (include/mpf_c.h: mpf_solve_ir_trans, mpf_lange, mpf_geequ, mpf_gecon, mpf_gesvx)."""
import numpy as np
import pytest

import blk_helpers as H
import lacn2_model as M

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1000, 2085, 4096])
def test_solve_trans_sizes(ctx, n):
    """A^T x = b with fp64 factors: one solve within c kappa eps of numpy, refinement to 1e-12."""
    import torch
    A = H.rand(n, 100 + n)
    dA, W, ipiv, info = H.factor(ctx, A)
    assert info == 0
    b_np = np.random.default_rng(n).uniform(-1, 1, n)
    b = torch.from_numpy(b_np).to(ctx.device)
    x_ref = np.linalg.solve(A.T, b_np)
    kappa = np.linalg.norm(A, 1) * np.linalg.norm(np.linalg.inv(A), 1)
    x0, st0 = ctx.solve_ir_trans(dA, W, ipiv, b, max_iter=0)
    err = np.abs(x0.cpu().numpy() - x_ref).max() / np.abs(x_ref).max()
    assert err <= 10 * n * kappa * EPS, (err, kappa)
    x, st = ctx.solve_ir_trans(dA, W, ipiv, b, max_iter=10, tol=1e-12)
    assert st.converged == 1 and st.rel_residual <= 1e-12, list(st.history)[:st.iterations + 1]
    xh = x.cpu().numpy()
    assert np.linalg.norm(b_np - A.T @ xh) <= 1e-11 * np.linalg.norm(b_np)


def test_solve_trans_lda_nrhs_repeatable(ctx):
    """lda > N with the padding untouched, three right-hand sides, and two calls with the same bits."""
    import torch
    n, lda, nrhs = 777, 800, 3
    A = H.rand(n, 7, dominant=3.0)
    buf = ctx.colmajor(lda, n)
    buf.fill_(7.5)
    dA = buf[:n, :]
    dA.copy_(ctx.from_numpy_f(A))
    W = ctx.from_numpy_f(A)
    ipiv, info = ctx.factor(W, 128)
    B_np = np.asfortranarray(np.random.default_rng(1).uniform(-1, 1, (n, nrhs)))
    B = ctx.from_numpy_f(B_np)
    X1, st1 = ctx.solve_ir_trans(dA, W, ipiv, B, max_iter=5, tol=1e-13)
    X2, st2 = ctx.solve_ir_trans(dA, W, ipiv, B, max_iter=5, tol=1e-13)
    ctx.synchronize()
    assert torch.equal(X1, X2)
    assert bool((buf[n:, :] == 7.5).all())
    Xh = ctx.to_numpy_f(X1)
    for j in range(nrhs):
        assert st1[j].converged == 1
        assert np.linalg.norm(B_np[:, j] - A.T @ Xh[:, j]) <= 1e-12 * np.linalg.norm(B_np[:, j])


def test_solve_trans_fp16_factors(ctx):
    """fp16-mode factors of a diagonally dominant N = 8192 matrix: A^T x = b to 1e-12 within 3 corrections."""
    import torch
    n = 8192
    g = torch.Generator(device=ctx.device); g.manual_seed(3)
    G = (torch.randint(0, 100, (n, n), generator=g, device=ctx.device, dtype=torch.int32).to(torch.float64) / 10.0).t()
    idx = torch.arange(n, device=ctx.device)
    Ad = G.clone(); Ad[idx, idx] += G.sum(dim=1)
    W = Ad.clone()
    ipiv, info = ctx.factor(W, 256, trailing=1)
    xs = torch.ones(n, dtype=torch.float64, device=ctx.device)
    b = Ad.t() @ xs
    x, st = ctx.solve_ir_trans(Ad, W, ipiv, b, max_iter=3, tol=1e-12)
    assert st.converged == 1 and st.iterations <= 3, list(st.history)[:4]
    assert float((x - xs).abs().max()) < 1e-8


def test_lange(ctx):
    import torch
    rng = np.random.default_rng(2)
    for m, n in ((1, 1), (300, 517), (5000, 70), (70, 5000)):
        A = np.asfortranarray(rng.normal(size=(m, n)) * 10.0 ** rng.uniform(-3, 3, (m, 1)))
        buf = ctx.colmajor(m + 13, n)
        buf.fill_(1e300)
        dA = buf[:m, :]
        dA.copy_(ctx.from_numpy_f(A))
        assert ctx.lange(dA, "M") == np.abs(A).max()
        for norm, want in (("1", np.abs(A).sum(axis=0).max()), ("O", np.abs(A).sum(axis=0).max()),
                           ("I", np.abs(A).sum(axis=1).max()), ("F", np.sqrt(np.sum(A * A)))):
            got = ctx.lange(dA, norm)
            assert abs(got - want) <= 1e-14 * want, (m, n, norm, got, want)
            assert ctx.lange(dA, norm) == got
    with pytest.raises(Exception):
        ctx.lange(torch.zeros((4, 4), dtype=torch.float64, device=ctx.device).t(), "X")


def test_geequ_matches_restatement_and_scaled_copy(ctx, mpf):
    """Powers of two equal to the numpy restatement; the driver's Dr A Dc is bit-exact (its fp64 factors equal those of numpy's
    scaled matrix, bit for bit)."""
    import torch
    n = 512
    rng = np.random.default_rng(4)
    A = np.asfortranarray(rng.uniform(-1, 1, (n, n)) * np.logspace(-20, 20, n)[:, None] * np.logspace(3, -3, n)[None, :])
    dA = ctx.from_numpy_f(A)
    r, c, rowcnd, colcnd, amax, info = ctx.geequ(dA)
    rr, cc, rowcnd0, colcnd0, amax0, info0 = M.geequ(A)
    assert info == info0 == 0
    assert np.array_equal(r.cpu().numpy(), rr) and np.array_equal(c.cpu().numpy(), cc)
    assert rowcnd == rowcnd0 and colcnd == colcnd0 and amax == amax0
    assert np.all(np.frexp(rr)[0] == 0.5) and np.all(np.frexp(cc)[0] == 0.5)
    # equilibrate = 2, fp64: the work matrix holds the factors of Dr A Dc
    S = np.asfortranarray((A * rr[:, None]) * cc[None, :])
    _, W_ref, ip_ref, _ = H.factor(ctx, S, nb=256, check=False)
    b = torch.from_numpy(rng.uniform(-1, 1, n)).to(ctx.device)
    A0 = dA.clone()
    x, st, W, ipiv, r2, c2 = ctx.gesvx(dA, b, nb=256, equilibrate=2, try_fp16=0, want_scales=True)
    ctx.synchronize()
    assert st.equed == 3 and st.path == 2
    assert torch.equal(r2, r) and torch.equal(c2, c)
    assert torch.equal(W, W_ref) and torch.equal(ipiv, ip_ref)
    assert torch.equal(dA, A0)
    # zero row / column: LAPACK's info
    Z = A.copy(); Z[7] = 0
    assert ctx.geequ(ctx.from_numpy_f(Z))[5] == 8
    Z = A.copy(); Z[:, 11] = 0
    assert ctx.geequ(ctx.from_numpy_f(Z))[5] == n + 12


@pytest.mark.parametrize("n", [1, 5, 64, 300, 1024, 2048])
def test_gecon_against_restatement(ctx, n):
    A = H.rand(n, 30 + n, dominant=None)
    if n > 1:
        A[:, 0] *= 1e3
    dA, W, ipiv, info = H.factor(ctx, A, check=False)
    LU = ctx.to_numpy_f(W)
    Lm = np.tril(LU, -1) + np.eye(n)
    Um = np.triu(LU)
    inv = np.linalg.inv(Lm @ Um)
    for norm, o in (("1", 1), ("I", np.inf)):
        anorm = ctx.lange(dA, norm)
        rcond, st = ctx.gecon(W, anorm, norm)
        ref, it = M.gecon_ainvnm(LU, norm)
        assert abs(st.ainvnm - ref) <= 1e-6 * ref, (norm, st.ainvnm, ref)
        true = np.linalg.norm(inv, o)
        assert true / 10 <= st.ainvnm <= true * (1 + 1e-8), (norm, st.ainvnm, true)
        assert rcond > 0 and abs(rcond - (1 / st.ainvnm) / anorm) <= 1e-15 * rcond
        assert st.solves + st.solves_t >= (1 if n == 1 else 3)
        again, st2 = ctx.gecon(W, anorm, norm)
        assert again == rcond and st2.ainvnm == st.ainvnm


def test_gecon_degenerate(ctx):
    n = 100
    A = H.rand(n, 9, dominant=None)
    dA, W, ipiv, info = H.factor(ctx, A, check=False)
    rcond, _ = ctx.gecon(W, 0.0, "1")
    assert rcond == 0.0
    W[3, 3] = 0.0
    rcond, st = ctx.gecon(W, ctx.lange(dA, "1"), "1")
    assert rcond == 0.0 and st.solves == 0
    assert ctx.cond(dA, W) == float("inf")


def test_gesvx_n8192(ctx):
    """The C5-type matrix (rows scaled by logspace(0, 8)) is equilibrated by rows and solved on fp16 factors, where mpf_gesv
    needs the fp64 fallback; the raw generator matrix is sent to fp64 by its rcond; trans = 1 converges; equilibrate = 0 falls
    back; d_A is preserved."""
    import torch
    n, nb = 8192, 256
    g = torch.Generator(device=ctx.device); g.manual_seed(3)
    G = (torch.randint(0, 100, (n, n), generator=g, device=ctx.device, dtype=torch.int32).to(torch.float64) / 10.0).t()
    idx = torch.arange(n, device=ctx.device)
    Ad = G.clone(); Ad[idx, idx] += G.sum(dim=1)
    Ak = (Ad * torch.logspace(0, 8, n, dtype=torch.float64, device=ctx.device)[:, None]).t().contiguous().t()
    Ak0 = Ak.clone()
    xs = torch.ones(n, dtype=torch.float64, device=ctx.device)
    b = Ak @ xs
    work = ctx.colmajor(n, n)
    x, st, _, _ = ctx.gesvx(Ak, b, nb, work=work)
    print("C5 gesvx: path", st.path, "equed", st.equed, "rcond_lowp", st.rcond_lowp, "history", list(st.ir_final.history)[:4],
          f"{st.ms_total:.1f} ms")
    assert st.equed == 1 and st.path == 1 and st.skipped_by_rcond == 0
    assert st.ir_final.converged == 1 and st.ir_final.rel_residual <= 1e-12 and st.ir_final.iterations <= 3
    assert float((x - xs).abs().max()) < 1e-8
    _, gst, _, _ = ctx.gesv(Ak, b, nb, work=work)
    assert gst.path == 2
    # trans = 1 on the same matrix
    bt = Ak.t() @ xs
    x, st, _, _ = ctx.gesvx(Ak, bt, nb, trans=True, work=work)
    assert st.equed == 1 and st.ir_final.converged == 1 and st.ir_final.rel_residual <= 1e-12
    assert float((x - xs).abs().max()) < 1e-6     # A^T = Ad^T D mixes the scales: kappa ~ 1e8 in the forward error
    # no equilibration: the fp16 attempt cannot be used
    x, st, _, _ = ctx.gesvx(Ak, b, nb, equilibrate=0, work=work)
    assert st.path == 2 and st.equed == 0 and st.ir_final.converged == 1
    assert torch.equal(Ak, Ak0)
    # the raw generator matrix: kappa ~ 1e6 > 1e4, so no refinement on the fp16 factors
    x, st, _, _ = ctx.gesvx(G, G @ xs, nb, work=work)
    print("generator gesvx: rcond_lowp", st.rcond_lowp, "rcond", st.rcond)
    assert st.path == 2 and st.skipped_by_rcond == 1 and st.ir_lowp.iterations == 0
    assert st.ir_final.converged == 1 and st.ir_final.rel_residual <= 1e-12
