"""GPU tests of tournament pivoting (include/mpf_c.h: mpf_dgetf2_tp, mpf_opts.pivot_search = 2, option pivot_fp64 = 2; csrc/dpivot.hip).

Panel shapes, each the smallest that reaches a seam of the tournament (groups of 256 active rows, merged eight at a time):
1 x 1 and 2 x 2; 33 x 32 (one group); 256 x 32 and 257 x 32 (the second group appears, with one row); 300 x 40 (a tail sub-panel of
8 columns; a second group of 44, then 12 rows); 513 x 300 (more columns than 256, a group of one row); 1000 x 256 (eight sub-panels,
the group count falls from 4 to 3); 2305 x 64 (10 groups -> 2 -> 1: two merge levels, the second merge group of two lists);
4099 x 64 (17 -> 3 -> 1, a last group of three rows); 16390 x 32 (65 -> 9 -> 2 -> 1: three merge levels; kind "normal" only).
Whole factorizations: the N / nb pairs of tests/test_gpu_pivot64.py, each crossing another seam of the loop.

Bit checks need no tolerance.  The model (tests/pivot_tp_model.py) selects unfused whatever `fused` is -- that is the rule -- and for
fused = 1 factors with the oracle's one-FMA update, so info is compared on the arithmetic the device ran."""
import functools

import numpy as np
import pytest

import pivot_tp_model as M

pytestmark = pytest.mark.gpu

SMALL = [(1, 1), (2, 2), (33, 32), (256, 32)]                      # rows <= 256: one group everywhere
SHAPES = SMALL + [(257, 32), (300, 40), (513, 300), (1000, 256), (2305, 64), (4099, 64)]
KINDS = ["normal", "ints", "tiny", "sorted", "last_row", "zero_col"]
CASES = [(r, c, k) for (r, c) in SHAPES for k in KINDS] + [(16390, 32, "normal")]


def _bits(a):
    if hasattr(a, "cpu"):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a).view(np.uint64)


def _panel(rows, cols, kind):
    rng = np.random.default_rng(rows * 1009 + cols * 13 + KINDS.index(kind))
    P = rng.standard_normal((rows, cols))
    if kind == "ints":                    # many exact ties: the smallest position must win, at every level
        P = rng.integers(-3, 4, (rows, cols)).astype(np.float64)
    elif kind == "tiny":                  # far below fp16's range
        P *= 2.0 ** -40
    elif kind == "sorted":                # rows pre-permuted by this model's pivots (rows <= 256: no interchange is left)
        piv, _ = M.panel_tp(np.asfortranarray(P.copy()))
        P = M.permute_rows(np.asfortranarray(P), piv)
    elif kind == "last_row":              # the last row -- the last group's last position -- is the largest of every column
        P[rows - 1, :] = 100.0
        for j in range(min(rows - 1, cols - 1)):
            P[j, j + 1] = 1000.0
    elif kind == "zero_col":
        P[:, cols // 2] = 0.0
    return np.asfortranarray(P)


def _fma_rank1(oracle):
    return lambda Cm, l, u: oracle.dgemm_minus(Cm, l, u)


@functools.lru_cache(maxsize=None)
def _model(rows, cols, kind, fused, oracle):
    """(pivots for offset 0, info) of the model on _panel(rows, cols, kind): computed once, shared by every option of the case."""
    W = _panel(rows, cols, kind).copy(order="F")
    piv, info = M.panel_tp(W, 0, _fma_rank1(oracle) if fused else None)
    piv.setflags(write=False)
    return piv, info


def _dev(ctx, A, ld, fill=-7.25):
    """Column-major device copy of A with leading dimension ld: (the view, the whole buffer)."""
    import torch
    rows, cols = A.shape
    buf = ctx.colmajor(ld, cols)
    buf.fill_(fill)
    v = buf[:rows]
    v.copy_(torch.from_numpy(np.ascontiguousarray(A)))
    return v, buf


@pytest.mark.parametrize("rows,cols,kind", CASES)
def test_panel_operator(ctx, oracle, rows, cols, kind):
    P = _panel(rows, cols, kind)
    piv_u, _ = _model(rows, cols, kind, False, oracle)
    for fused in (False, True):
        piv_m, info_m = _model(rows, cols, kind, fused, oracle)
        assert np.array_equal(piv_m, piv_u)                       # the selection is unfused whatever the panel's form is
        if kind == "sorted" and rows <= 256:
            assert np.array_equal(piv_m, np.arange(1, min(rows, cols) + 1))
        if kind == "zero_col":
            assert info_m == cols // 2 + 1
        # the no-pivot panel on the rows pre-permuted by the model's pivots: what the factored panel must equal, bit for bit
        dQ, _ = _dev(ctx, M.permute_rows(P, piv_m), rows)
        ctx.dgetf2_npv(dQ, fused=fused)
        want = _bits(dQ)
        for ld in (rows, rows + 5):
            for off in (0, 7):
                dP, buf = _dev(ctx, P, ld)
                piv, info = ctx.dgetf2_tp(dP, fused=fused, ipiv_offset=off)
                tag = (rows, cols, kind, fused, ld, off)
                assert np.array_equal(piv.cpu().numpy(), piv_m + off), tag
                assert np.array_equal(_bits(dP), want), tag
                assert info == info_m, tag
                if ld > rows:
                    assert bool((buf[rows:] == -7.25).all()), tag


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows,cols", SMALL)
def test_small_panels_are_partial_pivoting(ctx, rows, cols, kind):
    """At most 256 active rows at every sub-panel: one group, so pivots and bits are mpf_dgetf2_piv's."""
    P = _panel(rows, cols, kind)
    for fused in (False, True):
        d1, _ = _dev(ctx, P, rows)
        d2, _ = _dev(ctx, P, rows)
        p1, i1 = ctx.dgetf2_piv(d1, fused=fused, ipiv_offset=3)
        p2, i2 = ctx.dgetf2_tp(d2, fused=fused, ipiv_offset=3)
        assert np.array_equal(p1.cpu().numpy(), p2.cpu().numpy()) and i1 == i2
        assert np.array_equal(_bits(d1), _bits(d2))


def _step_loop(ctx, dA, nb):
    """The loop of mpf_factor_dev with pivot_search = 2, driven from outside through the step operators."""
    import torch
    n = dA.shape[0]
    ipiv = torch.arange(1, n + 1, dtype=torch.int32, device=ctx.device)
    for k in range(0, n, nb):
        pc, pr = min(nb, n - k), n - k
        if pr <= 1:
            break
        pv, _ = ctx.dgetf2_tp(dA[k:, k:k + pc], fused=False, ipiv_offset=k)
        ipiv[k:k + pc] = pv
        if k > 0:
            ctx.laswp(dA[:, :k], k, pc, pv)
        if k + pc < n:
            ctx.laswp(dA[:, k + pc:], k, pc, pv)
            ctx.dtrsm_llnu(dA[k:k + pc, k:k + pc], dA[k:k + pc, k + pc:])
            ctx.dgemm_minus(dA[k + pc:, k + pc:], dA[k + pc:, k:k + pc], dA[k:k + pc, k + pc:])
    ctx.synchronize()
    return ipiv


FACTOR_CASES = [(n, nb, 0) for n in (1, 2, 31, 64, 257, 515, 1024) for nb in (1, 7, 32, 128, 256, 300) if nb <= n]
FACTOR_CASES += [(31, 32, 0), (257, 32, 3)]           # nb > N; lda = N + 3


@pytest.mark.parametrize("n,nb,pad", FACTOR_CASES)
def test_factor_equals_the_loop_over_the_step_operators(ctx, mpf, n, nb, pad):
    A = np.asfortranarray(np.random.default_rng(n * 7 + nb).standard_normal((n, n)))
    d1, b1 = _dev(ctx, A, n + pad)
    ip1, info = ctx.factor(d1, nb, trailing=mpf.TRAIL_FP64, pivot_search=2)
    st = ctx.stats()
    assert info == 0 and st.pivot_search == 2 and st.lookahead == 0 and st.superpanel == 1
    d2, _ = _dev(ctx, A, n + pad)
    ip2 = _step_loop(ctx, d2, nb)
    assert np.array_equal(ip1.cpu().numpy(), ip2.cpu().numpy())
    assert np.array_equal(_bits(d1), _bits(d2))
    if pad:
        assert bool((b1[n:] == -7.25).all())
    assert ip1.cpu().numpy()[n - 1] == n                  # a 1 x 1 tail leaves IPIV[N-1] untouched; a pivot of the last row is N
    d3, _ = _dev(ctx, A, n + pad)
    ip3, _ = ctx.factor(d3, nb, trailing=mpf.TRAIL_FP64, pivot_search=2)
    assert np.array_equal(ip1.cpu().numpy(), ip3.cpu().numpy()) and np.array_equal(_bits(d1), _bits(d3))
    if n <= 256:                                          # never more than 256 active rows: partial pivoting's factorization
        d4, _ = _dev(ctx, A, n + pad)
        ip4, _ = ctx.factor(d4, nb, trailing=mpf.TRAIL_FP64, pivot_search=1)
        assert ctx.stats().pivot_search == 1
        assert np.array_equal(ip1.cpu().numpy(), ip4.cpu().numpy()) and np.array_equal(_bits(d1), _bits(d4))


def test_scale_invariance(ctx, mpf):
    """A and A 2^-40: the same pivots, the same L bits, U scaled exactly."""
    n, nb = 515, 128
    A = np.asfortranarray(np.random.default_rng(515).standard_normal((n, n)))
    s = 2.0 ** -40
    out = []
    for Ak in (A, A * s):
        dA = ctx.from_numpy_f(Ak)
        W = dA.clone()
        ip, info = ctx.factor(W, nb, trailing=mpf.TRAIL_FP64, pivot_search=2)
        assert info == 0 and ctx.stats().pivot_search == 2
        _, fro = ctx.check_plu(dA, W, ip)
        print(f"fro_rel_err = {fro:.3e}")
        out.append((ctx.to_numpy_f(W), ip.cpu().numpy()))
    (LU, ip), (LUs, ips) = out
    assert np.array_equal(ip, ips)
    assert np.array_equal(np.tril(LU, -1).view(np.uint64), np.tril(LUs, -1).view(np.uint64))
    assert np.array_equal((np.triu(LU) * s).view(np.uint64), np.triu(LUs).view(np.uint64))


def test_accuracy_against_partial_pivoting(ctx, mpf):
    """N = 1024, nb = 256, standard normal: ||PA - LU||_F / ||A||_F of the tournament is at most 8 x partial pivoting's on the same
    matrix.  The numpy model's worst ratio over N = 515 .. 2500 is 4.5; the margin of about two covers another summation order in
    the device's TRSM and GEMM."""
    n, nb = 1024, 256
    A = np.asfortranarray(np.random.default_rng(1024).standard_normal((n, n)))
    dA = ctx.from_numpy_f(A)
    fro = {}
    for mode in (2, 1):
        W = dA.clone()
        ip, info = ctx.factor(W, nb, trailing=mpf.TRAIL_FP64, pivot_search=mode)
        assert info == 0 and ctx.stats().pivot_search == mode
        _, fro[mode] = ctx.check_plu(dA, W, ip)
        print(f"pivot_search = {mode}: fro_rel_err = {fro[mode]:.3e}, max |l_ij| = {float(W.tril(-1).abs().max()):.3f}")
    assert fro[2] <= 8.0 * fro[1]


@pytest.mark.parametrize("mode_name", ["TRAIL_FP16", "TRAIL_FP16X3"])
def test_fp16_trailing_modes(ctx, mpf, mode_name):
    """The pivots are the tournament's, the update operands still fp16.  The matrix is diagonally dominant by columns, and so is every
    Schur complement of it: in every stack that holds it the diagonal row wins its step, so the tournament -- like the default rule --
    takes no interchange and the factors are the default mode's up to the panel's arithmetic (twice its error at most, the bound
    tests/test_gpu_pivot64.py sets for the other fp64 rule); they precondition the blocked refinement to 1e-12."""
    n, nb = 1024, 256
    rng = np.random.default_rng(1024)
    A = rng.uniform(-1, 1, (n, n))
    A[np.arange(n), np.arange(n)] += 0.6 * n                  # diagonally dominant by rows and by columns
    A = np.asfortranarray(A)
    mode = getattr(mpf, mode_name)
    dA = ctx.from_numpy_f(A)
    W0 = dA.clone()
    ip0, _ = ctx.factor(W0, nb, trailing=mode)
    _, fro0 = ctx.check_plu(dA, W0, ip0)
    W2 = dA.clone()
    ip2, info = ctx.factor(W2, nb, trailing=mode, pivot_search=2)
    assert info == 0 and ctx.stats().pivot_search == 2
    _, fro2 = ctx.check_plu(dA, W2, ip2)
    print(f"{mode_name}: fro_rel_err default {fro0:.3e}, pivot_search = 2 {fro2:.3e}")
    assert fro2 <= 2.0 * fro0
    B = ctx.from_numpy_f(np.asfortranarray(A @ rng.uniform(-1, 1, (n, 3))))
    X, st = ctx.solve_ir_block(dA, W2, ip2, B, max_iter=20, tol=1e-12)
    for s in st:
        assert s.converged and s.rel_residual <= 1e-12, s.rel_residual


def test_drivers_follow_the_context_option(mpf):
    import torch
    n, nb = 515, 128
    rng = np.random.default_rng(77)
    A = np.asfortranarray(rng.standard_normal((n, n)) * 2.0 ** -40)
    c = mpf.MPFContext(0, options={"pivot_fp64": 2})
    try:
        assert c.get_option("pivot_fp64") == 2
        c.set_option("pivot_fp64", 0)
        assert c.get_option("pivot_fp64") == 0
        c.set_option("pivot_fp64", 2)
        assert c.get_option("pivot_fp64") == 2
        dA = c.from_numpy_f(A)
        xt = torch.from_numpy(rng.uniform(-1, 1, n)).to(c.device)
        b = dA @ xt
        x, st, work, ipiv = c.gesv(dA, b, nb=nb, try_fp16=0)
        assert st.path == 2 and st.ir_final.converged and st.ir_final.rel_residual <= 1e-12
        assert c.stats().pivot_search == 2
        # the driver's factors are those of the explicit mode
        W = dA.clone()
        ip, _ = c.factor(W, nb, pivot_search=2)
        assert np.array_equal(ip.cpu().numpy(), ipiv.cpu().numpy()) and np.array_equal(_bits(W), _bits(work))
        B = c.from_numpy_f(np.asfortranarray(A @ rng.uniform(-1, 1, (n, 5))))
        X, ferr, berr, gst, ist, rst, work, ipiv = c.gesvx_block(dA, B, nb=nb, equilibrate=0, try_fp16=0)
        assert all(s.converged for s in ist) and c.stats().pivot_search == 2
        # an explicit rule wins over the option; no rule given follows it
        c.factor(dA.clone(), nb, pivot_search=1)
        assert c.stats().pivot_search == 1
        c.factor(dA.clone(), nb)
        assert c.stats().pivot_search == 2
        one = mpf.MpfDist(rank=0, world=1)
        with pytest.raises(mpf.MPFError) as ei:
            c.factor_dist(dA.clone(), n, nb, one)
        assert "single-GPU" in str(ei.value)
    finally:
        c.close()


def test_rejected_values(ctx, mpf):
    n, nb = 64, 32
    dA = ctx.from_numpy_f(np.asfortranarray(np.random.default_rng(3).standard_normal((n, n))))
    with pytest.raises(mpf.MPFError) as ei:
        ctx.factor(dA.clone(), nb, pivot_search=3)
    assert "pivot_search" in str(ei.value) and "tournament" in str(ei.value)
    with pytest.raises(mpf.MPFError) as ei:
        ctx.factor_dist(dA.clone(), n, nb, mpf.MpfDist(rank=0, world=1), pivot_search=2)
    assert "single-GPU" in str(ei.value)
