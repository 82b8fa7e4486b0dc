"""GPU tests of the fp64 pivot search (include/mpf_c.h: mpf_dgetf2_piv, mpf_opts.pivot_search = 1, option pivot_fp64; csrc/dpivot.hip).

Panel shapes: 1 x 1 and 2 x 2 (no row below / one), 33 x 32 (one full sub-panel, one row below the tile), 257 x 32 (a second
workgroup of one row), 300 x 40 (a narrow tail sub-panel), 1000 x 256 (eight sub-panels, four workgroups), 513 x 300 (more columns
than the fp16 pivot kernels' 256, a workgroup of one row), 4099 x 64 (17 workgroups, the last one of three rows).
Whole factorizations: every N / nb pair crosses another seam of the loop (1 x 1 tail, nb = 1, tail panels narrower than nb, panels
wider than 256, nb > N).

Bit checks need no tolerance.  The model of the panel (tests/pivot64_model.py) is unfused; for fused = 1 its rank-1 update is the
oracle's one-FMA update, so the pivots are compared on the arithmetic the device ran."""
import functools

import numpy as np
import pytest

import pivot64_model as M

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 2), (33, 32), (257, 32), (300, 40), (1000, 256), (513, 300), (4099, 64)]
KINDS = ["normal", "ints", "tiny", "sorted", "last_row", "zero_col"]


def _bits(a):
    if hasattr(a, "cpu"):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a).view(np.uint64)


def _panel(rows, cols, kind):
    rng = np.random.default_rng(rows * 1009 + cols * 13 + KINDS.index(kind))
    P = rng.standard_normal((rows, cols))
    if kind == "ints":                    # many exact ties: the first maximum must win
        P = rng.integers(-3, 4, (rows, cols)).astype(np.float64)
    elif kind == "tiny":                  # far below fp16's range
        P *= 2.0 ** -40
    elif kind == "sorted":                # rows in pivot order already: no interchange at all
        piv, _ = M.panel_piv(np.asfortranarray(P.copy()))
        P = M.permute_rows(np.asfortranarray(P), piv)
    elif kind == "last_row":              # every column takes its pivot from the LAST row: the row that moves there carries 1000 in the next column
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
    piv, info = M.panel_piv(W, 0, _fma_rank1(oracle) if fused else None)
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


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_panel_operator(ctx, oracle, rows, cols, kind):
    P = _panel(rows, cols, kind)
    for fused in (False, True):
        piv_m, info_m = _model(rows, cols, kind, fused, oracle)
        if kind == "sorted" and not fused:
            assert np.array_equal(piv_m, np.arange(1, min(rows, cols) + 1))
        if kind == "last_row" and not fused:
            assert np.all(piv_m == rows)
        if kind == "zero_col":
            assert info_m == cols // 2 + 1
        # the no-pivot panel on the rows pre-permuted by the model's pivots: what the factored panel must equal, bit for bit
        dQ, _ = _dev(ctx, M.permute_rows(P, piv_m), rows)
        ctx.dgetf2_npv(dQ, fused=fused)
        want = _bits(dQ)
        for ld in (rows, rows + 5):
            for off in (0, 7):
                dP, buf = _dev(ctx, P, ld)
                piv, info = ctx.dgetf2_piv(dP, fused=fused, ipiv_offset=off)
                tag = (rows, cols, kind, fused, ld, off)
                assert np.array_equal(piv.cpu().numpy(), piv_m + off), tag
                assert np.array_equal(_bits(dP), want), tag
                assert info == info_m, tag
                if ld > rows:
                    assert bool((buf[rows:] == -7.25).all()), tag
                if kind in ("normal", "tiny", "sorted", "last_row"):
                    assert float(dP.tril(-1).abs().max()) <= 1.0, tag


def _step_loop(ctx, dA, nb):
    """The loop of mpf_factor_dev with pivot_search = 1, driven from outside through the step operators."""
    import torch
    n = dA.shape[0]
    ipiv = torch.arange(1, n + 1, dtype=torch.int32, device=ctx.device)
    for k in range(0, n, nb):
        pc, pr = min(nb, n - k), n - k
        if pr <= 1:
            break
        pv, _ = ctx.dgetf2_piv(dA[k:, k:k + pc], fused=False, ipiv_offset=k)
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
    ip1, info = ctx.factor(d1, nb, trailing=mpf.TRAIL_FP64, pivot_search=1)
    st = ctx.stats()
    assert info == 0 and st.pivot_search == 1 and st.lookahead == 0 and st.superpanel == 1
    d2, _ = _dev(ctx, A, n + pad)
    ip2 = _step_loop(ctx, d2, nb)
    assert np.array_equal(ip1.cpu().numpy(), ip2.cpu().numpy())
    assert np.array_equal(_bits(d1), _bits(d2))
    if pad:
        assert bool((b1[n:] == -7.25).all())
    if n > 1:
        assert float(d1.tril(-1).abs().max()) <= 1.0
    assert ip1.cpu().numpy()[n - 1] == n                  # a 1 x 1 tail leaves IPIV[N-1] untouched; a pivot of the last row is N
    d3, _ = _dev(ctx, A, n + pad)
    ip3, _ = ctx.factor(d3, nb, trailing=mpf.TRAIL_FP64, pivot_search=1)
    assert np.array_equal(ip1.cpu().numpy(), ip3.cpu().numpy()) and np.array_equal(_bits(d1), _bits(d3))
    # the default mode reports what it ran, too
    d4, _ = _dev(ctx, A, n + pad)
    ctx.factor(d4, nb, trailing=mpf.TRAIL_FP64)
    assert ctx.stats().pivot_search == 0


def test_scale_invariance(ctx, mpf):
    """A and A 2^-40: same pivots, same L bits, U scaled exactly; |l_ij| <= 1.  The default mode sees an all-zero fp16 image of the
    scaled matrix and does not pivot at all: the hole pivot_search = 1 closes."""
    n, nb = 515, 128
    A = np.asfortranarray(np.random.default_rng(515).standard_normal((n, n)))
    s = 2.0 ** -40
    out = []
    for Ak in (A, A * s):
        dA = ctx.from_numpy_f(Ak)
        W = dA.clone()
        ip, info = ctx.factor(W, nb, trailing=mpf.TRAIL_FP64, pivot_search=1)
        assert info == 0 and ctx.stats().pivot_search == 1
        _, fro = ctx.check_plu(dA, W, ip)
        print(f"fro_rel_err = {fro:.3e}")
        assert fro <= 1e-14
        out.append((ctx.to_numpy_f(W), ip.cpu().numpy()))
    (LU, ip), (LUs, ips) = out
    assert np.array_equal(ip, ips)
    assert np.array_equal(np.tril(LU, -1).view(np.uint64), np.tril(LUs, -1).view(np.uint64))
    assert np.array_equal((np.triu(LU) * s).view(np.uint64), np.triu(LUs).view(np.uint64))
    assert np.abs(np.tril(LU, -1)).max() <= 1.0 and np.abs(np.tril(LUs, -1)).max() <= 1.0
    W = ctx.from_numpy_f(A * s)
    ip0, _ = ctx.factor(W, nb, trailing=mpf.TRAIL_FP64)
    assert ctx.stats().pivot_search == 0
    assert np.array_equal(ip0.cpu().numpy(), np.arange(1, n + 1))


@pytest.mark.parametrize("mode_name", ["TRAIL_FP16", "TRAIL_FP16X3"])
def test_fp16_trailing_modes(ctx, mpf, mode_name):
    """The pivots are fp64's, the update operands still fp16: the factors are as good as the default mode's on the same matrix (twice
    its error at most: other pivots can double the rounding constant) and precondition the blocked refinement to 1e-12."""
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
    W1 = dA.clone()
    ip1, info = ctx.factor(W1, nb, trailing=mode, pivot_search=1)
    assert info == 0 and ctx.stats().pivot_search == 1
    _, fro1 = ctx.check_plu(dA, W1, ip1)
    print(f"{mode_name}: fro_rel_err default {fro0:.3e}, pivot_search = 1 {fro1:.3e}")
    assert float(W1.tril(-1).abs().max()) <= 1.0
    assert fro1 <= 2.0 * fro0
    B = ctx.from_numpy_f(np.asfortranarray(A @ rng.uniform(-1, 1, (n, 3))))
    X, st = ctx.solve_ir_block(dA, W1, ip1, B, max_iter=20, tol=1e-12)
    for s in st:
        assert s.converged and s.rel_residual <= 1e-12, s.rel_residual


def test_drivers_follow_the_context_option(mpf):
    import torch
    n, nb = 515, 128
    rng = np.random.default_rng(77)
    A = np.asfortranarray(rng.standard_normal((n, n)) * 2.0 ** -40)
    c = mpf.MPFContext(0, options={"pivot_fp64": 1})
    try:
        assert c.get_option("pivot_fp64") == 1
        c.set_option("pivot_fp64", 0)
        assert c.get_option("pivot_fp64") == 0
        c.set_option("pivot_fp64", 1)
        assert "pivot_fp64" in mpf.option_names()
        dA = c.from_numpy_f(A)
        xt = torch.from_numpy(rng.uniform(-1, 1, n)).to(c.device)
        b = dA @ xt
        x, st, work, ipiv = c.gesv(dA, b, nb=nb, try_fp16=0)
        assert st.path == 2 and st.ir_final.converged and st.ir_final.rel_residual <= 1e-12
        assert c.stats().pivot_search == 1
        assert float(work.tril(-1).abs().max()) <= 1.0
        B = c.from_numpy_f(np.asfortranarray(A @ rng.uniform(-1, 1, (n, 5))))
        X, ferr, berr, gst, ist, rst, work, ipiv = c.gesvx_block(dA, B, nb=nb, equilibrate=0, try_fp16=0)
        assert all(s.converged for s in ist) and c.stats().pivot_search == 1
        assert float(work.tril(-1).abs().max()) <= 1.0
        one = mpf.MpfDist(rank=0, world=1)
        with pytest.raises(mpf.MPFError) as ei:
            c.factor_dist(dA.clone(), n, nb, one)
        assert "single-GPU" in str(ei.value)
        c.set_option("pivot_fp64", 0)
        with pytest.raises(mpf.MPFError):
            c.factor_dist(dA.clone(), n, nb, one, pivot_search=1)
    finally:
        c.close()
