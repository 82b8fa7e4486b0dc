"""GPU tests of the error bounds for solves (include/mpf_c.h: mpf_gerfs), against the numpy restatement of dgerfs in
tests/gerfs_model.py and against quantities recomputed in extended precision.

For the returned X of a column (x), with op(A) = A or A^T, nz = N + 1, eps = 2^-53:
    r_ld       = b - op(A) x in np.longdouble,   w2 = |b| + |op(A)| |x|
    berr_exact = the componentwise backward error from r_ld and w2
    lo         = max_i (|op(A)^-1| (nz eps w2))_i / max|x|
    hi         = max_i (|op(A)^-1| (|r_ld| + 2 nz eps w2))_i / max|x|
The bounds asserted:
    |berr - berr_exact| <= 2 nz eps           the rounding error of an fp64 residual relative to w
    berr <= max(4 berr_model, 2^-52)          fp64 factors (4: another summation order may decide one correction more or fewer)
    max|x - x_ref| / max|x| <= ferr           x_ref: numpy's solution after one refinement with a longdouble residual
    lo / 3 <= ferr <= 1.01 hi (1.1 hi on fp16 factors)      dlacn2 never overestimates and is within Higham's factor 3; the device's
                                              |r| exceeds the true one by at most nz eps w2; the margins cover the solves' own error
    1/3 <= ferr / ferr_model <= 3
"""
import ctypes as C

import numpy as np
import pytest

import blk_helpers as H
import gerfs_model as G

pytestmark = pytest.mark.gpu
EPS = G.EPS
LD = np.longdouble


def _ld_product(Al, Xl):
    """Al @ Xl in np.longdouble (no BLAS behind it), row blocks on a few threads."""
    from concurrent.futures import ThreadPoolExecutor
    n = Al.shape[0]
    if n < 1024:
        return Al @ Xl
    cuts = np.linspace(0, n, 9).astype(int)
    with ThreadPoolExecutor(8) as ex:
        return np.vstack(list(ex.map(lambda k: Al[cuts[k]:cuts[k + 1]] @ Xl, range(8))))


class _Ref:
    """Everything the assertions need about one (A, trans, B), computed once."""

    def __init__(self, A, trans, B):
        self.n = A.shape[0]
        self.Aop = np.ascontiguousarray(A.T if trans else A)
        self.B = B
        self.inv = np.linalg.inv(self.Aop)
        self.Al = self.Aop.astype(LD)
        self.X0 = self.inv @ B

    def exact(self, X):
        """(berr_exact, err, lo, hi) per column of the returned X."""
        n, nz = self.n, self.n + 1
        safe1 = nz * G.SAFMIN
        safe2 = safe1 / EPS
        nc = X.shape[1]
        R = np.hstack([self.B, self.B]).astype(LD) - _ld_product(self.Al, np.hstack([X, self.X0]).astype(LD))   # one product for both
        r_ld, r0 = R[:, :nc], R[:, nc:].astype(np.float64)
        x_ref = self.X0 + self.inv @ r0          # numpy's solution, refined once with a longdouble residual
        w2 = np.abs(self.B) + np.abs(self.Aop) @ np.abs(X)
        big = w2 > safe2
        q = np.where(big, np.abs(r_ld) / np.where(big, w2, 1.0).astype(LD), (np.abs(r_ld) + safe1) / (w2.astype(LD) + safe1))
        berr_exact = q.max(axis=0).astype(np.float64)
        xmax = np.abs(X).max(axis=0)
        xmax = np.where(xmax == 0, 1.0, xmax)
        err = np.abs(X - x_ref).max(axis=0) / xmax
        absinv = np.abs(self.inv)
        lo = (absinv @ (nz * EPS * w2)).max(axis=0) / xmax
        hi = (absinv @ (np.abs(r_ld).astype(np.float64) + 2 * nz * EPS * w2)).max(axis=0) / xmax
        return berr_exact, err, lo, hi


def _check(ref, X, ferr, berr, model, fp16, bound_holds=True, cols=None, tag=None):
    """Assertions 1 and 2 of the module docstring on the columns `cols` (default: all); model = gerfs_model's result."""
    n = ref.n
    berr_exact, err, lo, hi = ref.exact(X)
    _, ferr_m, berr_m, _, _ = model
    cols = np.arange(X.shape[1]) if cols is None else np.asarray(cols)
    margin = 1.1 if fp16 else 1.01
    print(tag, "berr/eps", (berr / EPS)[cols].max(), "|berr - exact| / (nz eps)", (np.abs(berr - berr_exact) / ((n + 1) * EPS))[cols].max(),
          "err/ferr", (err[cols] / ferr[cols]).max(), "ferr/lo", (ferr[cols] / lo[cols]).min(), "ferr/hi", (ferr[cols] / hi[cols]).max(),
          "ferr/model", (ferr[cols] / ferr_m[cols]).min(), (ferr[cols] / ferr_m[cols]).max())
    assert np.all(np.abs(berr - berr_exact)[cols] <= 2 * (n + 1) * EPS), (tag, berr[cols], berr_exact[cols])
    if not fp16:
        assert np.all(berr[cols] <= np.maximum(4 * berr_m[cols], 2.0 ** -52)), (tag, berr[cols], berr_m[cols])
    if bound_holds:
        assert np.all(err[cols] <= ferr[cols]), (tag, err[cols], ferr[cols])
    assert np.all(lo[cols] / 3 <= ferr[cols]) and np.all(ferr[cols] <= margin * hi[cols]), (tag, lo[cols], ferr[cols], hi[cols])
    ratio = ferr[cols] / ferr_m[cols]
    assert np.all((ratio >= 1 / 3) & (ratio <= 3)), (tag, ratio)


def _run(ctx, A, trans, B_np, trailing, ld=None, nb=128, itmax=0):
    """Factor, start from getrs, refine on the device and in the model.  Returns (ref, X, ferr, berr, stats, model, buffers)."""
    n = A.shape[0]
    dA, W, ipiv, _ = H.factor(ctx, A, ld=ld, nb=nb, trailing=trailing)
    B, Bbuf = H.dev(ctx, B_np, ld)
    X0 = ctx.getrs(W, ipiv, B, trans=trans)
    Xv, Xbuf = H.dev(ctx, X0.cpu().numpy(), ld)
    X, ferr, berr, st = ctx.gerfs(dA, W, ipiv, B, Xv, trans=trans, itmax=itmax, overwrite=True)
    ctx.synchronize()
    assert X.data_ptr() == Xv.data_ptr()
    solve, solve_t = H.host_solvers(ctx.to_numpy_f(W), ipiv.cpu().numpy(), trans)
    model = G.gerfs_model(A, solve, solve_t, B_np, X0.cpu().numpy(), trans, itmax)
    return _Ref(A, trans, B_np), X.cpu().numpy(), ferr, berr, st, model, (Bbuf, Xbuf)


# sizes: tile edges (63), 256-block edges (256, 257), a padded leading dimension (777 in 800), a second 4096-column partial (4100);
# column counts: one, a partial tile, two tiles + 1, more than two tiles
SHAPES = [(1, 1, None), (2, 17, None), (63, 33, None), (256, 65, None), (257, 17, None), (777, 33, 800), (1000, 65, None), (4100, 3, None)]


@pytest.mark.parametrize("trailing", [0, 1], ids=["fp64", "fp16"])
@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("n,nrhs,ld", SHAPES)
def test_bounds(ctx, n, nrhs, ld, trans, trailing):
    """berr is what it says, ferr bounds the error and is not slack: fp64 factors of every shape, fp16 factors of the diagonally
    dominant matrix of every shape.  Rows N .. ld - 1 of X and B keep their sentinel."""
    A = H.rand(n, 500 + n, dominant=float(n) ** 0.5 if trailing else 2.0)
    B_np = np.random.default_rng(nrhs).uniform(-1, 1, (n, nrhs))
    ref, X, ferr, berr, st, model, (Bbuf, Xbuf) = _run(ctx, A, trans, B_np, trailing, ld=ld, itmax=10 if trailing else 0)
    _check(ref, X, ferr, berr, model, fp16=bool(trailing), tag=(n, nrhs, trans, trailing))
    for s in st:
        assert 0 <= s.iterations <= (10 if trailing else 5)
        assert (s.lacn2_iterations == 1) if n == 1 else (2 <= s.lacn2_iterations <= 5)
        assert s.solves >= s.iterations + (1 if n == 1 else 4) and s.ms_total == st[0].ms_total
    if ld:
        assert bool((Xbuf[n:] == 7.5).all()) and bool((Bbuf[n:] == 7.5).all()), "padding rows were written"


def test_bounds_grow_with_kappa(ctx):
    """Ill-conditioned matrices on fp64 factors: assertions 1 and 2 hold, and ferr grows with kappa.  (On fp16 factors of these
    matrices error <= ferr is false in the model too: not asserted.)"""
    ferrs = []
    for n, kappa, seed in ((257, 1e6, 6), (300, 1e10, 7)):
        A = H.ill(n, kappa, seed)
        B_np = np.random.default_rng(seed).uniform(-1, 1, (n, 17))
        for trans in (0, 1):
            ref, X, ferr, berr, st, model, _ = _run(ctx, A, trans, B_np, 0)
            _check(ref, X, ferr, berr, model, fp16=False, tag=(n, kappa, trans))
            ferrs.append(ferr)
    assert min(ferrs[2].min(), ferrs[3].min()) > max(ferrs[0].max(), ferrs[1].max()), ferrs


@pytest.fixture(scope="module")
def lowp(ctx):
    """N = 4096, 40 columns scaled 1e-6 .. 1e6 and one zero column, fp16 factors of a diagonally dominant matrix, both op(A): the
    device's and the model's refinement from getrs's X, itmax = 10.  Shared and left unchanged."""
    n, nrhs = 4096, 40
    A = H.rand(n, 21, dominant=float(n) ** 0.5)
    B_np = np.random.default_rng(5).uniform(-1, 1, (n, nrhs)) * np.logspace(-6, 6, nrhs)
    B_np[:, 7] = 0.0
    return {trans: _run(ctx, A, trans, B_np, 1, nb=256, itmax=10) for trans in (0, 1)}


@pytest.mark.parametrize("trans", [0, 1])
def test_refinement_on_fp16_factors(lowp, trans):
    """Every non-zero column gets at least one correction; the bounds hold; the zero column gives what dgerfs gives there
    (berr = 1 after one empty correction, x = 0), as the model."""
    ref, X, ferr, berr, st, model, _ = lowp[trans]
    Xm, ferr_m, berr_m, its_m, _ = model
    nz_cols = [j for j in range(X.shape[1]) if j != 7]
    for j in nz_cols:
        assert 1 <= st[j].iterations <= 10, j
    _check(ref, X, ferr, berr, model, fp16=True, cols=nz_cols, tag=("lowp", trans))
    assert berr[7] == berr_m[7] and not X[:, 7].any() and not Xm[:, 7].any() and st[7].iterations == its_m[7]


@pytest.mark.parametrize("trans", [0, 1])
def test_refinement_reaches_four_eps(lowp, trans):
    """Every column ends with berr <= 4 * 2^-53, or else within 4 x the model's value.  (berr's floor is the rounding error of the
    residual itself: this is the check that needs the fused kernel's two-level sum)"""
    ref, X, ferr, berr, st, model, _ = lowp[trans]
    berr_m = model[2]
    print("berr/eps", berr / EPS, "model", berr_m / EPS, "iterations", [s.iterations for s in st], "model", model[3])
    for j in range(X.shape[1]):
        if j != 7:
            assert berr[j] <= 4 * EPS or berr[j] <= 4 * berr_m[j], (j, berr[j] / EPS, berr_m[j] / EPS)


@pytest.mark.parametrize("trans", [0, 1])
def test_zero_column_ferr_equals_the_model(lowp, trans):
    """The zero column's ferr against the model's (its weights are safe1 = nz DBL_MIN everywhere, its estimate lives at the bottom of
    the exponent range)."""
    ref, X, ferr, berr, st, model, _ = lowp[trans]
    print("ferr", ferr[7], "model", model[1][7], "ratio", ferr[7] / model[1][7])
    assert ferr[7] == model[1][7]


@pytest.fixture(scope="module")
def small16(ctx):
    """N = 1000 on fp16 factors, 37 columns scaled 1e-3 .. 1e3 (test_column_independence's setting in test_gpu_getrs.py)."""
    import torch
    n, nrhs = 1000, 37
    A = H.rand(n, 11)
    dA, W, ipiv, _ = H.factor(ctx, A, trailing=1)
    B = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (n, nrhs)) * np.logspace(-3, 3, nrhs)).to(ctx.device)
    return dA, W, ipiv, B.t().contiguous().t()


def _key(X, ferr, berr, st, j):
    return (H.bits(X.cpu().numpy()[:, j]).tolist(), H.bits(ferr[j:j + 1])[0], H.bits(berr[j:j + 1])[0], st[j].iterations, st[j].lacn2_iterations)


@pytest.mark.parametrize("trans", [0, 1])
def test_itmax(ctx, small16, trans):
    """itmax = 1: at most one correction and a larger berr than with itmax = 10; itmax = 0 is LAPACK's 5; a value above 31 is
    taken and gives what 31 gives."""
    dA, W, ipiv, B = small16
    X0 = ctx.getrs(W, ipiv, B, trans=trans)
    r1 = ctx.gerfs(dA, W, ipiv, B, X0, trans=trans, itmax=1)
    r10 = ctx.gerfs(dA, W, ipiv, B, X0, trans=trans, itmax=10)
    r0 = ctx.gerfs(dA, W, ipiv, B, X0, trans=trans, itmax=0)
    r5 = ctx.gerfs(dA, W, ipiv, B, X0, trans=trans, itmax=5)
    print("berr itmax 1", r1[2], "itmax 10", r10[2], "iterations", [s.iterations for s in r10[3]])
    assert all(s.iterations <= 1 for s in r1[3])
    assert np.all(r1[2] > r10[2])
    assert all(s.iterations <= 10 for s in r10[3]) and all(s.iterations <= 5 for s in r0[3])
    r31 = ctx.gerfs(dA, W, ipiv, B, X0, trans=trans, itmax=31)
    r99 = ctx.gerfs(dA, W, ipiv, B, X0, trans=trans, itmax=99)
    for j in range(B.shape[1]):
        assert _key(*r0, j) == _key(*r5, j), j
        assert _key(*r99, j) == _key(*r31, j) and r99[3][j].iterations <= 31, j


@pytest.mark.parametrize("trans", [0, 1])
def test_column_independence(ctx, small16, trans):
    """X[:, j], ferr[j], berr[j], iterations and lacn2_iterations have the same bits for a column solved alone, among 37, at a permuted
    position, and in a second call."""
    import torch
    dA, W, ipiv, B = small16
    nrhs = B.shape[1]
    perm = np.random.default_rng(4).permutation(nrhs)
    Bp = B[:, torch.from_numpy(perm).to(ctx.device)].t().contiguous().t()
    X0 = ctx.getrs(W, ipiv, B, trans=trans)
    Xp0 = ctx.getrs(W, ipiv, Bp, trans=trans)
    full = ctx.gerfs(dA, W, ipiv, B, X0, trans=trans, itmax=10)
    again = ctx.gerfs(dA, W, ipiv, B, X0, trans=trans, itmax=10)
    permd = ctx.gerfs(dA, W, ipiv, Bp, Xp0, trans=trans, itmax=10)
    assert all(s.ms_total == full[3][0].ms_total and s.solves == full[3][0].solves for s in full[3])
    where = {int(j): i for i, j in enumerate(perm)}
    for j in range(nrhs):
        assert _key(*full, j) == _key(*again, j), j
        assert _key(*full, j) == _key(*permd, where[j]), j
    for j in (0, 16, 36):
        bj = B[:, j:j + 1].contiguous()
        alone = ctx.gerfs(dA, W, ipiv, bj, ctx.getrs(W, ipiv, bj, trans=trans), trans=trans, itmax=10)
        assert _key(*alone, 0) == _key(*full, j), j


def test_arguments(ctx, mpf):
    """nrhs = 0 -> 0; bad trans, N <= 0, a leading dimension < N, a null pointer -> -1 with the error set; a bad ipiv entry -> -1
    naming ipiv; rows N .. ld - 1 of X and B keep their sentinel."""
    import torch
    n, ld = 64, 80
    A = H.rand(n, 9)
    dA, W, ipiv, _ = H.factor(ctx, A)
    B, Bbuf = H.dev(ctx, np.ones((n, 2)), ld)
    X, Xbuf = H.dev(ctx, np.linalg.solve(A, np.ones((n, 2))), ld)
    L, h = ctx.L, ctx.h
    p = lambda t: C.c_void_p(t.data_ptr())
    ctx._bind()
    st = (mpf.MpfGerfsStats * 2)()
    fe, be = (C.c_double * 2)(), (C.c_double * 2)()
    good = [0, p(dA), n, p(W), n, p(ipiv), n, 2, p(B), ld, p(X), ld, 0, fe, be, st]
    assert L.mpf_gerfs(h, *good) == 0
    assert 0 < fe[0] < 1e-10 and 0 <= be[0] <= 4 * EPS
    assert bool((Xbuf[n:] == 7.5).all()) and bool((Bbuf[n:] == 7.5).all()), "padding rows were written"
    a = list(good)
    a[7] = 0
    assert L.mpf_gerfs(h, *a) == 0
    null = C.c_void_p(0)
    bad = {0: 2, 6: 0, 2: n - 1, 4: n - 1, 9: n - 1, 11: n - 1, 1: null, 3: null, 5: null, 8: null, 10: null, 13: None, 14: None}
    for pos, val in list(bad.items()) + [(6, -3), (0, -1)]:
        a = list(good)
        a[pos] = val
        assert L.mpf_gerfs(h, *a) == -1, (pos, val)
        assert "gerfs" in L.mpf_last_error(h).decode(), (pos, val)
    wrong = ipiv.clone()
    wrong[5] = n + 7
    a = list(good)
    a[5] = p(wrong)
    assert L.mpf_gerfs(h, *a) == -1
    assert "ipiv" in L.mpf_last_error(h).decode()
    torch.cuda.synchronize()
