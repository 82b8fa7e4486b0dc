"""GPU tests of the batched expert layer (include/mpf_c.h: mpf_lange_batched, mpf_gecon_batched, mpf_residual_batched,
mpf_gerfs_batched; csrc/batched_refine.hip).  Every comparison is bit for bit against tests/batched_refine_model.py; a NaN compares
with a NaN.

Sizes: the family's seams (the team widths 8, 16, 32, the crossover to the workgroup form, one and two rows per lane, the largest).
Inputs are "stale factors": LU = getrf_batched(A + 2^-k E), A and E standard normal, refinement against A, X0 = getrs of B, with
k in {none, 40, 20, 12, 8, 4, 2}, one per batch slot -- the family reaches all three stop reasons of the rule."""
import ctypes as C

import numpy as np
import pytest

import batched_inv_model as MI
import batched_refine_model as R

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 7, 8, 9, 16, 17, 31, 32, 33, 63, 64, 65, 100, 127, 128]
KS = [None, 40, 20, 12, 8, 4, 2]
NB = len(KS)
NRHS = 5
_CASES, _MODELS = {}, {}


def _bits(a):
    if hasattr(a, "cpu"):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a).view(np.uint64)


def _same(got, want):
    """Equal bits where `want` is a number, NaN where it is NaN."""
    if hasattr(got, "cpu"):
        got = got.cpu().numpy()
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(_bits(np.where(nan, 0.0, got)), _bits(np.where(nan, 0.0, want)))


def _dev(ctx, a):
    """Packed column-major device batch of the numpy array (batch, rows, cols)."""
    import torch
    T = ctx.colmajor_batch(*a.shape)
    T.copy_(torch.from_numpy(np.array(a, order="C")))
    return T


def _padded(ctx, a, extra_rows=3, extra_cols=1, fill=777.0):
    """(buffer, view): the batch inside a buffer with a larger leading dimension and stride, the rest filled with `fill`."""
    import torch
    b, r, c = a.shape
    buf = ctx.colmajor_batch(b, r + extra_rows, c + extra_cols)
    buf.fill_(fill)
    view = buf[:, :r, :c]
    view.copy_(torch.from_numpy(np.array(a, order="C")))
    return buf, view


def _case(ctx, n):
    """The stale-factor family at order n: numpy inputs, device factors and first solutions; computed once, shared, read-only."""
    if n not in _CASES:
        rng = np.random.default_rng(7000 + n)
        A = rng.standard_normal((NB, n, n))
        E = rng.standard_normal((NB, n, n))
        B = rng.standard_normal((NB, n, NRHS))
        Af = np.stack([A[s] if k is None else A[s] + 2.0 ** -k * E[s] for s, k in enumerate(KS)])
        dA, dB = _dev(ctx, A), _dev(ctx, B)
        LU, ipiv, info = ctx.getrf_batched(_dev(ctx, Af))
        assert not info.cpu().numpy().any()
        X0 = {t: ctx.getrs_batched(LU, ipiv, dB, trans=bool(t)) for t in (0, 1)}
        c = dict(A=A, B=B, dA=dA, dB=dB, dLU=LU, dipiv=ipiv, dX0=X0, LU=LU.cpu().numpy(), ipiv=ipiv.cpu().numpy(),
                 X0={t: X0[t].cpu().numpy() for t in (0, 1)})
        for v in (c["A"], c["B"], c["LU"], c["ipiv"], c["X0"][0], c["X0"][1]):
            v.setflags(write=False)
        _CASES[n] = c
    return _CASES[n]


def _model(ctx, n, trans, itmax):
    """The model's (X, ferr, berr, iters, stops) per slot for the family's five columns; computed once, shared."""
    key = (n, trans, itmax)
    if key not in _MODELS:
        c = _case(ctx, n)
        _MODELS[key] = [R.gerfs_model(c["A"][s], c["LU"][s], c["ipiv"][s], c["B"][s], c["X0"][trans][s], bool(trans), itmax)
                        for s in range(NB)]
    return _MODELS[key]


def _check_gerfs(got, want, cols=slice(None)):
    X, ferr, berr, its = got
    for s, (Xm, fm, bm, im, _) in enumerate(want):
        assert _same(X[s], Xm[:, cols]), s
        assert _same(berr[s], bm[cols]), s
        assert _same(ferr[s], fm[cols]), s
        assert np.array_equal(its[s].cpu().numpy(), im[cols]), s


@pytest.mark.parametrize("n", SIZES)
def test_lange_three_norms_padded(ctx, n):
    c = _case(ctx, n)
    buf, view = _padded(ctx, c["A"])
    before = buf.clone()
    for norm in ("1", "O", "I", "M"):
        want = np.array([R.lange_model(c["A"][s], norm) for s in range(NB)])
        assert _same(ctx.lange_batched(view, norm), want), norm
        assert _same(ctx.lange_batched(c["dA"], norm), want), norm
    assert np.array_equal(_bits(buf), _bits(before))
    bad = c["A"].copy()
    bad[2, n - 1, 0] = np.nan
    for norm in ("1", "I", "M"):
        got = ctx.lange_batched(_dev(ctx, bad), norm).cpu().numpy()
        assert np.isnan(got[2]) and not np.isnan(np.delete(got, 2)).any()


@pytest.mark.parametrize("norm", ["1", "I"])
@pytest.mark.parametrize("n", SIZES)
def test_gecon_against_the_model(ctx, n, norm):
    c = _case(ctx, n)
    anorm = ctx.lange_batched(c["dA"], norm)
    an = anorm.cpu().numpy()
    rcond, ainv = ctx.gecon_batched(c["dLU"], anorm, norm, want_ainvnm=True)
    want = [R.gecon_model(c["LU"][s], an[s], norm) for s in range(NB)]
    assert _same(rcond, [w[0] for w in want]) and _same(ainv, [w[1] for w in want])
    assert np.all(rcond.cpu().numpy() > 0)
    if norm == "1":          # as a set, mpf_getri_batched's columns without interchanges
        cols = MI.getri_model_skipping(c["LU"][0], np.arange(1, n + 1))
        assert _same(ainv[0], np.max(R.tree_sum(np.abs(cols), axis=0)))
    buf, view = _padded(ctx, c["LU"])
    assert np.array_equal(_bits(ctx.gecon_batched(view, anorm, norm)), _bits(rcond))
    # a zero on U's diagonal, anorm 0, an Inf in the factors: rcond 0 there, the neighbours bit-unchanged
    LU = c["LU"].copy()
    LU[1, n // 2, n // 2] = 0.0
    LU[5, n - 1, 0] = np.inf
    an2 = an.copy()
    an2[3] = 0.0
    import torch
    r2, a2 = ctx.gecon_batched(_dev(ctx, LU), torch.from_numpy(an2).to(ctx.device), norm, want_ainvnm=True)
    r2, a2, r1, a1 = r2.cpu().numpy(), a2.cpu().numpy(), rcond.cpu().numpy(), ainv.cpu().numpy()
    assert r2[1] == 0 and np.isposinf(a2[1]) and r2[3] == 0 and r2[5] == 0 and not np.isnan(r2).any()
    assert np.array_equal(_bits(a2[3]), _bits(a1[3]))
    for s in (0, 2, 4, 6):
        assert np.array_equal(_bits(r2[s]), _bits(r1[s])) and np.array_equal(_bits(a2[s]), _bits(a1[s]))


@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_residual_against_the_model(ctx, n, trans):
    c = _case(ctx, n)
    want = [R.residual_model(c["A"][s], c["X0"][trans][s], c["B"][s], bool(trans)) for s in range(NB)]
    for nrhs in (1, 3, 5):
        Rr, W = ctx.residual_batched(c["dA"], c["dX0"][trans][:, :, :nrhs], c["dB"][:, :, :nrhs], trans=bool(trans))
        for s in range(NB):
            assert _same(Rr[s], want[s][0][:, :nrhs]) and _same(W[s], want[s][1][:, :nrhs]), (nrhs, s)
    R1, W1 = ctx.residual_batched(c["dA"], c["dX0"][trans][:, :, 0], c["dB"][:, :, 0], trans=bool(trans), want_w=False)
    assert W1 is None and _same(R1, np.stack([w[0][:, 0] for w in want]))


@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_gerfs_against_the_model(ctx, n, trans):
    """X, berr, iters and ferr for nrhs 1 and 5 and itmax 0, 1 and 40 (clamped to 31); a column alone equals the same column
    among five; A, LU, ipiv and B are preserved and the padding rows of X are untouched."""
    c = _case(ctx, n)
    keep = [t.clone() for t in (c["dA"], c["dLU"], c["dipiv"], c["dB"])]
    stops = set()
    for itmax in (0, 1, 40):
        want = _model(ctx, n, trans, itmax)
        stops.update(st for w in want for st in w[4])
        got = ctx.gerfs_batched(c["dA"], c["dLU"], c["dipiv"], c["dB"], c["dX0"][trans], trans=bool(trans), itmax=itmax)
        _check_gerfs(got, want)
        one = ctx.gerfs_batched(c["dA"], c["dLU"], c["dipiv"], c["dB"][:, :, 2:3], c["dX0"][trans][:, :, 2:3], trans=bool(trans),
                                itmax=itmax)
        _check_gerfs(one, want, slice(2, 3))
        if itmax == 40:
            assert max(int(w[3].max()) for w in want) <= 31
    if n in (3, 9, 33, 65, 128):
        assert stops >= {"berr <= eps", "not halved", "itmax"}, stops
    for t, k in zip((c["dA"], c["dLU"], c["dipiv"], c["dB"]), keep):
        assert t.equal(k)
    # in place on a padded X, without ferr
    buf, view = _padded(ctx, c["X0"][trans])
    Xr, ferr, berr, its = ctx.gerfs_batched(c["dA"], c["dLU"], c["dipiv"], c["dB"], view, trans=bool(trans), overwrite=True,
                                            want_ferr=False)
    want = _model(ctx, n, trans, 0)
    assert Xr.data_ptr() == view.data_ptr() and ferr is None
    for s in range(NB):
        assert _same(view[s], want[s][0]) and _same(berr[s], want[s][2])
    out = buf.cpu().numpy()
    assert np.all(out[:, n:, :] == 777.0) and np.all(out[:, :, NRHS:] == 777.0)


@pytest.mark.parametrize("n", SIZES)
def test_position_in_the_batch_changes_no_bit(ctx, n):
    """The same matrix at slot 0 and at the last slot of a batch of 67: several workgroups and a partial last one for the team forms."""
    c = _case(ctx, n)
    idx = [4] + [s % NB for s in range(1, 66)] + [4]
    A, LU, B, X0 = _dev(ctx, c["A"][idx]), _dev(ctx, c["LU"][idx]), _dev(ctx, c["B"][idx]), _dev(ctx, c["X0"][0][idx])
    import torch
    ipiv = torch.from_numpy(c["ipiv"][idx].copy()).to(ctx.device)
    want = _model(ctx, n, 0, 0)
    X, ferr, berr, its = ctx.gerfs_batched(A, LU, ipiv, B, X0)
    for s in (0, 66, 1, 65):
        m = want[idx[s]]
        assert _same(X[s], m[0]) and _same(ferr[s], m[1]) and _same(berr[s], m[2]) and np.array_equal(its[s].cpu().numpy(), m[3]), s
    an = ctx.lange_batched(A, "I")
    rc = ctx.gecon_batched(LU, an, "I")
    assert np.array_equal(_bits(an[0]), _bits(an[66])) and np.array_equal(_bits(rc[0]), _bits(rc[66]))
    assert _same(rc[66], R.gecon_model(c["LU"][4], R.lange_model(c["A"][4], "I"), "I")[0])


@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("n", [8, 32, 33, 128])
def test_gerfs_is_the_composition_of_the_step_operators(ctx, n, trans):
    """A host-driven loop of residual_batched + getrs_batched + add that takes the model's decisions gives gerfs_batched's X."""
    import torch
    c = _case(ctx, n)
    want = _model(ctx, n, trans, 0)
    its = torch.from_numpy(np.stack([w[3] for w in want])).to(ctx.device)            # (batch, nrhs)
    X = c["dX0"][trans].clone()
    for t in range(1, int(its.max()) + 1):
        Rr, _ = ctx.residual_batched(c["dA"], X, c["dB"], trans=bool(trans))
        D = ctx.getrs_batched(c["dLU"], c["dipiv"], Rr, trans=bool(trans))
        X = torch.where((its >= t)[:, None, :], X + D, X)
    got = ctx.gerfs_batched(c["dA"], c["dLU"], c["dipiv"], c["dB"], c["dX0"][trans], trans=bool(trans), want_ferr=False)[0]
    assert np.array_equal(_bits(got), _bits(X))
    Rr, W = ctx.residual_batched(c["dA"], X, c["dB"], trans=bool(trans))
    for s in range(NB):
        be = [R.backward_error(Rr[s, :, k].cpu().numpy(), W[s, :, k].cpu().numpy(), n) for k in range(NRHS)]
        assert _same(be, want[s][2])


@pytest.mark.parametrize("n", [3, 16, 33, 100])
def test_a_nan_stays_inside_its_matrix(ctx, n):
    c = _case(ctx, n)
    A = c["A"].copy()
    A[3, n - 1, 0] = np.nan
    want = _model(ctx, n, 0, 0)
    X, ferr, berr, its = ctx.gerfs_batched(_dev(ctx, A), c["dLU"], c["dipiv"], c["dB"], c["dX0"][0])
    assert np.isnan(berr[3].cpu().numpy()).all() and not its[3].cpu().numpy().any()
    assert np.array_equal(_bits(X[3]), _bits(c["X0"][0][3]))
    for s in (0, 1, 2, 4, 5, 6):
        m = want[s]
        assert _same(X[s], m[0]) and _same(ferr[s], m[1]) and _same(berr[s], m[2]) and np.array_equal(its[s].cpu().numpy(), m[3]), s


def _err(ctx):
    return ctx.L.mpf_last_error(ctx.h).decode()


def test_argument_errors(ctx):
    import torch
    L, h = ctx.L, ctx.h
    n, batch, nrhs = 4, 3, 2
    A = ctx.colmajor_batch(batch, n, n).fill_(1.0)
    Bm = ctx.colmajor_batch(batch, n, nrhs).fill_(1.0)
    X, Rr = Bm.clone(), Bm.clone()
    piv = torch.ones((batch, n), dtype=torch.int32, device=ctx.device)
    d = torch.zeros(batch * nrhs, dtype=torch.float64, device=ctx.device)
    it = torch.zeros(batch * nrhs, dtype=torch.int32, device=ctx.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    sa, sb = n * n, n * nrhs

    def lange(norm=b"1", a=p(A), lda=n, n_=n, batch_=batch, out=p(d)):
        return L.mpf_lange_batched(h, norm, a, lda, sa, n_, batch_, out)

    def gecon(norm=b"1", lu=p(A), ld=n, n_=n, batch_=batch, an=p(d), rc=p(d)):
        return L.mpf_gecon_batched(h, norm, lu, ld, sa, n_, batch_, an, rc, None)

    def resid(trans=0, a=p(A), lda=n, n_=n, batch_=batch, nrhs_=nrhs, x=p(X), ldx=n, r=p(Rr)):
        return L.mpf_residual_batched(h, trans, a, lda, sa, n_, batch_, nrhs_, x, ldx, sb, p(Bm), n, sb, r, n, sb, None)

    def gerfs(trans=0, a=p(A), lda=n, n_=n, batch_=batch, nrhs_=nrhs, piv_=p(piv), berr=p(d), ldx=n):
        return L.mpf_gerfs_batched(h, trans, a, lda, sa, p(A), n, sa, n_, batch_, piv_, n, nrhs_, p(Bm), n, sb, p(X), ldx, sb, 0, None,
                                   berr, p(it))

    for f, who in ((lange, "lange_batched"), (gecon, "gecon_batched"), (resid, "residual_batched"), (gerfs, "gerfs_batched")):
        assert f() == 0, _err(ctx)
        assert f(n_=129) == -1
        assert who in _err(ctx) and "128" in _err(ctx) and "mpf_gecon" in _err(ctx) and "mpf_gerfs" in _err(ctx)
        assert f(n_=0) == 0 and f(batch_=0) == 0
        assert f(n_=-1) == -1 and who in _err(ctx)
    assert resid(nrhs_=0) == 0 and gerfs(nrhs_=0) == 0
    assert lange(lda=n - 1) == -1 and "leading dimension of A" in _err(ctx)
    assert gecon(ld=n - 1) == -1 and "leading dimension of LU" in _err(ctx)
    assert resid(lda=n - 1) == -1 and "leading dimension of A" in _err(ctx)
    assert resid(ldx=n - 1) == -1 and "leading dimension of X" in _err(ctx)
    assert gerfs(lda=n - 1) == -1 and "leading dimension of A" in _err(ctx)
    assert gerfs(ldx=n - 1) == -1 and "leading dimension of X" in _err(ctx)
    assert resid(trans=2) == -1 and "trans must be 0 or 1" in _err(ctx)
    assert gerfs(trans=-1) == -1 and "trans must be 0 or 1" in _err(ctx)
    assert lange(norm=b"F") == -1 and "norm must be" in _err(ctx)
    assert gecon(norm=b"M") == -1 and "norm must be" in _err(ctx)
    assert lange(a=None) == -1 and "null pointer" in _err(ctx)
    assert lange(out=None) == -1 and "null pointer" in _err(ctx)
    assert gecon(lu=None) == -1 and gecon(an=None) == -1 and gecon(rc=None) == -1 and "null pointer" in _err(ctx)
    assert resid(a=None) == -1 and resid(x=None) == -1 and resid(r=None) == -1 and "null pointer" in _err(ctx)
    assert gerfs(a=None) == -1 and gerfs(piv_=None) == -1 and gerfs(berr=None) == -1 and "null pointer" in _err(ctx)
    assert resid(nrhs_=-1) == -1 and gerfs(nrhs_=-1) == -1
    ctx.synchronize()


@pytest.mark.parametrize("trans", [False, True])
def test_python_drivers_with_one_singular_slot(ctx, trans):
    import batched_model as M
    n, batch, nrhs = 9, 4, 3
    rng = np.random.default_rng(99)
    A = rng.standard_normal((batch, n, n))
    A[2, :, 4] = 0.0                                   # a zero column: a zero pivot at step 5
    B = rng.standard_normal((batch, n, nrhs))
    X, rcond, ferr, berr, info = ctx.solvex_batched(_dev(ctx, A), _dev(ctx, B), trans=trans)
    assert info.cpu().numpy().tolist() == [0, 0, 5, 0]
    norm = "I" if trans else "1"
    for s in (0, 1, 3):
        LU, ipiv, _ = M.getrf_model(A[s])
        X0 = M.getrs_model(LU, ipiv, B[s], trans=trans)
        Xm, fm, bm, _, _ = R.gerfs_model(A[s], LU, ipiv, B[s], X0, trans)
        assert _same(X[s], Xm) and _same(ferr[s], fm) and _same(berr[s], bm)
        assert _same(rcond[s], R.gecon_model(LU, R.lange_model(A[s], norm), norm)[0])
    assert float(rcond[2]) == 0.0
    rc = ctx.cond_batched(_dev(ctx, A), "1")
    assert float(rc[2]) == 0.0 and (_same(rc, rcond.cpu().numpy()) if not trans else True)
    with pytest.raises(Exception):
        ctx.solve_batched(_dev(ctx, A), _dev(ctx, B))     # the existing driver still raises
