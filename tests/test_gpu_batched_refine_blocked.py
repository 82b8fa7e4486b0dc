"""GPU tests of the blocked batched expert layer (include/mpf_c.h: mpf_lange_batched_blocked, mpf_gecon_batched_blocked,
mpf_residual_batched_blocked, mpf_gerfs_batched_blocked; csrc/batched_refine_blocked.hip).  Every comparison is bit for bit, a NaN
compares with a NaN; the one tolerance is the sanity check of cond_batched_blocked against numpy.

Sizes are the seams of the blocked kernels, not workloads.  SMALL: with option batched_blocked_min_n = 0 every n runs the new kernels
-- both sides of every 32-row block and 64-lane wave seam -- and is compared with tests/batched_refine_blocked_model.py AND with the
n <= 128 entries.  NATURAL: default options, against the model.  LARGE (batch 3): the norm and the residual against the model, gecon
against the device's own getrs_batched_blocked on an identity reduced by the model's tree and maximum, gerfs against the composition
residual_batched_blocked + the model's rule + getrs_batched_blocked driven from the host, its ferr with the rows of the inverse from
getrs_batched_blocked on an identity.

Inputs: batched_refine_blocked_model.family -- stale factors LU = getrf(A + 2^-k E), refinement against A, X0 = getrs of B -- whose
last column is exact (b = column j of op(A), x0 = e_j), so that every order reaches all three stop reasons.  The refinement kernel
takes four columns per workgroup (one below four right-hand sides): nrhs = 5 is the value just above the tile, nrhs = 1 the narrow
form."""
import ctypes as C

import numpy as np
import pytest

import batched_model as M
import batched_refine_blocked_model as RB
import batched_refine_model as R
from test_gpu_batched_refine import _bits, _dev, _err, _padded, _same

pytestmark = pytest.mark.gpu

SMALL = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128]
NATURAL = [129, 130, 161, 192, 193, 255, 256, 257]
LARGE = [511, 513, 1023, 1024]
LARGE_KS = [None, 12, 2]
NRHS = RB.NRHS
CHUNK = 1 << 15           # BB_MAX_LAUNCH of csrc/mpf_internal.h
ALL_STOPS = {"berr <= eps", "not halved", "itmax"}
_CASES, _MODELS, _ROWS = {}, {}, {}


@pytest.fixture(scope="module")
def bctx(mpf):
    """Every n through the blocked kernels."""
    c = mpf.MPFContext(0, options={"batched_blocked_min_n": 0})
    yield c
    c.close()


def _pick(bctx, ctx, n):
    return bctx if n <= 128 else ctx


def _case(c, n):
    """The family at order n: numpy inputs, device factors and first solutions per trans; computed once, shared, read-only."""
    if n not in _CASES:
        import torch
        ks = LARGE_KS if n > 257 else RB.KS
        A, Af, B = RB.family(n, ks)
        dA = _dev(c, A)
        LU, ipiv, info = c.getrf_batched_blocked(_dev(c, Af))
        assert not info.cpu().numpy().any()
        Bt, X0t, dB, dX0 = {}, {}, {}, {}
        for t in (0, 1):
            X0 = c.getrs_batched_blocked(LU, ipiv, _dev(c, B), trans=bool(t)).cpu().numpy().copy()
            Bx = B.copy()
            for s in range(len(ks)):
                Bx[s, :, -1], X0[s, :, -1] = RB.exact_column(A[s], bool(t))
            Bt[t], X0t[t], dB[t], dX0[t] = Bx, X0, _dev(c, Bx), _dev(c, X0)
        case = dict(nb=len(ks), A=A, B=Bt, X0=X0t, dA=dA, dB=dB, dX0=dX0, dLU=LU, dipiv=ipiv, LU=LU.cpu().numpy(),
                    ipiv=ipiv.cpu().numpy(), keep=[x.clone(memory_format=torch.preserve_format) for x in (dA, LU, ipiv)])
        for v in [case["A"], case["LU"], case["ipiv"]] + list(Bt.values()) + list(X0t.values()):
            v.setflags(write=False)
        _CASES[n] = case
    return _CASES[n]


def _rows(c, n, trans):
    """|Y| per slot, Y[i] = the chain of 1 - trans for e_i with interchanges: the model's up to 257, above the device's own
    getrs_batched_blocked on an identity."""
    if (n, trans) not in _ROWS:
        import torch
        case = _case(c, n)
        if n <= 257:
            rows = [R.inverse_rows(case["LU"][s], case["ipiv"][s], bool(trans)) for s in range(case["nb"])]
        else:
            eye = c.colmajor_batch(case["nb"], n, n)
            eye.copy_(torch.eye(n, dtype=torch.float64, device=c.device).expand(case["nb"], n, n))
            Y = c.getrs_batched_blocked(case["dLU"], case["dipiv"], eye, trans=not trans, overwrite=True).cpu().numpy()
            rows = [np.abs(Y[s]).T.copy() for s in range(case["nb"])]
        _ROWS[(n, trans)] = rows
    return _ROWS[(n, trans)]


def _model(c, n, trans, itmax):
    """The model's (X, ferr, berr, iters, stops) per slot for the family's five columns; computed once, shared."""
    key = (n, trans, itmax)
    if key not in _MODELS:
        case, rows = _case(c, n), _rows(c, n, trans)
        _MODELS[key] = [RB.gerfs_model(case["A"][s], case["LU"][s], case["ipiv"][s], case["B"][trans][s], case["X0"][trans][s],
                                       bool(trans), itmax, True, rows[s]) for s in range(case["nb"])]
    return _MODELS[key]


def _compose(c, n, trans, itmax):
    """The same five outputs from the host-driven composition: residual_batched_blocked, the model's rule on the downloaded r and w,
    getrs_batched_blocked on r, x += dx for the columns that go on; ferr from the last r and w and _rows."""
    key = (n, trans, itmax, "composed")
    if key not in _MODELS:
        import torch
        case, rows = _case(c, n), _rows(c, n, trans)
        nb = case["nb"]
        cap = 5 if itmax <= 0 else min(itmax, 31)
        X = case["dX0"][trans].clone(memory_format=torch.preserve_format)
        lst, its = np.full((nb, NRHS), 3.0), np.zeros((nb, NRHS), dtype=np.int32)
        berr, act, stops = np.zeros((nb, NRHS)), np.ones((nb, NRHS), dtype=bool), [[None] * NRHS for _ in range(nb)]
        count = 1
        while True:
            Rr, W = c.residual_batched_blocked(case["dA"], X, case["dB"][trans], trans=bool(trans))
            r, w = Rr.cpu().numpy(), W.cpu().numpy()
            for s in range(nb):
                for k in range(NRHS):
                    if act[s, k]:
                        berr[s, k] = RB.backward_error(r[s, :, k], w[s, :, k], n)
                        stops[s][k] = RB.rule(berr[s, k], lst[s, k], count, cap)
                        act[s, k] = stops[s][k] is None
            if not act.any():
                break
            D = c.getrs_batched_blocked(case["dLU"], case["dipiv"], Rr, trans=bool(trans))
            go = torch.from_numpy(act.copy()).to(c.device)
            X = torch.where(go[:, None, :], X + D, X)
            lst[act], its[act] = berr[act], count
            count += 1
        x = X.cpu().numpy()
        out = []
        for s in range(nb):
            ferr = np.array([RB.ferr_of(r[s, :, k], w[s, :, k], x[s, :, k], rows[s]) for k in range(NRHS)])
            out.append((x[s], ferr, berr[s], its[s], stops[s]))
        _MODELS[key] = out
    return _MODELS[key]


def _check_gerfs(got, want, cols=slice(None), ferr=True):
    X, fe, berr, its = got
    for s, (Xm, fm, bm, im, _) in enumerate(want):
        assert _same(X[s], Xm[:, cols]), s
        assert _same(berr[s], bm[cols]), s
        assert np.array_equal(its[s].cpu().numpy(), im[cols]), s
        if ferr:
            assert _same(fe[s], fm[cols]), s


# ---- norms ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SMALL + NATURAL + LARGE)
def test_lange_three_norms_padded(bctx, ctx, n):
    c = _pick(bctx, ctx, n)
    case = _case(c, n)
    buf, view = _padded(c, case["A"])
    before = buf.clone()
    for norm in ("1", "O", "I", "M"):
        want = np.array([RB.lange_model(case["A"][s], norm) for s in range(case["nb"])])
        got = c.lange_batched_blocked(view, norm)
        assert _same(got, want), norm
        assert np.array_equal(_bits(c.lange_batched_blocked(case["dA"], norm)), _bits(got)), norm
        if n <= 128:
            assert np.array_equal(_bits(ctx.lange_batched(case["dA"], norm)), _bits(got)), norm
    assert np.array_equal(_bits(buf), _bits(before))
    bad = case["A"].copy()
    bad[2, n - 1, 0] = np.nan
    for norm in ("1", "I", "M"):
        got = c.lange_batched_blocked(_dev(c, bad), norm).cpu().numpy()
        assert np.isnan(got[2]) and not np.isnan(np.delete(got, 2)).any()


# ---- reciprocal condition number -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", ["1", "I"])
@pytest.mark.parametrize("n", SMALL + NATURAL + LARGE)
def test_gecon(bctx, ctx, n, norm):
    import torch
    c = _pick(bctx, ctx, n)
    case = _case(c, n)
    nb = case["nb"]
    anorm = c.lange_batched_blocked(case["dA"], norm)
    an = anorm.cpu().numpy()
    rcond, ainv = c.gecon_batched_blocked(case["dLU"], anorm, norm, want_ainvnm=True)
    if n <= 257:
        want = [RB.gecon_model(case["LU"][s], an[s], norm) for s in range(nb)]
    else:                      # the device's own chains from an identity, no interchanges, reduced by the model's tree and maximum
        eye = c.colmajor_batch(nb, n, n)
        eye.copy_(torch.eye(n, dtype=torch.float64, device=c.device).expand(nb, n, n))
        nop = torch.arange(1, n + 1, dtype=torch.int32, device=c.device).expand(nb, n).contiguous()
        Xi = c.getrs_batched_blocked(case["dLU"], nop, eye, trans=(norm == "I"), overwrite=True).cpu().numpy()
        norms = [RB.ainvnm_of(Xi[s]) for s in range(nb)]
        want = [(RB.rcond_of(v, an[s]), v) for s, v in enumerate(norms)]
    assert _same(rcond, [w[0] for w in want]) and _same(ainv, [w[1] for w in want])
    assert np.all(rcond.cpu().numpy() > 0)
    if n <= 128:
        small = ctx.gecon_batched(case["dLU"], anorm, norm, want_ainvnm=True)
        assert np.array_equal(_bits(small[0]), _bits(rcond)) and np.array_equal(_bits(small[1]), _bits(ainv))
    buf, view = _padded(c, case["LU"])
    before = buf.clone()
    assert np.array_equal(_bits(c.gecon_batched_blocked(view, anorm, norm)), _bits(rcond))      # (and without d_ainvnm)
    assert np.array_equal(_bits(buf), _bits(before))
    # a zero on U's diagonal in slot 1, anorm 0 in slot 2: rcond 0 there, +Inf beside the zero, the neighbours bit-unchanged
    LU = case["LU"].copy()
    LU[1, n // 2, n // 2] = 0.0
    an2 = an.copy()
    an2[2] = 0.0
    r2, a2 = c.gecon_batched_blocked(_dev(c, LU), torch.from_numpy(an2).to(c.device), norm, want_ainvnm=True)
    r2, a2, r1, a1 = r2.cpu().numpy(), a2.cpu().numpy(), rcond.cpu().numpy(), ainv.cpu().numpy()
    assert r2[1] == 0 and np.isposinf(a2[1]) and r2[2] == 0 and not np.isnan(r2).any()
    assert np.array_equal(_bits(a2[2]), _bits(a1[2]))
    keep = [s for s in range(nb) if s not in (1, 2)]
    assert np.array_equal(_bits(r2[keep]), _bits(r1[keep])) and np.array_equal(_bits(a2[keep]), _bits(a1[keep]))
    for t, k in zip((case["dA"], case["dLU"], case["dipiv"]), case["keep"]):
        assert t.equal(k)


# ---- the step operator ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("n", SMALL + NATURAL + LARGE)
def test_residual(bctx, ctx, n, trans):
    import torch
    c = _pick(bctx, ctx, n)
    case = _case(c, n)
    nb, dB, dX = case["nb"], case["dB"][trans], case["dX0"][trans]
    want = [RB.residual_model(case["A"][s], case["X0"][trans][s], case["B"][trans][s], bool(trans)) for s in range(nb)]
    for nrhs in (1, 3, 5):
        Rr, W = c.residual_batched_blocked(case["dA"], dX[:, :, :nrhs], dB[:, :, :nrhs], trans=bool(trans))
        for s in range(nb):
            assert _same(Rr[s], want[s][0][:, :nrhs]) and _same(W[s], want[s][1][:, :nrhs]), (nrhs, s)
    assert not want[0][0][:, -1].any()                                      # the exact column: r = 0
    R1, W1 = c.residual_batched_blocked(case["dA"], dX[:, :, 0], dB[:, :, 0], trans=bool(trans), want_w=False)
    assert W1 is None and _same(R1, np.stack([w[0][:, 0] for w in want]))
    if n <= 128:
        Rs, Ws = ctx.residual_batched(case["dA"], dX, dB, trans=bool(trans))
        assert np.array_equal(_bits(Rs), _bits(Rr)) and np.array_equal(_bits(Ws), _bits(W))
    # R aliased to B, with W, through the C entry
    Bc = dB.clone(memory_format=torch.preserve_format)
    Wc = c.colmajor_batch(nb, n, NRHS)
    c._bind()
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = c.L.mpf_residual_batched_blocked(c.h, trans, p(case["dA"]), n, n * n, n, nb, NRHS, p(dX), n, n * NRHS, p(Bc), n, n * NRHS,
                                          p(Bc), n, n * NRHS, p(Wc))
    assert rc == 0, _err(c)
    assert np.array_equal(_bits(Bc), _bits(Rr)) and np.array_equal(_bits(Wc), _bits(W))


# ---- refinement ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("n", SMALL + NATURAL + LARGE)
def test_gerfs(bctx, ctx, n, trans):
    """X, berr, iters and ferr for nrhs 5 (one above the tile of four) and 1 and itmax 0, 1 and 31; a column alone equals the same
    column among five; with and without ferr; out of place and in place on a padded X; two calls give the same bits; A, LU and ipiv
    are preserved.  Up to 257 against the model, above against the composition."""
    c = _pick(bctx, ctx, n)
    case = _case(c, n)
    ref = _model if n <= 257 else _compose
    dA, dLU, dip, dB, dX = case["dA"], case["dLU"], case["dipiv"], case["dB"][trans], case["dX0"][trans]
    stops = set()
    for itmax in (0, 1, 31):
        want = ref(c, n, trans, itmax)
        stops.update(st for w in want for st in w[4])
        got = c.gerfs_batched_blocked(dA, dLU, dip, dB, dX, trans=bool(trans), itmax=itmax)
        _check_gerfs(got, want)
        one = c.gerfs_batched_blocked(dA, dLU, dip, dB[:, :, 2:3], dX[:, :, 2:3], trans=bool(trans), itmax=itmax)
        _check_gerfs(one, want, slice(2, 3))
        if n <= 128:
            small = ctx.gerfs_batched(dA, dLU, dip, dB, dX, trans=bool(trans), itmax=itmax)
            for g, s in zip(got[:3], small[:3]):
                assert _same(g, s.cpu().numpy())
            assert np.array_equal(got[3].cpu().numpy(), small[3].cpu().numpy())
    if n > 1:
        assert stops >= ALL_STOPS, stops
    again = c.gerfs_batched_blocked(dA, dLU, dip, dB, dX, trans=bool(trans), itmax=31)
    for g, a in zip(got[:3], again[:3]):
        assert _same(a, g.cpu().numpy())
    assert np.array_equal(got[3].cpu().numpy(), again[3].cpu().numpy())
    # in place on a padded X, without ferr
    want = ref(c, n, trans, 0)
    buf, view = _padded(c, case["X0"][trans])
    Xr, ferr, berr, its = c.gerfs_batched_blocked(dA, dLU, dip, dB, view, trans=bool(trans), overwrite=True, want_ferr=False)
    assert Xr.data_ptr() == view.data_ptr() and ferr is None
    _check_gerfs((view, None, berr, its), want, ferr=False)
    out = buf.cpu().numpy()
    assert np.all(out[:, n:, :] == 777.0) and np.all(out[:, :, NRHS:] == 777.0)
    for t, k in zip((dA, dLU, dip), case["keep"]):
        assert t.equal(k)
    assert np.array_equal(_bits(dB), _bits(case["B"][trans])) and np.array_equal(_bits(dX), _bits(case["X0"][trans]))


@pytest.mark.parametrize("n", [33, 161])
def test_position_and_batch_size_change_no_bit(bctx, ctx, n):
    """The same matrix at slot 0 and at the last slot of a batch of 67, against the batch of seven."""
    import torch
    c = _pick(bctx, ctx, n)
    case = _case(c, n)
    idx = [4] + [s % 7 for s in range(1, 66)] + [4]
    for trans in (0, 1):
        A, LU = _dev(c, case["A"][idx]), _dev(c, case["LU"][idx])
        B, X0 = _dev(c, case["B"][trans][idx]), _dev(c, case["X0"][trans][idx])
        ipiv = torch.from_numpy(case["ipiv"][idx].copy()).to(c.device)
        want = _model(c, n, trans, 0)
        X, ferr, berr, its = c.gerfs_batched_blocked(A, LU, ipiv, B, X0, trans=bool(trans))
        for s in (0, 66, 1, 65):
            m = want[idx[s]]
            assert _same(X[s], m[0]) and _same(ferr[s], m[1]) and _same(berr[s], m[2]) and np.array_equal(its[s].cpu().numpy(), m[3]), s
        norm = "I" if trans else "1"
        an = c.lange_batched_blocked(A, norm)
        rc = c.gecon_batched_blocked(LU, an, norm)
        assert np.array_equal(_bits(an[0]), _bits(an[66])) and np.array_equal(_bits(rc[0]), _bits(rc[66]))
        assert _same(rc[66], RB.gecon_model(case["LU"][4], RB.lange_model(case["A"][4], norm), norm)[0])
        Rr, W = c.residual_batched_blocked(A, X0, B, trans=bool(trans))
        assert np.array_equal(_bits(Rr[0]), _bits(Rr[66])) and np.array_equal(_bits(W[0]), _bits(W[66]))


@pytest.mark.parametrize("n", [33, 161])
def test_a_nan_stays_inside_its_matrix(bctx, ctx, n):
    c = _pick(bctx, ctx, n)
    case = _case(c, n)
    A = case["A"].copy()
    A[3, n - 1, 0] = np.nan
    want = _model(c, n, 0, 0)
    X, ferr, berr, its = c.gerfs_batched_blocked(_dev(c, A), case["dLU"], case["dipiv"], case["dB"][0], case["dX0"][0])
    assert np.isnan(berr[3].cpu().numpy()).all() and not its[3].cpu().numpy().any()
    assert np.array_equal(_bits(X[3]), _bits(case["X0"][0][3]))
    for s in (0, 1, 2, 4, 5, 6):
        m = want[s]
        assert _same(X[s], m[0]) and _same(ferr[s], m[1]) and _same(berr[s], m[2]) and np.array_equal(its[s].cpu().numpy(), m[3]), s
    # one NaN column of B stops that column alone
    B = case["B"][0].copy()
    B[1, 0, 2] = np.nan
    X, ferr, berr, its = c.gerfs_batched_blocked(case["dA"], case["dLU"], case["dipiv"], _dev(c, B), case["dX0"][0])
    got = berr.cpu().numpy()
    assert np.isnan(got[1, 2]) and np.isnan(got).sum() == 1
    keep = [k for k in range(NRHS) if k != 2]
    assert _same(X[1][:, keep], want[1][0][:, keep]) and _same(ferr[1][keep], want[1][1][keep])


@pytest.mark.parametrize("n", [2, 33])
def test_chunk_seam(bctx, n):
    """A batch just above 32768: the entries go in two chunks; the matrices past the seam repeat the first seven."""
    import torch
    case = _case(bctx, n)
    batch = CHUNK + 5
    idx = torch.arange(batch, device=bctx.device) % 7

    def rep(t):
        out = bctx.colmajor_batch(batch, t.shape[1], t.shape[2])
        out.copy_(t[idx])
        return out

    A, LU, B, X0 = rep(case["dA"]), rep(case["dLU"]), rep(case["dB"][0]), rep(case["dX0"][0])
    ipiv = case["dipiv"][idx].contiguous()
    tail = slice(CHUNK - 2, batch)
    ti = idx[tail]
    an7 = bctx.lange_batched_blocked(case["dA"], "1")
    rc7 = bctx.gecon_batched_blocked(case["dLU"], an7, "1")
    R7, W7 = bctx.residual_batched_blocked(case["dA"], case["dX0"][0], case["dB"][0])
    g7 = bctx.gerfs_batched_blocked(case["dA"], case["dLU"], case["dipiv"], case["dB"][0], case["dX0"][0])
    an = bctx.lange_batched_blocked(A, "1")
    rc = bctx.gecon_batched_blocked(LU, an, "1")
    Rr, W = bctx.residual_batched_blocked(A, X0, B)
    g = bctx.gerfs_batched_blocked(A, LU, ipiv, B, X0)
    assert np.array_equal(_bits(an[tail]), _bits(an7[ti])) and np.array_equal(_bits(rc[tail]), _bits(rc7[ti]))
    assert np.array_equal(_bits(Rr[tail]), _bits(R7[ti])) and np.array_equal(_bits(W[tail]), _bits(W7[ti]))
    for a, b in zip(g[:3], g7[:3]):
        assert _same(a[tail], b[ti].cpu().numpy())
    assert np.array_equal(g[3][tail].cpu().numpy(), g7[3][ti].cpu().numpy())
    assert bool((an[:7] == an7).all()) and bool((g[3][:7] == g7[3]).all())


def test_bound_workspace_seam(bctx):
    """With ferr a chunk is also bounded by the workspace (2^25 doubles: n + 1 per column and one per column and tile of 16 chains):
    n = 33 with 40 right-hand sides crosses that seam below 2^15 matrices.  The matrices past it repeat the first seven."""
    import torch
    n, reps = 33, 8
    case = _case(bctx, n)
    nrhs = NRHS * reps
    fit = (1 << 25) // (nrhs * (n + 1 + (n + 15) // 16))
    assert fit < CHUNK
    batch = fit + 4
    idx = torch.arange(batch, device=bctx.device) % 7

    def rep(t, k=1):
        out = bctx.colmajor_batch(batch, t.shape[1], t.shape[2] * k)
        out.copy_(t[idx].repeat(1, 1, k))
        return out

    B7, X7 = _dev(bctx, np.tile(case["B"][0], (1, 1, reps))), _dev(bctx, np.tile(case["X0"][0], (1, 1, reps)))
    g7 = bctx.gerfs_batched_blocked(case["dA"], case["dLU"], case["dipiv"], B7, X7)
    five = bctx.gerfs_batched_blocked(case["dA"], case["dLU"], case["dipiv"], case["dB"][0], case["dX0"][0])
    assert _same(g7[1], np.tile(five[1].cpu().numpy(), (1, reps)))                       # a column among forty is the column among five
    g = bctx.gerfs_batched_blocked(rep(case["dA"]), rep(case["dLU"]), case["dipiv"][idx].contiguous(), rep(case["dB"][0], reps),
                                   rep(case["dX0"][0], reps))
    tail = slice(fit - 3, batch)
    for a, b in zip(g[:3], g7[:3]):
        assert _same(a[tail], b[idx[tail]].cpu().numpy())
    assert np.array_equal(g[3][tail].cpu().numpy(), g7[3][idx[tail]].cpu().numpy())


def test_default_options_forward_small_orders(ctx):
    """n = 65 < batched_blocked_min_n = 129: the n <= 128 entries take it; the bits are the same either way."""
    assert ctx.get_option("batched_blocked_min_n") == 129
    n = 65
    A, Af, B = RB.family(n)
    dA, dB = _dev(ctx, A), _dev(ctx, B)
    LU, ipiv, _ = ctx.getrf_batched_blocked(_dev(ctx, Af))
    X0 = ctx.getrs_batched_blocked(LU, ipiv, dB)
    for norm in ("1", "I", "M"):
        assert np.array_equal(_bits(ctx.lange_batched_blocked(dA, norm)), _bits(ctx.lange_batched(dA, norm)))
    an = ctx.lange_batched(dA, "1")
    assert np.array_equal(_bits(ctx.gecon_batched_blocked(LU, an, "1")), _bits(ctx.gecon_batched(LU, an, "1")))
    for a, b in zip(ctx.residual_batched_blocked(dA, X0, dB), ctx.residual_batched(dA, X0, dB)):
        assert np.array_equal(_bits(a), _bits(b))
    for a, b in zip(ctx.gerfs_batched_blocked(dA, LU, ipiv, dB, X0), ctx.gerfs_batched(dA, LU, ipiv, dB, X0)):
        assert _same(a, b.cpu().numpy())


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
    ctx._bind()

    def lange(norm=b"1", a=p(A), lda=n, n_=n, batch_=batch, out=p(d)):
        return L.mpf_lange_batched_blocked(h, norm, a, lda, sa, n_, batch_, out)

    def gecon(norm=b"1", lu=p(A), ld=n, n_=n, batch_=batch, an=p(d), rc=p(d)):
        return L.mpf_gecon_batched_blocked(h, norm, lu, ld, sa, n_, batch_, an, rc, None)

    def resid(trans=0, a=p(A), lda=n, n_=n, batch_=batch, nrhs_=nrhs, x=p(X), ldx=n, r=p(Rr)):
        return L.mpf_residual_batched_blocked(h, trans, a, lda, sa, n_, batch_, nrhs_, x, ldx, sb, p(Bm), n, sb, r, n, sb, None)

    def gerfs(trans=0, a=p(A), lda=n, n_=n, batch_=batch, nrhs_=nrhs, piv_=p(piv), berr=p(d), ldx=n):
        return L.mpf_gerfs_batched_blocked(h, trans, a, lda, sa, p(A), n, sa, n_, batch_, piv_, n, nrhs_, p(Bm), n, sb, p(X), ldx, sb, 0,
                                           None, berr, p(it))

    for f, who in ((lange, "lange_batched_blocked"), (gecon, "gecon_batched_blocked"), (resid, "residual_batched_blocked"),
                   (gerfs, "gerfs_batched_blocked")):
        assert f() == 0, _err(ctx)
        assert f(n_=1025) == -1
        assert who in _err(ctx) and "1024" in _err(ctx) and "mpf_gecon" in _err(ctx) and "mpf_gerfs" in _err(ctx)
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


# ---- the Python drivers --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trans", [False, True])
def test_solvex_with_one_singular_slot(ctx, trans):
    n, batch, nrhs = 130, 4, 3
    rng = np.random.default_rng(99)
    A = rng.standard_normal((batch, n, n))
    A[2, :, 4] = 0.0                                   # a zero column: a zero pivot at step 5
    B = rng.standard_normal((batch, n, nrhs))
    dA, dB = _dev(ctx, A), _dev(ctx, B)
    X, rcond, ferr, berr, info = ctx.solvex_batched_blocked(dA, dB, trans=trans)
    assert info.cpu().numpy().tolist() == [0, 0, 5, 0]
    assert float(rcond[2]) == 0.0
    norm = "I" if trans else "1"
    LU, ipiv, _ = ctx.getrf_batched_blocked(dA)
    rc = ctx.gecon_batched_blocked(LU, ctx.lange_batched_blocked(dA, norm), norm)
    X0 = ctx.getrs_batched_blocked(LU, ipiv, dB, trans=trans)
    Xc, fc, bc, _ = ctx.gerfs_batched_blocked(dA, LU, ipiv, dB, X0, trans=trans)
    for s in (0, 1, 3):
        assert np.array_equal(_bits(X[s]), _bits(Xc[s])) and np.array_equal(_bits(ferr[s]), _bits(fc[s]))
        assert np.array_equal(_bits(berr[s]), _bits(bc[s])) and np.array_equal(_bits(rcond[s]), _bits(rc[s]))
        assert float(rcond[s]) > 0 and float(berr[s].max()) < 1e-14 and np.isfinite(ferr[s].cpu().numpy()).all()
    # the composition's pieces are the model's (one slot)
    LUm, ipm = LU[0].cpu().numpy(), ipiv[0].cpu().numpy()
    want = RB.gerfs_model(A[0], LUm, ipm, B[0], M.getrs_model(LUm, ipm, B[0], trans=trans), trans)
    assert _same(X[0], want[0]) and _same(ferr[0], want[1]) and _same(berr[0], want[2])
    assert float(ctx.cond_batched_blocked(dA, norm)[2]) == 0.0
    with pytest.raises(Exception):
        ctx.solve_batched_blocked(dA, dB)                 # the existing driver still raises


def test_cond_against_numpy(ctx):
    """A sanity check only (the bit checks are above): 1 / (||A|| ||A^-1||) from numpy to a relative 1e-10 on well-conditioned
    input (kappa_2 = 100: the inverse's entries are good to about 100 eps)."""
    n, batch = 200, 3
    rng = np.random.default_rng(12)
    A = np.empty((batch, n, n))
    for s in range(batch):
        Q1, _ = np.linalg.qr(rng.standard_normal((n, n)))
        Q2, _ = np.linalg.qr(rng.standard_normal((n, n)))
        A[s] = (Q1 * np.logspace(0, -2, n)) @ Q2.T
    for norm, o in (("1", 1), ("I", np.inf)):
        got = ctx.cond_batched_blocked(_dev(ctx, A), norm).cpu().numpy()
        want = np.array([1.0 / (np.linalg.norm(A[s], o) * np.linalg.norm(np.linalg.inv(A[s]), o)) for s in range(batch)])
        assert np.all(np.abs(got - want) <= 1e-10 * want), (norm, got, want)
