"""GPU tests of the batched equilibration (include/mpf_c.h: mpf_geequ_batched, mpf_laqge_batched, mpf_lascl2_batched, their
_batched_blocked and _vbatched siblings; csrc/batched_equil.hip) and of the Python drivers gesvx_batched, gesvx_batched_blocked and
VBatch.gesvx.

Every comparison is of bits against tests/batched_equil_model.py, a NaN comparing equal to a NaN: every product is a product with a
power of two and every extreme an order-free maximum, so there is nothing to tolerate.  Outputs are pre-filled with a sentinel NaN that
no computation here produces, so "not written" is checked, not assumed.  Inputs: the model's family, one batch slot per kind
(well-scaled, rows / columns / both scaled by 2^+-40, times 2^-1000, subnormal entries, a zero row, a zero column, a NaN, an Inf).
The orders are the seams of the kernel forms: 8 / 16 / 32 lanes per matrix, the workgroup forms up to 64 and 128, the spread forms'
tiles of 64 rows and 16 columns, and the launch groups of a descriptor."""
import ctypes as C
import functools

import numpy as np
import pytest

import batched_equil_model as EQ
from test_gpu_batched_refine import _err, _padded, _same

pytestmark = pytest.mark.gpu

SMALL_ORDERS = [1, 2, 7, 8, 9, 16, 17, 32, 33, 64, 65, 128]
BLOCKED_ORDERS = [129, 255, 256, 257]
MIN0_ORDERS = [1, 31, 33, 128]
# a descriptor: order 0, and one order on each side of every class top (8 .. 128), group top (256, 512) and expert launch group top
DESC_ORDERS = [0, 1, 8, 9, 16, 17, 32, 33, 48, 49, 64, 65, 96, 97, 128, 129, 256, 257, 512, 513, 1024]
SENT = np.array([0xFFF8DEADBEEF0001], dtype=np.uint64).view(np.float64)[0]
SENT_I = int(np.array([SENT]).view(np.int64)[0])
SENT_32 = -77


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _sent(ctx, *shape):
    import torch
    return torch.full(shape, SENT_I, dtype=torch.int64, device=ctx.device).view(torch.float64)


def _sent32(ctx, n):
    import torch
    return torch.full((n,), SENT_32, dtype=torch.int32, device=ctx.device)


def _bits(t):
    return t.cpu().contiguous().numpy().view(np.int64) if t.dtype.is_floating_point else t.cpu().numpy()


def _eq_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _fill(v, shape):
    """The model's value, or the sentinel where the contract writes nothing."""
    return np.full(shape, SENT) if v is None else np.asarray(v, dtype=np.float64).reshape(shape)


def _same_s(got, want):
    """_same, the sentinel NaN compared by its bits."""
    got = got.cpu().numpy()
    want = np.asarray(want, dtype=np.float64)
    s = want.view(np.int64) == SENT_I
    return got.shape == want.shape and np.array_equal(got.view(np.int64) == SENT_I, s) and _same(np.where(s, 0.0, got), np.where(s, 0.0, want))


@functools.lru_cache(maxsize=None)
def _family(n, kinds=tuple(EQ.KINDS)):
    fam = EQ.family(n, kinds=list(kinds))
    fam.setflags(write=False)
    return fam, tuple(EQ.geequ(A) for A in fam)


def _want_geequ(eqs, n):
    return [np.stack([_fill(e[k], (n,)) for e in eqs]) for k in (0, 1)] + [np.array([_fill(e[k], ()) for e in eqs]) for k in (2, 3, 4)] + \
        [np.array([e[5] for e in eqs], dtype=np.int32)]


def _geequ_raw(ctx, entry, view, n, batch):
    """The C entry on a (possibly padded) view, every output pre-filled with the sentinel."""
    r, c = _sent(ctx, batch, n), _sent(ctx, batch, n)
    rowcnd, colcnd, amax, info = _sent(ctx, batch), _sent(ctx, batch), _sent(ctx, batch), _sent32(ctx, batch)
    lda, stride = ctx._batch_layout(view)
    rc = getattr(ctx.L, "mpf_" + entry)(ctx.h, p(view), lda, stride, n, batch, p(r), p(c), p(rowcnd), p(colcnd), p(amax), p(info))
    assert rc == 0, _err(ctx)
    return r, c, rowcnd, colcnd, amax, info


def _check_geequ(ctx, entry, n, kinds=tuple(EQ.KINDS)):
    fam, eqs = _family(n, kinds)
    buf, view = _padded(ctx, fam)
    before = buf.clone()
    got = _geequ_raw(ctx, entry, view, n, fam.shape[0])
    for g, w, name in zip(got[:5], _want_geequ(eqs, n), ("r", "c", "rowcnd", "colcnd", "amax")):
        assert _same_s(g, w), (entry, n, name)
    assert np.array_equal(got[5].cpu().numpy(), _want_geequ(eqs, n)[5]), (entry, n)
    assert _eq_bits(buf, before)
    return got


class _min_n:
    """batched_blocked_min_n = 0 for a scope: every order through the spread kernels."""
    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.saved = self.ctx.get_option("batched_blocked_min_n")
        self.ctx.set_option("batched_blocked_min_n", 0)

    def __exit__(self, *a):
        self.ctx.set_option("batched_blocked_min_n", self.saved)


# ---- 1. geequ ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SMALL_ORDERS)
def test_geequ_small(ctx, n):
    _check_geequ(ctx, "geequ_batched", n)


@pytest.mark.parametrize("n", BLOCKED_ORDERS)
def test_geequ_blocked(ctx, n):
    _check_geequ(ctx, "geequ_batched_blocked", n)


def test_geequ_blocked_1024(ctx):
    _check_geequ(ctx, "geequ_batched_blocked", 1024, ("both", "zero_col"))


@pytest.mark.parametrize("n", MIN0_ORDERS)
def test_geequ_blocked_kernels_at_small_orders_equal_the_small_entry(ctx, n):
    small = _check_geequ(ctx, "geequ_batched", n)
    with _min_n(ctx):
        spread = _check_geequ(ctx, "geequ_batched_blocked", n)
    for a, b in zip(small, spread):
        assert _eq_bits(a, b)


# ---- 2. laqge ------------------------------------------------------------------------------------------------------------------------------
def _check_laqge(ctx, suffix, n, kinds=tuple(EQ.KINDS)):
    import torch
    fam, eqs = _family(n, kinds)
    batch = fam.shape[0]
    dev = [torch.from_numpy(np.ascontiguousarray(np.nan_to_num(w, nan=0.0) if i < 5 else w)).to(ctx.device) for i, w in enumerate(_want_geequ(eqs, n))]
    # (the sentinel NaN of unwritten entries replaced by 0: a flagged matrix's scales must not be looked at, whatever they hold)
    for rule in (0, 1, 2):
        models = [EQ.laqge(A, e, rule) for A, e in zip(fam, eqs)]
        # out of place through the Python method, on a padded input
        buf, view = _padded(ctx, fam)
        As, equed, spread = getattr(ctx, "laqge_batched" + suffix)(view, *dev, rule=rule)
        assert As.data_ptr() != view.data_ptr()
        assert _same(As, np.stack([m[0] for m in models])), (suffix, n, rule)
        assert np.array_equal(equed.cpu().numpy(), np.array([m[1] for m in models], dtype=np.int32)), (suffix, n, rule)
        assert _same(spread, np.stack([m[2] for m in models])), (suffix, n, rule)
        # in place through the C entry: the padding and the matrices that are not scaled keep their bytes
        before = buf.clone()
        eq2, sp2 = _sent32(ctx, batch), _sent(ctx, batch, 2)
        lda, stride = ctx._batch_layout(view)
        rc = getattr(ctx.L, "mpf_laqge_batched" + suffix)(ctx.h, rule, p(view), lda, stride, n, batch, *[p(d) for d in dev], p(view), p(eq2), p(sp2))
        assert rc == 0, _err(ctx)
        assert _same(view, np.stack([m[0] for m in models])) and _eq_bits(eq2, equed) and _eq_bits(sp2, spread)
        pad = torch.ones_like(buf, dtype=torch.bool)
        pad[:, :n, :n] = False
        assert _eq_bits(buf[pad], before[pad])
        for b, m in enumerate(models):
            if m[1] == 0:
                assert _eq_bits(view[b], before[b, :n, :n])
    rc = getattr(ctx.L, "mpf_laqge_batched" + suffix)(ctx.h, 3, p(view), lda, stride, n, batch, *[p(d) for d in dev], p(view), p(eq2), p(sp2))
    assert rc == -1 and "rule must be 0, 1 or 2" in _err(ctx)


@pytest.mark.parametrize("n", SMALL_ORDERS)
def test_laqge_small(ctx, n):
    _check_laqge(ctx, "", n)


@pytest.mark.parametrize("n", BLOCKED_ORDERS)
def test_laqge_blocked(ctx, n):
    _check_laqge(ctx, "_blocked", n)


def test_laqge_blocked_1024(ctx):
    _check_laqge(ctx, "_blocked", 1024, ("both", "zero_col"))


@pytest.mark.parametrize("n", MIN0_ORDERS)
def test_laqge_blocked_kernels_at_small_orders(ctx, n):
    with _min_n(ctx):
        _check_laqge(ctx, "_blocked", n)


# ---- 3. lascl2 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,suffix", [(n, "") for n in (1, 7, 33, 128)] + [(129, "_blocked"), (257, "_blocked")])
def test_lascl2(ctx, n, suffix):
    import torch
    batch, nrhs = 6, 3
    rng = np.random.default_rng(40 + n)
    s = np.ldexp(1.0, rng.integers(-50, 50, (batch, n)))
    V = rng.standard_normal((batch, n, nrhs))
    equed = np.array([0, 1, 2, 3, 1, 2], dtype=np.int32)
    sd, qd = torch.from_numpy(s).to(ctx.device), torch.from_numpy(equed).to(ctx.device)
    for bit in (1, 2):
        want = np.stack([EQ.lascl2(s[b], V[b], int(equed[b]), bit) for b in range(batch)])
        buf, view = _padded(ctx, V)
        before = buf.clone()
        out = getattr(ctx, "lascl2_batched" + suffix)(sd, view, qd, bit, overwrite=True)
        assert out.data_ptr() == view.data_ptr() and _same(view, want)
        pad = torch.ones_like(buf, dtype=torch.bool)
        pad[:, :n, :nrhs] = False
        assert _eq_bits(buf[pad], before[pad])
        for b in range(batch):
            if not equed[b] & bit:
                assert _eq_bits(view[b], before[b, :n, :nrhs])
        new = getattr(ctx, "lascl2_batched" + suffix)(sd, torch.from_numpy(V).to(ctx.device), qd, bit)     # a copy, any layout
        assert _same(new, want)
    every = getattr(ctx, "lascl2_batched" + suffix)(sd, torch.from_numpy(V[:, :, 0].copy()).to(ctx.device))  # equed None, one column
    assert _same(every, s * V[:, :, 0])


# ---- descriptors: 1 - 3 and the path independence of 4 in one mixed list --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _desc_mats(limit):
    orders = [n for n in DESC_ORDERS if n <= limit]
    rng = np.random.default_rng(77)
    mats = []
    for i, n in enumerate(orders):
        mats.append(np.zeros((0, 0)) if n == 0 else EQ.member(EQ.KINDS[i % len(EQ.KINDS)], n, rng))
    order = rng.permutation(len(mats))                      # the list is not in ascending order of n
    return tuple(mats[i] for i in order)


@pytest.mark.parametrize("blocked", [False, True])
def test_descriptor(ctx, blocked):
    import torch
    mats = _desc_mats(1024 if blocked else 128)
    ns = np.array([M.shape[0] for M in mats], dtype=np.int32)
    ld = ns.astype(np.int64) + 2
    off = np.concatenate([[5], 5 + np.cumsum(ld * ns + 3)[:-1]]).astype(np.int64)
    vb = (ctx.vbatch_blocked if blocked else ctx.vbatch)(ns, ld, off)
    A = vb.pack(mats, fill=SENT)
    before = A.clone()
    tn, batch = vb.total_n, vb.batch
    for rule in (1, 2, 0):
        wr, wc, wrow, wcol, wamax, winfo, wout, wequed, wspread = EQ.descriptor(mats, rule, fill=SENT)
        r, c = _sent(ctx, tn), _sent(ctx, tn)
        rowcnd, colcnd, amax, info = _sent(ctx, batch), _sent(ctx, batch), _sent(ctx, batch), _sent32(ctx, batch)
        rc = ctx.L.mpf_geequ_vbatched(ctx.h, vb.h, p(A), p(r), p(c), p(rowcnd), p(colcnd), p(amax), p(info))
        assert rc == 0, _err(ctx)
        for g, w, name in ((r, wr, "r"), (c, wc, "c"), (rowcnd, wrow, "rowcnd"), (colcnd, wcol, "colcnd"), (amax, wamax, "amax")):
            assert _same_s(g, w), (blocked, name)
        assert np.array_equal(info.cpu().numpy(), winfo)
        assert _eq_bits(A, before)
        # laqge out of place (the Python method), then in place (the C entry) with the fill bytes watched
        clean = [torch.nan_to_num(t, nan=0.0) for t in (r, c, rowcnd, colcnd, amax)]
        As, equed, spread = vb.laqge(A, *clean, info, rule=rule)
        for b, M in enumerate(vb.unpack(As)):
            assert _same(M, wout[b]), (blocked, rule, b)
        assert np.array_equal(equed.cpu().numpy(), wequed) and _same(spread, wspread)
        work = A.clone()
        eq2, sp2 = _sent32(ctx, batch), _sent(ctx, batch, 2)
        rc = ctx.L.mpf_laqge_vbatched(ctx.h, vb.h, rule, p(work), *[p(t) for t in clean], p(info), p(work), p(eq2), p(sp2))
        assert rc == 0, _err(ctx)
        assert _eq_bits(eq2, equed) and _eq_bits(sp2, spread)
        inside = torch.zeros(work.numel(), dtype=torch.bool, device=ctx.device)
        for b, M in enumerate(vb.unpack(work)):
            assert _same(M, wout[b])
            if ns[b]:
                vb.unpack(inside)[b].fill_(True)
            if wequed[b] == 0:
                assert _eq_bits(M, vb.unpack(before)[b])
        assert _eq_bits(work[~inside], before[~inside])
    # lascl2 on the tall right-hand sides
    rng = np.random.default_rng(5)
    s = np.ldexp(1.0, rng.integers(-50, 50, tn))
    V = rng.standard_normal((tn, 3))
    equed = (np.arange(batch) % 4).astype(np.int32)
    sd, qd = torch.from_numpy(s).to(ctx.device), torch.from_numpy(equed).to(ctx.device)
    for bit in (1, 2):
        want = V.copy()
        for b in range(batch):
            rows = slice(int(vb.offv[b]), int(vb.offv[b]) + int(ns[b]))
            want[rows] = EQ.lascl2(s[rows], V[rows], int(equed[b]), bit)
        assert _same(vb.lascl2(sd, torch.from_numpy(V).to(ctx.device), qd, bit), want)
    assert _same(vb.lascl2(sd, torch.from_numpy(V[:, 0].copy()).to(ctx.device)), s * V[:, 0])
    vb.close()


# ---- 4. a matrix's results do not depend on its position or its neighbours ------------------------------------------------------------------
@pytest.mark.parametrize("n,suffix", [(7, ""), (33, ""), (129, "_blocked")])
def test_position_and_neighbours(ctx, n, suffix):
    import torch
    fam, _ = _family(n)
    perm = np.random.default_rng(n).permutation(fam.shape[0])
    other = np.concatenate([fam[perm], EQ.family(n, seed=1)])       # shuffled, among new neighbours
    geequ, laqge = getattr(ctx, "geequ_batched" + suffix), getattr(ctx, "laqge_batched" + suffix)
    a = geequ(torch.from_numpy(np.array(fam)).to(ctx.device))
    b = geequ(torch.from_numpy(other).to(ctx.device))
    for x, y in zip(a, b):
        assert _eq_bits(x[perm], y[:len(perm)])
    sa = laqge(torch.from_numpy(np.array(fam)).to(ctx.device), *a, rule=2)
    sb = laqge(torch.from_numpy(other).to(ctx.device), *b, rule=2)
    for x, y in zip(sa, sb):
        assert _eq_bits(x[perm], y[:len(perm)])


# ---- 5. the drivers are the chain of the existing entries on the model-scaled system ---------------------------------------------------------
def _rhs(fam, nrhs, seed):
    return np.random.default_rng(seed).standard_normal((fam.shape[0], fam.shape[1], nrhs))


@pytest.mark.parametrize("n,suffix", [(7, ""), (33, ""), (128, ""), (129, "_blocked")])
def test_gesvx_is_the_chain_of_the_existing_entries(ctx, n, suffix):
    import torch
    fam, eqs = _family(n)
    B = _rhs(fam, 2, n)
    dev = lambda a: torch.from_numpy(np.array(a, order="C")).to(ctx.device)         # noqa: E731
    for trans in (False, True):
        for rule in (1, 2):
            got = getattr(ctx, "gesvx_batched" + suffix)(dev(fam), dev(B), trans=trans, equilibrate=rule)
            models = [EQ.laqge(A, e, rule) for A, e in zip(fam, eqs)]
            As = np.stack([m[0] for m in models])
            Bs = np.stack([EQ.lascl2(e[1] if trans else e[0], B[b], m[1], 2 if trans else 1) for b, (e, m) in enumerate(zip(eqs, models))])
            X, rcond, ferr, berr, info = getattr(ctx, "solvex_batched" + suffix)(dev(As), dev(Bs), trans=trans)
            X, ferr = X.cpu().numpy(), ferr.cpu().numpy()
            Xw = np.stack([EQ.lascl2(e[0] if trans else e[1], X[b], m[1], 1 if trans else 2) for b, (e, m) in enumerate(zip(eqs, models))])
            with np.errstate(all="ignore"):
                fw = ferr * np.array([m[2][0 if trans else 1] for m in models])[:, None]
            assert _same(got[0], Xw) and _same(got[2], fw), (n, trans, rule)
            assert _eq_bits(got[1], rcond) and _eq_bits(got[3], berr) and _eq_bits(got[4], info)
            assert np.array_equal(got[5].cpu().numpy(), np.array([m[1] for m in models], dtype=np.int32))
        plain = getattr(ctx, "solvex_batched" + suffix)(dev(fam), dev(B), trans=trans)
        got = getattr(ctx, "gesvx_batched" + suffix)(dev(fam), dev(B), trans=trans, equilibrate=0)
        for x, y in zip(got[:5], plain):
            assert _eq_bits(x, y)
        assert not got[5].any()


def test_descriptor_gesvx_is_the_chain_of_the_existing_entries(ctx):
    import torch
    mats = [M for M in _desc_mats(1024) if M.shape[0] <= 257]
    ns = np.array([M.shape[0] for M in mats], dtype=np.int32)
    vb = ctx.vbatch_blocked(ns)
    A = vb.pack(mats)
    B = np.random.default_rng(9).standard_normal((vb.total_n, 2))
    Bd = ctx.colmajor(vb.total_n, 2)
    Bd.copy_(torch.from_numpy(B))
    rows = [slice(int(vb.offv[b]), int(vb.offv[b]) + int(ns[b])) for b in range(vb.batch)]
    for trans in (False, True):
        got = vb.gesvx(A, Bd, trans=trans, equilibrate=1)
        _, _, _, _, _, _, wout, wequed, wspread = EQ.descriptor(mats, 1)
        eqs = [EQ.geequ(M) for M in mats]
        Bs = B.copy()
        for b, e in enumerate(eqs):
            Bs[rows[b]] = EQ.lascl2(e[1] if trans else e[0], B[rows[b]], int(wequed[b]), 2 if trans else 1)
        Bsd = ctx.colmajor(vb.total_n, 2)
        Bsd.copy_(torch.from_numpy(Bs))
        X, rcond, ferr, berr, info = vb.solvex(vb.pack(wout), Bsd, trans=trans)
        Xw = X.cpu().numpy()
        for b, e in enumerate(eqs):
            Xw[rows[b]] = EQ.lascl2(e[0] if trans else e[1], Xw[rows[b]], int(wequed[b]), 1 if trans else 2)
        with np.errstate(all="ignore"):
            fw = ferr.cpu().numpy() * wspread[:, 0 if trans else 1][:, None]
        assert _same(got[0], Xw) and _same(got[2], fw)
        assert _eq_bits(got[1], rcond) and _eq_bits(got[3], berr) and _eq_bits(got[4], info)
        assert np.array_equal(got[5].cpu().numpy(), wequed)
        for x, y in zip(vb.gesvx(A, Bd, trans=trans, equilibrate=0)[:5], vb.solvex(A, Bd, trans=trans)):
            assert _eq_bits(x, y)
    vb.close()


# ---- 6. the reason for the feature -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 33, 129])
def test_equilibration_undoes_a_row_scaling_exactly(ctx, n):
    """D = diag(2^k), k in [-40, 40] with both ends present (n >= 2), A0 well-scaled.  With equilibrate = 2 the row factors absorb D
    exactly, so gesvx(D A0, D B) returns gesvx(A0, B)'s bits, rcond included, while the plain rcond of D A0 is at most 2^-60:
    ||D A0||_1 >= 2^39 and ||(D A0)^-1||_1 >= 2^40 / n, so kappa_1 >= 2^69 for n <= 1024, nine bits of margin for the rounding of the
    computed inverse.  (The bound needs both ends of the scale, so it is asserted for n >= 2.)"""
    import torch
    suffix = "_blocked" if n > 128 else ""
    rng = np.random.default_rng(600 + n)
    batch = 3
    A0 = np.stack([EQ.well_scaled(n, rng) for _ in range(batch)])
    B = rng.standard_normal((batch, n, 2))
    D = np.stack([EQ.pow2_diag(n, rng) for _ in range(batch)])
    dev = lambda a: torch.from_numpy(np.array(a, order="C")).to(ctx.device)         # noqa: E731
    gesvx = getattr(ctx, "gesvx_batched" + suffix)
    a = gesvx(dev(A0), dev(B), equilibrate=2)
    b = gesvx(dev(D[:, :, None] * A0), dev(D[:, :, None] * B), equilibrate=2)
    for k in range(5):                                               # X, rcond, ferr, berr, info
        assert _eq_bits(a[k], b[k]), (n, k)
    assert _eq_bits(a[7], b[7]) and not a[4].any()                   # c; every matrix was factored
    plain = getattr(ctx, "cond_batched" + suffix)(dev(D[:, :, None] * A0))
    print(f"n = {n}: rcond equilibrated {a[1].cpu().numpy()}, plain {plain.cpu().numpy()}")
    assert (a[1] > 2.0 ** -30).all()
    if n >= 2:
        assert (plain <= 2.0 ** -60).all()


# ---- 7. refusals, empty cases, the Python surface ----------------------------------------------------------------------------------------------
def test_argument_errors_and_empty_cases(ctx):
    import torch
    L, h = ctx.L, ctx.h
    n, batch = 4, 3
    A = ctx.colmajor_batch(batch, n, n).fill_(1.0)
    out = ctx.colmajor_batch(batch, n, n)
    v, w = torch.ones(batch * n, dtype=torch.float64, device=ctx.device), torch.ones(batch * 2, dtype=torch.float64, device=ctx.device)
    i32 = torch.zeros(batch, dtype=torch.int32, device=ctx.device)
    geequ = lambda e, nn, bb, lda=n, st=n * n: getattr(L, e)(h, p(A), lda, st, nn, bb, p(v), p(v), p(w), p(w), p(w), p(i32))   # noqa: E731
    assert geequ("mpf_geequ_batched", 129, 1) == -1 and "n > 128 is not a small matrix" in _err(ctx)
    assert geequ("mpf_geequ_batched_blocked", 1025, 1) == -1 and "n > 1024" in _err(ctx) and "mpf_factor_dev" in _err(ctx)
    assert geequ("mpf_geequ_batched", -1, 1) == -1 and geequ("mpf_geequ_batched", n, -1) == -1
    assert geequ("mpf_geequ_batched", n, batch, lda=n - 1) == -1 and "leading dimension of A < n" in _err(ctx)
    assert geequ("mpf_geequ_batched", n, batch, st=n * n - 1) == -1 and "stride of A" in _err(ctx)
    assert L.mpf_geequ_batched(h, None, n, n * n, n, batch, p(v), p(v), p(w), p(w), p(w), p(i32)) == -1 and "null pointer" in _err(ctx)
    assert geequ("mpf_geequ_batched", 0, batch) == 0 and geequ("mpf_geequ_batched_blocked", n, 0) == 0
    laq = lambda e, rule, nn, o: getattr(L, e)(h, rule, p(A), n, n * n, nn, batch, p(v), p(v), p(w), p(w), p(w), p(i32), o, p(i32), None)   # noqa: E731
    assert laq("mpf_laqge_batched", 3, n, p(out)) == -1 and laq("mpf_laqge_batched", -1, n, p(out)) == -1
    assert laq("mpf_laqge_batched", 1, 129, p(out)) == -1 and laq("mpf_laqge_batched_blocked", 1, 1025, p(out)) == -1
    assert laq("mpf_laqge_batched", 1, n, C.c_void_p(A.data_ptr() + 8)) == -1 and "overlaps" in _err(ctx)
    assert laq("mpf_laqge_batched", 1, n, None) == -1 and laq("mpf_laqge_batched", 1, 0, p(out)) == 0
    Vt = ctx.colmajor_batch(batch, n, 2).fill_(1.0)
    las = lambda e, nn, nrhs, ldv=n: getattr(L, e)(h, p(v), nn, batch, nrhs, p(Vt), ldv, 2 * n, None, 0)   # noqa: E731
    assert las("mpf_lascl2_batched", 129, 2) == -1 and las("mpf_lascl2_batched_blocked", 1025, 2) == -1
    assert las("mpf_lascl2_batched", n, -1) == -1 and las("mpf_lascl2_batched", n, 2, ldv=n - 1) == -1
    assert las("mpf_lascl2_batched", n, 0) == 0 and las("mpf_lascl2_batched", 0, 2) == 0
    # descriptors: another context's descriptor is refused by vb_enter like everywhere; an empty descriptor and order 0 do no work
    vb = ctx.vbatch(np.array([0, 0], dtype=np.int32))
    r, c, rowcnd, colcnd, amax, info = vb.geequ(torch.zeros(1, dtype=torch.float64, device=ctx.device))
    assert r.numel() == 0 and (rowcnd == 1).all() and (colcnd == 1).all() and (amax == 0).all() and not info.any()
    assert L.mpf_geequ_vbatched(h, None, None, None, None, None, None, None, None) == -1
    assert L.mpf_laqge_vbatched(h, vb.h, 3, None, None, None, p(w), p(w), p(w), p(i32), None, p(i32), None) == -1
    assert L.mpf_lascl2_vbatched(h, vb.h, None, -1, None, 1, None, 0) == -1
    vb.close()
    empty = ctx.vbatch(np.zeros(0, dtype=np.int32))
    assert L.mpf_geequ_vbatched(h, empty.h, None, None, None, None, None, None, None) == 0
    empty.close()


def test_python_surface(ctx, mpf):
    import torch
    for name in ("geequ", "laqge", "lascl2", "gesvx"):
        assert hasattr(ctx, name + "_batched") and hasattr(ctx, name + "_batched_blocked") and hasattr(mpf.VBatch, name)
    fam, _ = _family(5)
    A = torch.from_numpy(np.array(fam)).to(ctx.device)
    B = torch.ones((fam.shape[0], 5), dtype=torch.float64, device=ctx.device)                 # one right-hand side each
    X, rcond, ferr, berr, info, equed, r, c = ctx.gesvx_batched(A, B)
    assert X.shape == B.shape and rcond.shape == (fam.shape[0],) and ferr.shape == berr.shape == (fam.shape[0], 1)
    assert equed.dtype == torch.int32 and r.shape == c.shape == (fam.shape[0], 5)
    assert torch.equal(torch.from_numpy(np.array(fam)).to(ctx.device).view(torch.int64), A.view(torch.int64))   # the inputs are left alone
