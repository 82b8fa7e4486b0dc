"""GPU tests of the expert layer for matrices of different orders (include/mpf_c.h: mpf_lange_vbatched, mpf_gecon_vbatched,
mpf_residual_vbatched, mpf_gerfs_vbatched on a descriptor of either kind; csrc/vbatched_refine.hip, csrc/batched_refine_blocked_body.h,
csrc/vbatch_plan.h: refine_chunks).

Every comparison is of bits, with no tolerance: the contract is that every output of matrix b is what the fixed-size BLOCKED expert
entry returns for that matrix alone (and, for n <= 128, what the small expert entry returns), so the yardsticks are those entries, each
called on one matrix, and for the orders up to 65 tests/batched_refine_blocked_model.py directly.

Inputs: batched_refine_blocked_model.family -- stale factors LU = getrf(A + 2^-k E), refinement against A, X0 = getrs of B, the last of
the five columns exact (b = column j of op(A), x0 = e_j) -- two slots of the family per order, so that the descriptor as a whole
reaches every stop reason.  The sizes are the seams of the kernels, not workloads: the chain tile (16), the sweep block (32), the wave
and the first top (64), the tops 128 and 256, and in a test of its own the last top (1024)."""
import ctypes as C
import functools

import numpy as np
import pytest

import batched_refine_blocked_model as RB
import batched_refine_model as R
from test_gpu_batched_refine import _dev, _err, _same

pytestmark = pytest.mark.gpu

ORDERS = [0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257]
MODEL_UPTO = 65
NRHS = RB.NRHS
ALL_STOPS = {"berr <= eps", "not halved", "itmax"}
SENT = np.array([0xFFF8DEADBEEF0001], dtype=np.uint64).view(np.float64)[0]     # a NaN no computation here produces
SENT_I = int(np.array([SENT]).view(np.int64)[0])
BLOCKED, SMALL = "_batched_blocked", "_batched"


def _teq(a, b):
    import torch
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)))


def _sentinel(ctx, count):
    import torch
    return torch.full((max(count, 1),), SENT_I, dtype=torch.int64, device=ctx.device).view(torch.float64)


def _is_sentinel(t):
    import torch
    return t.contiguous().view(torch.int64) == SENT_I


def _rows(vb, b):
    return slice(int(vb.offv[b]), int(vb.offv[b]) + int(vb.n[b]))


def _col1(c, T):
    """A packed column-major (1, rows, cols) batch holding the 2-d device tensor T."""
    W = c.colmajor_batch(1, *T.shape)
    W[0].copy_(T)
    return W


@functools.lru_cache(maxsize=None)
def _family(n):
    return RB.family(n)


@functools.lru_cache(maxsize=None)
def _items(orders):
    """Two slots of the family per order (different perturbations of the factors), in a fixed shuffled order.  [(n, slot)]."""
    items = [(n, (i + 3 * j) % len(RB.KS)) for i, n in enumerate(orders) for j in (0, 1)]
    order = np.random.default_rng(2026).permutation(len(items))
    return tuple(items[i] for i in order)


def _tall(c, vb, cols):
    """The column-major (total_n, nrhs) device tensor whose rows offv[b] .. are cols[b] (n[b], nrhs)."""
    import torch
    nrhs = next(v.shape[1] for v in cols if v.shape[0])
    T = c.colmajor(vb.total_n, nrhs)
    T.copy_(torch.from_numpy(np.concatenate([np.asarray(v).reshape(-1, nrhs) for v in cols], axis=0)))
    return T


def _build(c, vb, items, mats=None, stale=None, rhs=None):
    """Everything the comparisons share for one descriptor, computed once and left unchanged: the matrices and the factors of the
    stale matrices (VBatch.getrf), per trans the right-hand sides and first solutions with the exact last column, and per matrix the
    packed single-matrix batches the fixed-size entries take."""
    import torch
    if mats is None:
        mats = [_family(n)[0][s] if n else np.zeros((0, 0)) for n, s in items]
        stale = [_family(n)[1][s] if n else np.zeros((0, 0)) for n, s in items]
        rhs = [_family(n)[2][s] if n else np.zeros((0, NRHS)) for n, s in items]
    A = vb.pack(mats)
    LU, ipiv, info = vb.getrf(vb.pack(stale))
    assert not bool(info.any())
    B0 = _tall(c, vb, rhs)
    dB, dX0, hB, hX0 = {}, {}, {}, {}
    for t in (0, 1):
        X0 = vb.getrs(LU, ipiv, B0, trans=bool(t)).cpu().numpy().copy()
        Bx = B0.cpu().numpy().copy()
        for b, (n, _) in enumerate(items):
            if n:
                Bx[_rows(vb, b), -1], X0[_rows(vb, b), -1] = RB.exact_column(mats[b], bool(t))
        hB[t], hX0[t] = Bx, X0
        dB[t], dX0[t] = _tall(c, vb, [Bx]), _tall(c, vb, [X0])
    views = vb.unpack(LU)
    alone = [(_dev(c, mats[b][None]), _col1(c, views[b]), ipiv[_rows(vb, b)].view(1, n).contiguous()) if n else None
             for b, (n, _) in enumerate(items)]
    host = dict(LU=[v.cpu().numpy() for v in views], ipiv=ipiv.cpu().numpy())
    keep = [x.clone() for x in (A, LU, ipiv)]
    return dict(vb=vb, items=items, mats=mats, A=A, LU=LU, ipiv=ipiv, dB=dB, dX0=dX0, hB=hB, hX0=hX0, alone=alone, host=host, keep=keep)


def _unchanged(d):
    import torch
    return all(bool(torch.equal(a, k)) if a.dtype == torch.int32 else _teq(a, k) for a, k in zip((d["A"], d["LU"], d["ipiv"]), d["keep"]))


def _check_norms_and_rcond(c, d, suffix, model_upto=MODEL_UPTO):
    vb, items = d["vb"], d["items"]
    for norm in ("1", "O", "I", "M"):
        got = vb.lange(d["A"], norm)
        for b, (n, _) in enumerate(items):
            if n == 0:
                assert float(got[b]) == 0.0
                continue
            assert _teq(got[b:b + 1], getattr(c, "lange" + suffix)(d["alone"][b][0], norm)), (n, norm)
            if n <= model_upto:
                assert _same(got[b:b + 1], [RB.lange_model(d["mats"][b], norm)]), (n, norm)
    for norm in ("1", "I"):
        anorm = vb.lange(d["A"], norm)
        rcond, ainv = vb.gecon(d["LU"], anorm, norm, want_ainvnm=True)
        assert _teq(vb.gecon(d["LU"], anorm, norm), rcond)                       # (and without d_ainvnm)
        an = anorm.cpu().numpy()
        for b, (n, _) in enumerate(items):
            if n == 0:
                assert (float(rcond[b]), float(ainv[b])) == (1.0, 0.0)
                continue
            rf, af = getattr(c, "gecon" + suffix)(d["alone"][b][1], anorm[b:b + 1], norm, want_ainvnm=True)
            assert _teq(rcond[b:b + 1], rf) and _teq(ainv[b:b + 1], af) and float(rf[0]) > 0, (n, norm)
            if n <= model_upto:
                rm, am = RB.gecon_model(d["host"]["LU"][b], an[b], norm)
                assert _same(rcond[b:b + 1], [rm]) and _same(ainv[b:b + 1], [am]), (n, norm)
    assert _unchanged(d)


_MODEL = {}


def _model_columns(d, b, trans, itmax, nrhs):
    """The model's (X, ferr, berr, iters, stops) for the first nrhs columns of family matrix b.  A column's result depends on nothing
    but the column (and every descriptor here leaves the same factors for a slot of the family), so each is computed once."""
    vb, (n, slot) = d["vb"], d["items"][b]
    LU, ipiv = d["host"]["LU"][b], d["host"]["ipiv"][_rows(vb, b)]
    if (n, slot, trans) not in _MODEL:
        _MODEL[(n, slot, trans)] = R.inverse_rows(LU, ipiv, bool(trans))
    rows, cols = _MODEL[(n, slot, trans)], []
    for k in range(nrhs):
        key = (n, slot, trans, itmax, k)
        if key not in _MODEL:
            _MODEL[key] = RB.gerfs_column(d["mats"][b], LU, ipiv, d["hB"][trans][_rows(vb, b), k], d["hX0"][trans][_rows(vb, b), k],
                                          bool(trans), itmax, True, rows)
        cols.append(_MODEL[key])
    X = np.stack([c[0] for c in cols], axis=1)
    return X, np.array([c[1] for c in cols]), np.array([c[2] for c in cols]), np.array([c[3] for c in cols], dtype=np.int32), [c[4] for c in cols]


def _check_residual_and_gerfs(c, d, suffix, trans, model_upto=MODEL_UPTO, nrhs_list=(1, 3, 4, 5), itmaxes=(0, 1, 31)):
    """nrhs 1 and 3: one-column tiles; 4: one four-column tile; 5: a partial second tile.  With and without ferr."""
    vb, items = d["vb"], d["items"]
    stops = set()
    for nrhs in nrhs_list:
        Bd, Xd = d["dB"][trans][:, :nrhs], d["dX0"][trans][:, :nrhs]
        Rr, W = vb.residual(d["A"], Xd, Bd, trans=bool(trans))
        R1, W1 = vb.residual(d["A"], Xd, Bd, trans=bool(trans), want_w=False)
        assert W1 is None and _teq(R1, Rr)
        for itmax in (itmaxes if nrhs == NRHS else (0,)):
            X, ferr, berr, its = vb.gerfs(d["A"], d["LU"], d["ipiv"], Bd, Xd, trans=bool(trans), itmax=itmax)
            X2, f2, berr2, its2 = vb.gerfs(d["A"], d["LU"], d["ipiv"], Bd, Xd, trans=bool(trans), itmax=itmax, want_ferr=False)
            assert f2 is None and _teq(X2, X) and _teq(berr2, berr) and bool((its2 == its).all())
            for b, (n, _) in enumerate(items):
                if n == 0:
                    assert not bool(ferr[b].any()) and not bool(berr[b].any()) and not bool(its[b].any())
                    continue
                Ab, LUb, pb = d["alone"][b]
                Bb, Xb = Bd[_rows(vb, b)].unsqueeze(0), Xd[_rows(vb, b)].unsqueeze(0)
                if itmax == 0:
                    Rf, Wf = getattr(c, "residual" + suffix)(Ab, Xb, Bb, trans=bool(trans))
                    assert _teq(Rr[_rows(vb, b)], Rf[0]) and _teq(W[_rows(vb, b)], Wf[0]), (n, nrhs, trans)
                Xf, ff, bf, itf = getattr(c, "gerfs" + suffix)(Ab, LUb, pb, Bb, Xb, trans=bool(trans), itmax=itmax)
                assert _teq(X[_rows(vb, b)], Xf[0]), (n, nrhs, trans, itmax)
                assert _teq(ferr[b], ff[0]) and _teq(berr[b], bf[0]) and bool((its[b] == itf[0]).all()), (n, nrhs, trans, itmax)
                if n <= model_upto:
                    hB, hX = d["hB"][trans][_rows(vb, b), :nrhs], d["hX0"][trans][_rows(vb, b), :nrhs]
                    if itmax == 0:
                        rm, wm = RB.residual_model(d["mats"][b], hX, hB, bool(trans))
                        assert _same(Rr[_rows(vb, b)], rm) and _same(W[_rows(vb, b)], wm), (n, nrhs, trans)
                    Xm, fm, bm, im, st = _model_columns(d, b, trans, itmax, nrhs)
                    assert _same(X[_rows(vb, b)], Xm) and _same(ferr[b], fm) and _same(berr[b], bm), (n, nrhs, trans, itmax)
                    assert np.array_equal(its[b].cpu().numpy(), im), (n, nrhs, trans, itmax)
                    stops.update(st)
    assert _teq(d["dB"][trans], _tall(c, vb, [d["hB"][trans]])) and _teq(d["dX0"][trans], _tall(c, vb, [d["hX0"][trans]]))   # out of place
    assert _unchanged(d)
    return stops


@pytest.fixture(scope="module")
def bctx(mpf):
    """Every order through the blocked kernels in the factorization, the solve and the fixed-size expert entries alike."""
    c = mpf.MPFContext(0, options={"batched_blocked_min_n": 0})
    yield c
    c.close()


_BUILT = {}


def _mixed(kind, bctx, ctx):
    """kind 'min_n 0': vbatch_blocked on the context with batched_blocked_min_n = 0; 'default': vbatch_blocked with default options
    (its orders up to 128 are factored and solved by the small kernels, and the fixed-size blocked entries forward them there)."""
    if kind not in _BUILT:
        c = bctx if kind == "min_n 0" else ctx
        items = _items(tuple(ORDERS))
        _BUILT[kind] = (c, _build(c, c.vbatch_blocked([n for n, _ in items]), items))
    return _BUILT[kind]


# ---- 1. one mixed descriptor of either kind against the fixed-size blocked entries and the model ---------------------------------------
@pytest.mark.parametrize("kind", ["min_n 0", "default"])
def test_mixed_norms_and_rcond(bctx, ctx, kind):
    c, d = _mixed(kind, bctx, ctx)
    assert c.get_option("batched_blocked_min_n") == (0 if kind == "min_n 0" else 129)
    assert d["vb"].batch == 2 * len(ORDERS) and d["vb"].total_n == 2 * sum(ORDERS)
    _check_norms_and_rcond(c, d, BLOCKED)


@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("kind", ["min_n 0", "default"])
def test_mixed_residual_and_refinement(bctx, ctx, kind, trans):
    c, d = _mixed(kind, bctx, ctx)
    stops = _check_residual_and_gerfs(c, d, BLOCKED, trans)
    assert stops == ALL_STOPS, stops


# ---- 2. a descriptor of the small kind against the small expert entries -----------------------------------------------------------------
@pytest.fixture(scope="module")
def small(ctx):
    items = _items(tuple(n for n in ORDERS if n <= 128))
    return _build(ctx, ctx.vbatch([n for n, _ in items]), items)


def test_small_descriptor_norms_and_rcond(ctx, small):
    _check_norms_and_rcond(ctx, small, SMALL)


@pytest.mark.parametrize("trans", [0, 1])
def test_small_descriptor_residual_and_refinement(ctx, small, trans):
    assert _check_residual_and_gerfs(ctx, small, SMALL, trans) == ALL_STOPS


# ---- 3. the largest orders: the last top, tiles far outside a smaller neighbour of the launch, a small matrix beside them -------------------
def test_largest_orders(ctx):
    orders = [1023, 1024, 3, 513]
    rng = np.random.default_rng(1024 + 26)
    mats = [rng.standard_normal((n, n)) for n in orders]
    stale = [m + 2.0 ** -12 * rng.standard_normal(m.shape) for m in mats]
    rhs = [rng.standard_normal((n, NRHS)) for n in orders]
    items = tuple((n, 0) for n in orders)
    d = _build(ctx, ctx.vbatch_blocked(orders), items, mats, stale, rhs)
    _check_norms_and_rcond(ctx, d, BLOCKED, model_upto=0)
    for trans in (0, 1):
        _check_residual_and_gerfs(ctx, d, BLOCKED, trans, model_upto=0, nrhs_list=(1, 5), itmaxes=(0,))


# ---- 4. bytes that must stay untouched ----------------------------------------------------------------------------------------------------
def test_explicit_layout_leaves_every_other_byte_alone(bctx):
    import torch
    c = bctx
    n = [33, 161, 0, 129, 7, 257, 64]
    ld = [v + 3 if v else 0 for v in n]
    slots = [4, 1, 6, 0, 5, 2, 3]                            # the matrices lie in another order than the batch's, with gaps between them
    size, off = (257 + 3) * 257 + 5, [0] * len(n)
    for b, s in enumerate(slots):
        off[b] = s * size + (b % 3)
    vb = c.vbatch_blocked(n, ld, off)
    items = tuple((v, 1) for v in n)
    mats = [_family(v)[0][1] if v else np.zeros((0, 0)) for v in n]
    stale = [_family(v)[1][1] if v else np.zeros((0, 0)) for v in n]
    total = vb.extent + 4
    inside = torch.zeros(total, dtype=torch.bool, device=c.device)
    for m in vb.unpack(inside):
        m.fill_(True)

    def spread(ms):
        buf = _sentinel(c, total)
        for m, M, v in zip(vb.unpack(buf), ms, n):
            if v:
                m.copy_(torch.from_numpy(np.ascontiguousarray(M)))
        return buf
    A, LU = spread(mats), spread(stale)
    _, ipiv, info = vb.getrf(LU, overwrite=True)
    assert not bool(info.any()) and bool(_is_sentinel(LU)[~inside].all())
    views = vb.unpack(LU)
    alone = [(_dev(c, mats[b][None]), _col1(c, views[b]), ipiv[_rows(vb, b)].view(1, v).contiguous()) if v else None for b, v in enumerate(n)]
    keepA, keepLU = A.clone(), LU.clone()
    for norm in ("1", "I", "M"):
        got = vb.lange(A, norm)
        assert not bool(torch.isnan(got).any())
        for b, v in enumerate(n):
            if v:
                assert _teq(got[b:b + 1], c.lange_batched_blocked(alone[b][0], norm)), (v, norm)
    for norm in ("1", "I"):
        anorm = vb.lange(A, norm)
        rcond, ainv = vb.gecon(LU, anorm, norm, want_ainvnm=True)
        assert not bool(torch.isnan(rcond).any()) and not bool(torch.isnan(ainv).any())
        for b, v in enumerate(n):
            if v:
                rf, af = c.gecon_batched_blocked(alone[b][1], anorm[b:b + 1], norm, want_ainvnm=True)
                assert _teq(rcond[b:b + 1], rf) and _teq(ainv[b:b + 1], af), (v, norm)
    # the tall operands: leading dimension total_n + 5, the rows beyond total_n hold the sentinel
    ldt, nrhs = vb.total_n + 5, NRHS
    Bn = torch.from_numpy(np.random.default_rng(44).standard_normal((vb.total_n, nrhs))).to(c.device)

    def tall(src=None):
        buf = _sentinel(c, ldt * nrhs)
        T = buf.as_strided((vb.total_n, nrhs), (1, ldt))
        if src is not None:
            T.copy_(src)
        return buf, T
    p = lambda t: C.c_void_p(t.data_ptr())                   # noqa: E731
    c._bind()
    for trans in (0, 1):
        X0 = vb.getrs(LU, ipiv, Bn, trans=bool(trans))
        (bb, Bd), (xb, Xd), (rb, Rd), (wb, Wd) = tall(Bn), tall(X0), tall(), tall()
        rc = c.L.mpf_residual_vbatched(c.h, vb.h, trans, p(A), nrhs, p(Xd), ldt, p(Bd), ldt, p(Rd), ldt, p(Wd))
        assert rc == 0, _err(c)
        ferr, berr = torch.zeros((vb.batch, nrhs), dtype=torch.float64, device=c.device), torch.zeros((vb.batch, nrhs), dtype=torch.float64, device=c.device)
        its = torch.zeros((vb.batch, nrhs), dtype=torch.int32, device=c.device)
        rc = c.L.mpf_gerfs_vbatched(c.h, vb.h, trans, p(A), p(LU), p(ipiv), nrhs, p(Bd), ldt, p(Xd), ldt, 0, p(ferr), p(berr), p(its))
        assert rc == 0, _err(c)
        for buf in (bb, xb, rb, wb):
            assert bool(_is_sentinel(buf).view(nrhs, ldt)[:, vb.total_n:].all())
        assert _teq(Bd, Bn)
        for T in (Xd, Rd, Wd, ferr, berr):
            assert not bool(torch.isnan(T).any())
        for b, v in enumerate(n):
            if v:
                Ab, LUb, pb = alone[b]
                Bb, Xb = Bn[_rows(vb, b)].unsqueeze(0), X0[_rows(vb, b)].unsqueeze(0)
                Rf, Wf = c.residual_batched_blocked(Ab, Xb, Bb, trans=bool(trans))
                Xf, ff, bf, itf = c.gerfs_batched_blocked(Ab, LUb, pb, Bb, Xb, trans=bool(trans))
                assert _teq(Rd[_rows(vb, b)], Rf[0]) and _teq(Wd[_rows(vb, b)], Wf[0]) and _teq(Xd[_rows(vb, b)], Xf[0]), (v, trans)
                assert _teq(ferr[b], ff[0]) and _teq(berr[b], bf[0]) and bool((its[b] == itf[0]).all()), (v, trans)
        # d_R may be d_B
        (bb2, Bd2) = tall(Bn)
        (xb2, Xd2) = tall(X0)
        rc = c.L.mpf_residual_vbatched(c.h, vb.h, trans, p(A), nrhs, p(Xd2), ldt, p(Bd2), ldt, p(Bd2), ldt, None)
        assert rc == 0, _err(c)
        assert _teq(Bd2, Rd) and bool(_is_sentinel(bb2).view(nrhs, ldt)[:, vb.total_n:].all())
    assert _teq(A, keepA) and _teq(LU, keepLU)               # (the sentinels in the gaps and in rows n .. ld-1 included)


# ---- 5. singular and NaN matrices between healthy neighbours ------------------------------------------------------------------------------
def test_singular_and_nan_matrices_touch_no_neighbour(bctx):
    import torch
    c = bctx
    orders = [130, 65, 161, 40, 33, 256]
    items = tuple((n, 2) for n in orders)
    d = _build(c, c.vbatch_blocked(orders), items)
    vb = d["vb"]
    LU = d["LU"].clone()
    views = vb.unpack(LU)
    views[1][32, 32] = 0.0                                   # a zero on U's diagonal in matrices 1 and 4
    views[4][0, 0] = 0.0
    for norm in ("1", "I"):
        anorm = vb.lange(d["A"], norm)
        r0, a0 = vb.gecon(d["LU"], anorm, norm, want_ainvnm=True)
        r1, a1 = vb.gecon(LU, anorm, norm, want_ainvnm=True)
        for b in range(vb.batch):
            if b in (1, 4):
                assert float(r1[b]) == 0.0 and float(a1[b]) == float("inf"), (b, norm)
            else:
                assert _teq(r1[b:b + 1], r0[b:b + 1]) and _teq(a1[b:b + 1], a0[b:b + 1]), (b, norm)
    A = d["A"].clone()
    vb.unpack(A)[2][160, 0] = float("nan")                   # a NaN in matrix 2
    vb.unpack(A)[3][5, 7] = float("nan")                     # and in matrix 3
    for norm in ("1", "I", "M"):
        g0, g1 = vb.lange(d["A"], norm), vb.lange(A, norm)
        assert bool(torch.isnan(g1[2])) and bool(torch.isnan(g1[3]))
        keep = [0, 1, 4, 5]
        assert _teq(g1[keep], g0[keep]), norm
    for trans in (0, 1):
        Bd, Xd = d["dB"][trans], d["dX0"][trans]
        X0, f0, b0, i0 = vb.gerfs(d["A"], d["LU"], d["ipiv"], Bd, Xd, trans=bool(trans))
        X1, f1, b1, i1 = vb.gerfs(A, d["LU"], d["ipiv"], Bd, Xd, trans=bool(trans))
        for b in range(vb.batch):
            if b in (2, 3):
                assert bool(torch.isnan(b1[b]).all()) and not bool(i1[b].any()), (b, trans)
                assert _teq(X1[_rows(vb, b)], Xd[_rows(vb, b)])                  # the column stops before any correction
            else:
                assert _teq(X1[_rows(vb, b)], X0[_rows(vb, b)]) and _teq(f1[b], f0[b]) and _teq(b1[b], b0[b]) and bool((i1[b] == i0[b]).all())
                Ab, LUb, pb = d["alone"][b]
                Xf, ff, bf, itf = c.gerfs_batched_blocked(Ab, LUb, pb, Bd[_rows(vb, b)].unsqueeze(0), Xd[_rows(vb, b)].unsqueeze(0), trans=bool(trans))
                assert _teq(X1[_rows(vb, b)], Xf[0]) and _teq(f1[b], ff[0]) and _teq(b1[b], bf[0]), (b, trans)


# ---- 6. position and batch ------------------------------------------------------------------------------------------------------------------
def test_position_and_neighbours_change_no_bit(bctx):
    import torch
    c = bctx
    one_n, slot = 161, 3
    others = [(130, 0), (256, 1), (17, 2), (64, 4)]
    seen = []
    for at, more in ((0, others), (2, others[::-1]), (4, others), (1, [(161, 5), (1023, 0)])):
        items = tuple(more[:at] + [(one_n, slot)] + more[at:])
        if any(n > 257 for n, _ in items):                   # (the family's seven slots are too much numpy at 1023: one random matrix)
            rng = np.random.default_rng(61)
            mats = [_family(n)[0][s] if n <= 257 else rng.standard_normal((n, n)) for n, s in items]
            stale = [_family(n)[1][s] if n <= 257 else m for (n, s), m in zip(items, mats)]
            rhs = [_family(n)[2][s] if n <= 257 else rng.standard_normal((n, NRHS)) for n, s in items]
            d = _build(c, c.vbatch_blocked([n for n, _ in items]), items, mats, stale, rhs)
        else:
            d = _build(c, c.vbatch_blocked([n for n, _ in items]), items)
        vb = d["vb"]
        out = []
        for again in (0, 1):                                 # two calls give the same bits
            res = [vb.lange(d["A"], nm)[at:at + 1] for nm in ("1", "I", "M")]
            for nm in ("1", "I"):
                rc, ai = vb.gecon(d["LU"], vb.lange(d["A"], nm), nm, want_ainvnm=True)
                res += [rc[at:at + 1], ai[at:at + 1]]
            for trans in (0, 1):
                Rr, W = vb.residual(d["A"], d["dX0"][trans], d["dB"][trans], trans=bool(trans))
                X, fe, be, its = vb.gerfs(d["A"], d["LU"], d["ipiv"], d["dB"][trans], d["dX0"][trans], trans=bool(trans))
                res += [Rr[_rows(vb, at)], W[_rows(vb, at)], X[_rows(vb, at)], fe[at], be[at], its[at].to(torch.float64)]
            out.append([r.clone() for r in res])
        assert all(_teq(a, b) for a, b in zip(out[0], out[1]))
        seen.append(out[0])
    for other in seen[1:]:
        assert len(other) == len(seen[0]) and all(_teq(a, b) for a, b in zip(other, seen[0]))


# ---- 7. long groups ---------------------------------------------------------------------------------------------------------------------
def _gather(vb, n, v, device):
    """Index tensors of the matrices of order v: (members, matrix elements, vector elements)."""
    import torch
    off, offv = torch.from_numpy(vb.off).to(device), torch.from_numpy(vb.offv).to(device)
    mem = torch.from_numpy(np.nonzero(n == v)[0]).to(device)
    me = (off[mem][:, None] + torch.arange(v * v, device=device)[None, :]).view(-1)
    ve = (offv[mem][:, None] + torch.arange(v, device=device)[None, :]).view(-1)
    return mem, me, ve


def test_group_longer_than_one_launch(bctx):
    """2^15 + 3 matrices of orders 1 and 2 alternating, all in the first launch group: two chunks, the first with both orders.  The
    yardstick is the fixed-size blocked entry on all matrices of an order at once, whose results are each matrix's alone."""
    import torch
    c = bctx
    batch = (1 << 15) + 3
    n = np.ones(batch, dtype=np.int32)
    n[1::2] = 2
    vb = c.vbatch_blocked(n)
    nrhs = 2
    a = torch.from_numpy(np.random.default_rng(15).uniform(1.0, 2.0, vb.extent)).to(c.device)
    af = a + 2.0 ** -20 * torch.from_numpy(np.random.default_rng(17).standard_normal(vb.extent)).to(c.device)
    Bd = c.colmajor(vb.total_n, nrhs)
    Bd.copy_(torch.from_numpy(np.random.default_rng(16).standard_normal((vb.total_n, nrhs))))
    LU, ipiv, info = vb.getrf(af)
    assert not bool(info.any())
    X0 = vb.getrs(LU, ipiv, Bd)
    norms = {nm: vb.lange(a, nm) for nm in ("1", "I", "M")}
    rcond = {nm: vb.gecon(LU, norms[nm], nm, want_ainvnm=True) for nm in ("1", "I")}
    Rr, W = vb.residual(a, X0, Bd)
    X, ferr, berr, its = vb.gerfs(a, LU, ipiv, Bd, X0)
    for v in (1, 2):
        mem, me, ve = _gather(vb, n, v, c.device)
        as_batch = lambda flat: flat[me].view(-1, v, v).transpose(1, 2)                # noqa: E731  ((count, v, v) column-major)
        cols = lambda T: T[ve].view(-1, v, nrhs)                                        # noqa: E731
        Af, LUf, pf = as_batch(a), as_batch(LU), ipiv[ve].view(-1, v).contiguous()
        for nm in ("1", "I", "M"):
            assert _teq(norms[nm][mem], c.lange_batched_blocked(Af, nm)), (v, nm)
        for nm in ("1", "I"):
            rf, aif = c.gecon_batched_blocked(LUf, norms[nm][mem], nm, want_ainvnm=True)
            assert _teq(rcond[nm][0][mem], rf) and _teq(rcond[nm][1][mem], aif), (v, nm)
        Rf, Wf = c.residual_batched_blocked(Af, cols(X0), cols(Bd))
        assert _teq(cols(Rr), Rf) and _teq(cols(W), Wf), v
        Xf, ff, bf, itf = c.gerfs_batched_blocked(Af, LUf, pf, cols(Bd), cols(X0))
        assert _teq(cols(X), Xf) and _teq(ferr[mem], ff) and _teq(berr[mem], bf) and bool(torch.equal(its[mem], itf)), v


def test_refinement_whose_workspace_takes_more_than_one_chunk(ctx):
    """500 matrices of order 60 and 520 of order 64 with 512 columns: n + 1 + ceil(n / 16) doubles per (matrix, column) come to
    500 x 512 x 65 + 520 x 512 x 69 = 35.0 M doubles, more than the 2^25 = 33.6 M a chunk may use -- the first chunk ends inside the
    matrices of order 64 (after 478 of them), where neither fixed-size call (one per order, each below the limit) has a seam."""
    import torch
    c = ctx
    n = np.array([60] * 500 + [64] * 520, dtype=np.int32)
    n = n[np.random.default_rng(3).permutation(n.size)]
    nrhs = 512
    assert 512 * (500 * 65 + 520 * 69) > 1 << 25 and 512 * (500 * 65 + 478 * 69) <= 1 << 25 < 512 * (500 * 65 + 479 * 69)
    vb = c.vbatch_blocked(n)
    gen = torch.Generator(device=c.device)
    gen.manual_seed(7)
    a = torch.randn(vb.extent, dtype=torch.float64, device=c.device, generator=gen)
    af = a + 2.0 ** -30 * torch.randn(vb.extent, dtype=torch.float64, device=c.device, generator=gen)
    Bd = c.colmajor(vb.total_n, nrhs)
    Bd.copy_(torch.randn((nrhs, vb.total_n), dtype=torch.float64, device=c.device, generator=gen).t())
    LU, ipiv, info = vb.getrf(af)
    assert not bool(info.any())
    X0 = vb.getrs(LU, ipiv, Bd)
    X, ferr, berr, its = vb.gerfs(a, LU, ipiv, Bd, X0, trans=False)
    assert bool((its > 0).any()) and not bool(torch.isnan(ferr).any())
    for v in (60, 64):
        mem, me, ve = _gather(vb, n, v, c.device)
        as_batch = lambda flat: flat[me].view(-1, v, v).transpose(1, 2)                # noqa: E731
        cols = lambda T: T[ve].view(-1, v, nrhs)                                        # noqa: E731
        Xf, ff, bf, itf = c.gerfs_batched_blocked(as_batch(a), as_batch(LU), ipiv[ve].view(-1, v).contiguous(), cols(Bd), cols(X0))
        assert _teq(cols(X), Xf) and _teq(ferr[mem], ff) and _teq(berr[mem], bf) and bool(torch.equal(its[mem], itf)), v


# ---- 8. the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_refusals_and_empty_cases_through_the_c_abi(ctx, mpf):
    import torch
    L, h = ctx.L, ctx.h
    ctx._bind()
    n = [3, 0, 200, 0]
    vb = ctx.vbatch_blocked(n)
    tn, nrhs = vb.total_n, 2
    A = vb.pack([np.eye(3), np.zeros((0, 0)), np.eye(200), np.zeros((0, 0))])
    ipiv = torch.cat([torch.arange(1, v + 1, dtype=torch.int32) for v in n]).to(ctx.device)
    T = [ctx.colmajor(tn, nrhs).fill_(1.0) for _ in range(4)]
    per = [torch.full((vb.batch,), 7.0, dtype=torch.float64, device=ctx.device) for _ in range(3)]
    col = [torch.full((vb.batch * nrhs,), 7.0, dtype=torch.float64, device=ctx.device) for _ in range(2)]
    its = torch.full((vb.batch * nrhs,), 7, dtype=torch.int32, device=ctx.device)
    p = lambda t: C.c_void_p(t.data_ptr())                   # noqa: E731
    null = None
    pa, pp = p(A), p(ipiv)
    X, B, Rr, W = [p(t) for t in T]
    out, rc_, ai = [p(t) for t in per]
    fe, be = [p(t) for t in col]

    def refused(rc, text):
        assert rc < 0 and _err(ctx) == text, (rc, _err(ctx))

    refused(L.mpf_lange_vbatched(h, null, b"1", pa, out), "lange_vbatched: null pointer (descriptor)")
    refused(L.mpf_lange_vbatched(h, vb.h, b"X", pa, out), "lange_vbatched: norm must be '1', 'O', 'I' or 'M'")
    refused(L.mpf_lange_vbatched(h, vb.h, b"1", null, out), "lange_vbatched: null pointer")
    refused(L.mpf_lange_vbatched(h, vb.h, b"1", pa, null), "lange_vbatched: null pointer")
    refused(L.mpf_gecon_vbatched(h, null, b"1", pa, out, rc_, ai), "gecon_vbatched: null pointer (descriptor)")
    refused(L.mpf_gecon_vbatched(h, vb.h, b"M", pa, out, rc_, ai), "gecon_vbatched: norm must be '1', 'O' or 'I'")
    refused(L.mpf_gecon_vbatched(h, vb.h, b"1", null, out, rc_, ai), "gecon_vbatched: null pointer")
    refused(L.mpf_gecon_vbatched(h, vb.h, b"1", pa, null, rc_, ai), "gecon_vbatched: null pointer")
    refused(L.mpf_gecon_vbatched(h, vb.h, b"1", pa, out, null, ai), "gecon_vbatched: null pointer")
    refused(L.mpf_residual_vbatched(h, null, 0, pa, nrhs, X, tn, B, tn, Rr, tn, W), "residual_vbatched: null pointer (descriptor)")
    refused(L.mpf_residual_vbatched(h, vb.h, 0, pa, -1, X, tn, B, tn, Rr, tn, W), "residual_vbatched: nrhs must not be negative")
    refused(L.mpf_residual_vbatched(h, vb.h, 2, pa, nrhs, X, tn, B, tn, Rr, tn, W), "residual_vbatched: trans must be 0 or 1")
    refused(L.mpf_residual_vbatched(h, vb.h, 0, pa, nrhs, X, tn - 1, B, tn, Rr, tn, W), "residual_vbatched: leading dimension of X < total_n")
    refused(L.mpf_residual_vbatched(h, vb.h, 0, pa, nrhs, X, tn, B, tn - 1, Rr, tn, W), "residual_vbatched: leading dimension of B < total_n")
    refused(L.mpf_residual_vbatched(h, vb.h, 0, pa, nrhs, X, tn, B, tn, Rr, tn - 1, W), "residual_vbatched: leading dimension of R < total_n")
    for args in ((null, X, B, Rr), (pa, null, B, Rr), (pa, X, null, Rr), (pa, X, B, null)):
        refused(L.mpf_residual_vbatched(h, vb.h, 0, args[0], nrhs, args[1], tn, args[2], tn, args[3], tn, W), "residual_vbatched: null pointer")
    refused(L.mpf_gerfs_vbatched(h, null, 0, pa, pa, pp, nrhs, B, tn, X, tn, 0, fe, be, p(its)), "gerfs_vbatched: null pointer (descriptor)")
    refused(L.mpf_gerfs_vbatched(h, vb.h, 0, pa, pa, pp, -1, B, tn, X, tn, 0, fe, be, p(its)), "gerfs_vbatched: nrhs must not be negative")
    refused(L.mpf_gerfs_vbatched(h, vb.h, 3, pa, pa, pp, nrhs, B, tn, X, tn, 0, fe, be, p(its)), "gerfs_vbatched: trans must be 0 or 1")
    refused(L.mpf_gerfs_vbatched(h, vb.h, 0, pa, pa, pp, nrhs, B, tn - 1, X, tn, 0, fe, be, p(its)), "gerfs_vbatched: leading dimension of B < total_n")
    refused(L.mpf_gerfs_vbatched(h, vb.h, 0, pa, pa, pp, nrhs, B, tn, X, tn - 1, 0, fe, be, p(its)), "gerfs_vbatched: leading dimension of X < total_n")
    for args in ((null, pa, pp, B, X, be), (pa, null, pp, B, X, be), (pa, pa, null, B, X, be), (pa, pa, pp, null, X, be), (pa, pa, pp, B, null, be),
                 (pa, pa, pp, B, X, null)):
        refused(L.mpf_gerfs_vbatched(h, vb.h, 0, args[0], args[1], args[2], nrhs, args[3], tn, args[4], tn, 0, fe, args[5], p(its)),
                "gerfs_vbatched: null pointer")
    other = mpf.MPFContext(0)
    try:
        text = ": the descriptor belongs to another context"
        assert L.mpf_lange_vbatched(other.h, vb.h, b"1", pa, out) < 0 and _err(other) == "lange_vbatched" + text
        assert L.mpf_gecon_vbatched(other.h, vb.h, b"1", pa, out, rc_, ai) < 0 and _err(other) == "gecon_vbatched" + text
        assert L.mpf_residual_vbatched(other.h, vb.h, 0, pa, nrhs, X, tn, B, tn, Rr, tn, W) < 0 and _err(other) == "residual_vbatched" + text
        assert L.mpf_gerfs_vbatched(other.h, vb.h, 0, pa, pa, pp, nrhs, B, tn, X, tn, 0, fe, be, p(its)) < 0 and _err(other) == "gerfs_vbatched" + text
    finally:
        other.close()
    ctx.synchronize()
    assert all(bool((t == 7.0).all()) for t in per + col) and bool((its == 7).all()) and all(bool((t == 1.0).all()) for t in T)   # nothing written
    # nrhs == 0: no work, not even on the order-0 outputs (there are no columns)
    assert L.mpf_residual_vbatched(h, vb.h, 0, pa, 0, X, tn, B, tn, Rr, tn, W) == 0
    assert L.mpf_gerfs_vbatched(h, vb.h, 0, pa, pa, pp, 0, B, tn, X, tn, 0, fe, be, p(its)) == 0
    ctx.synchronize()
    assert all(bool((t == 7.0).all()) for t in col) and bool((its == 7).all()) and all(bool((t == 1.0).all()) for t in T)
    # the order-0 outputs, beside the identity matrices' own: norm 0, rcond 1 and ainvnm 0; berr = ferr = 0 and iters = 0 per column
    assert L.mpf_lange_vbatched(h, vb.h, b"1", pa, out) == 0 and per[0].cpu().tolist() == [1.0, 0.0, 1.0, 0.0]
    assert L.mpf_gecon_vbatched(h, vb.h, b"1", pa, out, rc_, ai) == 0
    assert per[1].cpu().tolist() == [1.0, 1.0, 1.0, 1.0] and per[2].cpu().tolist() == [1.0, 0.0, 1.0, 0.0]
    assert L.mpf_gerfs_vbatched(h, vb.h, 0, pa, pa, pp, nrhs, B, tn, X, tn, 0, fe, be, p(its)) == 0, _err(ctx)
    assert not bool(col[0].view(-1, nrhs)[[1, 3]].any()) and not bool(col[1].view(-1, nrhs)[[1, 3]].any()) and not bool(its.view(-1, nrhs)[[1, 3]].any())
    assert bool((col[0].view(-1, nrhs)[[0, 2]] > 0).all())                      # (identity matrices, x = b = 1: berr 0, ferr from g > 0)
    # a descriptor of order-0 matrices only, and an empty one: the outputs of the former, no work for the latter, NULL operands accepted
    for orders in ([0, 0], []):
        e = ctx.vbatch_blocked(orders)
        o2 = [torch.full((3,), 7.0, dtype=torch.float64, device=ctx.device) for _ in range(5)]
        i2 = torch.full((3,), 7, dtype=torch.int32, device=ctx.device)
        assert L.mpf_lange_vbatched(h, e.h, b"I", null, p(o2[0])) == 0, _err(ctx)
        assert L.mpf_gecon_vbatched(h, e.h, b"I", null, null, p(o2[1]), p(o2[2])) == 0, _err(ctx)
        assert L.mpf_residual_vbatched(h, e.h, 0, null, 1, null, 0, null, 0, null, 0, null) == 0, _err(ctx)
        assert L.mpf_gerfs_vbatched(h, e.h, 1, null, null, null, 1, null, 0, null, 0, 0, p(o2[3]), p(o2[4]), p(i2)) == 0, _err(ctx)
        k = len(orders)
        want = [[0.0] * k, [1.0] * k, [0.0] * k, [0.0] * k, [0.0] * k]
        for t, w in zip(o2, want):
            assert t.cpu().tolist() == w + [7.0] * (3 - k)
        assert i2.cpu().tolist() == [0] * k + [7] * (3 - k)
        e.close()


# ---- 9. the Python surface -----------------------------------------------------------------------------------------------------------
def test_python_surface(ctx, mpf):
    import torch
    n = [4, 0, 140, 40, 200]
    rng = np.random.default_rng(10)
    mats = [rng.standard_normal((v, v)) for v in n]
    vb = ctx.vbatch_blocked(n, ld=[v + 1 for v in n])
    flat = vb.pack(mats)
    B = torch.from_numpy(rng.standard_normal((vb.total_n, 3))).to(ctx.device)
    for norm in ("1", "I"):
        LU, _, _ = vb.getrf(flat)
        assert _teq(vb.cond(flat, norm), vb.gecon(LU, vb.lange(flat, norm), norm))
    rc = vb.cond(flat).cpu().numpy()
    for b, M in enumerate(mats):
        if n[b]:
            assert abs(rc[b] * np.linalg.cond(M, 1) - 1.0) < 1e-8, b           # (a sanity check, the one tolerance of this file)
    for trans in (False, True):
        X, rcond, ferr, berr, info = vb.solvex(flat, B, trans=trans)
        assert not bool(info.any()) and float(rcond.min()) > 0 and float(berr.max()) <= 2.0 ** -50 and ferr.shape == (5, 3)
        for b, M in enumerate(mats):
            if n[b]:
                Xs, rs, fs, bs, _ = ctx.solvex_batched_blocked(torch.from_numpy(M).to(ctx.device).unsqueeze(0), B[_rows(vb, b)].unsqueeze(0), trans=trans)
                assert _teq(X[_rows(vb, b)], Xs[0]) and _teq(rcond[b:b + 1], rs) and _teq(ferr[b], fs[0]) and _teq(berr[b], bs[0]), (b, trans)
    x1 = vb.solvex(flat, B[:, 0].contiguous())[0]
    assert x1.shape == (vb.total_n,) and _teq(x1, vb.solvex(flat, B[:, :1])[0][:, 0])
    mats[2] = mats[2].copy()
    mats[2][:, 130] = 0.0                                    # exactly singular: u_jj = 0 at j = 130
    bad = vb.pack(mats)
    X, rcond, ferr, berr, info = vb.solvex(bad, B)           # never raises
    assert info.cpu().tolist() == [0, 0, 131, 0, 0] and float(rcond[2]) == 0.0 and bool((rcond[[0, 3, 4]] > 0).all())
    good = vb.solvex(flat, B)
    for b in (0, 3, 4):
        assert _teq(X[_rows(vb, b)], good[0][_rows(vb, b)]) and _teq(ferr[b], good[2][b]) and _teq(berr[b], good[3][b])
    with pytest.raises(mpf.MPFError):
        vb.solve(bad, B)                                     # VBatch.solve stays as it is
    small = ctx.vbatch([4, 40, 128])
    sm = [rng.standard_normal((v, v)) for v in (4, 40, 128)]
    assert _teq(small.cond(small.pack(sm)), torch.cat([ctx.cond_batched(torch.from_numpy(M).to(ctx.device).unsqueeze(0)) for M in sm]))
