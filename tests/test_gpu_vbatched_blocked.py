"""GPU tests of the variable-size batched layer for orders up to 1024 (include/mpf_c.h: mpf_vbatch_create_blocked and the four
mpf_*_vbatched entries on its descriptor; csrc/vbatched_blocked.hip, csrc/batched_blocked_body.h, csrc/vbatch_plan.h).

Every comparison is of bits (torch.equal on an int64 view, or numpy on a uint64 view): the contract is that matrix b's result is what
the fixed-size BLOCKED entry returns for that matrix alone, so the yardsticks are those entries, each called on one matrix, and for
the orders up to 65 tests/batched_model.py directly.  With option batched_blocked_min_n = 0 every order >= 1 takes the ragged blocked
kernels, which is how the small shapes reach them."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gpu_batched import KINDS, _bits, _dev_batch, _matrix, _model, _same_with_nans

pytestmark = pytest.mark.gpu

# both sides of the panel width, the wave, the 64 x 64 update tile, the 256-column row-block chunk, the 256-entry determinant chunk and
# the group top at 256
ORDERS = [0, 1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 160, 161, 255, 256, 257, 289, 290]
MODEL_UPTO = 65
BIG_KINDS = ["normal", "tiny", "last_row"]                                    # (the other two cost a numpy pivot search to build)
SENT = np.array([0xFFF8DEADBEEF0001], dtype=np.uint64).view(np.float64)[0]     # a NaN no computation here produces
SENT_I = int(np.array([SENT]).view(np.int64)[0])


def _teq(a, b):
    import torch
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)))


def _sentinel(ctx, count):
    import torch
    return torch.full((max(count, 1),), SENT_I, dtype=torch.int64, device=ctx.device).view(torch.float64)


def _is_sentinel(t):
    import torch
    return t.contiguous().view(torch.int64) == SENT_I


def _kind(n, i):
    return KINDS[i % 5] if n <= MODEL_UPTO else BIG_KINDS[i % 3]


@functools.lru_cache(maxsize=None)
def _mixed_items():
    """Two matrices per order, of different kinds, in a fixed shuffled order.  [(n, kind)]."""
    items = [(n, _kind(n, i + j)) for i, n in enumerate(ORDERS) for j in (0, 1)]
    order = np.random.default_rng(2025).permutation(len(items))
    return tuple(items[i] for i in order)


def _rows(vb, b):
    return slice(int(vb.offv[b]), int(vb.offv[b]) + int(vb.n[b]))


def _piv(vb, ipiv, b):
    return ipiv[_rows(vb, b)]


@pytest.fixture(scope="module")
def bctx(mpf):
    """Every order through the blocked kernels, ragged and fixed-size alike; the tests set the width options as they go."""
    c = mpf.MPFContext(0, options={"batched_blocked_min_n": 0})
    yield c
    c.close()


def _alone(c, mat, fused=False):
    """The fixed-size blocked factorization of one matrix alone: (LU (1, n, n), ipiv (1, n), info (1,))."""
    return c.getrf_batched_blocked(_dev_batch(c, [mat]), fused=fused)


@pytest.fixture(scope="module")
def mixed(bctx):
    """The mixed batch factored once (unfused), and every matrix factored alone by the fixed-size entry -- shared, left unchanged."""
    items = _mixed_items()
    vb = bctx.vbatch_blocked([n for n, _ in items])
    mats = [_matrix(n, k) if n else np.zeros((0, 0)) for n, k in items]
    A = vb.pack(mats)
    LU, ipiv, info = vb.getrf(A)
    alone = [_alone(bctx, m) if n else None for m, (n, _) in zip(mats, items)]
    return dict(vb=vb, items=items, mats=mats, A=A, LU=LU, ipiv=ipiv, info=info, alone=alone)


# ---- 1. one mixed descriptor, every order on the new kernels -----------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True])
def test_mixed_factors_equal_the_fixed_size_entry_and_the_model(bctx, oracle, mixed, fused):
    vb, items = mixed["vb"], mixed["items"]
    assert vb.batch == len(items) == 2 * len(ORDERS) and vb.total_n == 2 * sum(ORDERS) and vb.extent == 2 * sum(n * n for n in ORDERS)
    assert bctx.get_option("batched_blocked_min_n") == 0
    LU, ipiv, info = vb.getrf(mixed["A"], fused=fused)
    views, inf, host = vb.unpack(LU), info.cpu().numpy(), None
    for b, (n, kind) in enumerate(items):
        if n == 0:
            assert inf[b] == 0
            continue
        LUf, pf, inff = mixed["alone"][b] if not fused else _alone(bctx, mixed["mats"][b], True)
        assert inf[b] == int(inff[0]) == 0, (b, n, kind)
        assert bool((_piv(vb, ipiv, b) == pf[0]).all()), (b, n, kind, fused)
        assert _teq(views[b], LUf[0]), (b, n, kind, fused)
        if n <= MODEL_UPTO:
            host = host if host is not None else (LU.cpu().numpy(), ipiv.cpu().numpy())
            LU_m, piv_m, info_m = _model(n, kind, fused, oracle)
            o = int(vb.off[b])
            assert info_m == 0 and np.array_equal(host[1][_rows(vb, b)], piv_m), (b, n, kind, fused)
            assert np.array_equal(_bits(host[0][o:o + n * n].reshape(n, n).T), _bits(LU_m)), (b, n, kind, fused)
    assert _teq(mixed["A"], vb.pack(mixed["mats"]))                              # out of place: the input stays


# ---- 2. the same descriptor's solve, inverse and determinant ------------------------------------------------------------------------------
@pytest.mark.parametrize("trans", [False, True])
def test_mixed_solve_equals_the_fixed_size_entry(bctx, mixed, trans):
    import torch
    vb = mixed["vb"]
    for nrhs in (1, 3, 4, 9):                                # the one-column tile, and the eight-column tile with a partial last tile
        B = torch.from_numpy(np.random.default_rng(100 + nrhs).standard_normal((vb.total_n, nrhs))).to(bctx.device)
        X = vb.getrs(mixed["LU"], mixed["ipiv"], B, trans=trans)
        for b, (n, _) in enumerate(mixed["items"]):
            if n:
                LUf, pf, _ = mixed["alone"][b]
                Xf = bctx.getrs_batched_blocked(LUf, pf, B[_rows(vb, b)].unsqueeze(0), trans=trans)
                assert _teq(X[_rows(vb, b)], Xf[0]), (b, n, nrhs, trans)


def test_mixed_inverse_and_determinant_equal_the_fixed_size_entry(bctx, mixed):
    vb = mixed["vb"]
    want = {}
    for b, (n, _) in enumerate(mixed["items"]):
        if n:
            LUf, pf, _ = mixed["alone"][b]
            want[b] = (bctx.getri_batched_blocked(LUf, pf)[0], bctx.getdet_batched_blocked(LUf, pf))
    try:
        for ct in (8, 16):
            bctx.set_option("batched_blocked_inv_ct", ct)
            inv, info = vb.getri(mixed["LU"], mixed["ipiv"])
            assert not bool(info.any())
            for b, m in enumerate(vb.unpack(inv)):
                if b in want:
                    assert _teq(m, want[b][0][0]), (b, mixed["items"][b], ct)
    finally:
        bctx.set_option("batched_blocked_inv_ct", 0)
    mant, expo = vb.getdet(mixed["LU"], mixed["ipiv"])
    for b, (n, _) in enumerate(mixed["items"]):
        if n:
            assert _teq(mant[b:b + 1], want[b][1][0]) and int(expo[b]) == int(want[b][1][1][0]), (b, n)
        else:
            assert (float(mant[b]), int(expo[b])) == (0.5, 1)


# ---- 3. the panel width changes no bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True])
def test_panel_width_changes_no_bit(bctx, fused):
    orders = [1, 7, 9, 31, 33, 65, 129, 161, 257]
    vb = bctx.vbatch_blocked(orders)
    mats = [_matrix(n, "normal", seed=2) for n in orders]
    A = vb.pack(mats)
    alone = [_alone(bctx, m, fused) for m in mats]
    try:
        for nb in (8, 16, 32):
            bctx.set_option("batched_blocked_nb", nb)
            LU, ipiv, info = vb.getrf(A, fused=fused)
            assert not bool(info.any())
            for b, m in enumerate(vb.unpack(LU)):
                assert _teq(m, alone[b][0][0]) and bool((_piv(vb, ipiv, b) == alone[b][1][0]).all()), (orders[b], nb, fused)
    finally:
        bctx.set_option("batched_blocked_nb", 0)


# ---- 4. default options: the small classes and the large list in one descriptor ------------------------------------------------------------
def test_default_options_split_the_descriptor(ctx):
    import torch
    assert ctx.get_option("batched_blocked_min_n") == 129
    orders = [5, 40, 128, 129, 300]                          # the first three take the small kernels, the other two the new ones
    vb = ctx.vbatch_blocked(orders)
    mats = [_matrix(n, "normal", seed=4) for n in orders]
    A = vb.pack(mats)
    B = torch.from_numpy(np.random.default_rng(4).standard_normal((vb.total_n, 3))).to(ctx.device)
    for fused in (False, True):
        LU, ipiv, info = vb.getrf(A, fused=fused)
        assert not bool(info.any())
        for b, m in enumerate(vb.unpack(LU)):
            LUf, pf, _ = _alone(ctx, mats[b], fused)
            assert _teq(m, LUf[0]) and bool((_piv(vb, ipiv, b) == pf[0]).all()), (orders[b], fused)
    inv, info2 = vb.getri(LU, ipiv)
    mant, expo = vb.getdet(LU, ipiv)
    X = [vb.getrs(LU, ipiv, B, trans=t) for t in (False, True)]
    assert not bool(info2.any())
    for b, m in enumerate(vb.unpack(inv)):
        LUf, pf, _ = _alone(ctx, mats[b], True)
        mf, ef = ctx.getdet_batched_blocked(LUf, pf)
        assert _teq(m, ctx.getri_batched_blocked(LUf, pf)[0][0]), orders[b]
        assert _teq(mant[b:b + 1], mf) and int(expo[b]) == int(ef[0]), orders[b]
        for t in (False, True):
            assert _teq(X[t][_rows(vb, b)], ctx.getrs_batched_blocked(LUf, pf, B[_rows(vb, b)].unsqueeze(0), trans=t)[0]), (orders[b], t)


# ---- 5. the largest ratio inside one launch group, and across groups ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def large(ctx):
    orders = [513, 1023, 1024, 129]
    rng = np.random.default_rng(1024 + 5)
    mats = [rng.standard_normal((n, n)) for n in orders]
    vb = ctx.vbatch_blocked(orders)
    return dict(vb=vb, orders=orders, mats=mats, A=vb.pack(mats))


@pytest.mark.parametrize("fused", [False, True])
def test_large_orders_in_one_descriptor(ctx, large, fused):
    import torch
    vb, orders = large["vb"], large["orders"]
    LU, ipiv, info = vb.getrf(large["A"], fused=fused)
    assert not bool(info.any())
    alone = [_alone(ctx, m, fused) for m in large["mats"]]
    for b, m in enumerate(vb.unpack(LU)):
        assert bool((_piv(vb, ipiv, b) == alone[b][1][0]).all()), (orders[b], fused)
        assert _teq(m, alone[b][0][0]), (orders[b], fused)
    if fused:
        return
    Bv = torch.from_numpy(np.random.default_rng(6).standard_normal(vb.total_n)).to(ctx.device)
    x = vb.getrs(LU, ipiv, Bv)
    mant, expo = vb.getdet(LU, ipiv)
    inv, info2 = vb.getri(LU, ipiv)
    assert not bool(info2.any())
    for b, n in enumerate(orders):
        LUf, pf, _ = alone[b]
        assert _teq(x[_rows(vb, b)], ctx.getrs_batched_blocked(LUf, pf, Bv[_rows(vb, b)].view(1, n, 1))[0, :, 0]), n
        mf, ef = ctx.getdet_batched_blocked(LUf, pf)
        assert _teq(mant[b:b + 1], mf) and int(expo[b]) == int(ef[0]), n
    assert _teq(vb.unpack(inv)[0], ctx.getri_batched_blocked(*alone[0][:2])[0][0])       # (the 513 matrix)


# ---- 6. neighbours and padding -------------------------------------------------------------------------------------------------------------
def test_explicit_layout_leaves_every_other_byte_alone(bctx):
    import torch
    n = [33, 161, 0, 129, 7, 257, 64]
    ld = [v + 3 if v else 0 for v in n]
    slots = [4, 1, 6, 0, 5, 2, 3]                            # the matrices lie in another order than the batch's, with gaps between them
    size, off = (257 + 3) * 257 + 5, [0] * len(n)
    for b, s in enumerate(slots):
        off[b] = s * size + (b % 3)
    vb = bctx.vbatch_blocked(n, ld, off)
    mats = [_matrix(v, "normal", seed=6) if v else np.zeros((0, 0)) for v in n]
    alone = [_alone(bctx, m) if v else None for m, v in zip(mats, n)]
    total = vb.extent + 4
    inside = torch.zeros(total, dtype=torch.bool, device=bctx.device)
    for m in vb.unpack(inside):
        m.fill_(True)
    buf = _sentinel(bctx, total)
    for m, A, v in zip(vb.unpack(buf), mats, n):
        if v:
            m.copy_(torch.from_numpy(np.ascontiguousarray(A)))
    pbuf = torch.full((vb.total_n + 3,), -7, dtype=torch.int32, device=bctx.device)
    LU, ipiv, info = vb.getrf(buf, overwrite=True, ipiv=pbuf)
    assert LU.data_ptr() == buf.data_ptr() and bool(_is_sentinel(buf)[~inside].all()) and bool((pbuf[vb.total_n:] == -7).all())
    assert not bool(info.any())
    for b, m in enumerate(vb.unpack(LU)):
        if n[b]:
            assert _teq(m, alone[b][0][0]) and bool((_piv(vb, pbuf, b) == alone[b][1][0]).all()), n[b]
    # the solve: ldb = total_n + 5
    ldb, nrhs = vb.total_n + 5, 9
    Bn = torch.from_numpy(np.random.default_rng(44).standard_normal((vb.total_n, nrhs))).to(bctx.device)
    for trans in (False, True):
        bbuf = _sentinel(bctx, ldb * nrhs)
        Bd = bbuf.as_strided((vb.total_n, nrhs), (1, ldb))
        Bd.copy_(Bn)
        X = vb.getrs(LU, pbuf, Bd, trans=trans, overwrite=True)
        assert X.data_ptr() == bbuf.data_ptr() and bool(_is_sentinel(bbuf).view(nrhs, ldb)[:, vb.total_n:].all())
        for b in range(vb.batch):
            if n[b]:
                Xf = bctx.getrs_batched_blocked(alone[b][0], alone[b][1], Bn[_rows(vb, b)].unsqueeze(0), trans=trans)
                assert _teq(X[_rows(vb, b)], Xf[0]), (n[b], trans)
    # the inverse and the determinant: LU and ipiv unchanged, nothing outside the matrices written
    keep_LU, keep_piv = buf.clone(), pbuf.clone()
    out = _sentinel(bctx, total)
    inv, info2 = vb.getri(LU, pbuf, out=out)
    assert bool(_is_sentinel(out)[~inside].all()) and not bool(info2.any())
    mant, expo = vb.getdet(LU, pbuf)
    assert _teq(keep_LU, buf) and bool(torch.equal(keep_piv, pbuf)) and bool(_is_sentinel(out)[~inside].all())
    for b, m in enumerate(vb.unpack(inv)):
        if n[b]:
            mf, ef = bctx.getdet_batched_blocked(alone[b][0], alone[b][1])
            assert _teq(m, bctx.getri_batched_blocked(alone[b][0], alone[b][1])[0][0]), n[b]
            assert _teq(mant[b:b + 1], mf) and int(expo[b]) == int(ef[0]), n[b]


# ---- 7. singular matrices -------------------------------------------------------------------------------------------------------------------
def test_singular_matrices_keep_their_inverse_and_their_neighbours(bctx):
    orders = [130, 161, 40, 33, 256]
    mats = [_matrix(n, "normal", seed=7).copy() for n in orders]
    mats[1][:, 100] = 0.0                                    # exactly singular: the zero column stays zero, u_jj = 0 at j = 100 and j = 6
    mats[3][:, 6] = 0.0
    vb = bctx.vbatch_blocked(orders)
    LU, ipiv, info = vb.getrf(vb.pack(mats))
    assert info.cpu().numpy().tolist() == [0, 101, 0, 7, 0]
    alone = [_alone(bctx, m) for m in mats]
    for b, m in enumerate(vb.unpack(LU)):
        assert int(alone[b][2][0]) == int(info[b]) and bool((_piv(vb, ipiv, b) == alone[b][1][0]).all()), orders[b]
        if b in (1, 3):                                      # (a NaN's sign and payload are not part of the contract)
            assert _same_with_nans(m.cpu().numpy(), alone[b][0][0].cpu().numpy()), orders[b]
        else:
            assert _teq(m, alone[b][0][0]), orders[b]
    out = _sentinel(bctx, vb.extent)
    inv, info2 = vb.getri(LU, ipiv, out=out)
    assert info2.cpu().numpy().tolist() == [0, 101, 0, 7, 0]
    for b, m in enumerate(vb.unpack(inv)):
        if b in (1, 3):
            assert bool(_is_sentinel(m).all()), orders[b]
        else:
            assert _teq(m, bctx.getri_batched_blocked(alone[b][0], alone[b][1])[0][0]), orders[b]


# ---- 8. position --------------------------------------------------------------------------------------------------------------------------
def test_position_changes_no_bit(bctx):
    import torch
    one = _matrix(161, "normal", seed=8)
    others = [_matrix(130, "normal", seed=8), _matrix(256, "normal", seed=8), _matrix(130, "tiny", seed=8), _matrix(256, "last_row", seed=8)]
    rhs = torch.from_numpy(np.random.default_rng(8).standard_normal((161, 4))).to(bctx.device)
    seen = []
    for at in (0, 2, 4):
        mats = others[:at] + [one] + others[at:]
        vb = bctx.vbatch_blocked([m.shape[0] for m in mats])
        LU, ipiv, info = vb.getrf(vb.pack(mats), fused=True)
        B = torch.zeros((vb.total_n, 4), dtype=torch.float64, device=bctx.device)
        B[_rows(vb, at)] = rhs
        X = vb.getrs(LU, ipiv, B)
        inv, _ = vb.getri(LU, ipiv)
        mant, expo = vb.getdet(LU, ipiv)
        assert not bool(info.any())
        seen.append((vb.unpack(LU)[at].clone(), _piv(vb, ipiv, at).clone(), X[_rows(vb, at)].clone(), vb.unpack(inv)[at].clone(),
                     mant[at:at + 1].clone(), expo[at:at + 1].clone()))
    for other in seen[1:]:
        for got, want in zip(other, seen[0]):
            assert bool(torch.equal(got, want)) if got.dtype == torch.int32 else _teq(got, want)
    LUf, pf, _ = _alone(bctx, one, True)
    assert _teq(seen[0][0], LUf[0]) and bool((seen[0][1] == pf[0]).all())


# ---- 9. the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_refusals_through_the_c_abi(ctx, mpf):
    import torch
    L, h = ctx.L, ctx.h

    def err(handle=h):
        return L.mpf_last_error(handle).decode()

    def create(fn, n, ld=None, off=None, batch=None):
        arr = [np.ascontiguousarray(v, dtype=t) if v is not None else None for v, t in ((n, np.int32), (ld, np.int64), (off, np.int64))]
        out = C.c_void_p()
        rc = fn(h, len(n) if batch is None else batch, *[C.c_void_p(a.ctypes.data) if a is not None else None for a in arr], C.byref(out))
        assert (rc == 0) == bool(out.value)
        if out.value:
            L.mpf_vbatch_destroy(out)
        return rc

    new, old = L.mpf_vbatch_create_blocked, L.mpf_vbatch_create
    assert create(new, [3, 1025]) < 0
    assert err() == "vbatch_create_blocked: n > 1024 is not a batch-sized matrix: factor it with mpf_factor_dev (and solve with mpf_getrs) (matrix 1)"
    assert create(new, [3, -1]) < 0 and err() == "vbatch_create_blocked: n must not be negative (matrix 1)"
    assert create(new, [3, 400], ld=[3, 399]) < 0 and err() == "vbatch_create_blocked: leading dimension < n (matrix 1)"
    assert create(new, [3, 400], off=[0, 8]) < 0 and err() == "vbatch_create_blocked: matrices 0 and 1 overlap"
    assert create(new, [3], batch=-1) < 0 and err() == "vbatch_create_blocked: batch must not be negative"
    assert create(new, [3, 400], off=[0, 9]) == 0 and create(new, []) == 0 and create(new, [0, 0]) == 0 and create(new, [1024, 129, 5]) == 0
    assert create(old, [3, 129]) < 0
    assert err() == "vbatch_create: n > 128 is not a small matrix: factor it with mpf_factor_dev (and solve with mpf_getrs) (matrix 1)"

    vb = ctx.vbatch_blocked([3, 200])
    A = vb.pack([np.eye(3), np.eye(200)])
    ipiv = torch.zeros(vb.total_n, dtype=torch.int32, device=ctx.device)
    det = torch.zeros(2, dtype=torch.float64, device=ctx.device)
    pa, pp, pd, null = [C.c_void_p(t.data_ptr()) for t in (A, ipiv, det)] + [C.c_void_p(0)]
    other = mpf.MPFContext(0)
    try:
        assert L.mpf_getrf_vbatched(other.h, vb.h, pa, pp, null, 0) < 0
        assert err(other.h) == "getrf_vbatched: the descriptor belongs to another context"
        assert L.mpf_getrs_vbatched(other.h, vb.h, 0, pa, pp, 1, pa, vb.total_n) < 0 and "another context" in err(other.h)
        assert L.mpf_getri_vbatched(other.h, vb.h, pa, pp, pa, null) < 0 and "another context" in err(other.h)
        assert L.mpf_getdet_vbatched(other.h, vb.h, pa, pp, pd, pp) < 0 and "another context" in err(other.h)
    finally:
        other.close()
    ctx.synchronize()
    assert not bool(ipiv.any()) and _teq(A, vb.pack([np.eye(3), np.eye(200)]))


# ---- 10. a group longer than one launch, and the probe library's VALU form of the fused update ------------------------------------------
def test_group_longer_than_one_launch(bctx):
    """2^15 + 3 matrices of orders 1 and 2 alternating, every one in the first launch group: two chunks, the first with both orders.
    The yardstick is the fixed-size blocked entry on all matrices of an order at once."""
    import torch
    batch = (1 << 15) + 3                                    # BB_MAX_LAUNCH of csrc/mpf_internal.h, and three
    n = np.ones(batch, dtype=np.int32)
    n[1::2] = 2
    vb = bctx.vbatch_blocked(n)
    a = torch.from_numpy(np.random.default_rng(15).uniform(1.0, 2.0, vb.extent)).to(bctx.device)
    rhs = torch.from_numpy(np.random.default_rng(16).standard_normal(vb.total_n)).to(bctx.device)
    LU, ipiv, info = vb.getrf(a)
    x = vb.getrs(LU, ipiv, rhs)
    inv, info2 = vb.getri(LU, ipiv)
    mant, expo = vb.getdet(LU, ipiv)
    assert not bool(info.any()) and not bool(info2.any())
    off, offv = torch.from_numpy(vb.off).to(bctx.device), torch.from_numpy(vb.offv).to(bctx.device)
    for v in (1, 2):
        mem = torch.from_numpy(np.nonzero(n == v)[0]).to(bctx.device)
        me = (off[mem][:, None] + torch.arange(v * v, device=bctx.device)[None, :]).view(-1)
        ve = (offv[mem][:, None] + torch.arange(v, device=bctx.device)[None, :]).view(-1)
        as_batch = lambda flat: flat[me].view(-1, v, v).transpose(1, 2)                # noqa: E731  ((count, v, v) column-major)
        LUf, pf, inff = bctx.getrf_batched_blocked(as_batch(a))
        assert _teq(as_batch(LU), LUf) and bool(torch.equal(ipiv[ve].view(-1, v), pf)) and not bool(inff.any()), v
        assert _teq(x[ve].view(-1, v, 1), bctx.getrs_batched_blocked(LUf, pf, rhs[ve].view(-1, v, 1))), v
        assert _teq(as_batch(inv), bctx.getri_batched_blocked(LUf, pf)[0]), v
        mf, ef = bctx.getdet_batched_blocked(LUf, pf)
        assert _teq(mant[mem], mf) and bool(torch.equal(expo[mem], ef)), v


@pytest.mark.parametrize("fused", [False, True])
def test_fused_update_on_the_valu_kernel(mpf, bctx, fused):
    """Probe library: the VALU instantiation of the ragged fused update is the MFMA kernel's cross-check."""
    orders = [33, 49, 161, 257]
    mats = [_matrix(n, "normal", seed=3) for n in orders]
    pc = mpf.MPFContext(0, probe=True, options={"batched_blocked_min_n": 0, "batched_blocked_valu": 1})
    try:
        vb, vb1 = bctx.vbatch_blocked(orders), pc.vbatch_blocked(orders)
        LU, ipiv, _ = vb.getrf(vb.pack(mats), fused=fused)
        LU1, ipiv1, _ = vb1.getrf(vb1.pack(mats), fused=fused)
        assert _teq(LU, LU1) and bool((ipiv == ipiv1).all())
        vb1.close()
    finally:
        pc.close()


# ---- 11. the Python surface -----------------------------------------------------------------------------------------------------------
def test_python_surface(ctx, mpf):
    import torch
    n = [4, 0, 140, 40, 200]
    rng = np.random.default_rng(10)
    mats = [rng.standard_normal((v, v)) for v in n]
    vb = ctx.vbatch_blocked(n, ld=[v + 1 for v in n])
    assert isinstance(vb, mpf.VBatch) and (vb.batch, vb.total_n) == (5, sum(n))
    flat = vb.pack(mats)
    assert flat.shape == (vb.extent,) and [m.shape for m in vb.unpack(flat)] == [(v, v) for v in n]
    B = torch.from_numpy(rng.standard_normal(vb.total_n)).to(ctx.device)
    x = vb.solve(flat, B)
    X = vb.unpack(vb.inv(flat))
    sign, logdet = vb.slogdet(flat)
    for b, A in enumerate(mats):
        if n[b]:
            Ad = torch.from_numpy(A).to(ctx.device).unsqueeze(0)
            s1, l1 = ctx.slogdet_batched_blocked(Ad)
            assert float(sign[b]) == float(s1[0]) and float(logdet[b]) == float(l1[0]), b
            assert _teq(x[_rows(vb, b)], ctx.solve_batched_blocked(Ad, B[_rows(vb, b)].view(1, -1, 1)).reshape(-1)), b
            assert _teq(X[b], ctx.inv_batched_blocked(Ad)[0]), b
    assert float(sign[1]) == 1.0 and abs(float(logdet[1])) <= 2.0 ** -52         # the empty product: log 0.5 + ln 2, each rounded once
    mats[2] = mats[2].copy()
    mats[2][:, 130] = 0.0
    mats[4] = mats[4].copy()
    mats[4][:, 6] = 0.0
    bad = vb.pack(mats)
    for call in (lambda: vb.solve(bad, B), lambda: vb.inv(bad)):
        with pytest.raises(mpf.MPFError) as ei:
            call()
        assert "matrix 2" in str(ei.value) and "zero pivot 131" in str(ei.value)  # the first singular matrix
    with pytest.raises(mpf.MPFError) as ei:
        ctx.vbatch_blocked([4, 1025])
    assert "mpf_factor_dev" in str(ei.value)
    with pytest.raises(mpf.MPFError) as ei:
        ctx.vbatch([4, 129])
    assert "n > 128" in str(ei.value) and "mpf_factor_dev" in str(ei.value)
