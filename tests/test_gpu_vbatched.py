"""GPU tests of the variable-size batched layer (include/mpf_c.h: mpf_vbatch_create, mpf_getrf_vbatched, mpf_getrs_vbatched,
mpf_getri_vbatched, mpf_getdet_vbatched; csrc/vbatched.hip, csrc/vbatch_plan.h).

Every comparison is of bits: the contract is that matrix b's result is what the fixed-size entry returns for that matrix alone, so the
models are the fixed-size layer's (tests/batched_model.py, tests/pivot64_model.py through it, tests/getri_model.py) and the fixed-size
entries themselves.  The matrices and the cached models are those of tests/test_gpu_batched.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import batched_model as M
import getri_model as GM
from test_gpu_batched import KINDS, _bits, _matrix, _model

pytestmark = pytest.mark.gpu

ORDERS = [0, 1, 2, 3, 7, 8, 9, 16, 17, 31, 32, 33, 63, 64, 65, 100, 127, 128]
SENT = np.array([0xFFF8DEADBEEF0001], dtype=np.uint64).view(np.float64)[0]     # a NaN no computation here produces
SENT_I = int(np.array([SENT]).view(np.int64)[0])


@functools.lru_cache(maxsize=None)
def _mixed():
    """The mixed batch: every order with the five kinds, in a fixed shuffled order.  [(n, kind)]."""
    items = [(n, k) for n in ORDERS for k in KINDS]
    order = np.random.default_rng(2024).permutation(len(items))
    return tuple(items[i] for i in order)


def _sentinel(ctx, count):
    import torch
    return torch.full((max(count, 1),), SENT_I, dtype=torch.int64, device=ctx.device).view(torch.float64)


def _is_sentinel(t):
    import torch
    return t.contiguous().view(torch.int64) == SENT_I


def _mats(vb, flat):
    return [m.cpu().numpy() for m in vb.unpack(flat)]


def _pivs(vb, ipiv):
    p = ipiv.cpu().numpy()
    return [p[o:o + n] for o, n in zip(vb.offv, vb.n)]


@pytest.fixture(scope="module")
def mixed(ctx):
    """The mixed batch factored once (unfused): descriptor, matrices, factors -- shared and left unchanged."""
    items = _mixed()
    vb = ctx.vbatch([n for n, _ in items])
    mats = [_matrix(n, k) if n else np.zeros((0, 0)) for n, k in items]
    A = vb.pack(mats)
    LU, ipiv, info = vb.getrf(A)
    return dict(vb=vb, items=items, mats=mats, A=A, LU=LU, ipiv=ipiv, info=info, LUs=_mats(vb, LU), pivs=_pivs(vb, ipiv))


# ---- 1. one mixed batch against the models -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True])
def test_mixed_batch_against_the_model(ctx, oracle, mixed, fused):
    vb, items = mixed["vb"], mixed["items"]
    assert vb.batch == len(items) == 90 and vb.total_n == 5 * sum(ORDERS) and vb.extent == 5 * sum(n * n for n in ORDERS)
    LU, ipiv, info = vb.getrf(mixed["A"], fused=fused)
    got, piv, inf = _mats(vb, LU), _pivs(vb, ipiv), info.cpu().numpy()
    for b, (n, kind) in enumerate(items):
        if n == 0:
            assert inf[b] == 0
            continue
        LU_m, piv_m, info_m = _model(n, kind, fused, oracle)
        assert inf[b] == info_m == 0, (b, n, kind)
        assert np.array_equal(piv[b], piv_m), (b, n, kind, fused)
        assert np.array_equal(_bits(got[b]), _bits(LU_m)), (b, n, kind, fused)
    assert np.array_equal(_bits(mixed["A"]), _bits(vb.pack(mixed["mats"])))       # out of place: the input stays


# ---- 2. the same batch against the fixed-size entries ------------------------------------------------------------------------------
def _by_order(items):
    groups = {}
    for b, (n, _) in enumerate(items):
        if n:
            groups.setdefault(n, []).append(b)
    return groups


def _fixed_batch(ctx, mats):
    import torch
    mats = np.stack(mats)
    T = ctx.colmajor_batch(*mats.shape)
    T.copy_(torch.from_numpy(np.ascontiguousarray(mats)))
    return T


@pytest.fixture(scope="module")
def fixed(ctx, mixed):
    """mpf_getrf_batched on the matrices of every distinct order: {n: (members, LU, ipiv)}."""
    out = {}
    for n, members in _by_order(mixed["items"]).items():
        LU, ipiv, info = ctx.getrf_batched(_fixed_batch(ctx, [mixed["mats"][b] for b in members]))
        assert not info.cpu().numpy().any()
        out[n] = (members, LU, ipiv)
    return out


def test_factors_equal_the_fixed_size_entry(mixed, fixed):
    for n, (members, LU, ipiv) in fixed.items():
        LUf, pf = LU.cpu().numpy(), ipiv.cpu().numpy()
        for i, b in enumerate(members):
            assert np.array_equal(mixed["pivs"][b], pf[i]), (n, b)
            assert np.array_equal(_bits(mixed["LUs"][b]), _bits(LUf[i])), (n, b)


@pytest.mark.parametrize("trans", [False, True])
def test_solve_equals_the_fixed_size_entry(ctx, mixed, fixed, trans):
    import torch
    vb = mixed["vb"]
    for nrhs in (1, 3, 5):                                   # 5 wraps the four-wave form
        B = np.random.default_rng(100 + nrhs).standard_normal((vb.total_n, nrhs))
        X = ctx.to_numpy_f(vb.getrs(mixed["LU"], mixed["ipiv"], ctx.from_numpy_f(B), trans=trans))
        for n, (members, LU, ipiv) in fixed.items():
            Bf = torch.from_numpy(np.stack([B[vb.offv[b]:vb.offv[b] + n] for b in members])).to(ctx.device)
            Xf = ctx.getrs_batched(LU, ipiv, Bf, trans=trans).cpu().numpy()
            for i, b in enumerate(members):
                assert np.array_equal(_bits(X[vb.offv[b]:vb.offv[b] + n]), _bits(Xf[i])), (n, b, nrhs, trans)
    # one right-hand side as a vector
    xv = vb.getrs(mixed["LU"], mixed["ipiv"], torch.from_numpy(np.ascontiguousarray(B[:, 0])).to(ctx.device), trans=trans)
    assert xv.shape == (vb.total_n,) and np.array_equal(_bits(xv), _bits(X[:, 0]))


def test_inverse_and_determinant_equal_the_fixed_size_entry(ctx, mixed, fixed):
    vb = mixed["vb"]
    inv, info = vb.getri(mixed["LU"], mixed["ipiv"])
    mant, expo = vb.getdet(mixed["LU"], mixed["ipiv"])
    invs, mant, expo = _mats(vb, inv), mant.cpu().numpy(), expo.cpu().numpy()
    assert not info.cpu().numpy().any()
    for n, (members, LU, ipiv) in fixed.items():
        If, _ = ctx.getri_batched(LU, ipiv)
        mf, ef = ctx.getdet_batched(LU, ipiv)
        If, mf, ef = If.cpu().numpy(), mf.cpu().numpy(), ef.cpu().numpy()
        for i, b in enumerate(members):
            assert np.array_equal(_bits(invs[b]), _bits(If[i])), (n, b)
            assert _bits(mant[b:b + 1]) == _bits(mf[i:i + 1]) and expo[b] == ef[i], (n, b)
    for b, (n, _) in enumerate(mixed["items"]):
        if n == 0:
            assert (mant[b], expo[b]) == (0.5, 1)


# ---- 3. neighbours and positions ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W, small", [(8, 3), (16, 9), (32, 17)])
def test_wave_mates_of_another_order_and_every_position(ctx, oracle, W, small):
    """One matrix of order `small` shares a wave of the W-lane form with matrices of order W; class counts 1, G - 1, G, G + 1; the
    small matrix first, in the middle and last in the batch; one n = 33 and one n = 65 matrix alone in their classes."""
    G = 64 // W
    for count in sorted({1, G - 1, G, G + 1} - {0}):
        for where in ("first", "middle", "last"):
            items = [(W, KINDS[i % 5]) for i in range(count - 1)] + [(33, "normal"), (65, "normal")]
            items.insert({"first": 0, "middle": len(items) // 2, "last": len(items)}[where], (small, "normal"))
            vb = ctx.vbatch([n for n, _ in items])
            LU, ipiv, info = vb.getrf(vb.pack([_matrix(n, k) for n, k in items]))
            inv, info2 = vb.getri(LU, ipiv)
            B = np.random.default_rng(7).standard_normal((vb.total_n, 2))
            X = ctx.to_numpy_f(vb.getrs(LU, ipiv, ctx.from_numpy_f(B)))
            assert not info.cpu().numpy().any() and not info2.cpu().numpy().any()
            for b, (got, piv, gi) in enumerate(zip(_mats(vb, LU), _pivs(vb, ipiv), _mats(vb, inv))):
                n, kind = items[b]
                LU_m, piv_m, _ = _model(n, kind, False, oracle)
                assert np.array_equal(piv, piv_m) and np.array_equal(_bits(got), _bits(LU_m)), (W, count, where, b)
                if n <= W:                                   # (the models of the solve on orders 33 and 65: case 2 has them)
                    rows = slice(int(vb.offv[b]), int(vb.offv[b]) + n)
                    assert np.array_equal(_bits(X[rows]), _bits(M.getrs_model(LU_m, piv_m, B[rows]))), (W, count, where, b)
                    assert np.array_equal(_bits(gi), _bits(M.getrs_model(LU_m, piv_m, np.eye(n)))), (W, count, where, b)


# ---- 4. explicit layout and untouched bytes --------------------------------------------------------------------------------------------
def test_explicit_layout_leaves_every_other_byte_alone(ctx, oracle):
    import torch
    items = [(n, "normal") for n in (3, 8, 0, 9, 16, 17, 32, 48, 33, 64, 49, 100, 65, 128, 5)]
    n = [v for v, _ in items]
    ld = [v + 3 for v in n]
    off, at = [], 0
    for b, v in enumerate(n):                                # even offsets for the even b, odd ones for the odd b: the 16-byte path needs an
        at += (at + b) % 2                                   # even offset and an even ld (33, 49, 65 here), all else takes the 8-byte path;
        off.append(at)                                       # gaps between the matrices
        at += ld[b] * v + 6
    vb = ctx.vbatch(n, ld, off)
    assert {o % 2 for o in off} == {0, 1} and vb.extent == max(o + (v - 1) * l + v for v, l, o in zip(n, ld, off) if v)
    inside = torch.zeros(vb.extent + 4, dtype=torch.bool, device=ctx.device)
    for m in vb.unpack(inside):
        m.fill_(True)
    buf = _sentinel(ctx, vb.extent + 4)
    for m, (v, k) in zip(vb.unpack(buf), items):
        if v:
            m.copy_(torch.from_numpy(_matrix(v, k)))
    pbuf = torch.full((vb.total_n + 3,), -7, dtype=torch.int32, device=ctx.device)
    LU, ipiv, info = vb.getrf(buf, overwrite=True, ipiv=pbuf)
    assert LU.data_ptr() == buf.data_ptr() and bool(_is_sentinel(buf)[~inside].all()) and bool((pbuf[vb.total_n:] == -7).all())
    models = [_model(v, k, False, oracle) if v else None for v, k in items]
    for b, (got, piv) in enumerate(zip(_mats(vb, LU), _pivs(vb, ipiv))):
        if n[b]:
            assert np.array_equal(piv, models[b][1]) and np.array_equal(_bits(got), _bits(models[b][0])), b
    # the solve: ldb = total_n + 5
    ldb, nrhs = vb.total_n + 5, 3
    Bn = np.random.default_rng(44).standard_normal((vb.total_n, nrhs))
    for trans in (False, True):
        bbuf = _sentinel(ctx, ldb * nrhs)
        Bd = bbuf.as_strided((vb.total_n, nrhs), (1, ldb))
        Bd.copy_(torch.from_numpy(Bn))
        X = vb.getrs(LU, pbuf, Bd, trans=trans, overwrite=True)
        assert X.data_ptr() == bbuf.data_ptr()
        assert bool(_is_sentinel(bbuf).view(nrhs, ldb)[:, vb.total_n:].all())
        Xn = X.cpu().numpy()
        for b in range(vb.batch):
            if n[b]:
                rows = slice(int(vb.offv[b]), int(vb.offv[b]) + n[b])
                assert np.array_equal(_bits(Xn[rows]), _bits(M.getrs_model(models[b][0], models[b][1], Bn[rows], trans))), (b, trans)
    # the inverse: LU and ipiv unchanged, nothing outside the matrices written
    keep_LU, keep_piv = buf.clone(), pbuf.clone()
    out = _sentinel(ctx, vb.extent + 4)
    inv, info2 = vb.getri(LU, pbuf, out=out)
    assert bool(_is_sentinel(out)[~inside].all()) and not info2.cpu().numpy().any()
    assert np.array_equal(keep_LU.view(torch.int64).cpu().numpy(), buf.view(torch.int64).cpu().numpy())
    assert np.array_equal(keep_piv.cpu().numpy(), pbuf.cpu().numpy())
    for b, gi in enumerate(_mats(vb, inv)):
        if n[b]:
            assert np.array_equal(_bits(gi), _bits(M.getrs_model(models[b][0], models[b][1], np.eye(n[b])))), b


# ---- 5. inverse contract ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_each(ctx, oracle):
    """One matrix of every order of ORDERS plus 40 and 80 (all seven classes), factored by the model."""
    orders = ORDERS + [40, 80]
    vb = ctx.vbatch(orders)
    fac = [_model(n, "normal", False, oracle)[:2] if n else (np.zeros((0, 0)), np.zeros(0, dtype=np.int32)) for n in orders]
    import torch
    LU = vb.pack([f[0] for f in fac])
    ipiv = torch.from_numpy(np.concatenate([f[1] for f in fac]).astype(np.int32)).to(ctx.device)
    return dict(vb=vb, orders=orders, fac=fac, LU=LU, ipiv=ipiv)


def test_inverse_is_the_solve_on_a_block_identity(ctx, one_each):
    vb, orders = one_each["vb"], one_each["orders"]
    inv, info = vb.getri(one_each["LU"], one_each["ipiv"])
    E = np.zeros((vb.total_n, 128))
    for b, n in enumerate(orders):
        E[vb.offv[b]:vb.offv[b] + n, :n] = np.eye(n)
    X = ctx.to_numpy_f(vb.getrs(one_each["LU"], one_each["ipiv"], ctx.from_numpy_f(E)))
    assert not info.cpu().numpy().any()
    for b, gi in enumerate(_mats(vb, inv)):
        n = orders[b]
        assert np.array_equal(_bits(gi), _bits(X[vb.offv[b]:vb.offv[b] + n, :n])), (b, n)


def test_singular_matrices_keep_their_result_and_their_neighbours(ctx, one_each):
    import torch
    vb, orders = one_each["vb"], one_each["orders"]
    clean, _ = vb.getri(one_each["LU"], one_each["ipiv"])
    clean = _mats(vb, clean)
    zero_at = {7: 4, 16: 9, 31: 30, 40: 0, 64: 33, 80: 79, 128: 100}               # one per class (order: the zero's row), 0-based
    LU = one_each["LU"].clone()
    views = vb.unpack(LU)
    for b, n in enumerate(orders):
        if n in zero_at:
            views[b][zero_at[n], zero_at[n]] = 0.0
            if n == 80:
                views[b][3, 3] = 0.0                         # two zeros: info names the first
    ipiv = one_each["ipiv"].clone()
    b17 = orders.index(17)
    ipiv[int(vb.offv[b17]) + 2] = 99                         # out of range: reads as "no interchange", nothing else is affected
    out = _sentinel(ctx, vb.extent)
    inv, info = vb.getri(LU, ipiv, out=out)
    info = info.cpu().numpy()
    for b, (n, m) in enumerate(zip(orders, vb.unpack(inv))):
        if n in zero_at:
            assert info[b] == (4 if n == 80 else zero_at[n] + 1), (n, info[b])
            assert bool(_is_sentinel(m).all()), n
        elif n:
            assert info[b] == 0
            if b != b17:
                assert np.array_equal(_bits(m), _bits(clean[b])), n
            else:
                piv = one_each["fac"][b][1].copy()
                piv[2] = 3                                   # no interchange at step 2
                assert np.array_equal(_bits(m), _bits(M.getrs_model(one_each["fac"][b][0], piv, np.eye(17))))


# ---- 6. determinant -------------------------------------------------------------------------------------------------------------------
def test_determinant_against_the_model(ctx, one_each):
    vb, orders = one_each["vb"], one_each["orders"]
    LU = one_each["LU"].clone()
    views = vb.unpack(LU)
    views[orders.index(9)][4, 4] = 0.0
    views[orders.index(100)][70, 70] = float("inf")
    views[orders.index(65)][64, 64] = 0.0
    views[orders.index(65)][2, 2] = float("nan")             # non-finite wins over zero
    mant, expo = vb.getdet(LU, one_each["ipiv"])
    mant, expo = mant.cpu().numpy(), expo.cpu().numpy()
    for b, n in enumerate(orders):
        if n == 0:
            assert (mant[b], expo[b]) == (0.5, 1)
        elif n == 9:
            assert (mant[b], expo[b]) == (0.0, 0)
        elif n in (100, 65):
            assert np.isnan(mant[b]) and expo[b] == 0
        else:
            m_m, e_m = GM.getdet_model(np.diag(views[b].cpu().numpy()), one_each["fac"][b][1])
            assert _bits(np.array([mant[b]])) == _bits(np.array([m_m])) and expo[b] == e_m, n


# ---- 7. a uniform descriptor ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 32, 33, 128])
def test_uniform_descriptor_gives_the_fixed_size_bits(ctx, n):
    import torch
    batch = 11
    A = _fixed_batch(ctx, np.random.default_rng(n).standard_normal((batch, n, n)))
    flat = A.transpose(1, 2).reshape(-1)                     # the packed column-major buffer itself
    assert flat.data_ptr() == A.data_ptr()
    vb = ctx.vbatch([n] * batch)
    LU, ipiv, info = vb.getrf(flat)
    LUf, ipivf, infof = ctx.getrf_batched(A)
    assert np.array_equal(_bits(LU), _bits(LUf.transpose(1, 2).reshape(-1))) and np.array_equal(ipiv.cpu().numpy(), ipivf.reshape(-1).cpu().numpy())
    assert np.array_equal(info.cpu().numpy(), infof.cpu().numpy())
    inv, _ = vb.getri(LU, ipiv)
    invf, _ = ctx.getri_batched(LUf, ipivf)
    assert np.array_equal(_bits(inv), _bits(invf.transpose(1, 2).reshape(-1)))
    mant, expo = vb.getdet(LU, ipiv)
    mf, ef = ctx.getdet_batched(LUf, ipivf)
    assert np.array_equal(_bits(mant), _bits(mf)) and np.array_equal(expo.cpu().numpy(), ef.cpu().numpy())
    B = torch.from_numpy(np.random.default_rng(n + 1).standard_normal((batch, n, 3))).to(ctx.device)
    for trans in (False, True):
        Xf = ctx.getrs_batched(LUf, ipivf, B, trans=trans)
        X = vb.getrs(LU, ipiv, B.reshape(batch * n, 3), trans=trans)
        assert np.array_equal(_bits(X), _bits(Xf.reshape(batch * n, 3))), (n, trans)


# ---- 8. chunking ----------------------------------------------------------------------------------------------------------------------
def test_class_longer_than_one_launch(ctx):
    """2^22 + 3 matrices of orders 1 and 2 alternating: one class, two chunks.  The class list holds the order-1 matrices first."""
    import torch
    batch = (1 << 22) + 3
    n = np.ones(batch, dtype=np.int32)
    n[1::2] = 2
    vb = ctx.vbatch(n)
    assert vb.extent == int(np.sum(n.astype(np.int64) ** 2)) and vb.total_n == int(n.sum())
    a = np.random.default_rng(8).uniform(1.0, 2.0, vb.extent)
    LU, ipiv, info = vb.getrf(torch.from_numpy(a).to(ctx.device))
    assert not bool(info.any())
    ones = (batch + 1) // 2                                  # list position p >= ones is the matrix 2 (p - ones) + 1
    seam = [2 * (p - ones) + 1 for p in range((1 << 22) - 2, (1 << 22) + 2)]
    LUn, pn = LU.cpu().numpy(), ipiv.cpu().numpy()
    for b in [0, 1, 2, batch - 2, batch - 1] + seam:
        nb, o, ov = int(n[b]), int(vb.off[b]), int(vb.offv[b])
        LU_m, piv_m, _ = M.getrf_model(a[o:o + nb * nb].reshape(nb, nb).T)
        assert np.array_equal(pn[ov:ov + nb], piv_m), b
        assert np.array_equal(_bits(LUn[o:o + nb * nb]), _bits(LU_m.T.reshape(-1))), b
    mant, expo = vb.getdet(LU, ipiv)
    assert bool(torch.isfinite(mant).all()) and bool((mant != 0).all())


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_through_the_c_abi(ctx, mpf):
    import torch
    L, h = ctx.L, ctx.h

    def err():
        return L.mpf_last_error(h).decode()

    def create(n, ld=None, off=None, batch=None):
        arr = [np.ascontiguousarray(v, dtype=t) if v is not None else None for v, t in ((n, np.int32), (ld, np.int64), (off, np.int64))]
        out = C.c_void_p()
        rc = L.mpf_vbatch_create(h, len(n) if batch is None else batch, *[C.c_void_p(a.ctypes.data) if a is not None else None for a in arr],
                                 C.byref(out))
        assert (rc == 0) == bool(out.value)
        if out.value:
            L.mpf_vbatch_destroy(out)
        return rc

    assert create([3, 129]) < 0 and "mpf_factor_dev" in err()
    assert create([3, -1]) < 0 and "negative" in err()
    assert create([3], batch=-1) < 0 and "negative" in err()
    assert create([3], batch=1 << 31) < 0 and "2^31" in err()
    assert create([3, 4], ld=[3, 3]) < 0 and "leading dimension" in err()
    assert create([3, 4], off=[0, -1]) < 0 and "offset" in err()
    assert create([3, 4], off=[0, 8]) < 0 and "overlap" in err()
    assert create([3, 4], off=[0, 9]) == 0 and create([]) == 0 and create([0, 0]) == 0

    n = [3, 0, 20, 40]
    vb = ctx.vbatch(n)
    offM, offV = np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.int64)
    assert L.mpf_vbatch_offsets(vb.h, C.c_void_p(offM.ctypes.data), C.c_void_p(offV.ctypes.data)) == 0
    assert offM.tolist() == [0, 9, 9, 409] and offV.tolist() == [0, 3, 3, 23]
    assert np.array_equal(vb.off, offM) and np.array_equal(vb.offv, offV) and (vb.batch, vb.total_n, vb.extent) == (4, 63, 2009)
    A = vb.pack([np.eye(v) for v in n])
    keep = A.clone()
    ipiv = torch.zeros(vb.total_n, dtype=torch.int32, device=ctx.device)
    B = torch.ones(vb.total_n * 2, dtype=torch.float64, device=ctx.device)
    inv = torch.zeros(vb.extent, dtype=torch.float64, device=ctx.device)
    det = torch.zeros(4, dtype=torch.float64, device=ctx.device)
    pa, pp, pb, pd, null = [C.c_void_p(t.data_ptr()) for t in (A, ipiv, B, det)] + [C.c_void_p(0)]
    assert L.mpf_getrf_vbatched(h, vb.h, null, pp, null, 0) < 0 and "null" in err()
    assert L.mpf_getrf_vbatched(h, vb.h, pa, null, null, 0) < 0 and "null" in err()
    assert L.mpf_getrf_vbatched(h, null, pa, pp, null, 0) < 0 and "null" in err()
    assert L.mpf_getrs_vbatched(h, vb.h, 2, pa, pp, 2, pb, vb.total_n) < 0 and "trans" in err()
    assert L.mpf_getrs_vbatched(h, vb.h, 0, pa, pp, -1, pb, vb.total_n) < 0 and "nrhs" in err()
    assert L.mpf_getrs_vbatched(h, vb.h, 0, pa, pp, 2, pb, vb.total_n - 1) < 0 and "total_n" in err()
    assert L.mpf_getrs_vbatched(h, vb.h, 0, pa, pp, 2, null, vb.total_n) < 0 and "null" in err()
    assert L.mpf_getrs_vbatched(h, vb.h, 0, pa, pp, 0, pb, vb.total_n) == 0
    assert L.mpf_getri_vbatched(h, vb.h, pa, pp, null, null) < 0 and "null" in err()
    assert L.mpf_getri_vbatched(h, vb.h, pa, pp, pa, null) < 0 and "overlaps" in err()
    assert L.mpf_getri_vbatched(h, vb.h, pa, pp, C.c_void_p(A.data_ptr() + 8 * (vb.extent - 1)), null) < 0 and "overlaps" in err()
    assert L.mpf_getdet_vbatched(h, vb.h, pa, pp, null, null) < 0 and "null" in err()
    other = mpf.MPFContext(0)
    try:
        assert L.mpf_getrf_vbatched(other.h, vb.h, pa, pp, null, 0) < 0 and "another context" in L.mpf_last_error(other.h).decode()
        assert L.mpf_getdet_vbatched(other.h, vb.h, pa, pp, pd, pp) < 0
    finally:
        other.close()
    ctx.synchronize()
    assert np.array_equal(_bits(A), _bits(keep)) and not bool(ipiv.any()) and bool((B == 1.0).all()) and not bool(inv.any())


# ---- 10. the Python surface -----------------------------------------------------------------------------------------------------------
def test_python_surface(ctx, mpf):
    import torch
    n = [4, 0, 12, 40, 7]
    rng = np.random.default_rng(10)
    mats = [rng.standard_normal((v, v)) for v in n]
    vb = ctx.vbatch(n, ld=[v + 1 for v in n])
    flat = vb.pack(mats)
    assert flat.shape == (vb.extent,) and [m.shape for m in vb.unpack(flat)] == [(v, v) for v in n]
    for m, want in zip(vb.unpack(flat), mats):
        assert np.array_equal(_bits(m), _bits(want))
    B = rng.standard_normal(vb.total_n)
    x = vb.solve(flat, torch.from_numpy(B).to(ctx.device)).cpu().numpy()
    X = vb.unpack(vb.inv(flat))
    sign, logdet = vb.slogdet(flat)
    for b, A in enumerate(mats):
        if n[b]:
            rows = slice(int(vb.offv[b]), int(vb.offv[b]) + n[b])
            s1, l1 = ctx.slogdet_batched(torch.from_numpy(A).to(ctx.device).unsqueeze(0))
            assert float(sign[b]) == float(s1[0]) and float(logdet[b]) == float(l1[0]), b
            assert np.array_equal(_bits(x[rows]), _bits(ctx.solve_batched(torch.from_numpy(A).to(ctx.device).unsqueeze(0),
                                                                        torch.from_numpy(B[rows]).to(ctx.device).view(1, -1, 1)).reshape(-1)))
            assert np.array_equal(_bits(X[b]), _bits(ctx.inv_batched(torch.from_numpy(A).to(ctx.device).unsqueeze(0))[0]))
    assert float(sign[1]) == 1.0 and abs(float(logdet[1])) <= 2.0 ** -52         # the empty product: log 0.5 + ln 2, each rounded once
    mats[3] = mats[3].copy()
    mats[3][:, 6] = 0.0
    bad = vb.pack(mats)
    for call in (lambda: vb.solve(bad, torch.from_numpy(B).to(ctx.device)), lambda: vb.inv(bad)):
        with pytest.raises(mpf.MPFError) as ei:
            call()
        assert "matrix 3" in str(ei.value) and "zero pivot 7" in str(ei.value)
    with pytest.raises(mpf.MPFError) as ei:
        ctx.vbatch([4, 129])
    assert "mpf_factor_dev" in str(ei.value)
