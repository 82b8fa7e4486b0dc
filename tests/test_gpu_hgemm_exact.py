"""Every fp16 trailing-update kernel (trailing_f16.hip, hgemm16.hip, hgemm_pp.hip) through the step operators, compared
ELEMENT FOR ELEMENT with an exact model (tests/hgemm_exact_model.py): operands whose products and partial sums are integers
below 2^24 make the fp32 accumulation exact in any order, so nothing here carries a tolerance.

  (a) every kernel launch_hgemm_ptrs can select, on the plain and the split operand family;
  (b) the operand rules of contract C6 on the device: subnormals kept, saturation, the split's correction term, NaN;
  (c) one MFMA family, one set of bits: the forms of a family on ordinary N(0,1) data, where the order matters."""
import numpy as np
import pytest

import hgemm_exact_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def contexts(mpf):
    """contexts(options) -> the module's context with these options: one per option set, made at first use, closed at the end."""
    made = {}

    def get(options):
        key = tuple(sorted(options.items()))
        if key not in made:
            made[key] = mpf.MPFContext(0, options=dict(options))
        return made[key]
    yield get
    for c in made.values():
        c.close()


def _update(c, A, B, C, m, split, c32):
    """C[:m] -= A B on the device (C is taller than m); returns all of C: float64, or float32 for the fp32 copy."""
    import torch
    dA, dB, dC = c.from_numpy_f(A), c.from_numpy_f(B), c.from_numpy_f(C)
    if not c32:
        c.hgemm_minus(dC[:m, :], dA, dB, split=split)
        c.synchronize()
        return c.to_numpy_f(dC)
    d32 = torch.empty((C.shape[1], C.shape[0]), dtype=torch.float32, device=c.device).t()   # column-major, ldc = rows of C
    d32.copy_(dC)
    c.hgemm_minus_f32(d32[:m, :], dA, dB, split=split)
    c.synchronize()
    return d32.t().contiguous().cpu().numpy().T


def _assert_same(got, want, C, m):
    bad = ~((got[:m] == want[:m]) | (np.isnan(got[:m]) & np.isnan(want[:m])))
    if bad.any():
        i, j = np.argwhere(bad)[0]
        rows, cols = np.unique(np.argwhere(bad)[:, 0]), np.unique(np.argwhere(bad)[:, 1])
        pytest.fail(f"{int(bad.sum())} wrong elements; first at ({i}, {j}): got {got[i, j]!r}, want {want[i, j]!r}; "
                    f"rows {rows[:8]}.. ({rows.size}), columns {cols[:8]}.. ({cols.size})")
    assert np.array_equal(got[:m], want[:m], equal_nan=True)
    assert np.array_equal(got[m:], C[m:]), "rows below m were touched"


# ---- (a) every kernel, exact -------------------------------------------------------------------------------------------------------
# "big" = m >= 1024, n >= 1024 and K padded to 64 >= 256 (launch_hgemm_ptrs).  C is m + pad rows tall: pad 3 unless stated.
SMALL = [(1, 1, 1), (64, 64, 16),         # one element; one exact 64 x 64 wave block, half a stage of K
         (200, 130, 32),                  # one stage
         (129, 257, 100),                 # ragged both ways, K padded 100 -> 128, the ring wraps once
         (300, 200, 512),
         (1023, 1100, 2048)]              # the largest K, just under the big threshold
SMALL_F64 = [s for s in SMALL if s not in ((1, 1, 1), (300, 200, 512))]
BIG = [(1024, 1024, 256),                 # exact tiles; ldc = 1027
       (1025, 1281, 200),                 # K neither a multiple of 8 nor of 64 (-> 256); ragged in 128- and 256-row tiles; ldc = 1028
       (1100, 1030, 512),
       (1300, 1500, 2048)]                # the ring wraps many times
BIG3 = [BIG[0], BIG[1], BIG[3]]           # exact tiles; ragged tiles and ragged K; K = 2048
OVER = (4097, 4097, 256)                  # 17 x 17 = 289 tiles of 256 x 256 > 256 CUs: a persistent workgroup walks two, the last is ragged

DEFAULT, NO_BIG, M32, M32_RING = {}, {"hgemm_big": 0}, {"hgemm_mfma16": 0}, {"hgemm_mfma16": 0, "hgemm_big": 0}


def _tile(t, **more):
    return dict({"hgemm_big_tile": t}, **more)


def _pad_aligned(m):      # smallest pad >= 1 with 4 * ldc a multiple of 16 bytes
    return (-m) % 4 or 4


def _pad_odd(m):          # pad with ldc no multiple of 4
    return 3 if (m + 3) % 4 else 2


def _rows(split, c32s, options, shapes, pad=None):
    out = []
    for c32 in c32s:
        for s in shapes:
            p = 3 if pad is None else pad(s[0])
            name = "-".join([("split" if split else "plain"), ("f32" if c32 else "f64"),
                             "_".join(f"{k[6:]}{v}" for k, v in sorted(options.items())) or "default", "x".join(map(str, s)), f"pad{p}"])
            out.append(pytest.param(split, c32, options, s, p, id=name))
    return out


KERNEL_CASES = (
    # plain operands, default options, small shapes: hgemm16_ring_kernel<C32>
    _rows(False, [True], DEFAULT, SMALL) + _rows(False, [False], DEFAULT, SMALL_F64)
    # plain, default, big shapes: hgemm16_big_kernel<C32> (fp32: also more tiles than CUs)
    + _rows(False, [False], DEFAULT, BIG) + _rows(False, [True], DEFAULT, BIG + [OVER])
    # plain, hgemm_big = 0, big shapes: hgemm16_ring_kernel<C32> on many tiles
    + _rows(False, [False, True], NO_BIG, BIG)
    # plain, hgemm_mfma16 = 0, small shapes: hgemm_ring_kernel<false, C32>
    + _rows(False, [True], M32, SMALL) + _rows(False, [False], M32, SMALL_F64)
    # plain, fp32 C with 16-byte-aligned columns, hgemm_mfma16 = 0, tile 0 (stand-alone call) and 5: hgemm_pp_kernel
    + _rows(False, [True], M32, BIG3 + [OVER], _pad_aligned)
    + _rows(False, [True], _tile(5, hgemm_mfma16=0), BIG3 + [OVER], _pad_aligned)
    # plain, fp32 C with ldc % 4 != 0, hgemm_mfma16 = 0, tile 0: hgemm_big_kernel<false, true, 4, 2, 2, 4, 4, false, 1, EPI = 2> (slot 5)
    + _rows(False, [True], M32, BIG, _pad_odd)
    # plain, fp32 C, hgemm_mfma16 = 0, tiles 1, 2, 3, 4: hgemm_big_kernel slots 3 (128 x 256), 4 (two workgroups per CU),
    # 7 (serial C batches), 5 (EPI = 2, whatever the alignment)
    + _rows(False, [True], _tile(1, hgemm_mfma16=0), BIG3) + _rows(False, [True], _tile(2, hgemm_mfma16=0), BIG3)
    + _rows(False, [True], _tile(3, hgemm_mfma16=0), BIG3) + _rows(False, [True], _tile(4, hgemm_mfma16=0), BIG3)
    # plain, fp64 C, hgemm_mfma16 = 0, tiles 1 and 3: hgemm_big_kernel<false, false, ...> slots 3 and 5
    + _rows(False, [False], _tile(1, hgemm_mfma16=0), BIG3) + _rows(False, [False], _tile(3, hgemm_mfma16=0), BIG3)
    # split operands, default, small shapes: hgemm_ring_kernel<true, C32>
    + _rows(True, [True], DEFAULT, SMALL) + _rows(True, [False], DEFAULT, SMALL_F64)
    # split, fp64 C, default, big shapes: hgemm_big_kernel<true, false, 2, 2, 4, 2, 4, false> (slot 2)
    + _rows(True, [False], DEFAULT, BIG)
    # split, fp32 C, big shapes: default = slot 2 with the pipelined C stream (EPI = 1); tile 3 = slot 6 (serial batches)
    + _rows(True, [True], DEFAULT, BIG) + _rows(True, [True], _tile(3), BIG)
)

_PRODUCTS = {}     # (split, m, n, k) -> the exact product, computed once and left unchanged


def _family_case(split, m, n, k, pad):
    seed = 1000003 * m + 1009 * n + k + (1 << 40) * int(split)
    A, B, C = (M.split_family if split else M.plain_family)(m, n, k, pad, seed)     # (A and B do not depend on pad)
    key = (split, m, n, k)
    if key not in _PRODUCTS:
        _PRODUCTS[key] = M.product_terms(A, B, split)
        _PRODUCTS[key].setflags(write=False)
    return A, B, C, _PRODUCTS[key]


@pytest.mark.parametrize("split,c32,options,shape,pad", KERNEL_CASES)
def test_every_kernel_exact(contexts, split, c32, options, shape, pad):
    m, n, k = shape
    A, B, C, P = _family_case(split, m, n, k, pad)
    want = M.apply_update(C, P, c32)
    got = _update(contexts(options), A, B, C, m, split, c32)
    _assert_same(got, want, C, m)


def test_model_of_the_cached_product_is_expected():
    """The kernel tests reuse one product per shape; M.expected on the same data is the same matrix."""
    for split in (False, True):
        A, B, C, P = _family_case(split, 129, 257, 100, 3)
        for c32 in (False, True):
            assert np.array_equal(M.apply_update(C, P, c32), M.expected(C, A, B, split, c32))


# ---- (b) the operand rules of contract C6 on the device ---------------------------------------------------------------------------
RK = 48            # K of the small case
SUB = 2.0 ** -24   # the fp16 subnormal grid


def _pad_to(v, n):
    v = list(v)
    assert len(v) <= n
    return v + [0.0] * (n - len(v))


def _special_rows(group):
    """Rows of RK special values; every row keeps its products on one grid (the model checks it)."""
    sgn = [1.0, -1.0]
    if group == "subnormal":
        j24 = list(range(1, 37)) + [511, 512, 513, 767, 1000, 1001, 1020, 1021, 1022, 1023, 64, 96]
        return np.array([
            [SUB * j * sgn[i % 2] for i, j in enumerate(j24)],                                       # every 2^-24 j is an fp16 subnormal
            [2.0 ** -17 * (1 + i % 7) * sgn[(i // 7) % 2] for i in range(RK)],                        # 2^-17 j, j = 1 .. 7
            _pad_to([2.0 ** -14 - SUB, -(2.0 ** -14 - SUB), 3 * 2.0 ** -20, -5 * 2.0 ** -17], RK),     # the largest subnormal, ...
            # values off the grid: rounded to nearest, ties to even -- 0, 0, 1, 2, 2, 2 grid steps, and 1023.5 -> 1024 = 2^-14
            _pad_to([0.4 * SUB, 0.5 * SUB, 0.6 * SUB, 1.5 * SUB, 2.5 * SUB, 1.75 * SUB, 1023.5 * SUB, -1.75 * SUB, 2.0 ** -25], RK),
        ])
    assert group == "normal"
    return np.array([
        _pad_to([2.0 ** -14, -2.0 ** -14, 2.0 ** -14 + SUB, 2.0 ** -13], RK),                          # the flush threshold of C1: kept here
        _pad_to([65504.0, 65520.0, 1e6, -1e9, 65519.9, -65504.0, 1e300], RK),                         # saturation; split: lo = 32768 for 65520 only
        _pad_to([np.inf, -np.inf, np.inf], RK),                                                       # saturates too (C6: clamp, then convert)
        _pad_to([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 0.1, -1.0 / 3.0, 2.718281828, -3.999], RK),      # round to nearest even; split: the rest in lo
        _pad_to([2.0, np.nan, -1.0], RK),                                                             # its row (column) of C is NaN, no other
    ])


def _rules_case(group, where, split, big):
    """Special values in rows of A (where = 'A') or columns of B ('B') against integer partners; the other rows of that operand come
    from the mode's family.  big: the same data inside an otherwise zero 1024 x 1024 x 256 update, across tile and stage seams."""
    rng = np.random.default_rng(7 + 2 * int(split) + (where == "B"))
    rows, other = 40, 24
    S = _special_rows(group)
    fill = M.split_values(rng, (rows - S.shape[0], RK))[0] if split else rng.integers(-3, 4, (rows - S.shape[0], RK)).astype(np.float64)
    blk = np.vstack([fill[:3], S, fill[3:]])
    partner = rng.integers(-3, 4, (RK, other)).astype(np.float64)
    partner[:, 0] = 1.0                                                                  # one column of plain sums
    a, b = (blk, partner) if where == "A" else (partner.T.copy(), blk.T.copy())
    if not big:
        m, n = a.shape[0], b.shape[1]
        A, B = a, b
    else:
        m = n = 1024
        A, B = np.zeros((m, 256)), np.zeros((256, n))
        A[236:236 + a.shape[0], 40:40 + RK] = a                                          # rows across the 256-row seam, k across a 64-k stage
        B[40:40 + RK, 120:120 + b.shape[1]] = b                                          # columns across the 128-column seam
    C = rng.integers(-64, 65, (m + 3, n)).astype(np.float64)
    return np.asfortranarray(A), np.asfortranarray(B), np.asfortranarray(C), m


# (the 32x32x16 family shares its conversion kernels with the others: operand A is enough there)
RULES_CASES = [(g, w, md, big) for g in ("subnormal", "normal") for w, md in (("A", "plain"), ("B", "plain"), ("A", "split"), ("B", "split"), ("A", "plain32"))
               for big in (False, True)]


@pytest.mark.parametrize("group,where,mode,big", RULES_CASES, ids=[f"{g}-{w}-{md}-{'big' if b else 'ring'}" for g, w, md, b in RULES_CASES])
def test_operand_rules_on_the_device(contexts, group, where, mode, big):
    """d2h_sat / d2h_lo as contract C6 states them, seen through exact products: fp16 subnormals are KEPT (the panel's C1 would
    flush them) and reach the MFMA as they are, values off the fp16 grid round to nearest even, everything beyond +-65504 -- Inf
    included -- saturates, the split's lo carries 65520 exactly and is dropped where it overflows, and a NaN makes exactly its row
    or column of C NaN.  plain: hgemm16_ring_kernel / hgemm16_big_kernel; split: hgemm_ring_kernel<true> / hgemm_big_kernel slot 2;
    plain32 (hgemm_mfma16 = 0): hgemm_ring_kernel<false> / hgemm_big_kernel slot 5."""
    split = mode == "split"
    A, B, C, m = _rules_case(group, where, split, big)
    want = M.expected(C, A, B, split, False)
    got = _update(contexts(M32 if mode == "plain32" else DEFAULT), A, B, C, m, split, False)
    _assert_same(got, want, C, m)
    nan = np.isnan(got)
    if group == "normal":    # exactly one row (column) of NaN
        assert nan.sum() == (C.shape[1] if where == "A" else m)
        assert (nan.any(axis=1).sum(), nan.any(axis=0).sum()) == ((1, C.shape[1]) if where == "A" else (m, 1))
    else:
        assert not nan.any()


# ---- (c) one family, one set of bits -------------------------------------------------------------------------------------------------
ORDER_SHAPES = [(1100, 1030, 512), (1300, 1500, 2048)]
_ORDER_RESULTS = {}


def _ordinary_result(contexts, options, shape, split, c32):
    """The update on the suite's usual N(0,1) data (C: m + 4 rows, so the fp32 copy's columns are 16-byte aligned); one run per
    (options, shape, mode), kept."""
    key = (tuple(sorted(options.items())), shape, split, c32)
    if key not in _ORDER_RESULTS:
        m, n, k = shape
        assert (m + 4) % 4 == 0
        rng = np.random.default_rng(m + n + k)
        A = np.asfortranarray(rng.standard_normal((m, k)))
        B = np.asfortranarray(rng.standard_normal((k, n)) * 4.0)
        C = np.asfortranarray(rng.standard_normal((m + 4, n)) * 10.0)
        if c32:
            C = np.asfortranarray(C.astype(np.float32).astype(np.float64))
        got = _update(contexts(options), A, B, C, m, split, c32)
        assert np.array_equal(got[m:], C[m:]) and not np.array_equal(got[:m], C[:m])
        got.setflags(write=False)
        _ORDER_RESULTS[key] = got
    return _ORDER_RESULTS[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


ORDER_CASES = [
    # the 16x16x32 family (hgemm16.hip): hgemm16_ring_kernel on many tiles against hgemm16_big_kernel -- the multi-rank runs rely on it
    ("mfma16", False, False, NO_BIG, DEFAULT), ("mfma16", False, True, NO_BIG, DEFAULT),
    # the 32x32x16 family, fp32 C: hgemm_ring_kernel<false, true> against slots 3, 4, 7, 5 (EPI = 2) and hgemm_pp_kernel
    ("mfma32", False, True, M32_RING, _tile(1, hgemm_mfma16=0)), ("mfma32", False, True, M32_RING, _tile(2, hgemm_mfma16=0)),
    ("mfma32", False, True, M32_RING, _tile(3, hgemm_mfma16=0)), ("mfma32", False, True, M32_RING, _tile(4, hgemm_mfma16=0)),
    ("mfma32", False, True, M32_RING, _tile(5, hgemm_mfma16=0)),
    # ... fp64 C: hgemm_ring_kernel<false, false> against slots 3 and 5
    ("mfma32", False, False, M32_RING, _tile(1, hgemm_mfma16=0)), ("mfma32", False, False, M32_RING, _tile(3, hgemm_mfma16=0)),
    # split operands: hgemm_ring_kernel<true, C32> against slot 2 (fp64; fp32 with EPI = 1) and slot 6
    ("split", True, False, NO_BIG, DEFAULT), ("split", True, True, NO_BIG, DEFAULT), ("split", True, True, NO_BIG, _tile(3)),
]


@pytest.mark.parametrize("shape", ORDER_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("family,split,c32,ring,other", ORDER_CASES,
                         ids=[f"{f}-{'f32' if c else 'f64'}-" + ("_".join(f"{k[6:]}{v}" for k, v in sorted(o.items())) or "default")
                              for f, _, c, _, o in ORDER_CASES])
def test_one_family_one_set_of_bits(contexts, family, split, c32, ring, other, shape):
    """Contract C6, the header of hgemm16.hip and the header of hgemm_pp.hip: the kernels of one MFMA family add the same products in
    the same order, so the 128 x 128 ring form and every big-tile form give the same bits on ordinary data.  (The two plain families
    differ from each other by design -- 32 against 16 k per MFMA -- and are not compared.)"""
    a = _ordinary_result(contexts, ring, shape, split, c32)
    b = _ordinary_result(contexts, other, shape, split, c32)
    same = _bits(a) == _bits(b)
    assert same.all(), f"{int((~same).sum())} elements differ; first at {tuple(np.argwhere(~same)[0])}"
    assert np.array_equal(_bits(a), _bits(b))
