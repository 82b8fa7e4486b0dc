"""CPU checks of tests/hgetf2_fused_model.py, the reference for contract C2f (option fp16_fused: the fp16 pivot panel's rank-1 step as
one fused multiply-add).  The model's fma against exact rational arithmetic; the exactness shown to matter (triples on which an fp32 fma
rounded again to fp16 gives another answer); the model with fused=False against oracle.hgetf2; the C model against the literal
thread-by-thread restatement in both settings; and the GPU tests' input cases checked for zero pivots, so that none of the kinds
that must run there is skipped."""
from fractions import Fraction

import numpy as np
import pytest

import hgetf2_fused_model as M
from test_gpu_steps import _panel_case

KINDS = ["gen", "ties", "sparse", "normal"]
NAN16 = 0x7E00


# ---- the fma ------------------------------------------------------------------------------------------------------------------
def _frac(h):
    """Finite binary16 bit pattern -> Fraction, from the format's definition."""
    e, f = (h >> 10) & 31, h & 1023
    v = Fraction(1024 + f, 1024) * Fraction(2) ** (e - 15) if e else Fraction(f, 1024) * Fraction(2) ** -14
    return -v if h & 0x8000 else v


# every finite binary16 value, ascending, and its bit pattern: rounding = the nearest entry, ties to the even significand
_POS = [(_frac(h), h) for h in range(0x7C00)]
_MAXF = _POS[-1][0]


def _round_fraction(v, zero_sign):
    """Exact rational -> binary16 by searching the table of all finite values (no formula shared with the model)."""
    if v == 0:
        return 0x8000 if zero_sign else 0
    sign, a = (0x8000, -v) if v < 0 else (0, v)
    if a >= _MAXF + Fraction(2) ** 4:        # half an ulp (2^5) past the largest finite value: the tie goes to the even one, infinity
        return sign | 0x7C00
    lo, hi = 0, 0x7BFF                       # largest entry <= a
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if _POS[mid][0] <= a:
            lo = mid
        else:
            hi = mid - 1
    if lo == 0x7BFF:
        return sign | 0x7BFF
    dl, dh = a - _POS[lo][0], _POS[lo + 1][0] - a
    if dl < dh or (dl == dh and lo % 2 == 0):
        return sign | lo
    return sign | (lo + 1)


def _fma_reference(m, u, x):
    """fma(-m, u, x) from IEEE 754's text: special operands by rule, everything else the exact rational rounded once."""
    nan = lambda h: (h & 0x7FFF) > 0x7C00
    inf = lambda h: (h & 0x7FFF) == 0x7C00
    zero = lambda h: (h & 0x7FFF) == 0
    if nan(m) or nan(u) or nan(x):
        return NAN16
    pneg = ((m >> 15) ^ 1 ^ (u >> 15)) & 1                     # sign of (-m) * u
    if inf(m) or inf(u):
        if zero(m) or zero(u):
            return NAN16                                       # inf * 0
        p = 0x7C00 | (pneg << 15)
        return NAN16 if inf(x) and x != p else p               # inf - inf
    if inf(x):
        return x
    return _round_fraction(_frac(x) - _frac(m) * _frac(u), pneg & (x >> 15))


def _triples():
    rng = np.random.default_rng(20260101)
    special = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x0400, 0x8400, 0x3C00, 0xBC00, 0x3C01, 0x7BFF, 0xFBFF,
                        0x7C00, 0xFC00, 0x7E00, 0xFE00, 0x7C01, 0x0002, 0x3800, 0x1400, 0x6BFF, 0x5BFF, 0x5C00], dtype=np.uint16)
    parts = []
    g = np.array(np.meshgrid(special, special, special, indexing="ij")).reshape(3, -1)     # 24^3: every special against every other
    parts.append(g)
    parts.append(rng.integers(0, 65536, (3, 60000)).astype(np.uint16))                       # uniform bit patterns
    sub = rng.integers(0, 0x0400, (3, 10000)).astype(np.uint16) | (rng.integers(0, 2, (3, 10000)).astype(np.uint16) << 15)
    mix = rng.integers(0, 65536, (3, 10000)).astype(np.uint16)
    mix[rng.integers(0, 3, 10000), np.arange(10000)] = sub[0]                               # one subnormal operand among normal ones
    parts += [sub, mix]
    big = (rng.integers(0x6C00, 0x7C00, (3, 10000)).astype(np.uint16)) | (rng.integers(0, 2, (3, 10000)).astype(np.uint16) << 15)
    parts.append(big)                                                                        # products beyond 65504: overflow
    near = rng.integers(0, 65536, (3, 10000)).astype(np.uint16)                              # x close to m * u: cancellation
    with np.errstate(all="ignore"):
        near[2] = (near[0].view(np.float16) * near[1].view(np.float16)).view(np.uint16) ^ rng.integers(0, 4, 10000).astype(np.uint16)
    parts.append(near)
    return np.concatenate(parts, axis=1)


def test_model_fma_is_the_exact_result_rounded_once():
    m, u, x = _triples()
    assert m.size >= 100000
    got = M.fnma(m, u, x)
    want = np.array([_fma_reference(int(a), int(b), int(c)) for a, b, c in zip(m, u, x)], dtype=np.uint16)
    bad = np.flatnonzero(~((got == want) | (((got & 0x7FFF) > 0x7C00) & ((want & 0x7FFF) > 0x7C00))))
    assert bad.size == 0, [(hex(m[i]), hex(u[i]), hex(x[i]), hex(got[i]), hex(want[i])) for i in bad[:5]]
    # both ways through the C model (two-sum shortcut, 128-bit fixed point) and the Python integers of the literal restatement
    assert M.same_bits(M.fnma(m, u, x, exact_only=True), want)
    k = slice(0, None, 7)
    assert M.same_bits(np.array([M.fnma_exact(a, b, c) for a, b, c in zip(m[k], u[k], x[k])], dtype=np.uint16), want[k])
    # the classes the contract names are all in the sample
    fin = lambda h: (h & 0x7C00) != 0x7C00
    allfin = fin(m) & fin(u) & fin(x)
    assert np.any(allfin & ((want & 0x7C00) == 0) & ((want & 0x3FF) != 0)), "no subnormal result"
    assert np.any(allfin & ((want & 0x7FFF) == 0x7C00)), "no overflow to infinity from finite operands"
    assert np.any(want == 0x8000) and np.any(want == 0x0000), "both zeros"
    assert np.any(~allfin & ((want & 0x7FFF) > 0x7C00)) and np.any(~allfin & ((want & 0x7FFF) == 0x7C00))


# (m, u, x) bit patterns, found by a random search over finite operands: fma(-m, u, x) in binary32 lands within the rounding error
# of a binary16 rounding boundary, so rounding it AGAIN to binary16 gives the neighbour of the correctly rounded result
DOUBLE_ROUNDING_TRIPLES = [
    (33023, 13063, 38896), (34627, 12586, 4770), (38052, 19756, 52841), (17316, 9817, 49762), (20984, 51072, 195),
    (16142, 25088, 33734), (50258, 9064, 55725), (25664, 50728, 229), (16000, 30748, 5193), (15689, 59904, 33227),
    (26044, 19840, 37672), (13408, 30768, 36146), (8748, 22268, 34175), (59368, 12418, 7684), (53120, 50008, 32822),
    (24933, 45165, 25478), (26455, 6236, 61641), (18848, 24656, 35245), (23967, 43077, 62414), (56576, 14164, 62),
    (5208, 2910, 4236), (20139, 21507, 63841), (20400, 58944, 34607), (14325, 6423, 10834), (18176, 60506, 32795),
    (60016, 18368, 5073), (59596, 14991, 8699), (19034, 58624, 1933), (61680, 17504, 490), (63622, 48896, 35462),
    (21760, 23922, 35511), (14599, 57529, 39813), (20708, 22272, 1518), (38968, 63552, 26), (58688, 20208, 37870),
    (34718, 61022, 52340), (13383, 3245, 43705), (16768, 29068, 33365), (22136, 44591, 60730), (12180, 49209, 24915),
    (55040, 24556, 5158), (27520, 18712, 38293), (55416, 56384, 131), (52480, 26260, 2592), (58424, 49600, 33455),
    (56431, 48663, 64320), (21968, 57152, 4376), (56064, 23690, 36939)]


def test_exactness_matters_fp32_fma_then_round_is_another_function():
    m, u, x = (np.array(c, dtype=np.uint16) for c in zip(*DOUBLE_ROUNDING_TRIPLES))
    want = np.array([_fma_reference(*t) for t in DOUBLE_ROUNDING_TRIPLES], dtype=np.uint16)
    assert np.array_equal(M.fnma(m, u, x), want)
    assert np.array_equal(M.fnma(m, u, x, exact_only=True), want)
    twice = M.fma32_then_round(m, u, x)
    assert np.all(twice != want), "every committed triple is one where the double rounding shows"
    # ... by exactly one unit in the last place
    assert np.all(np.abs(twice.astype(np.int32) - want.astype(np.int32)) == 1)


# ---- the panel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows,cols", [(2, 2), (33, 32), (257, 32), (300, 128), (1000, 256)])
def test_unfused_model_is_the_oracle(oracle, kind, rows, cols):
    P = _panel_case(oracle, kind, rows, cols, rows * 131 + cols)
    want = np.asfortranarray(oracle.double_to_fp16(P))
    want_piv = oracle.hgetf2(want)
    got_piv, got = M.panel_pivots(P, oracle, fused=False)
    assert np.array_equal(got_piv, want_piv), f"first diff at column {np.argmax(got_piv != want_piv)}"
    assert M.same_bits(got, want)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("kind,rows,cols", [("gen", 2, 2), ("ties", 40, 40), ("gen", 257, 12), ("normal", 300, 40), ("sparse", 300, 40),
                                            ("gen", 300, 40), ("ties", 520, 9), ("zero", 130, 9)])
def test_c_model_equals_the_literal_restatement(oracle, kind, rows, cols, fused):
    if kind == "zero":      # a zero column: 0 / 0, NaN spreads -- IEEE rules in the fma, ordered compares in the search
        P = _panel_case(oracle, "gen", rows, cols, 3)
        P[:, 4] = 0.0
    else:
        P = _panel_case(oracle, kind, rows, cols, rows * 7 + cols)
    bits = np.asfortranarray(oracle.double_to_fp16(P))
    a, b = bits.copy(order="F"), bits.copy(order="F")
    pa, pb = M.hgetf2(a, fused), M.literal_hgetf2(b, fused)
    assert np.array_equal(pa, pb)
    assert M.same_bits(a, b)


def test_the_two_contracts_differ_on_the_committed_panels(oracle):
    import test_gpu_hgetf2_fused as G
    for kind, rows, cols, seed in G.DIFFERING_PANELS:
        assert rows <= 1024 and cols <= 128
        P = _panel_case(oracle, kind, rows, cols, seed)
        p0, _ = M.panel_pivots(P, oracle, fused=False)
        p1, _ = M.panel_pivots(P, oracle, fused=True)
        assert not np.array_equal(p0, p1)


def test_gpu_cases_of_the_kinds_that_must_run_meet_no_zero_pivot(oracle):
    """The GPU tests skip panels whose fp16 factorization meets a zero pivot (inf / NaN: outside the parity contract).  The
    generator-style and the normal kind must never be among them (the tests there assert it again instead of skipping)."""
    import test_gpu_hgetf2_fused as G
    for rows, cols, seed in G.all_panel_cases():
        for kind in ("gen", "normal"):
            _, bits = M.panel_pivots(_panel_case(oracle, kind, rows, cols, seed), oracle, True)
            assert G.finite16(bits), (kind, rows, cols)
