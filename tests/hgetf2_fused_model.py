"""Reference for contract C2f (option fp16_fused): the fp16 pivot panel of hgetf2_kernel.cu:15-120 with the rank-1 step
`panel[k*ld+row] -= multiplier * panel[k*ld+j]` (:113) as ONE fused multiply-add, fma(-m, u, x) rounded once to binary16 --
and, with fused=False, as the rounded product and rounded difference of contract C2 (what oracle.hgetf2 computes).

Two restatements that share no arithmetic:
  * hgetf2(bits, fused): tests/hgetf2_fused_model.c, compiled here on first use -- exact 128-bit fixed point, fast enough for
    2049 x 256 and larger;
  * literal_hgetf2(bits, fused): thread by thread in Python like cuda_style_hgetf2 in tests/test_oracle_independent.py, every
    operation as an exact Python integer (fixed point) rounded once by round16() -- slow, for panels up to about 300 x 40.
Panels are (rows, cols) uint16 arrays of binary16 bit patterns, Fortran order, factored in place; pivots are 1-based int32."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
BLOCK = 256
NAN16 = 0x7E00

_lib = None
_tmp = None


def lib():
    """The C model as a shared library (gcc, -ffp-contract=off: the two-sum in it must not be contracted)."""
    global _lib, _tmp
    if _lib is None:
        _tmp = tempfile.TemporaryDirectory(prefix="hgetf2_fused_model_")
        so = os.path.join(_tmp.name, "libhgetf2_fused_model.so")
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-o", so,
                        os.path.join(HERE, "hgetf2_fused_model.c"), "-lm"], check=True)
        L = C.CDLL(so)
        u16p, i32p = C.POINTER(C.c_uint16), C.POINTER(C.c_int32)
        L.hfm_init.restype = None
        L.hfm_fnma_n.argtypes = [u16p, u16p, u16p, u16p, C.c_int64, C.c_int]
        L.hfm_mulsub_n.argtypes = [u16p, u16p, u16p, u16p, C.c_int64]
        L.hfm_fma32_n.argtypes = [u16p, u16p, u16p, u16p, C.c_int64]
        L.hfm_div_n.argtypes = [u16p, u16p, u16p, C.c_int64]
        L.hfm_hgetf2.argtypes = [u16p, C.c_int64, C.c_int, C.c_int, i32p, C.c_int]
        for f in (L.hfm_fnma_n, L.hfm_mulsub_n, L.hfm_fma32_n, L.hfm_div_n, L.hfm_hgetf2):
            f.restype = None
        L.hfm_init()
        _lib = L
    return _lib


def _u16(a):
    return np.ascontiguousarray(a, dtype=np.uint16)


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint16))


def _ternary(fn, m, u, x, *extra):
    m, u, x = _u16(m), _u16(u), _u16(x)
    out = np.empty_like(m)
    fn(_p(m), _p(u), _p(x), _p(out), m.size, *extra)
    return out


def fnma(m, u, x, exact_only=False):
    """round16(x - m * u) element-wise on bit patterns: the model's fused step (exact_only: the 128-bit path alone)."""
    return _ternary(lib().hfm_fnma_n, m, u, x, int(exact_only))


def mulsub(m, u, x):
    """round16(x - round16(m * u)): contract C2's step."""
    return _ternary(lib().hfm_mulsub_n, m, u, x)


def fma32_then_round(m, u, x):
    """NOT the contract: an fp32 fma whose result is rounded again to binary16 (finite operands)."""
    return _ternary(lib().hfm_fma32_n, m, u, x)


def hdiv(a, b):
    a, b = _u16(a), _u16(b)
    out = np.empty_like(a)
    lib().hfm_div_n(_p(a), _p(b), _p(out), a.size)
    return out


def hgetf2(bits, fused):
    """Factor the panel in place; returns the 1-based pivots."""
    assert bits.dtype == np.uint16 and bits.flags.f_contiguous and bits.ndim == 2
    rows, cols = bits.shape
    ipiv = np.zeros(cols, dtype=np.int32)
    lib().hfm_hgetf2(_p(bits), rows, rows, cols, ipiv.ctypes.data_as(C.POINTER(C.c_int32)), int(bool(fused)))
    return ipiv


def panel_pivots(P64, oracle, fused):
    """fp64 panel -> (pivots, factored fp16 bits): contract C1's conversion (the oracle's), then hgetf2."""
    bits = np.asfortranarray(oracle.double_to_fp16(np.asfortranarray(P64)))
    piv = hgetf2(bits, fused)
    return piv, bits


def same_bits(a, b):
    """Equal bit patterns; NaN payloads are outside the contract (any NaN equals any NaN)."""
    a, b = np.asarray(a, dtype=np.uint16), np.asarray(b, dtype=np.uint16)
    nan = ((a & 0x7FFF) > 0x7C00) & ((b & 0x7FFF) > 0x7C00)
    return a.shape == b.shape and bool(np.all((a == b) | nan))


# ---- exact integer arithmetic on single values (Python integers: no width limit) ---------------------------------------------
def value24(h):
    """Finite binary16 bit pattern -> signed integer in units of 2^-24."""
    h = int(h)
    e, f = (h >> 10) & 31, h & 1023
    v = (1024 | f) << (e - 1) if e else f
    return -v if h & 0x8000 else v


def _isnan(h):
    return (h & 0x7FFF) > 0x7C00


def _isinf(h):
    return (h & 0x7FFF) == 0x7C00


def round16(n, unit_exp, zero_sign=0):
    """n * 2^unit_exp (n a Python integer) -> binary16 bits: round to nearest even, subnormals kept, overflow to infinity; an exact
    zero takes zero_sign."""
    if n == 0:
        return 0x8000 if zero_sign else 0
    sign = 0x8000 if n < 0 else 0
    a = -n if n < 0 else n
    e = a.bit_length() - 1 + unit_exp                               # 2^e <= |value| < 2^(e+1)
    q = max(e, -14) - 10                                            # the result is a multiple of 2^q
    sh = q - unit_exp
    if sh <= 0:
        k = a << -sh
    else:
        k, rem, half = a >> sh, a & ((1 << sh) - 1), 1 << (sh - 1)
        if rem > half or (rem == half and k & 1):
            k += 1
    if k == 2048:
        k, q = 1024, q + 1
    if k < 1024:
        return sign | k
    be = q + 25
    return sign | (0x7C00 if be >= 31 else (be << 10) | (k & 1023))


def fnma_exact(m, u, x):
    """fma(-m, u, x) by IEEE 754 on bit patterns; the product and the sum are exact integers in units of 2^-48."""
    m, u, x = int(m), int(u), int(x)
    if _isnan(m) or _isnan(u) or _isnan(x):
        return NAN16
    pneg = ((m ^ 0x8000 ^ u) >> 15) & 1
    if _isinf(m) or _isinf(u):
        if (m & 0x7FFF) == 0 or (u & 0x7FFF) == 0:
            return NAN16
        pinf = 0x7C00 | (pneg << 15)
        if _isinf(x):
            return x if x == pinf else NAN16
        return pinf
    if _isinf(x):
        return x
    return round16((value24(x) << 24) - value24(m) * value24(u), -48, zero_sign=pneg & (x >> 15))


def _mul(m, u):
    m, u = int(m), int(u)
    sign = (m ^ u) & 0x8000
    if _isnan(m) or _isnan(u):
        return NAN16
    if _isinf(m) or _isinf(u):
        return NAN16 if (m & 0x7FFF) == 0 or (u & 0x7FFF) == 0 else 0x7C00 | sign
    return round16(value24(m) * value24(u), -48, zero_sign=sign >> 15)


def _sub(x, t):
    x, t = int(x), int(t) ^ 0x8000
    if _isnan(x) or _isnan(t):
        return NAN16
    if _isinf(x) or _isinf(t):
        if _isinf(x) and _isinf(t):
            return x if x == t else NAN16
        return x if _isinf(x) else t
    return round16(value24(x) + value24(t), -24, zero_sign=(x >> 15) & (t >> 15))


def _div(a, b):
    """IEEE fp32 quotient rounded once to binary16 (numpy's float32 division is IEEE)."""
    with np.errstate(all="ignore"):
        q = np.float32(np.uint16(a).view(np.float16)) / np.float32(np.uint16(b).view(np.float16))
    if np.isnan(q):
        return NAN16
    if np.isinf(q) or q == 0:
        return (0x8000 if np.signbit(q) else 0) | (0x7C00 if np.isinf(q) else 0)
    mant, ex = np.frexp(np.float64(q))                              # q = mant * 2^ex, 24 significant bits
    return round16(int(mant * (1 << 24)), int(ex) - 24)


def _gt(a, b):
    """__hgt on |values| given as bit patterns without sign: ordered compare, false for NaN."""
    if a > 0x7C00 or b > 0x7C00:
        return False
    return a > b


def literal_hgetf2(bits, fused):
    """hgetf2_kernel.cu:15-120, thread (bid, tid) simulated literally, in place on a (rows, cols) uint16 array."""
    rows, cols = bits.shape
    nblocks = (rows + BLOCK - 1) // BLOCK
    P = [[int(bits[r, c]) for c in range(cols)] for r in range(rows)]
    ipiv = np.zeros(cols, dtype=np.int32)
    for j in range(cols):
        g_vals, g_idx = [0] * nblocks, [j] * nblocks
        for bid in range(nblocks):                                    # :32-62
            max_vals, piv = [0] * BLOCK, [j] * BLOCK                  # :34-35
            for tid in range(BLOCK):
                row = bid * BLOCK + tid + j                           # :39
                if row < rows:
                    max_vals[tid], piv[tid] = P[row][j] & 0x7FFF, row  # :41 __habs
            stride = BLOCK // 2
            while stride > 0:                                         # :47-56
                for tid in range(stride):
                    if _gt(max_vals[tid + stride], max_vals[tid]):
                        max_vals[tid], piv[tid] = max_vals[tid + stride], piv[tid + stride]
                stride //= 2
            g_vals[bid], g_idx[bid] = max_vals[0], piv[0]             # :59-62
        gmax, gidx = g_vals[0], g_idx[0]                              # :70-78
        for b in range(1, nblocks):
            if _gt(g_vals[b], gmax):
                gmax, gidx = g_vals[b], g_idx[b]
        ipiv[j] = gidx + 1                                            # :80-81
        if gidx != j:                                                 # :92-98
            P[j], P[gidx] = P[gidx], P[j]
        pivot_val = P[j][j]
        for row in range(j + 1, rows):                                # :104-115, one thread per row
            mult = _div(P[row][j], pivot_val)                         # :108
            P[row][j] = mult                                          # :109
            for k in range(j + 1, cols):                              # :112-114
                P[row][k] = fnma_exact(mult, P[j][k], P[row][k]) if fused else _sub(P[row][k], _mul(mult, P[j][k]))
    bits[:, :] = np.array(P, dtype=np.uint16)
    return ipiv
