/* The fp16 pivot panel of the reference (hgetf2_kernel.cu:15-120) with the rank-1 step under either rounding contract:
 *   fused = 0 (C2):  t = round16(m * u);  x = round16(x - t)
 *   fused = 1 (C2f): x = round16(x - m * u)   -- fma(-m, u, x), ONE rounding
 * The shared library behind tests/hgetf2_fused_model.py (compiled by the tests, plain C, no fp16 hardware or compiler type).
 *
 * Every arithmetic result is formed EXACTLY and rounded once by round16_fixed().  Finite binary16 values are integer
 * multiples of 2^-24 below 2^16, so a value is an integer of at most 41 bits in units of 2^-24, a product one of at most
 * 81 bits in units of 2^-48, and x - m * u fits a signed 128-bit integer in units of 2^-48 with room to spare.  The panel
 * loop takes a shorter way where it is provably the same: x and m * u are exact doubles, their double sum s comes with its
 * exact error e (Knuth's two-sum); e == 0 means s IS the exact result and is rounded once from its bits, anything else goes
 * through the 128-bit path.  (An fp32 fma followed by a rounding to fp16 would be a double rounding: hfm_fma32_n is kept
 * for the tests that show the difference.)
 * The pivot search is the reference's, thread by thread: 256-row blocks of t = row - j, a strict-'>' tree over strides
 * 128 .. 1 inside a block, a strict-'>' serial scan over the blocks; '>' is false for NaN. */
#include <math.h>
#include <stdint.h>
#include <string.h>

typedef __int128 i128;
typedef unsigned __int128 u128;

#define H_NAN 0x7E00u
#define H_INF 0x7C00u

static int h_isnan(unsigned h) { return (h & 0x7FFFu) > H_INF; }
static int h_isinf(unsigned h) { return (h & 0x7FFFu) == H_INF; }
static int h_iszero(unsigned h) { return (h & 0x7FFFu) == 0; }

/* |h| as an integer in units of 2^-24 (finite h) */
static int64_t h_mag24(unsigned h) {
    const unsigned e = (h >> 10) & 31u, f = h & 1023u;
    return e ? (int64_t)(1024u | f) << (e - 1) : (int64_t)f;
}
static double h_table[65536];
static int h_table_done;
static void h_table_init(void) {
    for (unsigned h = 0; h < 65536; ++h) {
        const double v = ldexp((double)h_mag24(h), -24);
        h_table[h] = (h & 0x8000u) ? -v : v;
    }
    h_table_done = 1;
}
static double h_double(unsigned h) { return h_table[h & 0xFFFFu]; }   /* finite h, exact */

/* mag * 2^unit_exp (mag > 0, exact) -> binary16 bits with the given sign: round to nearest, ties to even, subnormals kept,
 * overflow to infinity */
static unsigned round16_fixed(u128 mag, int unit_exp, unsigned sign) {
    const uint64_t hi = (uint64_t)(mag >> 64), lo = (uint64_t)mag;
    const int top = hi ? 127 - __builtin_clzll(hi) : 63 - __builtin_clzll(lo);   /* mag = 1.xxx * 2^(top + unit_exp) */
    int e = top + unit_exp;                        /* binade of the value */
    int q = (e < -14 ? -14 : e) - 10;              /* the result is a multiple of 2^q */
    int sh = q - unit_exp;                         /* drop sh low bits of mag */
    u128 kept;
    if (sh <= 0) kept = mag << (-sh);              /* exact (cannot overflow: top + (-sh) <= 10) */
    else if (sh > 127) kept = 0;                   /* far below half of the smallest subnormal (mag < 2^127 <= half) */
    else {
        kept = mag >> sh;
        const u128 rem = mag & (((u128)1 << sh) - 1), half = (u128)1 << (sh - 1);
        if (rem > half || (rem == half && (kept & 1))) ++kept;
    }
    /* kept in [0, 2048]: multiples of 2^q */
    if (kept == 2048) { kept = 1024; ++q; if (e < -14) { /* cannot happen: subnormal keeps < 1024 before rounding */ } }
    unsigned bits;
    if (kept < 1024) bits = (unsigned)kept;                         /* subnormal or zero (q = -24) */
    else {
        const int be = q + 10 + 15;                                 /* biased exponent */
        if (be >= 31) bits = H_INF;
        else bits = ((unsigned)be << 10) | ((unsigned)kept & 1023u);
    }
    return bits | sign;
}

/* a + b for two exact terms given as signed integers in units of 2^unit_exp, with the signs the terms carry when they are
 * zero (IEEE: an exact zero sum is +0 unless both terms are negative) */
static unsigned round16_sum(i128 a, unsigned a_neg, i128 b, unsigned b_neg, int unit_exp) {
    const i128 s = a + b;
    if (s == 0) return (a_neg && b_neg) ? 0x8000u : 0u;
    return s < 0 ? round16_fixed((u128)(-s), unit_exp, 0x8000u) : round16_fixed((u128)s, unit_exp, 0u);
}

/* a double that holds the exact result (non-zero, finite) -> binary16, one rounding */
static unsigned round16_double(double s) {
    uint64_t b;
    memcpy(&b, &s, 8);                                         /* (a normal double: every value here is a multiple of 2^-149 or larger) */
    const unsigned sign = (unsigned)(b >> 63) << 15;
    const int e = (int)((b >> 52) & 0x7FF) - 1023;             /* |s| = mant * 2^(e - 52), 2^52 <= mant < 2^53 */
    const uint64_t mant = (b & ((1ull << 52) - 1)) | (1ull << 52);
    int q = (e < -14 ? -14 : e) - 10;                          /* as in round16_fixed, in 64 bits: sh >= 42 */
    const int sh = q - (e - 52);
    if (sh > 63) return sign;                                  /* |s| < 2^-34: far below half of the smallest subnormal */
    uint64_t kept = mant >> sh;
    const uint64_t rem = mant & ((1ull << sh) - 1), half = 1ull << (sh - 1);
    if (rem > half || (rem == half && (kept & 1))) ++kept;
    if (kept == 2048) { kept = 1024; ++q; }
    if (kept < 1024) return sign | (unsigned)kept;
    return sign | (q + 25 >= 31 ? H_INF : ((unsigned)(q + 25) << 10) | ((unsigned)kept & 1023u));
}
/* round16(m * u) */
static unsigned h_mul(unsigned m, unsigned u) {
    const unsigned sign = (m ^ u) & 0x8000u;
    if (h_isnan(m) || h_isnan(u)) return H_NAN;
    if (h_isinf(m) || h_isinf(u)) return (h_iszero(m) || h_iszero(u)) ? H_NAN : (H_INF | sign);
    const double p = h_double(m) * h_double(u);    /* two 11-bit significands: the double product is exact */
    return p == 0.0 ? sign : round16_double(p);
}
/* round16(x - t) */
static unsigned h_sub(unsigned x, unsigned t) {
    if (h_isnan(x) || h_isnan(t)) return H_NAN;
    const unsigned tn = t ^ 0x8000u;
    if (h_isinf(x) || h_isinf(tn)) {
        if (h_isinf(x) && h_isinf(tn)) return x == tn ? x : H_NAN;
        return h_isinf(x) ? x : tn;
    }
    const double s = h_double(x) + h_double(tn);   /* multiples of 2^-24 below 2^16: the double sum is exact */
    if (s == 0.0) return (x & tn & 0x8000u);       /* IEEE: an exact zero sum is +0 unless both terms are negative */
    return round16_double(s);
}
/* round16(x - m * u) = fma(-m, u, x): the exact 128-bit path */
static unsigned h_fnma_exact(unsigned m, unsigned u, unsigned x) {
    if (h_isnan(m) || h_isnan(u) || h_isnan(x)) return H_NAN;
    const unsigned pneg = (((m ^ 0x8000u) ^ u) >> 15) & 1;    /* sign of (-m) * u */
    if (h_isinf(m) || h_isinf(u)) {
        if (h_iszero(m) || h_iszero(u)) return H_NAN;
        const unsigned pinf = H_INF | (pneg << 15);
        if (h_isinf(x)) return x == pinf ? x : H_NAN;
        return pinf;
    }
    if (h_isinf(x)) return x;
    const i128 pm = (i128)h_mag24(m) * (i128)h_mag24(u);
    const i128 xm = (i128)h_mag24(x) << 24;
    return round16_sum((x & 0x8000u) ? -xm : xm, x >> 15 & 1, pneg ? -pm : pm, pneg, -48);
}
/* the same through doubles where that is exact (see the head of the file) */
static unsigned h_fnma(unsigned m, unsigned u, unsigned x) {
    if (((m & 0x7C00u) == 0x7C00u) || ((u & 0x7C00u) == 0x7C00u) || ((x & 0x7C00u) == 0x7C00u)) return h_fnma_exact(m, u, x);
    const double a = h_double(x), b = -(h_double(m) * h_double(u));   /* the product of two 11-bit significands is exact */
    const double s = a + b;
    const double bb = s - a, e = (a - (s - bb)) + (b - bb);           /* two-sum: a + b = s + e exactly */
    if (e != 0.0 || s == 0.0) return h_fnma_exact(m, u, x);           /* (zeros: the sign rules live in the exact path) */
    return round16_double(s);
}
/* the '/' of hgetf2_kernel.cu:108: the IEEE fp32 quotient rounded once to fp16 */
static unsigned h_div(unsigned a, unsigned b) {
    if (h_isnan(a) || h_isnan(b)) return H_NAN;
    const unsigned sign = (a ^ b) & 0x8000u;
    if (h_isinf(a)) return h_isinf(b) ? H_NAN : (H_INF | sign);
    if (h_isinf(b)) return sign;
    if (h_iszero(b)) return h_iszero(a) ? H_NAN : (H_INF | sign);
    if (h_iszero(a)) return sign;
    volatile float fa = (float)h_double(a & 0x7FFFu), fb = (float)h_double(b & 0x7FFFu);
    const float q = fa / fb;                                   /* IEEE binary32 division */
    return round16_double((double)q) | sign;                   /* q > 0: far above fp32's subnormals */
}
static float h_abs_float(unsigned h) {   /* __habs for the search: NaN stays NaN */
    if (h_isnan(h)) return NAN;
    if (h_isinf(h)) return INFINITY;
    return (float)h_double(h & 0x7FFFu);
}

/* ---- exported: element-wise entry points for the tests ------------------------------------------------------------ */
void hfm_init(void) { if (!h_table_done) h_table_init(); }   /* once, before anything else (the Python wrapper does) */
void hfm_fnma_n(const uint16_t *m, const uint16_t *u, const uint16_t *x, uint16_t *out, int64_t n, int exact_only) {
    for (int64_t i = 0; i < n; ++i) out[i] = (uint16_t)(exact_only ? h_fnma_exact(m[i], u[i], x[i]) : h_fnma(m[i], u[i], x[i]));
}
void hfm_mulsub_n(const uint16_t *m, const uint16_t *u, const uint16_t *x, uint16_t *out, int64_t n) {
    for (int64_t i = 0; i < n; ++i) out[i] = (uint16_t)h_sub(x[i], h_mul(m[i], u[i]));
}
void hfm_div_n(const uint16_t *a, const uint16_t *b, uint16_t *out, int64_t n) {
    for (int64_t i = 0; i < n; ++i) out[i] = (uint16_t)h_div(a[i], b[i]);
}
/* NOT the contract: fmaf in binary32, then a second rounding to binary16 (finite operands only) */
void hfm_fma32_n(const uint16_t *m, const uint16_t *u, const uint16_t *x, uint16_t *out, int64_t n) {
    for (int64_t i = 0; i < n; ++i) {
        const float r = fmaf(-(float)h_double(m[i]), (float)h_double(u[i]), (float)h_double(x[i]));
        out[i] = (uint16_t)(r == 0.0f ? (signbit(r) ? 0x8000u : 0u) : isinf(r) ? (H_INF | (r < 0 ? 0x8000u : 0u)) : round16_double((double)r));
    }
}

/* ---- exported: the panel -------------------------------------------------------------------------------------------- */
/* panel: rows x cols binary16 bit patterns, column-major with leading dimension ld, factored in place; ipiv: 1-based */
void hfm_hgetf2(uint16_t *panel, int64_t ld, int rows, int cols, int32_t *ipiv, int fused) {
    enum { BLOCK = 256 };
    float max_vals[BLOCK];
    int piv[BLOCK];
    uint16_t urow[65536];
    for (int j = 0; j < cols; ++j) {
        uint16_t *cj = panel + (int64_t)j * ld;
        const int nblocks = (rows + BLOCK - 1) / BLOCK;            /* the grid is sized for the whole panel (:6) */
        float gmax = 0.0f;
        int gidx = j;
        for (int bid = 0; bid < nblocks; ++bid) {                  /* :32-62 */
            for (int tid = 0; tid < BLOCK; ++tid) {
                const int row = bid * BLOCK + tid + j;
                max_vals[tid] = 0.0f; piv[tid] = j;
                if (row < rows) { max_vals[tid] = h_abs_float(cj[row]); piv[tid] = row; }
            }
            for (int stride = BLOCK / 2; stride > 0; stride >>= 1) /* :47-56 */
                for (int tid = 0; tid < stride; ++tid)
                    if (max_vals[tid + stride] > max_vals[tid]) { max_vals[tid] = max_vals[tid + stride]; piv[tid] = piv[tid + stride]; }
            if (bid == 0 || max_vals[0] > gmax) { gmax = max_vals[0]; gidx = piv[0]; }   /* :70-78 */
        }
        ipiv[j] = gidx + 1;                                        /* :80-81 */
        if (gidx != j)                                             /* :92-98 */
            for (int c = 0; c < cols; ++c) {
                uint16_t *col = panel + (int64_t)c * ld;
                const uint16_t t = col[j]; col[j] = col[gidx]; col[gidx] = t;
            }
        if (j + 1 >= rows) continue;
        const unsigned pivot_val = cj[j];
        for (int k = j + 1; k < cols; ++k) urow[k] = panel[j + (int64_t)k * ld];
        for (int r = j + 1; r < rows; ++r) cj[r] = (uint16_t)h_div(cj[r], pivot_val);   /* :108-109 */
        for (int k = j + 1; k < cols; ++k) {                       /* :112-114 */
            uint16_t *ck = panel + (int64_t)k * ld;
            const unsigned u = urow[k];
            if (fused) for (int r = j + 1; r < rows; ++r) ck[r] = (uint16_t)h_fnma(cj[r], u, ck[r]);
            else for (int r = j + 1; r < rows; ++r) ck[r] = (uint16_t)h_sub(ck[r], h_mul(cj[r], u));
        }
    }
}
