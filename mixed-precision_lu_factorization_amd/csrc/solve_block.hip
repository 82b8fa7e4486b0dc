// Kernels of the blocked multi-right-hand-side solve (mpf_block.cpp: mpf_getrs, mpf_solve_ir_block).
// Right-hand sides live in TILES: column-major, BLK_T columns per tile, `ldt` = N rounded up to 256 rows, rows N .. ldt - 1 and
// the columns beyond nrhs zero.  Every product is one kernel, blk_gemm_kernel, on v_mfma_f64_16x16x4_f64:
//     O[m, c]  (=, or -=)  sum_k op(F)[m, k] Y[k, c]          op(F)[m, k] = F[fr0 + m, fc0 + k]  or  F[fr0 + k, fc0 + m] (TR)
// for a 64 x BLK_T block of O per workgroup and one tile per blockIdx.y.  It is the diagonal step of the triangular solves
// (Y_k = inv256(F_kk) B_k, inv256 from launch_trsv_prepare), their update step (B_rows -= F_rows,k Y_k) and the residual's
// GEMM (partials per 4096-column chunk, reduced in ascending chunk order).  The K order of every element is fixed (32-wide chunks
// ascending, four k per MFMA, the same for every column and every tile position) and a column's arithmetic reads no other
// column: X[:, j] has the same bits whatever the other columns, nrhs or j's position.  No atomics; plain vector stores only.
#include "mpf_internal.h"

namespace {
typedef double d4_t __attribute__((ext_vector_type(4)));
constexpr int TW = 256;        // diagonal block of the solves (ir.hip's 256 x 256 inverses)
constexpr int BM = 64;         // rows of O per workgroup (16 per wave)
constexpr int BK = 32;         // K chunk staged in LDS (64: 10.1 ms against 9.4 for getrs of 64 columns at N = 32768)
constexpr int BT = BLK_T;      // tile width
constexpr int RKC = 4096;      // columns of A per partial of the residual
static_assert(BT == 32, "the wave layout below covers two 16-column MFMA tiles");
static_assert(TW % BK == 0 && BK % 4 == 0, "a diagonal block is a whole number of K chunks");
} // namespace

// O = (or -=) op(F)[m0 .. m0 + 64, k0 .. k1) Y[k0 .. k1, tile] (k0 = blockIdx.z * kc, k1 = min(kw, k0 + kc)); rows of O from mlim
// on are neither read nor written, op(F) and Y read as zero from k1 on.  O of chunk z at O + z * ozs.
// ABS (the fused residual and bound of mpf_gerfs): a second accumulator pair takes |op(F)| |Y| from the same staged operands and goes
// to Oa (same layout as O).  Its plain product is summed in TWO levels: every staged chunk of BK = 32 k starts from zero and is then
// added to a running total (chunks ascending).  The componentwise backward error is measured against the residual's own rounding: one
// chain of 4096 accumulations reads 4 .. 5 x 2^-53 for an x that is correct to working precision, the two-level sum 0.9 (a BLAS
// product: 2.3), and dgerfs's stop rule and the caller both act on that figure.  So O's bits are NOT those of the kernel without ABS
// (launch_blk_residual); each form has one fixed order of its own.
template <bool TR, bool SUB, bool ABS = false>
__global__ __launch_bounds__(256) void blk_gemm_kernel(const double *__restrict__ F, long long ldf, long long fr0, long long fc0,
                                                       long long kw, long long kc, long long mlim, const double *__restrict__ Y,
                                                       long long ldy, double *__restrict__ O, long long ldo, long long ozs,
                                                       double *__restrict__ Oa = nullptr) {
    static_assert(!(ABS && SUB), "the bound is a plain product");
    __shared__ double As[BK][BM + 1], Ys[BK][BT + 1];
    const int tid = threadIdx.x, l = tid & 63, g = tid >> 6;
    const long long m0 = (long long)blockIdx.x * BM;
    const long long col0 = (long long)blockIdx.y * BT;
    const long long k0 = (long long)blockIdx.z * kc;
    const long long k1 = (k0 + kc) < kw ? (k0 + kc) : kw;
    const double *Yt = Y + col0 * ldy;
    double ra[BM * BK / 256], ry[BK * BT / 256];
    // staging map: op(F) chunk 64 x BK (lane along F's contiguous index), Y chunk BK x 32
    auto fetch = [&](long long kk) {
#pragma unroll
        for (int q = 0; q < BM * BK / 256; ++q) {
            const int m = TR ? (tid / BK) + (256 / BK) * q : (tid & 63);
            const int k = TR ? (tid % BK) : (tid >> 6) + 4 * q;
            const bool ok = m0 + m < mlim && kk + k < k1;
            ra[q] = ok ? (TR ? F[(fr0 + kk + k) + (fc0 + m0 + m) * ldf] : F[(fr0 + m0 + m) + (fc0 + kk + k) * ldf]) : 0.0;
        }
#pragma unroll
        for (int q = 0; q < BK * BT / 256; ++q) {
            const int k = tid % BK, cc = (tid / BK) + (256 / BK) * q;
            ry[q] = kk + k < k1 ? Yt[(kk + k) + (long long)cc * ldy] : 0.0;
        }
    };
    d4_t acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
    d4_t abs0 = {0.0, 0.0, 0.0, 0.0}, abs1 = {0.0, 0.0, 0.0, 0.0}, tot0 = {0.0, 0.0, 0.0, 0.0}, tot1 = {0.0, 0.0, 0.0, 0.0};
    if (k0 < k1) fetch(k0);
    for (long long kk = k0; kk < k1; kk += BK) {
#pragma unroll
        for (int q = 0; q < BM * BK / 256; ++q) {
            const int m = TR ? (tid / BK) + (256 / BK) * q : (tid & 63);
            const int k = TR ? (tid % BK) : (tid >> 6) + 4 * q;
            As[k][m] = ra[q];
        }
#pragma unroll
        for (int q = 0; q < BK * BT / 256; ++q) Ys[tid % BK][(tid / BK) + (256 / BK) * q] = ry[q];
        __syncthreads();
        if (kk + BK < k1) fetch(kk + BK);   // the next chunk's loads fly under this chunk's MFMAs
#pragma unroll
        for (int s = 0; s < BK / 4; ++s) {
            const int kr = 4 * s + (l >> 4);
            const double a = As[kr][16 * g + (l & 15)];
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Ys[kr][l & 15], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Ys[kr][16 + (l & 15)], acc1, 0, 0, 0);
            if (ABS) {
                abs0 = __builtin_amdgcn_mfma_f64_16x16x4f64(fabs(a), fabs(Ys[kr][l & 15]), abs0, 0, 0, 0);
                abs1 = __builtin_amdgcn_mfma_f64_16x16x4f64(fabs(a), fabs(Ys[kr][16 + (l & 15)]), abs1, 0, 0, 0);
            }
        }
        if (ABS) {   // second level of the plain product's sum
            tot0 += acc0; tot1 += acc1;
            acc0 = d4_t{0.0, 0.0, 0.0, 0.0}; acc1 = d4_t{0.0, 0.0, 0.0, 0.0};
        }
        __syncthreads();
    }
    // f64 MFMA C/D map: column = lane & 15, row = (lane >> 4) + 4 * reg
    double *Ot = O + (long long)blockIdx.z * ozs + col0 * ldo;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long long row = m0 + 16 * g + (l >> 4) + 4 * i;
        if (row >= mlim) continue;
        double *o0 = Ot + row + (long long)(l & 15) * ldo, *o1 = o0 + 16ll * ldo;
        if (SUB) { *o0 = *o0 - acc0[i]; *o1 = *o1 - acc1[i]; }
        else if (ABS) { *o0 = tot0[i]; *o1 = tot1[i]; }
        else { *o0 = acc0[i]; *o1 = acc1[i]; }
        if (ABS) {
            double *a0 = Oa + (long long)blockIdx.z * ozs + col0 * ldo + row + (long long)(l & 15) * ldo;
            a0[0] = abs0[i];
            a0[16ll * ldo] = abs1[i];
        }
    }
}

template <bool TR, bool SUB, bool ABS = false>
static int blk_gemm(mpf_ctx *c, const double *F, int64_t ldf, int64_t fr0, int64_t fc0, int64_t kw, int64_t kc, int64_t mlim,
                    const double *Y, int64_t ldy, double *O, int64_t ldo, int64_t ozs, int ntiles, double *Oa = nullptr) {
    if (mlim <= 0 || kw <= 0) return 0;
    const int64_t nz = (kw + kc - 1) / kc;
    dim3 grid((unsigned)((mlim + BM - 1) / BM), (unsigned)ntiles, (unsigned)nz);
    blk_gemm_kernel<TR, SUB, ABS><<<grid, 256, 0, c->stream>>>(F, ldf, fr0, fc0, kw, kc, mlim, Y, ldy, O, ldo, ozs, Oa);
    return 0;
}

// One triangular pass over `ntiles` tiles: x (consumed) -> y (the solution).  which: 0 = L (unit lower, blocks ascending),
// 1 = U (descending), 2 = U^T (ascending), 3 = L^T (descending).  Two launches per 256-block: the diagonal product writes y_k,
// the update takes y_k out of the rows (or, transposed, the columns) the block still touches.  Needs launch_trsv_prepare.
int launch_blk_tri(mpf_ctx *c, const double *LU, int64_t ld, int64_t n, int which, double *x, double *y, int64_t ldt, int ntiles) {
    const int64_t nblk = (n + TW - 1) / TW;
    const bool asc = which == 0 || which == 2, useL = which == 0 || which == 3, tr = which >= 2;
    const double *inv = c->trsv_inv256 + (useL ? 0 : nblk * TW * TW);
    for (int64_t s = 0; s < nblk; ++s) {
        const int64_t k = asc ? s : nblk - 1 - s;
        const int64_t kb = k * TW, w = (n - kb) < TW ? (n - kb) : TW;
        const double *ik = inv + k * TW * TW;
        int rc = tr ? blk_gemm<true, false>(c, ik, TW, 0, 0, TW, TW, TW, x + kb, ldt, y + kb, ldt, 0, ntiles)
                    : blk_gemm<false, false>(c, ik, TW, 0, 0, TW, TW, TW, x + kb, ldt, y + kb, ldt, 0, ntiles);
        if (rc) return rc;
        switch (which) {
        case 0: rc = blk_gemm<false, true>(c, LU, ld, kb + w, kb, w, w, n - kb - w, y + kb, ldt, x + kb + w, ldt, 0, ntiles); break;
        case 1: rc = blk_gemm<false, true>(c, LU, ld, 0, kb, w, w, kb, y + kb, ldt, x, ldt, 0, ntiles); break;
        case 2: rc = blk_gemm<true, true>(c, LU, ld, kb, kb + w, w, w, n - kb - w, y + kb, ldt, x + kb + w, ldt, 0, ntiles); break;
        default: rc = blk_gemm<true, true>(c, LU, ld, kb, 0, w, w, kb, y + kb, ldt, x, ldt, 0, ntiles); break;
        }
        if (rc) return rc;
    }
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

// r = b - sum over the chunks in ascending order (rows n .. ldt - 1 of r: zero)
__global__ __launch_bounds__(256) void blk_res_reduce_kernel(const double *__restrict__ part, int nchunks, long long zs,
                                                             const double *__restrict__ b, double *__restrict__ r, long long n, long long ldt) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= ldt) return;
    const long long e = i + (long long)blockIdx.y * ldt;
    double s = 0;
    if (i < n)
        for (int ch = 0; ch < nchunks; ++ch) s += part[ch * zs + e];
    r[e] = i < n ? b[e] - s : 0.0;
}
// R = B - op(A) X on `ntiles` tiles (op = A^T when trans): op(A) streamed once per tile, partial products per 4096 columns, at most
// RES_TILES tiles per launch (bounds the partials: 8 x 32768 x 64 doubles at N = 32768)
constexpr int RES_TILES = 2;
int launch_blk_residual(mpf_ctx *c, const double *A, int64_t lda, int64_t n, bool trans, const double *X, const double *B, double *R,
                        int64_t ldt, int ntiles) {
    const int nch = (int)((n + RKC - 1) / RKC);
    const int64_t zs = ldt * BT * RES_TILES;
    MPF_HIP_TRY(c, c->blk_part.grow((int64_t)nch * zs));
    for (int t0 = 0; t0 < ntiles; t0 += RES_TILES) {
        const int nt = ntiles - t0 < RES_TILES ? ntiles - t0 : RES_TILES;
        const int64_t off = (int64_t)t0 * BT * ldt;
        int rc = trans ? blk_gemm<true, false>(c, A, lda, 0, 0, n, RKC, n, X + off, ldt, c->blk_part, ldt, zs, nt)
                       : blk_gemm<false, false>(c, A, lda, 0, 0, n, RKC, n, X + off, ldt, c->blk_part, ldt, zs, nt);
        if (rc) return rc;
        dim3 grid((unsigned)((ldt + 255) / 256), (unsigned)(BT * nt));
        blk_res_reduce_kernel<<<grid, 256, 0, c->stream>>>(c->blk_part, nch, zs, B + off, R + off, n, ldt);
    }
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

// The reduce step of the fused residual and bound: r = b - sum, w = |b| + sum_abs (both sums over the chunks in ascending order) and
// q = the componentwise backward error's ratio of the element, LAPACK dgerfs's: |r| / w where w > safe2, else (|r| + safe1) / (w + safe1).
// Rows n .. ldt - 1 of all three: zero.
__global__ __launch_bounds__(256) void blk_res_abs_reduce_kernel(const double *__restrict__ part, const double *__restrict__ parta, int nchunks,
                                                                 long long zs, const double *__restrict__ b, double *__restrict__ r,
                                                                 double *__restrict__ w, double *__restrict__ q, long long n, long long ldt,
                                                                 double safe1, double safe2) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= ldt) return;
    const long long e = i + (long long)blockIdx.y * ldt;
    double s = 0, sa = 0;
    if (i < n)
        for (int ch = 0; ch < nchunks; ++ch) { s += part[ch * zs + e]; sa += parta[ch * zs + e]; }
    const double rv = i < n ? b[e] - s : 0.0, wv = i < n ? fabs(b[e]) + sa : 0.0;
    r[e] = rv;
    w[e] = wv;
    q[e] = i < n ? (wv > safe2 ? fabs(rv) / wv : (fabs(rv) + safe1) / (wv + safe1)) : 0.0;
}
// R = B - op(A) X, W = |B| + |op(A)| |X| and Q = the backward error's ratio per element, in ONE pass over op(A) per tile: the residual's
// launches and partials with the second accumulator pair and the two-level sum of blk_gemm_kernel's ABS form
int launch_blk_residual_bound(mpf_ctx *c, const double *A, int64_t lda, int64_t n, bool trans, const double *X, const double *B, double *R,
                              double *W, double *Q, int64_t ldt, int ntiles, double safe1, double safe2) {
    const int nch = (int)((n + RKC - 1) / RKC);
    const int64_t zs = ldt * BT * RES_TILES;
    MPF_HIP_TRY(c, c->blk_part.grow(2 * (int64_t)nch * zs));
    double *pa = c->blk_part + (int64_t)nch * zs;
    for (int t0 = 0; t0 < ntiles; t0 += RES_TILES) {
        const int nt = ntiles - t0 < RES_TILES ? ntiles - t0 : RES_TILES;
        const int64_t off = (int64_t)t0 * BT * ldt;
        int rc = trans ? blk_gemm<true, false, true>(c, A, lda, 0, 0, n, RKC, n, X + off, ldt, c->blk_part, ldt, zs, nt, pa)
                       : blk_gemm<false, false, true>(c, A, lda, 0, 0, n, RKC, n, X + off, ldt, c->blk_part, ldt, zs, nt, pa);
        if (rc) return rc;
        dim3 grid((unsigned)((ldt + 255) / 256), (unsigned)(BT * nt));
        blk_res_abs_reduce_kernel<<<grid, 256, 0, c->stream>>>(c->blk_part, pa, nch, zs, B + off, R + off, W + off, Q + off, n, ldt, safe1, safe2);
    }
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

// tile <- caller's columns: t[i, j] = src[p(i) + j lds] for i < n, j < ncols (p = perm or identity), zero elsewhere in the tiles.
// SC: times s[p(i)], the scale of the MATRIX row the element comes from (s: n doubles, exact powers of two; read below n only).
// Without SC the kernel is the unscaled one, instruction for instruction: the flag is a template argument, not a factor of 1.0.
template <bool SC>
__global__ __launch_bounds__(256) void blk_load_kernel(const double *__restrict__ src, long long lds, const int *__restrict__ perm,
                                                       const double *__restrict__ s, long long n, long long ncols, double *__restrict__ t,
                                                       long long ldt) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= ldt) return;
    double v = 0.0;
    if (i < n && j < ncols) {
        const long long row = perm ? (long long)perm[i] : i;
        v = src[row + j * lds];
        if (SC) v *= s[row];
    }
    t[i + j * ldt] = v;
}
int launch_blk_load(mpf_ctx *c, const double *src, int64_t lds, const int *perm, int64_t n, int64_t ncols, double *t, int64_t ldt, int ntiles,
                    const double *scale) {
    dim3 grid((unsigned)((ldt + 255) / 256), (unsigned)(BT * ntiles));
    if (scale) blk_load_kernel<true><<<grid, 256, 0, c->stream>>>(src, lds, perm, scale, n, ncols, t, ldt);
    else blk_load_kernel<false><<<grid, 256, 0, c->stream>>>(src, lds, perm, nullptr, n, ncols, t, ldt);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}
// caller's columns <- tile: dst[p(i) + j ldd] = t[i, j] for i < n, j < ncols (p = perm: the scatter of the transposed solve).
// SC: times s[p(i)], the scale of the matrix row the element goes to.
template <bool SC>
__global__ __launch_bounds__(256) void blk_store_kernel(const double *__restrict__ t, long long ldt, const int *__restrict__ perm,
                                                        const double *__restrict__ s, long long n, double *__restrict__ dst, long long ldd) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= n) return;
    const long long row = perm ? (long long)perm[i] : i;
    double v = t[i + j * ldt];
    if (SC) v *= s[row];
    dst[row + j * ldd] = v;
}
int launch_blk_store(mpf_ctx *c, const double *t, int64_t ldt, const int *perm, int64_t n, int64_t ncols, double *dst, int64_t ldd,
                     const double *scale) {
    if (ncols <= 0) return 0;
    dim3 grid((unsigned)((n + 255) / 256), (unsigned)ncols);
    if (scale) blk_store_kernel<true><<<grid, 256, 0, c->stream>>>(t, ldt, perm, scale, n, dst, ldd);
    else blk_store_kernel<false><<<grid, 256, 0, c->stream>>>(t, ldt, perm, nullptr, n, dst, ldd);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}
// x[:, j] += d[:, j] where mask[j] != 0 (the columns still refining)
__global__ __launch_bounds__(256) void blk_masked_axpy_kernel(const double *__restrict__ d, const int *__restrict__ mask, double *__restrict__ x,
                                                              long long ldt) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= ldt || !mask[j]) return;
    x[i + j * ldt] += d[i + j * ldt];
}
int launch_blk_masked_axpy(mpf_ctx *c, const double *d, const int *mask, double *x, int64_t ldt, int ntiles) {
    dim3 grid((unsigned)((ldt + 255) / 256), (unsigned)(BT * ntiles));
    blk_masked_axpy_kernel<<<grid, 256, 0, c->stream>>>(d, mask, x, ldt);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}
