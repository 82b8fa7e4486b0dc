// Kernels of the extra-precise refinement (mpf_block.cpp: mpf_residual_x, mpf_gerfsx; LAPACK dgerfsx with the XBLAS residual) on the
// tiles of solve_block.hip: the residual R = B - op(A) X accumulated in twice the working precision, and the three per-column
// reductions a refinement step is steered by; and the componentwise backward error of mpf_gerfsx_scaled, one more reduction after the loop.
// The residual is VALU work (no MFMA form): every element is an unevaluated pair (hi, lo) that takes each product exactly,
//     p = a x,  e = fma(a, x, -p),  (hi, t) = TwoSum(hi, -p),  lo += t - e            (Dekker / Knuth; Ogita, Rump, Oishi's Dot2)
// which needs the separately rounded operations of -ffp-contract=off; the one fused operation is spelled __builtin_fma.  A workgroup
// owns a 64 x BLK_T block of R and stages op(A) and X chunks as blk_gemm_kernel does; a thread owns 2 rows x 4 columns (16 accumulator
// doubles), so one LDS read of 6 operands feeds 8 products of ten fp64 instructions each.  Each element has one fixed order -- k
// ascending inside a partial of 4096 columns of op(A), the partials (pairs themselves) added in ascending order to (b, 0), the result
// hi + lo rounded once -- which is the same for every column and tile position, and no column reads another: R[:, j] has the same bits
// whatever stands beside it.  No atomics; plain vector stores only.
#include "mpf_internal.h"
#include <cfloat>

namespace {
constexpr int BM = 64;         // rows of R per workgroup
constexpr int BK = 32;         // K chunk staged in LDS
constexpr int BT = BLK_T;      // tile width
constexpr int RKC = 4096;      // columns of op(A) per partial
constexpr int RES_TILES = 2;   // tiles per launch, as launch_blk_residual (bounds the partials)
static_assert(BT == 32 && BM == 64, "256 threads own 2 rows x 4 columns each");

// Knuth's TwoSum: s + t = a + b exactly, whatever the magnitudes
__device__ __forceinline__ void two_sum(double a, double b, double &s, double &t) {
    s = a + b;
    const double bb = s - a;
    t = (a - (s - bb)) + (b - bb);
}
// (hi, lo) -= a x: the product and the sum of the leading parts are exact, their errors are gathered in lo
__device__ __forceinline__ void pair_sub_product(double &hi, double &lo, double a, double x) {
    const double p = a * x, e = __builtin_fma(a, x, -p);
    double s, t;
    two_sum(hi, -p, s, t);
    hi = s;
    lo += t - e;
}
__device__ __forceinline__ double maxn(double a, double b) { return (b > a || b != b) ? b : a; }   // max that keeps a NaN
__device__ __forceinline__ double wave_max(double s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s = maxn(s, __shfl_xor(s, o));
    return s;
}
} // namespace

// Partial z = blockIdx.z: (Ph, Pl)[z * zs + tile element] = (0, 0) - sum over k in [z kc, min(n, (z + 1) kc)) of op(A)[m, k] X[k, c] as a
// pair; rows m >= n are not written.  Staging map and prefetch are blk_gemm_kernel's.
template <bool TR>
__global__ __launch_bounds__(256) void blk_xres_kernel(const double *__restrict__ A, long long lda, long long n, long long kc,
                                                       const double *__restrict__ X, long long ldt, double *__restrict__ Ph,
                                                       double *__restrict__ Pl, long long zs) {
    __shared__ double As[BK][BM + 1], Ys[BK][BT + 1];
    const int tid = threadIdx.x, rp = tid & 31, cq = tid >> 5;   // rows rp and rp + 32, columns 4 cq .. 4 cq + 3 of the block
    const long long m0 = (long long)blockIdx.x * BM;
    const long long col0 = (long long)blockIdx.y * BT;
    const long long k0 = (long long)blockIdx.z * kc;
    const long long k1 = (k0 + kc) < n ? (k0 + kc) : n;
    const double *Xt = X + col0 * ldt;
    double ra[BM * BK / 256], ry[BK * BT / 256];
    auto fetch = [&](long long kk) {
#pragma unroll
        for (int q = 0; q < BM * BK / 256; ++q) {
            const int m = TR ? (tid / BK) + (256 / BK) * q : (tid & 63);
            const int k = TR ? (tid % BK) : (tid >> 6) + 4 * q;
            const bool ok = m0 + m < n && kk + k < k1;
            ra[q] = ok ? (TR ? A[(kk + k) + (m0 + m) * lda] : A[(m0 + m) + (kk + k) * lda]) : 0.0;
        }
#pragma unroll
        for (int q = 0; q < BK * BT / 256; ++q) {
            const int k = tid % BK, cc = (tid / BK) + (256 / BK) * q;
            ry[q] = kk + k < k1 ? Xt[(kk + k) + (long long)cc * ldt] : 0.0;
        }
    };
    double hi0[4] = {0.0, 0.0, 0.0, 0.0}, lo0[4] = {0.0, 0.0, 0.0, 0.0}, hi1[4] = {0.0, 0.0, 0.0, 0.0}, lo1[4] = {0.0, 0.0, 0.0, 0.0};
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
        if (kk + BK < k1) fetch(kk + BK);   // the next chunk's loads fly under this chunk's arithmetic
#pragma unroll 8
        for (int k = 0; k < BK; ++k) {
            const double a0 = As[k][rp], a1 = As[k][rp + 32];
            double x[4];
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) x[cc] = Ys[k][4 * cq + cc];
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) {
                pair_sub_product(hi0[cc], lo0[cc], a0, x[cc]);
                pair_sub_product(hi1[cc], lo1[cc], a1, x[cc]);
            }
        }
        __syncthreads();
    }
    const long long base = (long long)blockIdx.z * zs + col0 * ldt;
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) {
        const long long e = base + (long long)(4 * cq + cc) * ldt + m0 + rp;
        if (m0 + rp < n) { Ph[e] = hi0[cc]; Pl[e] = lo0[cc]; }
        if (m0 + rp + 32 < n) { Ph[e + 32] = hi1[cc]; Pl[e + 32] = lo1[cc]; }
    }
}

// r = (b, 0) + the partial pairs in ascending order, hi + lo rounded once (rows n .. ldt - 1 of r: zero)
__global__ __launch_bounds__(256) void blk_xres_reduce_kernel(const double *__restrict__ ph, const double *__restrict__ pl, int nchunks,
                                                              long long zs, const double *__restrict__ b, double *__restrict__ r, long long n,
                                                              long long ldt) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= ldt) return;
    const long long e = i + (long long)blockIdx.y * ldt;
    double hi = 0.0, lo = 0.0;
    if (i < n) {
        hi = b[e];
        for (int ch = 0; ch < nchunks; ++ch) {
            double s, t;
            two_sum(hi, ph[ch * zs + e], s, t);
            hi = s;
            lo += t + pl[ch * zs + e];
        }
    }
    r[e] = hi + lo;
}

// R = B - op(A) X on `ntiles` tiles with the residual accumulated in pairs (signature and tile conventions of launch_blk_residual; the
// partial pairs take twice its room in c->blk_part)
int launch_blk_residual_x(mpf_ctx *c, const double *A, int64_t lda, int64_t n, bool trans, const double *X, const double *B, double *R,
                          int64_t ldt, int ntiles) {
    const int nch = (int)((n + RKC - 1) / RKC);
    const int64_t zs = ldt * BT * RES_TILES;
    MPF_HIP_TRY(c, c->blk_part.grow(2 * (int64_t)nch * zs));
    double *ph = c->blk_part, *pl = ph + (int64_t)nch * zs;
    for (int t0 = 0; t0 < ntiles; t0 += RES_TILES) {
        const int nt = ntiles - t0 < RES_TILES ? ntiles - t0 : RES_TILES;
        const int64_t off = (int64_t)t0 * BT * ldt;
        dim3 grid((unsigned)((n + BM - 1) / BM), (unsigned)nt, (unsigned)nch);
        if (trans) blk_xres_kernel<true><<<grid, 256, 0, c->stream>>>(A, lda, n, RKC, X + off, ldt, ph, pl, zs);
        else blk_xres_kernel<false><<<grid, 256, 0, c->stream>>>(A, lda, n, RKC, X + off, ldt, ph, pl, zs);
        dim3 rgrid((unsigned)((ldt + 255) / 256), (unsigned)(BT * nt));
        blk_xres_reduce_kernel<<<rgrid, 256, 0, c->stream>>>(ph, pl, nch, zs, B + off, R + off, n, ldt);
    }
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

// The three measures of a refinement step, one workgroup per column: out[j] = max_i |x_i|, out[ncols + j] = max_i |d_i|,
// out[2 ncols + j] = max_i q_i with q_i = |d_i| / |x_i| where x_i != 0, else DBL_MAX where d_i != 0, else 0.  A NaN anywhere in the
// column makes the value NaN (a maximum has no order to fix: the bits do not depend on the reduction's shape).
__global__ __launch_bounds__(256) void blk_xr_measure_kernel(const double *__restrict__ X, const double *__restrict__ D, long long ldt,
                                                             long long n, long long ncols, double *__restrict__ out) {
    __shared__ double part[3][4];
    const long long j = blockIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const double *x = X + j * ldt, *d = D + j * ldt;
    double mx = 0.0, md = 0.0, mq = 0.0;
    for (long long i = threadIdx.x; i < n; i += 256) {
        const double xv = x[i], dv = d[i], ax = fabs(xv), ad = fabs(dv);
        mx = maxn(mx, ax);
        md = maxn(md, ad);
        mq = maxn(mq, xv != 0 ? ad / ax : (dv != dv ? dv : (dv != 0 ? DBL_MAX : 0.0)));
    }
    mx = wave_max(mx);
    md = wave_max(md);
    mq = wave_max(mq);
    if (lane == 0) { part[0][w] = mx; part[1][w] = md; part[2][w] = mq; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const double *p = part[threadIdx.x];
        out[(long long)threadIdx.x * ncols + j] = maxn(maxn(p[0], p[1]), maxn(p[2], p[3]));
    }
}
// One launch for all columns of the tiles X and D; the results land in c->blk_red: 3 x ncols doubles
int launch_blk_xr_measure(mpf_ctx *c, const double *X, const double *D, int64_t ldt, int64_t n, int64_t ncols) {
    if (ncols <= 0) return 0;
    MPF_HIP_TRY(c, c->blk_red.grow(3 * ncols));
    blk_xr_measure_kernel<<<(unsigned)ncols, 256, 0, c->stream>>>(X, D, ldt, n, ncols, c->blk_red);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

// dgerfs's componentwise backward error of mpf_gerfsx_scaled, one workgroup per column: out[j] = max_i of blk_res_abs_reduce_kernel's
// quotient (solve_block.hip) on the pair residual r and the weights w = |b| + |op(A)| |x|.  A NaN in r or w makes the value NaN.
__global__ __launch_bounds__(256) void blk_xr_berr_kernel(const double *__restrict__ R, const double *__restrict__ W, long long ldt,
                                                          long long n, double safe1, double safe2, double *__restrict__ out) {
    __shared__ double part[4];
    const long long j = blockIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const double *r = R + j * ldt, *wt = W + j * ldt;
    double m = 0.0;
    for (long long i = threadIdx.x; i < n; i += 256) {
        const double rv = fabs(r[i]), wv = wt[i];
        m = maxn(m, wv > safe2 ? rv / wv : (rv + safe1) / (wv + safe1));
    }
    m = wave_max(m);
    if (lane == 0) part[w] = m;
    __syncthreads();
    if (threadIdx.x == 0) out[j] = maxn(maxn(part[0], part[1]), maxn(part[2], part[3]));
}
// One launch for all columns of the tiles R and W; the results land in c->blk_red: ncols doubles
int launch_blk_xr_berr(mpf_ctx *c, const double *R, const double *W, int64_t ldt, int64_t n, int64_t ncols, double safe1, double safe2) {
    if (ncols <= 0) return 0;
    MPF_HIP_TRY(c, c->blk_red.grow(ncols));
    blk_xr_berr_kernel<<<(unsigned)ncols, 256, 0, c->stream>>>(R, W, ldt, n, safe1, safe2, c->blk_red);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}
