// Kernels of the error bounds for solves (mpf_block.cpp: mpf_gerfs; LAPACK dgerfs on the tiles of solve_block.hip): per-column
// reductions over tiles and the small elementwise steps of the forward bound's batched dlacn2.  (The fused residual and bound -- one
// pass over op(A) for op(A) X and |op(A)| |X| -- is blk_gemm_kernel's ABS form in solve_block.hip.)
// A column is reduced by ONE wave per chunk of CR rows: lane-strided partial sums, a fixed butterfly, the chunks combined in ascending
// order.  Nothing depends on the column's position or on the other columns, so a column's results have the same bits wherever it
// stands; no atomics, plain vector stores only.
#include "mpf_internal.h"

namespace {
constexpr int CR = 4096;   // rows per partial (64 lanes x 64)

__device__ __forceinline__ double wave_sum(double s) {   // butterfly: every lane ends with the same bits
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    return s;
}
__device__ __forceinline__ double maxn(double a, double b) { return (b > a || b != b) ? b : a; }   // max that keeps a NaN
__device__ __forceinline__ double wave_max(double s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s = maxn(s, __shfl_xor(s, o));
    return s;
}
// (|x| descending, index ascending): a total order, so the winner does not depend on the reduction's shape
__device__ __forceinline__ void amax_better(double &v, long long &k, double v2, long long k2) {
    if (v2 > v || (v2 == v && k2 < k)) { v = v2; k = k2; }
}
} // namespace

// OP: BR_AMAX   max_i |t_ij|, a NaN kept                                              part[0]
//     BR_ASUM   sum_i |t_ij| and the number of i with sign(t_ij) != sg_ij            part[0], part[1]      (sign(0) = +1, as dlacn2)
//     BR_IAMAX  the largest |t_ij| and the first i that has it                        part[0], part[1]
// part[(v * nchunks + chunk) * ncols + col]
enum { BR_AMAX = 0, BR_ASUM = 1, BR_IAMAX = 2 };
template <int OP>
__global__ __launch_bounds__(256) void blk_col_part_kernel(const double *__restrict__ T, long long ldt, long long n, long long ncols,
                                                           const double *__restrict__ sg, double *__restrict__ part) {
    const long long col = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (col >= ncols) return;                                     // (wave-uniform; no barrier below)
    const long long i0 = (long long)blockIdx.y * CR;
    const long long nr = (n - i0) < CR ? (n - i0) : CR;
    const double *t = T + col * ldt + i0;
    const long long nchunks = gridDim.y;
    double *p0 = part + (long long)blockIdx.y * ncols + col, *p1 = p0 + nchunks * ncols;
    if (OP == BR_IAMAX) {
        double v = -1.0;
        long long k = i0;                                         // (an all-NaN column beats nothing: its index is then 0, a valid row)
        for (int q = 0; q < CR / 64; ++q) {
            const long long i = lane + 64ll * q;
            if (i < nr) amax_better(v, k, fabs(t[i]), i0 + i);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double v2 = __shfl_xor(v, o);
            const long long k2 = __shfl_xor(k, o);
            amax_better(v, k, v2, k2);
        }
        if (lane == 0) { *p0 = v; *p1 = (double)k; }
        return;
    }
    double s[4] = {0, 0, 0, 0}, d = 0;
#pragma unroll 16
    for (int q = 0; q < CR / 64; ++q) {
        const long long i = lane + 64ll * q;
        if (i < nr) {
            const double e = t[i];
            if (OP == BR_AMAX) s[q & 3] = maxn(s[q & 3], fabs(e));
            else {
                s[q & 3] += fabs(e);
                if ((e >= 0 ? 1.0 : -1.0) != sg[col * ldt + i0 + i]) d += 1.0;
            }
        }
    }
    if (OP == BR_AMAX) {
        const double m = wave_max(maxn(maxn(s[0], s[1]), maxn(s[2], s[3])));
        if (lane == 0) *p0 = m;
    } else {
        const double a = wave_sum((s[0] + s[1]) + (s[2] + s[3]));
        d = wave_sum(d);                                          // (whole numbers below 2^53: exact in any order)
        if (lane == 0) { *p0 = a; *p1 = d; }
    }
}
// out[col], out[ncols + col] = the partials combined in ascending chunk order; BR_IAMAX: out[2 ncols + col] = T[at[col], col]
template <int OP>
__global__ __launch_bounds__(256) void blk_col_finish_kernel(const double *__restrict__ part, int nchunks, long long ncols,
                                                             const double *__restrict__ T, long long ldt, const int *__restrict__ at,
                                                             double *__restrict__ out) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= ncols) return;
    const double *p0 = part + j, *p1 = p0 + (long long)nchunks * ncols;
    if (OP == BR_IAMAX) {
        double v = -1.0;
        long long k = 1ll << 62;
        for (int ch = 0; ch < nchunks; ++ch) amax_better(v, k, p0[(long long)ch * ncols], (long long)p1[(long long)ch * ncols]);
        out[j] = v;
        out[ncols + j] = (double)k;
        out[2 * ncols + j] = T[(long long)at[j] + j * ldt];
        return;
    }
    double s = 0, d = 0;
    for (int ch = 0; ch < nchunks; ++ch) {
        const double p = p0[(long long)ch * ncols];
        s = OP == BR_AMAX ? maxn(s, p) : s + p;
        if (OP == BR_ASUM) d += p1[(long long)ch * ncols];
    }
    out[j] = s;
    if (OP == BR_ASUM) out[ncols + j] = d;
}
// One reduction of every column of the tiles T (n rows, ncols columns, ld = ldt): `what` 0 = max |t| (a NaN kept), 1 = sum |t| and the
// sign mismatches against sg, 2 = first argmax |t| and T[at[col], col] (0 <= at[col] < n).  The results land in c->blk_red: `ncols`
// doubles per value (1, 2 and 3 values); the partials lie behind them.
int launch_blk_col_reduce(mpf_ctx *c, int what, const double *T, int64_t ldt, int64_t n, int64_t ncols, const double *sg, const int *at) {
    const int nchunks = (int)((n + CR - 1) / CR);
    MPF_HIP_TRY(c, c->blk_red.grow((3 + 2 * (int64_t)nchunks) * ncols));
    double *out = c->blk_red, *part = out + 3 * ncols;
    dim3 grid((unsigned)((ncols + 3) / 4), (unsigned)nchunks);
    const unsigned fb = (unsigned)((ncols + 255) / 256);
    if (what == 0) {
        blk_col_part_kernel<BR_AMAX><<<grid, 256, 0, c->stream>>>(T, ldt, n, ncols, nullptr, part);
        blk_col_finish_kernel<BR_AMAX><<<fb, 256, 0, c->stream>>>(part, nchunks, ncols, T, ldt, nullptr, out);
    } else if (what == 1) {
        blk_col_part_kernel<BR_ASUM><<<grid, 256, 0, c->stream>>>(T, ldt, n, ncols, sg, part);
        blk_col_finish_kernel<BR_ASUM><<<fb, 256, 0, c->stream>>>(part, nchunks, ncols, T, ldt, nullptr, out);
    } else {
        blk_col_part_kernel<BR_IAMAX><<<grid, 256, 0, c->stream>>>(T, ldt, n, ncols, nullptr, part);
        blk_col_finish_kernel<BR_IAMAX><<<fb, 256, 0, c->stream>>>(part, nchunks, ncols, T, ldt, at, out);
    }
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

// v[i, j] *= w[i, j] on whole tiles
__global__ __launch_bounds__(256) void blk_scale_kernel(double *__restrict__ v, const double *__restrict__ w, long long ldt) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= ldt) return;
    v[i + j * ldt] *= w[i + j * ldt];
}
int launch_blk_scale(mpf_ctx *c, double *v, const double *w, int64_t ldt, int ntiles) {
    dim3 grid((unsigned)((ldt + 255) / 256), (unsigned)(BLK_T * ntiles));
    blk_scale_kernel<<<grid, 256, 0, c->stream>>>(v, w, ldt);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}
// dgerfs's weights of the forward bound from the last residual and bound: w <- |r| + nzeps w, + safe1 where w was <= safe2
// (rows n .. and columns ncols .. stay zero)
__global__ __launch_bounds__(256) void blk_ferr_weight_kernel(const double *__restrict__ r, double *__restrict__ w, long long n, long long ldt,
                                                              double nzeps, double safe1, double safe2) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= n) return;
    const double wv = w[i + j * ldt], t = fabs(r[i + j * ldt]) + nzeps * wv;
    w[i + j * ldt] = wv > safe2 ? t : t + safe1;
}
int launch_blk_ferr_weight(mpf_ctx *c, const double *r, double *w, int64_t n, int64_t ncols, int64_t ldt, double nzeps, double safe1,
                           double safe2) {
    if (ncols <= 0) return 0;
    dim3 grid((unsigned)((n + 255) / 256), (unsigned)ncols);
    blk_ferr_weight_kernel<<<grid, 256, 0, c->stream>>>(r, w, n, ldt, nzeps, safe1, safe2);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}
// dlacn2's start vectors, per column: kind[j] 0 = 1/n everywhere, 1 = e_at[j], 2 = x_i = (-1)^i (1 + i / (n - 1)), 3 = zero (a column
// that has finished and only rides along), anything else: the column is left as it is
__global__ __launch_bounds__(256) void blk_lacn2_fill_kernel(double *__restrict__ v, long long n, long long ldt, const int *__restrict__ kind,
                                                             const int *__restrict__ at) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    const int kd = kind[j];
    if (i >= n || kd < 0 || kd > 3) return;
    double x = 0.0;
    if (kd == 0) x = 1.0 / (double)n;
    else if (kd == 1) x = i == at[j] ? 1.0 : 0.0;
    else if (kd == 2) x = (i & 1 ? -1.0 : 1.0) * (1.0 + (double)i / (double)(n - 1));
    v[i + j * ldt] = x;
}
int launch_blk_lacn2_fill(mpf_ctx *c, double *v, int64_t n, int64_t ncols, int64_t ldt, const int *kind, const int *at) {
    if (ncols <= 0) return 0;
    dim3 grid((unsigned)((n + 255) / 256), (unsigned)ncols);
    blk_lacn2_fill_kernel<<<grid, 256, 0, c->stream>>>(v, n, ldt, kind, at);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}
// dlacn2's sign step: where live[j], v = isgn = sign(v) (+1 for 0); a column that has finished is cleared, so that the passes it still
// rides along in work on zeros
__global__ __launch_bounds__(256) void blk_lacn2_sign_kernel(double *__restrict__ v, double *__restrict__ isgn, long long n, long long ldt,
                                                             const int *__restrict__ live) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= n) return;
    if (!live[j]) { v[i + j * ldt] = 0.0; return; }
    const double s = v[i + j * ldt] >= 0 ? 1.0 : -1.0;
    v[i + j * ldt] = s;
    isgn[i + j * ldt] = s;
}
int launch_blk_lacn2_sign(mpf_ctx *c, double *v, double *isgn, int64_t n, int64_t ncols, int64_t ldt, const int *live) {
    if (ncols <= 0) return 0;
    dim3 grid((unsigned)((n + 255) / 256), (unsigned)ncols);
    blk_lacn2_sign_kernel<<<grid, 256, 0, c->stream>>>(v, isgn, n, ldt, live);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}
