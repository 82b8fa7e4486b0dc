// Kernels of the expert solve driver (mpf_expert.cpp): transposed triangular solves with the packed factors, the A^T x GEMV,
// matrix norms, equilibration factors and the dlacn2 vector helpers of the condition estimator.
// Every reduction has one fixed summation order (per-chunk partials combined in ascending order, fixed butterflies inside a
// wave, no floating-point atomics): every entry point returns the same bits when called twice.  Global memory is written with
// plain vector stores (and the relaxed agent-scope stores / counter adds of the solve steps' hand-off, as in ir.hip).
#include "mpf_internal.h"

namespace {
constexpr int TW = 256;          // diagonal block of the single-GPU solves (ir.hip's 256 x 256 inverses)
constexpr int TS_NEAR = TW / 64; // update workgroups that cover the next diagonal block
constexpr int CR = 4096;         // rows per partial of the column-dot kernels (64 lanes x 64)
constexpr int RCH = 512;         // columns per partial of the row kernels

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
} // namespace

// ---- transposed triangular solves ------------------------------------------------------------------------------------------------
// One step of  U^T w = b  (UT: blocks ascending, inverse of U's diagonal block transposed) or  L^T z = w  (!UT: blocks descending,
// L's).  The structure and the hand-off are trsv_step_kernel's (ir.hip): `kb` = first row of the block whose solution y[kb ..] is
// known (kb < 0: none yet), `kn` = the block this launch solves (kn < 0: none).  Update workgroups own 64 COLUMNS j each, nearest to
// the solved block first:  x[j] -= sum_i F[kb + i, j] y[kb + i]  -- the block ROW of F, read as contiguous column segments: each
// wave takes 16 columns, lane l reads rows l, l + 64, l + 128, l + 192 of every one and the wave reduces (fixed butterfly).  The
// first `nnear` update workgroups hold the next block's entries: write-through stores, s_waitcnt vmcnt(0) in every wave, barrier,
// one relaxed agent-scope add.  Diag workgroups nnear .. nnear + 3 poll (bounded; a give-up counts in *timeouts), then read x with
// sc1 loads and form  y[kn + c] = sum_k inv[k][c] x[kn + k]  (inv(F^T) = inv(F)^T).
template <bool UT>
__global__ __launch_bounds__(256) void trsv_t_step_kernel(const double *__restrict__ F, long long ld, const double *__restrict__ inv256n,
                                                          double *x, double *y, long long n, long long kb, int w, long long kn, int nnear,
                                                          int nupd, int *cnt, long long spin_limit, int *timeouts) {
    __shared__ double ys[TW], part[4 * 64];
    const int tid = threadIdx.x, r = tid & 63, g = tid >> 6;
    const int b = blockIdx.x;
    const bool diag = kn >= 0 && b >= nnear && b < nnear + 4;
    if (diag) {
        const int p = b - nnear;                         // entries 64 p .. of the next block
        const int wn = (int)((n - kn) < TW ? (n - kn) : TW);
        // thread (r, g): inv[64 g + j][64 p + r], j = 0 .. 63 -- a contiguous run of the inverse's column 64 p + r
        double iv[64];
        const double2 *ip = reinterpret_cast<const double2 *>(inv256n + 64 * g + (long long)(64 * p + r) * TW);
#pragma unroll
        for (int j = 0; j < 32; ++j) { const double2 t = ip[j]; iv[2 * j] = t.x; iv[2 * j + 1] = t.y; }
        if (nnear > 0) {
            if (tid == 0) {
                long long spins = 0;
                while (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < nnear) {
                    __builtin_amdgcn_s_sleep(1);
                    if (++spins > spin_limit) { atomicAdd(timeouts, 1); break; }
                }
            }
            __syncthreads();
        }
        ys[tid] = tid < wn ? __hip_atomic_load(&x[kn + tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
        __syncthreads();
        double sa[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 64; ++j) sa[j & 3] += iv[j] * ys[64 * g + j];
        part[g * 64 + r] = (sa[0] + sa[1]) + (sa[2] + sa[3]);
        __syncthreads();
        if (g == 0 && 64 * p + r < wn) y[kn + 64 * p + r] = (part[r] + part[64 + r]) + (part[128 + r] + part[192 + r]);
        return;
    }
    if (kb < 0) return;
    const int u = (kn >= 0 && b >= nnear + 4) ? b - 4 : b;
    if (u >= nupd) return;                                         // (workgroup-uniform)
    ys[tid] = tid < w ? y[kb + tid] : 0.0;
    __syncthreads();
    const long long col0 = (UT ? kb + w + 64ll * u : kb - 64ll * (u + 1)) + 16 * g;
    double v[16][4];                                               // all 64 loads of the lane in flight together
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const long long col = col0 + q;
        const bool live = col < n;
        const double *f = F + kb + col * ld;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[q][k] = (live && r + 64 * k < w) ? f[r + 64 * k] : 0.0;
    }
    const double y0 = ys[r], y1 = ys[r + 64], y2 = ys[r + 128], y3 = ys[r + 192];
    double mine = 0.0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const double s = wave_sum((v[q][0] * y0 + v[q][1] * y1) + (v[q][2] * y2 + v[q][3] * y3));
        if (r == q) mine = s;
    }
    const bool near = kn >= 0 && u < nnear;
    const long long col = col0 + r;
    if (r < 16 && col < n) {
        const double nv = x[col] - mine;
        if (near) __hip_atomic_store(&x[col], nv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // read by another workgroup of this launch
        else x[col] = nv;
    }
    if (near) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's write-through stores of x have been acknowledged
        __syncthreads();
        if (tid == 0) __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// x is consumed, the solution lands in y.  Needs launch_trsv_prepare on the same factors (the 256 x 256 inverses).
template <bool UT>
static int trsv_t_wide(mpf_ctx *c, const double *LU, int64_t ld, double *x, double *y, int64_t n) {
    const int64_t nblk = (n + TW - 1) / TW;
    const double *inv = c->trsv_inv256 + (UT ? nblk * TW * TW : 0);   // U^T: U's inverses, L^T: L's
    int *cnt = c->trsv_cnt + (UT ? 0 : nblk + 1);
    MPF_HIP_TRY(c, hipMemsetAsync(cnt, 0, (size_t)(nblk + 1) * sizeof(int), c->stream));
    const long long spin = c->tune.hp_spin_limit;
    for (int64_t s = 0; s <= nblk; ++s) {
        const int64_t kcur = s == 0 ? -1 : (UT ? s - 1 : nblk - s);
        const int64_t knext = s == nblk ? -1 : (UT ? s : nblk - 1 - s);
        const long long kb = kcur < 0 ? -1 : kcur * TW, kn = knext < 0 ? -1 : knext * TW;
        const int w = kcur < 0 ? 0 : (int)((n - kb) < TW ? (n - kb) : TW);
        const int64_t cols = kcur < 0 ? 0 : (UT ? n - kb - w : kb);      // columns the known block still has to be taken out of
        const int nupd = (int)((cols + 63) / 64);
        const int nnear = knext < 0 ? 0 : (nupd < TS_NEAR ? nupd : TS_NEAR);
        const int grid = nupd + (knext >= 0 ? 4 : 0);
        if (grid == 0) continue;
        trsv_t_step_kernel<UT><<<grid, 256, 0, c->stream>>>(LU, ld, knext >= 0 ? inv + knext * TW * TW : inv, x, y, n, kb, w, kn, nnear, nupd,
                                                            cnt + s, spin, &c->ws->flags[0]);
    }
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}
int launch_trsv_upper_t(mpf_ctx *c, const double *LU, int64_t ld, double *x, int64_t n) {
    double *y = c->solve_buf + 3 * c->solve_n;
    int rc = trsv_t_wide<true>(c, LU, ld, x, y, n);
    if (rc) return rc;
    MPF_HIP_TRY(c, hipMemcpyAsync(x, y, n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    return 0;
}
int launch_trsv_lower_unit_t(mpf_ctx *c, const double *LU, int64_t ld, double *x, int64_t n) {
    double *y = c->solve_buf + 3 * c->solve_n;
    int rc = trsv_t_wide<false>(c, LU, ld, x, y, n);
    if (rc) return rc;
    MPF_HIP_TRY(c, hipMemcpyAsync(x, y, n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

__global__ __launch_bounds__(256) void scatter_rows_kernel(const double *in, const int *perm, double *out, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[perm[i]] = in[i];
}
int launch_scatter_rows(mpf_ctx *c, const double *in, const int *perm, double *out, int64_t n) {
    scatter_rows_kernel<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(in, perm, out, n);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

// ---- column reductions: one wave per column, CR rows per partial --------------------------------------------------------------
// OP: CR_DOT  sum_i a_ij v_i          (v = x: the transposed residual's GEMV)
//     CR_ABS  sum_i |a_ij|            (column abs sums: ||A||_1)
//     CR_SQ   sum_i a_ij^2            (Frobenius)
//     CR_MAX  max_i |a_ij| (v_i)      (v optional: max |a_ij| r_i of dgeequ's column pass)
enum { CR_DOT = 0, CR_ABS = 1, CR_SQ = 2, CR_MAX = 3 };
template <int OP>
__global__ __launch_bounds__(256) void col_part_kernel(const double *__restrict__ A, long long lda, long long m, long long ncols,
                                                       const double *__restrict__ v, double *__restrict__ part) {
    const long long col = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (col >= ncols) return;                                     // (wave-uniform; no barrier below)
    const long long i0 = (long long)blockIdx.y * CR;
    const long long nr = (m - i0) < CR ? (m - i0) : CR;
    const double *a = A + col * lda + i0;
    double s[4] = {0, 0, 0, 0};
#pragma unroll 16
    for (int k = 0; k < CR / 64; ++k) {
        const long long i = lane + 64ll * k;
        if (i < nr) {
            const double e = a[i];
            double t;
            if (OP == CR_DOT) t = e * v[i0 + i];
            else if (OP == CR_ABS) t = fabs(e);
            else if (OP == CR_SQ) t = e * e;
            else t = v ? fabs(e) * v[i0 + i] : fabs(e);
            if (OP == CR_MAX) s[k & 3] = maxn(s[k & 3], t);
            else s[k & 3] += t;
        }
    }
    double t;
    if (OP == CR_MAX) t = wave_max(maxn(maxn(s[0], s[1]), maxn(s[2], s[3])));
    else t = wave_sum((s[0] + s[1]) + (s[2] + s[3]));
    if (lane == 0) part[(long long)blockIdx.y * ncols + col] = t;
}
// out[col] = combination of the partials in ascending chunk order; CR_DOT: out = (b or 0) - sum
template <int OP>
__global__ __launch_bounds__(256) void part_finish_kernel(const double *__restrict__ part, int nchunks, long long len, const double *__restrict__ b,
                                                          double *__restrict__ out) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= len) return;
    double s = 0;
    for (int ch = 0; ch < nchunks; ++ch) {
        const double p = part[(long long)ch * len + j];
        s = OP == CR_MAX ? maxn(s, p) : s + p;
    }
    out[j] = OP == CR_DOT ? (b ? b[j] : 0.0) - s : s;
}
template <int OP>
static int col_reduce(mpf_ctx *c, const double *A, int64_t lda, int64_t m, int64_t ncols, const double *v, const double *b, double *out) {
    const int nchunks = (int)((m + CR - 1) / CR);
    MPF_HIP_TRY(c, c->ext_part.grow((int64_t)(nchunks > 0 ? nchunks : 1) * ncols));
    if (nchunks > 0) {
        dim3 grid((unsigned)((ncols + 3) / 4), (unsigned)nchunks);
        col_part_kernel<OP><<<grid, 256, 0, c->stream>>>(A, lda, m, ncols, v, c->ext_part);
    }
    part_finish_kernel<OP><<<(unsigned)((ncols + 255) / 256), 256, 0, c->stream>>>(c->ext_part, nchunks, ncols, b, out);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}
// r = (b or 0) - A[0:n, 0:n]^T x
int launch_residual_t(mpf_ctx *c, const double *A, int64_t lda, const double *x, const double *b, double *r, int64_t n) {
    return col_reduce<CR_DOT>(c, A, lda, n, n, x, b, r);
}
int launch_col_abs_sums(mpf_ctx *c, const double *A, int64_t lda, int64_t m, int64_t n, double *out) {
    return col_reduce<CR_ABS>(c, A, lda, m, n, nullptr, nullptr, out);
}
int launch_col_sumsq(mpf_ctx *c, const double *A, int64_t lda, int64_t m, int64_t n, double *out) {
    return col_reduce<CR_SQ>(c, A, lda, m, n, nullptr, nullptr, out);
}
int launch_col_max_abs(mpf_ctx *c, const double *A, int64_t lda, int64_t m, int64_t n, const double *rs, double *out) {
    return col_reduce<CR_MAX>(c, A, lda, m, n, rs, nullptr, out);
}

// ---- row reductions (residual_kernel's shape: thread = row, RCH-column chunks, ordered partials) ------------------------------
template <int OP>
__global__ __launch_bounds__(256) void row_part_kernel(const double *__restrict__ A, long long lda, long long m, long long ncols,
                                                       double *__restrict__ part) {
    const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
    if (row >= m) return;
    const long long c0 = (long long)blockIdx.y * RCH;
    const int nc = (int)((ncols - c0) < RCH ? (ncols - c0) : RCH);
    const double *a = A + row + c0 * lda;
    double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    int cc = 0;
    for (; cc + 4 <= nc; cc += 4) {
        const double e0 = fabs(a[(long long)(cc + 0) * lda]), e1 = fabs(a[(long long)(cc + 1) * lda]);
        const double e2 = fabs(a[(long long)(cc + 2) * lda]), e3 = fabs(a[(long long)(cc + 3) * lda]);
        if (OP == CR_MAX) { s0 = maxn(s0, e0); s1 = maxn(s1, e1); s2 = maxn(s2, e2); s3 = maxn(s3, e3); }
        else { s0 += e0; s1 += e1; s2 += e2; s3 += e3; }
    }
    for (; cc < nc; ++cc) {
        const double e = fabs(a[(long long)cc * lda]);
        s0 = OP == CR_MAX ? maxn(s0, e) : s0 + e;
    }
    part[(long long)blockIdx.y * m + row] = OP == CR_MAX ? maxn(maxn(s0, s1), maxn(s2, s3)) : (s0 + s1) + (s2 + s3);
}
template <int OP>
static int row_reduce(mpf_ctx *c, const double *A, int64_t lda, int64_t m, int64_t ncols, double *out) {
    const int nchunks = (int)((ncols + RCH - 1) / RCH);
    MPF_HIP_TRY(c, c->ext_part.grow((int64_t)(nchunks > 0 ? nchunks : 1) * m));
    if (nchunks > 0) {
        dim3 grid((unsigned)((m + 255) / 256), (unsigned)nchunks);
        row_part_kernel<OP><<<grid, 256, 0, c->stream>>>(A, lda, m, ncols, c->ext_part);
    }
    part_finish_kernel<OP><<<(unsigned)((m + 255) / 256), 256, 0, c->stream>>>(c->ext_part, nchunks, m, nullptr, out);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}
int launch_row_abs_sums(mpf_ctx *c, const double *A, int64_t lda, int64_t m, int64_t n, double *out) {
    return row_reduce<CR_ABS>(c, A, lda, m, n, out);
}
int launch_row_max_abs(mpf_ctx *c, const double *A, int64_t lda, int64_t m, int64_t n, double *out) {
    return row_reduce<CR_MAX>(c, A, lda, m, n, out);
}

// ---- vector reductions to scalars (fixed grid for a given n, ordered final pass) -------------------------------------------------
// VR_SUM: sum x_i;  VR_ASUM: sum |x_i| (dasum);  VR_MAX: max x_i
enum { VR_SUM = 0, VR_ASUM = 1, VR_MAX = 2 };
constexpr int VR_BLOCKS = 1024;
template <int OP>
__global__ __launch_bounds__(256) void vec_part_kernel(const double *__restrict__ x, long long n, double *__restrict__ part) {
    __shared__ double ws[4];
    double s = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const double e = x[i];
        s = OP == VR_MAX ? maxn(s, e) : s + (OP == VR_ASUM ? fabs(e) : e);
    }
    s = OP == VR_MAX ? wave_max(s) : wave_sum(s);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = OP == VR_MAX ? maxn(maxn(ws[0], ws[1]), maxn(ws[2], ws[3])) : (ws[0] + ws[1]) + (ws[2] + ws[3]);
}
template <int OP>
__global__ __launch_bounds__(64) void vec_final_kernel(const double *part, int nparts, double *out) {
    double s = 0;
    for (int i = threadIdx.x; i < nparts; i += 64) s = OP == VR_MAX ? maxn(s, part[i]) : s + part[i];
    s = OP == VR_MAX ? wave_max(s) : wave_sum(s);
    if (threadIdx.x == 0) out[0] = s;
}
template <int OP>
static int vec_reduce(mpf_ctx *c, const double *x, int64_t n, double *d_out) {
    int blocks = (int)((n + 255) / 256);
    if (blocks > VR_BLOCKS) blocks = VR_BLOCKS;
    if (blocks < 1) blocks = 1;
    MPF_HIP_TRY(c, c->ext_red.grow(VR_BLOCKS));
    vec_part_kernel<OP><<<blocks, 256, 0, c->stream>>>(x, n, c->ext_red);
    vec_final_kernel<OP><<<1, 64, 0, c->stream>>>(c->ext_red, blocks, d_out);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}
int launch_vec_sum(mpf_ctx *c, const double *x, int64_t n, double *d_out) { return vec_reduce<VR_SUM>(c, x, n, d_out); }
int launch_vec_max(mpf_ctx *c, const double *x, int64_t n, double *d_out) { return vec_reduce<VR_MAX>(c, x, n, d_out); }
int launch_dasum(mpf_ctx *c, const double *x, int64_t n, double *d_out) { return vec_reduce<VR_ASUM>(c, x, n, d_out); }

// ---- dlacn2 helpers ---------------------------------------------------------------------------------------------------------
// xs_i = +1 where x_i >= 0 else -1; part[block] = {sum |x_i| of the block, number of i with xs_i != isgn_i} (isgn may be null)
__global__ __launch_bounds__(256) void lacn2_sign_kernel(const double *__restrict__ x, const double *__restrict__ isgn, long long n,
                                                         double *__restrict__ xs, double *__restrict__ part) {
    __shared__ double ws[2][4];
    double s = 0, d = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const double e = x[i];
        const double sg = e >= 0 ? 1.0 : -1.0;
        s += fabs(e);
        if (isgn && sg != isgn[i]) d += 1.0;
        xs[i] = sg;
    }
    s = wave_sum(s);
    d = wave_sum(d);
    if ((threadIdx.x & 63) == 0) { ws[0][threadIdx.x >> 6] = s; ws[1][threadIdx.x >> 6] = d; }
    __syncthreads();
    if (threadIdx.x == 0) {
        part[blockIdx.x] = (ws[0][0] + ws[0][1]) + (ws[0][2] + ws[0][3]);
        part[VR_BLOCKS + blockIdx.x] = (ws[1][0] + ws[1][1]) + (ws[1][2] + ws[1][3]);
    }
}
__global__ __launch_bounds__(64) void lacn2_sign_final_kernel(const double *part, int nparts, double *out) {
    double s = 0, d = 0;
    for (int i = threadIdx.x; i < nparts; i += 64) { s += part[i]; d += part[VR_BLOCKS + i]; }
    s = wave_sum(s);
    d = wave_sum(d);
    if (threadIdx.x == 0) { out[0] = s; out[1] = d; }
}
// d_out[0] = sum |x_i|, d_out[1] = number of sign changes against isgn; xs = sign(x)
int launch_lacn2_sign(mpf_ctx *c, const double *x, const double *isgn, int64_t n, double *xs, double *d_out) {
    int blocks = (int)((n + 255) / 256);
    if (blocks > VR_BLOCKS) blocks = VR_BLOCKS;
    MPF_HIP_TRY(c, c->ext_red.grow(2 * VR_BLOCKS));
    lacn2_sign_kernel<<<blocks, 256, 0, c->stream>>>(x, isgn, n, xs, c->ext_red);
    lacn2_sign_final_kernel<<<1, 64, 0, c->stream>>>(c->ext_red, blocks, d_out);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

// idamax: the first index of the largest |x_i| (order (|x| descending, index ascending): the result does not depend on the
// reduction's shape).  d_out[0] = that |x_i|, d_out[1] = the index (0-based, as a double)
__device__ __forceinline__ void amax_better(double &v, long long &k, double v2, long long k2) {
    if (v2 > v || (v2 == v && k2 < k)) { v = v2; k = k2; }
}
__global__ __launch_bounds__(256) void idamax_part_kernel(const double *__restrict__ x, long long n, double *__restrict__ part) {
    __shared__ double sv[256];
    __shared__ long long sk[256];
    double v = -1.0;
    long long k = n;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) amax_better(v, k, fabs(x[i]), i);
    sv[threadIdx.x] = v; sk[threadIdx.x] = k;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { double a = sv[threadIdx.x]; long long ka = sk[threadIdx.x]; amax_better(a, ka, sv[threadIdx.x + o], sk[threadIdx.x + o]); sv[threadIdx.x] = a; sk[threadIdx.x] = ka; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { part[blockIdx.x] = sv[0]; part[VR_BLOCKS + blockIdx.x] = (double)sk[0]; }
}
__global__ __launch_bounds__(64) void idamax_final_kernel(const double *part, int nparts, double *out) {
    __shared__ double sv[64];
    __shared__ long long sk[64];
    double v = -1.0;
    long long k = 1ll << 62;
    for (int i = threadIdx.x; i < nparts; i += 64) amax_better(v, k, part[i], (long long)part[VR_BLOCKS + i]);
    sv[threadIdx.x] = v; sk[threadIdx.x] = k;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 64; ++i) amax_better(v, k, sv[i], sk[i]);
        out[0] = v; out[1] = (double)k;
    }
}
int launch_idamax(mpf_ctx *c, const double *x, int64_t n, double *d_out) {
    int blocks = (int)((n + 255) / 256);
    if (blocks > VR_BLOCKS) blocks = VR_BLOCKS;
    MPF_HIP_TRY(c, c->ext_red.grow(2 * VR_BLOCKS));
    idamax_part_kernel<<<blocks, 256, 0, c->stream>>>(x, n, c->ext_red);
    idamax_final_kernel<<<1, 64, 0, c->stream>>>(c->ext_red, blocks, d_out);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

// x = 1/n everywhere (kind 0), e_j (kind 1), or dlacn2's final test vector x_i = (-1)^i (1 + i / (n - 1)) (kind 2)
__global__ __launch_bounds__(256) void lacn2_fill_kernel(double *x, long long n, int kind, long long j) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double v;
    if (kind == 0) v = 1.0 / (double)n;
    else if (kind == 1) v = i == j ? 1.0 : 0.0;
    else v = (i & 1 ? -1.0 : 1.0) * (1.0 + (double)i / (double)(n - 1));
    x[i] = v;
}
int launch_lacn2_fill(mpf_ctx *c, double *x, int64_t n, int kind, int64_t j) {
    lacn2_fill_kernel<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(x, n, kind, j);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

// first i with LU[i, i] == 0 (1-based) or 0, as a double in *out; one workgroup
__global__ __launch_bounds__(256) void diag_zero_kernel(const double *LU, long long ld, long long n, double *out) {
    __shared__ long long sk[256];
    long long k = n;
    for (long long i = threadIdx.x; i < n; i += 256)
        if (LU[i + i * ld] == 0.0 && i < k) k = i;
    sk[threadIdx.x] = k;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o && sk[threadIdx.x + o] < sk[threadIdx.x]) sk[threadIdx.x] = sk[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = sk[0] < n ? (double)(sk[0] + 1) : 0.0;
}
int launch_diag_zero(mpf_ctx *c, const double *LU, int64_t ld, int64_t n, double *d_out) {
    diag_zero_kernel<<<1, 256, 0, c->stream>>>(LU, ld, n, d_out);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

// ---- equilibration -------------------------------------------------------------------------------------------------------------
// From the maxima m_i (row or column): s_i = 2^-e_i, e_i = floor(log2 m_i) clamped to [-1022, 1022] (1 where m_i is 0 or not
// finite); stats[0] = min m_i, stats[1] = max m_i, stats[2] = first i with m_i == 0 (1-based) or 0.  One workgroup.
__global__ __launch_bounds__(256) void pow2_scale_kernel(const double *__restrict__ m, long long n, double *__restrict__ s, double *__restrict__ stats) {
    __shared__ double smin[256], smax[256];
    __shared__ long long sk[256];
    double lo = HUGE_VAL, hi = 0.0;
    long long k = n;
    for (long long i = threadIdx.x; i < n; i += 256) {
        const double v = m[i];
        lo = v < lo ? v : lo;
        hi = maxn(hi, v);
        if (v == 0.0 && i < k) k = i;
        int e = (v > 0.0 && v <= 1.7976931348623157e308) ? ilogb(v) : 0;
        e = e < -1022 ? -1022 : (e > 1022 ? 1022 : e);
        s[i] = ldexp(1.0, -e);
    }
    smin[threadIdx.x] = lo; smax[threadIdx.x] = hi; sk[threadIdx.x] = k;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            const int t = threadIdx.x;
            if (smin[t + o] < smin[t]) smin[t] = smin[t + o];
            smax[t] = maxn(smax[t], smax[t + o]);
            if (sk[t + o] < sk[t]) sk[t] = sk[t + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { stats[0] = smin[0]; stats[1] = smax[0]; stats[2] = sk[0] < n ? (double)(sk[0] + 1) : 0.0; }
}
int launch_pow2_scale(mpf_ctx *c, const double *m, int64_t n, double *s, double *d_stats) {
    pow2_scale_kernel<<<1, 256, 0, c->stream>>>(m, n, s, d_stats);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

// W = Dr A Dc: W[i, j] = (A[i, j] r_i) c_j (r / c null: 1); column-major, any lda / ldw
__global__ __launch_bounds__(256) void scaled_copy_kernel(const double *__restrict__ A, long long lda, const double *__restrict__ r,
                                                          const double *__restrict__ cs, double *__restrict__ W, long long ldw, long long m, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const double ri = r ? r[i] : 1.0;
    for (long long j = blockIdx.y; j < n; j += gridDim.y) {
        double v = A[i + j * lda];
        if (r) v = v * ri;
        if (cs) v = v * cs[j];
        W[i + j * ldw] = v;
    }
}
int launch_scaled_copy(mpf_ctx *c, const double *A, int64_t lda, const double *r, const double *cs, double *W, int64_t ldw, int64_t m, int64_t n) {
    dim3 grid((unsigned)((m + 255) / 256), (unsigned)(n < 65535 ? n : 65535));
    scaled_copy_kernel<<<grid, 256, 0, c->stream>>>(A, lda, r, cs, W, ldw, m, n);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

// y_i = x_i s_i (s null: y = x) times alpha
__global__ __launch_bounds__(256) void vscale_kernel(const double *__restrict__ x, const double *__restrict__ s, double alpha, double *__restrict__ y, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = (s ? x[i] * s[i] : x[i]) * alpha;
}
int launch_vscale(mpf_ctx *c, const double *x, const double *s, double alpha, double *y, int64_t n) {
    vscale_kernel<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(x, s, alpha, y, n);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

// ---- reciprocal pivot growth (mpf_gerpvgrw; LAPACK dla_gerpvgrw) ------------------------------------------------------------------
// One wave per column, four columns per workgroup: q[j] = amax_j / umax_j with amax_j = max_i (|a_ij| r_i) c_j and umax_j =
// max_{i <= j} |lu_ij|.  The lanes stride down the column, so A's column and U's part of LU's are each read once, coalesced.  c_j > 0
// multiplies after the maximum: rounding is monotone, so the product of the maximum is the maximum of the products.  umax_j = 0: the
// column is skipped (q = 1, the value the minimum starts from); a NaN in either maximum: q = NaN.
__global__ __launch_bounds__(256) void pivot_growth_cols_kernel(const double *__restrict__ A, long long lda, const double *__restrict__ LU,
                                                                long long ldlu, long long n, const double *__restrict__ r,
                                                                const double *__restrict__ cs, double *__restrict__ q) {
    const long long col = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (col >= n) return;                                         // (wave-uniform; no barrier below)
    const double *a = A + col * lda, *u = LU + col * ldlu;
    double am[4] = {0, 0, 0, 0}, um[4] = {0, 0, 0, 0};
    int k = 0;
    for (long long i = lane; i < n; i += 64, ++k) {
        const double e = fabs(a[i]);
        am[k & 3] = maxn(am[k & 3], r ? e * r[i] : e);
        if (i <= col) um[k & 3] = maxn(um[k & 3], fabs(u[i]));
    }
    double amax = wave_max(maxn(maxn(am[0], am[1]), maxn(am[2], am[3])));
    const double umax = wave_max(maxn(maxn(um[0], um[1]), maxn(um[2], um[3])));
    if (cs) amax = amax * cs[col];
    if (lane == 0) q[col] = (amax != amax || umax != umax) ? (amax != amax ? amax : umax) : (umax != 0 ? amax / umax : 1.0);
}
int launch_pivot_growth_cols(mpf_ctx *c, const double *A, int64_t lda, const double *LU, int64_t ldlu, int64_t n, const double *r,
                             const double *cs, double *q) {
    pivot_growth_cols_kernel<<<(unsigned)((n + 3) / 4), 256, 0, c->stream>>>(A, lda, LU, ldlu, n, r, cs, q);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}
// d_out[0] = min(1, min_j q[j]), a NaN kept; one workgroup
__global__ __launch_bounds__(256) void vec_min1_kernel(const double *__restrict__ q, long long n, double *__restrict__ out) {
    __shared__ double ws[4];
    double s = -1.0;                                              // the minimum as a maximum of the negatives: maxn keeps a NaN
    for (long long i = threadIdx.x; i < n; i += 256) s = maxn(s, -q[i]);
    s = wave_max(s);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = -maxn(maxn(ws[0], ws[1]), maxn(ws[2], ws[3]));
}
int launch_vec_min1(mpf_ctx *c, const double *q, int64_t n, double *d_out) {
    vec_min1_kernel<<<1, 256, 0, c->stream>>>(q, n, d_out);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}
