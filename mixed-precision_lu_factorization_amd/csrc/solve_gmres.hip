// Kernels of the blocked GMRES-IR (mpf_block.cpp: blk_gmres_core, mpf_solve_gmres_ir_block): the orthogonalisation of a group's
// vectors W (one tile set, solve_block.hip's layout: column j at W + j * ldt, rows N .. ldt - 1 zero) against its Krylov basis, slot i
// at V + i * vs in the same layout.  Classical Gram-Schmidt applied twice, three sweeps over the basis:
//     sweep 1   W = -W (the residual kernel left -op(A) v_k);  p1[i, j] = V_i[:, j] . W[:, j]
//     sweep 2   W -= sum_i h1[i, j] V_i (i ascending);         p2[i, j] = V_i[:, j] . W[:, j]
//     sweep 3   W -= sum_i h2[i, j] V_i;                       q[j] = W[:, j] . W[:, j]
// All three are gm_sweep_kernel: one workgroup per (chunk of GM_CH rows, column).  Phase A: each wave takes GM_CH / 4 rows of the
// chunk through its registers (negation or update, 16-byte loads and stores along the rows) and leaves them in LDS; phase B: each
// wave takes the WHOLE chunk from LDS into registers and dots it with the slots w, w + 4, ... -- W's chunk is loaded once and reused
// against every slot.  Partials per chunk (per wave for q), then gm_finish_kernel adds them in ascending order.
// Every sum has one fixed order: per lane the rows ascending, a butterfly over the 64 lanes, the chunks ascending -- nothing depends on
// the column's position, on the number of columns or tiles, or on another column's data.  A column whose live[j] is zero is not
// touched.  No atomics, no waiting between workgroups, plain vector stores only; rows N .. ldt - 1 are stored as zero.
#include "mpf_internal.h"

namespace {
typedef double d2_t __attribute__((ext_vector_type(2)));
constexpr int GM_CH = 2048;            // rows per workgroup: 16 chunks x 32 columns = 512 workgroups for one tile at N = 32768
constexpr int GM_WR = GM_CH / 4;       // rows of a wave in phase A
constexpr int GM_PA = GM_WR / 128;     // 16-byte passes of a wave over its rows (64 lanes x 2 doubles)
constexpr int GM_PB = GM_CH / 128;     // ... over the whole chunk

__device__ __forceinline__ double wave_sum64(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// MODE 0: W = -W, dots.  MODE 1: W -= sum_i h[i] V_i, dots.  MODE 2: W -= sum_i h[i] V_i, sum of squares.
// h: coefficients h[i * tc + j]; part: [chunk][slot][tc] (MODE 0, 1) or [chunk * 4 + wave][tc] (MODE 2); ns = slots 0 .. ns - 1.
template <int MODE>
__global__ __launch_bounds__(256) void gm_sweep_kernel(const double *__restrict__ V, long long vs, int ns, double *__restrict__ W, long long ldt,
                                                       long long n, const int *__restrict__ live, const double *__restrict__ h, long long tc,
                                                       double *__restrict__ part) {
    __shared__ d2_t ws[GM_CH / 2];
    const int j = blockIdx.y;
    if (!live[j]) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long c0 = (long long)blockIdx.x * GM_CH, col = (long long)j * ldt;
    // ---- phase A: this wave's rows -------------------------------------------------------------------------------------------------
    d2_t w[GM_PA];
    long long row[GM_PA];
#pragma unroll
    for (int p = 0; p < GM_PA; ++p) {
        row[p] = c0 + (long long)wv * GM_WR + 128 * p + 2 * lane;
        w[p] = row[p] < ldt ? *(const d2_t *)(W + col + row[p]) : d2_t{0.0, 0.0};   // (ldt is even: a pair is inside or outside)
    }
    if (MODE == 0) {
#pragma unroll
        for (int p = 0; p < GM_PA; ++p) w[p] = -w[p];
    } else {
#pragma unroll 4
        for (int i = 0; i < ns; ++i) {
            const double hi = h[(long long)i * tc + j];
            const double *vi = V + (long long)i * vs + col;
#pragma unroll
            for (int p = 0; p < GM_PA; ++p) {
                if (row[p] >= ldt) continue;
                const d2_t v = *(const d2_t *)(vi + row[p]);
                w[p].x = __builtin_fma(-hi, v.x, w[p].x);
                w[p].y = __builtin_fma(-hi, v.y, w[p].y);
            }
        }
    }
    double sq = 0;
#pragma unroll
    for (int p = 0; p < GM_PA; ++p) {
        if (row[p] >= n) w[p].x = 0.0;          // the pad rows stay zero whatever the coefficients hold
        if (row[p] + 1 >= n) w[p].y = 0.0;
        if (row[p] < ldt) *(d2_t *)(W + col + row[p]) = w[p];
        if (MODE == 2) { sq = __builtin_fma(w[p].x, w[p].x, sq); sq = __builtin_fma(w[p].y, w[p].y, sq); }
        else ws[(wv * GM_WR + 128 * p) / 2 + lane] = w[p];
    }
    if (MODE == 2) {
        sq = wave_sum64(sq);
        if (lane == 0) part[((long long)blockIdx.x * 4 + wv) * tc + j] = sq;
        return;
    }
    __syncthreads();
    // ---- phase B: the whole chunk against this wave's slots ------------------------------------------------------------------------
    d2_t wc[GM_PB];
#pragma unroll
    for (int p = 0; p < GM_PB; ++p) wc[p] = ws[64 * p + lane];
    const long long r0 = c0 + 2 * lane;
    for (int i = wv; i < ns; i += 4) {
        const double *vi = V + (long long)i * vs + col + r0;
        double s0 = 0, s1 = 0;
#pragma unroll
        for (int p = 0; p < GM_PB; ++p) {
            if (r0 + 128 * p >= ldt) continue;
            const d2_t v = *(const d2_t *)(vi + 128 * p);
            s0 = __builtin_fma(v.x, wc[p].x, s0);
            s1 = __builtin_fma(v.y, wc[p].y, s1);
        }
        const double s = wave_sum64(s0 + s1);
        if (lane == 0) part[((long long)blockIdx.x * ns + i) * tc + j] = s;
    }
}

// out[e] = sum over the partials in ascending order, e < len = values per partial; columns that are not live keep their entry
__global__ __launch_bounds__(256) void gm_finish_kernel(const double *__restrict__ part, int nparts, long long len, long long tc,
                                                        const int *__restrict__ live, double *__restrict__ out) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= len || !live[e % tc]) return;
    double s = 0;
    for (int q = 0; q < nparts; ++q) s += part[(long long)q * len + e];
    out[e] = s;
}

// dst[:, j] = src[:, j] * scale[j] where scale[j] != 0 (rows n .. ldt - 1: zero)
__global__ __launch_bounds__(256) void gm_append_kernel(const double *__restrict__ src, const double *__restrict__ scale, double *__restrict__ dst,
                                                        long long ldt, long long n) {
    const long long r = ((long long)blockIdx.x * 256 + threadIdx.x) * 2, j = blockIdx.y;
    const double s = scale[j];
    if (r >= ldt || s == 0) return;
    d2_t v = *(const d2_t *)(src + j * ldt + r);
    v.x = r < n ? v.x * s : 0.0;
    v.y = r + 1 < n ? v.y * s : 0.0;
    *(d2_t *)(dst + j * ldt + r) = v;
}

// X[:, j] += sum_{i < cnt[j]} y[i * tc + j] V_i[:, j], i ascending, rows below n only
__global__ __launch_bounds__(256) void gm_xupdate_kernel(const double *__restrict__ V, long long vs, const double *__restrict__ y,
                                                         const int *__restrict__ cnt, long long tc, double *__restrict__ X, long long ldt,
                                                         long long n) {
    const long long r = ((long long)blockIdx.x * 256 + threadIdx.x) * 2, j = blockIdx.y;
    const int k = cnt[j];
    if (r >= n || k <= 0) return;
    d2_t x = *(const d2_t *)(X + j * ldt + r);
    for (int i = 0; i < k; ++i) {
        const double yi = y[(long long)i * tc + j];
        const d2_t v = *(const d2_t *)(V + (long long)i * vs + j * ldt + r);
        x.x = __builtin_fma(yi, v.x, x.x);
        x.y = __builtin_fma(yi, v.y, x.y);
    }
    if (r + 1 >= n) x.y = 0.0;
    *(d2_t *)(X + j * ldt + r) = x;
}
} // namespace

int gmres_ortho_chunks(int64_t ldt) { return (int)((ldt + GM_CH - 1) / GM_CH); }

// The three sweeps of one inner step on the columns with live[j] != 0: W (holding -M^-1 op(A) v_k) becomes the orthogonalised w, and
// out = [h1 (ns x tc) | h2 (ns x tc) | ||w||^2 (tc)] (entries of the other columns: unchanged).  part: gmres_ortho_chunks(ldt) *
// max(ns, 4) * tc doubles.
int launch_gmres_ortho(mpf_ctx *c, const double *V, int64_t vs, int ns, double *W, int64_t ldt, int64_t n, int ntiles, const int *live,
                       double *part, double *out) {
    const int64_t tc = (int64_t)BLK_T * ntiles, len = (int64_t)ns * tc;
    const int nch = gmres_ortho_chunks(ldt);
    dim3 grid((unsigned)nch, (unsigned)tc);
    const unsigned fin = (unsigned)((len + 255) / 256);
    double *h1 = out, *h2 = out + len, *q = out + 2 * len;
    gm_sweep_kernel<0><<<grid, 256, 0, c->stream>>>(V, vs, ns, W, ldt, n, live, nullptr, tc, part);
    gm_finish_kernel<<<fin, 256, 0, c->stream>>>(part, nch, len, tc, live, h1);
    gm_sweep_kernel<1><<<grid, 256, 0, c->stream>>>(V, vs, ns, W, ldt, n, live, h1, tc, part);
    gm_finish_kernel<<<fin, 256, 0, c->stream>>>(part, nch, len, tc, live, h2);
    gm_sweep_kernel<2><<<grid, 256, 0, c->stream>>>(V, vs, ns, W, ldt, n, live, h2, tc, part);
    gm_finish_kernel<<<(unsigned)((tc + 255) / 256), 256, 0, c->stream>>>(part, 4 * nch, tc, tc, live, q);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}
int launch_gmres_append(mpf_ctx *c, const double *src, const double *scale, double *dst, int64_t ldt, int64_t n, int ntiles) {
    dim3 grid((unsigned)((ldt / 2 + 255) / 256), (unsigned)(BLK_T * ntiles));
    gm_append_kernel<<<grid, 256, 0, c->stream>>>(src, scale, dst, ldt, n);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}
int launch_gmres_xupdate(mpf_ctx *c, const double *V, int64_t vs, const double *y, const int *cnt, double *X, int64_t ldt, int64_t n,
                         int ntiles) {
    dim3 grid((unsigned)((n / 2 + 256) / 256), (unsigned)(BLK_T * ntiles));
    gm_xupdate_kernel<<<grid, 256, 0, c->stream>>>(V, vs, y, cnt, (int64_t)BLK_T * ntiles, X, ldt, n);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}
