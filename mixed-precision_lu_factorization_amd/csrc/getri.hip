// Kernels of mpf_getri and mpf_getdet (mpf_getri.cpp): the inverse and the determinant from the factors.
// The O(N^3) part of the inverse is launch_dgemm_minus (trailing_f64.hip) with K = 256; what lives here is everything around it:
//   getri_init_kernel        W = I (upper and lower triangle of the N x N result)
//   getri_transpose_kernel   the 256 x 256 inverses of L's diagonal blocks, transposed, so that both block products read their
//                            triangular operand the same (coalesced) way
//   getri_tri_kernel         the two block-inverse products, in place, on v_mfma_f64_16x16x4_f64:
//                              left   X(k, cols)  = inv(U_kk) R(k, cols)      256 x 256 times 256 x n
//                              right  X(rows, j)  = R(rows, j) inv(L_jj)      m x 256 times 256 x 256
//   getri_gather / _scatter  the column interchanges (one composed permutation) and the scales, a 256-row panel at a time
//   getdet_kernel            the determinant as mant 2^expo in the header's fixed order, one launch
// Every element has one fixed operation order; no atomics on data, plain vector stores only.
#include "mpf_internal.h"

namespace {
typedef double d4_t __attribute__((ext_vector_type(4)));
constexpr int GB = 256;   // diagonal block (ir.hip's 256 x 256 inverses)
constexpr int GC = 16;    // columns (left product) or rows (right product) a workgroup owns: one MFMA tile
constexpr int DCH = 256;  // mpf_getdet: consecutive diagonal entries per chunk
} // namespace

__global__ __launch_bounds__(256) void getri_init_kernel(double *__restrict__ W, long long ld, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    for (long long j = blockIdx.y; j < n; j += gridDim.y) W[i + j * ld] = i == j ? 1.0 : 0.0;
}

// out[K][i + 256 k] = in[K][k + 256 i]  (blockIdx.x = i, blockIdx.y = K, thread = k)
__global__ __launch_bounds__(256) void getri_transpose_kernel(const double *__restrict__ in, double *__restrict__ out) {
    const long long base = (long long)blockIdx.y * GB * GB;
    out[base + blockIdx.x + (long long)GB * threadIdx.x] = in[base + threadIdx.x + (long long)GB * blockIdx.x];
}

// P = G S in place of S, with G (256 x 256, column-major, UPPER triangular: G[i + 256 k] = 0 for k < i) the inverse of a diagonal
// block and S a 256 x 16 slice of W owned by this workgroup alone:
//   left  (RIGHT = false): S[k][j] = W[(r0 + k) + (c0 + 16 b + j) ld]     b = blockIdx.x over `extent` columns from c0
//   right (RIGHT = true):  S[k][j] = W[(r0 + 16 b + j) + (c0 + k) ld]     b over `extent` rows from r0; G = inv(L_jj)^T
// k < w only (the ragged last block: rows / columns from w on are neither read nor written, and read as zero).
// Element (i, j) is one chain: the accumulator starts at 0 and takes k = 16 floor(i / 16) .. in ascending order, four per MFMA --
// the k below are G's zero triangle and are not spent.  Wave g owns the 16-row tiles g, g + 4, g + 8, g + 12 of P.
template <bool RIGHT>
__global__ __launch_bounds__(256) void getri_tri_kernel(const double *__restrict__ G, double *__restrict__ W, long long ld, long long r0,
                                                        long long c0, int w, long long extent) {
    __shared__ double Ss[GB][GC + 1];
    const int tid = threadIdx.x, l = tid & 63, g = tid >> 6;
    const long long b0 = (long long)blockIdx.x * GC;
    const int nj = (int)((extent - b0) < GC ? (extent - b0) : GC);   // live columns / rows of this workgroup
    // element (k, j) of the slice
    auto at = [&](int k, int j) -> double * {
        return RIGHT ? W + (r0 + b0 + j) + (c0 + k) * ld : W + (r0 + k) + (c0 + b0 + j) * ld;
    };
    // staging map: lanes along W's contiguous index
    if (!RIGHT) {
#pragma unroll
        for (int j = 0; j < GC; ++j) Ss[tid][j] = (tid < w && j < nj) ? *at(tid, j) : 0.0;
    } else {
#pragma unroll
        for (int q = 0; q < GB / 16; ++q) {
            const int j = tid & 15, k = (tid >> 4) + 16 * q;
            Ss[k][j] = (k < w && j < nj) ? *at(k, j) : 0.0;
        }
    }
    __syncthreads();
    const int kt = (w + 15) / 16;   // 16-wide k groups that hold live rows of S (G is finite beyond w, S is zero there)
    d4_t acc[4];
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
        const int t = g + 4 * tt;
        d4_t a4 = {0.0, 0.0, 0.0, 0.0};
        const double *gp = G + (16 * t + (l & 15)) + (long long)(l >> 4) * GB;
        double a[4], an[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = t < kt ? gp[(long long)(16 * t + 4 * u) * GB] : 0.0;
        for (int kg = t; kg < kt; ++kg) {   // the next group's slice of G flies under this group's MFMAs
#pragma unroll
            for (int u = 0; u < 4; ++u) an[u] = kg + 1 < kt ? gp[(long long)(16 * (kg + 1) + 4 * u) * GB] : 0.0;
#pragma unroll
            for (int u = 0; u < 4; ++u)
                a4 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], Ss[16 * kg + 4 * u + (l >> 4)][l & 15], a4, 0, 0, 0);
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = an[u];
        }
        acc[tt] = a4;
    }
    __syncthreads();   // every wave has read the slice: it becomes the product
    // f64 MFMA C/D map: column = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
    for (int tt = 0; tt < 4; ++tt)
#pragma unroll
        for (int i = 0; i < 4; ++i) Ss[16 * (g + 4 * tt) + (l >> 4) + 4 * i][l & 15] = acc[tt][i];
    __syncthreads();
    if (!RIGHT) {
#pragma unroll
        for (int j = 0; j < GC; ++j)
            if (tid < w && j < nj) *at(tid, j) = Ss[tid][j];
    } else {
#pragma unroll
        for (int q = 0; q < GB / 16; ++q) {
            const int j = tid & 15, k = (tid >> 4) + 16 * q;
            if (k < w && j < nj) *at(k, j) = Ss[k][j];
        }
    }
}

// T[i + 256 j] = W[(i0 + i) + src[j] ld]  (blockIdx.x = j, thread = i < rows)
__global__ __launch_bounds__(256) void getri_gather_kernel(const double *__restrict__ W, long long ld, long long i0, int rows,
                                                           const int *__restrict__ src, long long n, double *__restrict__ T) {
    const int i = threadIdx.x;
    if (i >= rows) return;
    for (long long j = blockIdx.x; j < n; j += gridDim.x) T[i + (long long)GB * j] = W[(i0 + i) + (long long)src[j] * ld];
}
// W[(i0 + i) + j ld] = T[i + 256 j], with scales (cs_i t) r_j -- a factor that is absent is not a factor of 1.0; without SC the
// kernel is the plain copy
template <bool SC>
__global__ __launch_bounds__(256) void getri_scatter_kernel(double *__restrict__ W, long long ld, long long i0, int rows, long long n,
                                                            const double *__restrict__ T, const double *__restrict__ r,
                                                            const double *__restrict__ cs) {
    const int i = threadIdx.x;
    if (i >= rows) return;
    const double ci = (SC && cs) ? cs[i0 + i] : 1.0;
    for (long long j = blockIdx.x; j < n; j += gridDim.x) {
        double v = T[i + (long long)GB * j];
        if (SC) {
            if (cs) v = ci * v;
            if (r) v = v * r[j];
        }
        W[(i0 + i) + j * ld] = v;
    }
}

// mpf_getdet.  One workgroup; thread t takes the chunks t, t + 256, ... of 256 consecutive diagonal entries, each in ascending order
// from (1, 0): p = p m_i, (p, k) = frexp(p), e += k + e_i; thread 0 then combines the chunk results in ascending order by the same
// step.  part: 2 slots per chunk (mantissa, exponent as a 64-bit integer).  out[0] = mant, out[1] = expo (64-bit integer bits).
__global__ __launch_bounds__(256) void getdet_kernel(const double *__restrict__ LU, long long ld, const int *__restrict__ ipiv,
                                                     long long n, const double *__restrict__ r, const double *__restrict__ cs,
                                                     double *part, double *out) {
    __shared__ int s_zero, s_bad, s_flips;
    if (threadIdx.x == 0) { s_zero = 0; s_bad = 0; s_flips = 0; }
    __syncthreads();
    const long long nch = (n + DCH - 1) / DCH;
    int zero = 0, bad = 0, flips = 0;
    for (long long ch = threadIdx.x; ch < nch; ch += 256) {
        const long long i1 = (ch + 1) * DCH < n ? (ch + 1) * DCH : n;
        double p = 1.0;
        long long e = 0;
        for (long long i = ch * DCH; i < i1; ++i) {
            const double u = LU[i + i * ld];
            if (u == 0.0) zero = 1;
            if (!(fabs(u) <= 1.7976931348623157e308)) bad = 1;
            flips ^= (ipiv[i] != (int)(i + 1)) ? 1 : 0;
            int ei;
            const double m = frexp(u, &ei);
            long long es = ei;
            if (r) { int er; (void)frexp(r[i], &er); es -= er - 1; }
            if (cs) { int ec; (void)frexp(cs[i], &ec); es -= ec - 1; }
            mpf_det_step(p, e, m, es);
        }
        part[2 * ch] = p;
        ((long long *)part)[2 * ch + 1] = e;
    }
    if (zero) atomicOr(&s_zero, 1);
    if (bad) atomicOr(&s_bad, 1);
    if (flips) atomicXor(&s_flips, 1);
    __syncthreads();
    if (threadIdx.x != 0) return;
    double P = 1.0;
    long long E = 0;
    for (long long ch = 0; ch < nch; ++ch) {
        mpf_det_step(P, E, part[2 * ch], ((const long long *)part)[2 * ch + 1]);
    }
    if (s_flips) P = -P;
    if (s_bad) { P = __builtin_nan(""); E = 0; }
    else if (s_zero) { P = 0.0; E = 0; }
    out[0] = P;
    ((long long *)out)[1] = E;
}

int launch_getri_init(mpf_ctx *c, double *W, int64_t ld, int64_t n) {
    dim3 grid((unsigned)((n + 255) / 256), (unsigned)(n < 4096 ? n : 4096));
    getri_init_kernel<<<grid, 256, 0, c->stream>>>(W, ld, n);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}
int launch_getri_transpose(mpf_ctx *c, const double *inv, double *out, int64_t nblk) {
    getri_transpose_kernel<<<dim3(GB, (unsigned)nblk), 256, 0, c->stream>>>(inv, out);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}
int launch_getri_tri(mpf_ctx *c, bool right, const double *G, double *W, int64_t ld, int64_t r0, int64_t c0, int w, int64_t extent) {
    if (extent <= 0 || w <= 0) return 0;
    const unsigned grid = (unsigned)((extent + GC - 1) / GC);
    if (right) getri_tri_kernel<true><<<grid, 256, 0, c->stream>>>(G, W, ld, r0, c0, w, extent);
    else getri_tri_kernel<false><<<grid, 256, 0, c->stream>>>(G, W, ld, r0, c0, w, extent);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}
int launch_getri_permute(mpf_ctx *c, double *W, int64_t ld, int64_t n, const int *src, const double *r, const double *cs, double *T) {
    const unsigned grid = (unsigned)(n < 8192 ? n : 8192);
    for (int64_t i0 = 0; i0 < n; i0 += GB) {
        const int rows = (int)((n - i0) < GB ? (n - i0) : GB);
        getri_gather_kernel<<<grid, 256, 0, c->stream>>>(W, ld, i0, rows, src, n, T);
        if (r || cs) getri_scatter_kernel<true><<<grid, 256, 0, c->stream>>>(W, ld, i0, rows, n, T, r, cs);
        else getri_scatter_kernel<false><<<grid, 256, 0, c->stream>>>(W, ld, i0, rows, n, T, nullptr, nullptr);
    }
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}
int launch_getdet(mpf_ctx *c, const double *LU, int64_t ld, const int *ipiv, int64_t n, const double *r, const double *cs, double *part,
                  double *out) {
    getdet_kernel<<<1, 256, 0, c->stream>>>(LU, ld, ipiv, n, r, cs, part, out);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}
