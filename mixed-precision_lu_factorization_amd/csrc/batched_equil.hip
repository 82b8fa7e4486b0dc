// Equilibration of many matrices: mpf_geequ's power-of-two factors, dlaqge's scaling and the diagonal scaling of right-hand sides for
// the three batched layouts (mpf_geequ_batched, mpf_laqge_batched, mpf_lascl2_batched, their _batched_blocked and _vbatched siblings;
// contracts in include/mpf_c.h, host side in mpf_batched.cpp).
//
// Nothing here is summed: every result is a maximum, a minimum, a product with a power of two or one division of two such extremes.
// The maxima are taken on the bit pattern of |a| as an unsigned integer -- monotone in |a|, Inf above every finite value and every NaN
// above Inf -- so they are order-free, a NaN or Inf anywhere in a matrix is seen by one compare on the matrix's maximum, and a matrix's
// bits do not depend on the form that computed them.  All kernels stream; the forms differ in how a matrix is spread over the machine:
//   eq_geequ_team_kernel<W>   n <= 8 / 16 / 32: W lanes of a wave per matrix, lane = row, the row's n values in registers (A is read
//                             once).  Row maximum: a loop over the registers.  Column maxima of |a_ij| r_i: a transposing butterfly
//                             (at offset o a lane keeps the half of its columns that matches its bit o and sends the other half), W - 1
//                             exchanges after which lane j holds column j's maximum.
//   eq_geequ_wg_kernel<RP, G> n <= 64 / 128: one workgroup per matrix, RP rows x G = 4 / 8 column groups, 16 columns of a row in
//                             registers (A is read once); rows combine the groups through LDS, columns the waves of a group.
//   eq_rowmax / eq_rowfin / eq_colmax / eq_colfin   any n <= 1024, fixed or ragged: a matrix spread over ceil(n / 64) workgroups for the
//                             row maxima and ceil(n / 16) for the scaled column maxima (each reads A once, lanes along a column), and one
//                             small workgroup per matrix after each that forms r / rowcnd / amax / info and c / colcnd / info.  Four
//                             ordinary launches; the maxima of a chunk live in the context's workspace between them.
//   eq_decide_kernel<T>       the per-matrix decision of laqge (equed) and the spreads max r / min r, max c / min c: T lanes per matrix.
//   eq_laqge_flat_kernel      n <= 128: four elements of the whole batch per thread, all loads in flight before the first store.
//   eq_laqge_tile_kernel      any n: workgroup = (tile of 16 columns, matrix), thread = row.
//   eq_lascl2_flat_kernel, eq_lascl2_ragged_kernel   V = diag(s) V on the matrices whose bit is set.
// Ragged launches (bbv_fetch: batched_blocked_body.h) are sized for the largest matrix of the launch: a workgroup whose tile lies
// outside its own matrix leaves as a whole before its first barrier, and every load and store is predicated on the matrix's own n.
#include "batched_blocked_body.h"
#include <float.h>

namespace {

typedef unsigned long long eq_key;
constexpr eq_key EQ_INF = 0x7FF0000000000000ull;
constexpr int EQ_RT = 64;    // rows per workgroup of the row maxima
constexpr int EQ_CT = 16;    // columns per workgroup of the column maxima and of the tiled scaling

__device__ __forceinline__ eq_key eq_abs(double a) { return (eq_key)__double_as_longlong(a) & 0x7FFFFFFFFFFFFFFFull; }
__device__ __forceinline__ double eq_val(eq_key k) { return __longlong_as_double((long long)k); }
// mpf_geequ's factor of a maximum m: 2^-floor(log2 m), the exponent clamped to [-1022, 1022]; 1 for m = 0
__device__ __forceinline__ double eq_pow2_inv(eq_key k) {
    if (k == 0) return 1.0;
    int e = (int)(k >> 52) - 1023;                                  // (a subnormal: -1023, clamped below)
    e = e < -1022 ? -1022 : (e > 1022 ? 1022 : e);
    return __longlong_as_double((long long)(1023 - e) << 52);
}
// dgeequ's rowcnd / colcnd of the smallest and largest maximum, smlnum = DBL_MIN
__device__ __forceinline__ double eq_cnd(eq_key kmin, eq_key kmax) {
    const double lo = eq_val(kmin), hi = eq_val(kmax), small = DBL_MIN, big = 1.0 / DBL_MIN;
    return (lo > small ? lo : small) / (hi < big ? hi : big);
}
__device__ __forceinline__ eq_key eq_shfl_xor(eq_key k, int o) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)k, o), hi = (unsigned)__shfl_xor((int)(unsigned)(k >> 32), o);
    return ((eq_key)hi << 32) | lo;
}
__device__ __forceinline__ eq_key eq_max(eq_key a, eq_key b) { return a > b ? a : b; }
__device__ __forceinline__ eq_key eq_min(eq_key a, eq_key b) { return a < b ? a : b; }

// the largest and smallest key and the smallest index among the W lanes of a team (W <= 64, a power of two), in every lane
template <int W>
__device__ __forceinline__ void eq_team_reduce(eq_key &kmax, eq_key &kmin, int &z) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) {
        kmax = eq_max(kmax, eq_shfl_xor(kmax, o));
        kmin = eq_min(kmin, eq_shfl_xor(kmin, o));
        const int z1 = __shfl_xor(z, o);
        z = z1 < z ? z1 : z;
    }
}
// the same over a workgroup of whole waves (at most 16), through s[3][16]; a barrier on entry guards the arrays' reuse
__device__ __forceinline__ void eq_wg_reduce(eq_key &kmax, eq_key &kmin, int &z, eq_key (*s)[16]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (int)(blockDim.x >> 6);
    eq_team_reduce<64>(kmax, kmin, z);
    __syncthreads();
    if (lane == 0) { s[0][w] = kmax; s[1][w] = kmin; s[2][w] = (eq_key)(unsigned)z; }
    __syncthreads();
    for (int k = 0; k < nw; ++k) {
        kmax = eq_max(kmax, s[0][k]);
        kmin = eq_min(kmin, s[1][k]);
        const int z1 = (int)s[2][k];
        z = z1 < z ? z1 : z;
    }
}
// Column maxima of NC columns held by every lane of a group of W lanes (NC <= W <= 64, powers of two): on return x[0] of lane l is the
// maximum of column l & (NC - 1) over the group
template <int NC, int W>
__device__ __forceinline__ eq_key eq_col_reduce(eq_key (&x)[NC]) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = NC / 2; o > 0; o >>= 1) {
        const bool up = (lane & o) != 0;
#pragma unroll
        for (int k = 0; k < o; ++k) {
            const eq_key keep = up ? x[k + o] : x[k], send = up ? x[k] : x[k + o];
            x[k] = eq_max(keep, eq_shfl_xor(send, o));
        }
    }
    eq_key m = x[0];
#pragma unroll
    for (int o = NC; o < W; o <<= 1) m = eq_max(m, eq_shfl_xor(m, o));
    return m;
}

// What a matrix's thread 0 records after the row maxima (kmax, kmin, z = the first zero row or n).  Returns whether the matrix goes on to
// its columns; r is written by the caller when the maximum is finite
__device__ __forceinline__ bool eq_row_verdict(eq_key kmax, eq_key kmin, int z, int n, bool lead, double *rowcnd, double *amax, int *info) {
    if (lead) *amax = eq_val(kmax);
    if (kmax >= EQ_INF) {                                           // a NaN or Inf: before any scale is formed
        if (lead) *info = 2 * n + 1;
        return false;
    }
    if (z < n) {
        if (lead) { *rowcnd = 0.0; *info = z + 1; }
        return false;
    }
    if (lead) *rowcnd = eq_cnd(kmin, kmax);
    return true;
}
// the same after the scaled column maxima (z = the first zero column or n); c is written by the caller when it returns true
__device__ __forceinline__ bool eq_col_verdict(eq_key kmax, eq_key kmin, int z, int n, bool lead, double *colcnd, int *info) {
    if (z < n) {
        if (lead) *info = n + z + 1;
        return false;
    }
    if (lead) { *colcnd = eq_cnd(kmin, kmax); *info = 0; }
    return true;
}

// ---- n <= 32: W lanes per matrix ------------------------------------------------------------------------------------------------------
// (W = 32 keeps its columns as two arrays of 16: one array of 32 leaves the registers)
template <int W>
__global__ __launch_bounds__(256) void eq_geequ_team_kernel(const double *__restrict__ A, long long lda, long long stride, int n, long long batch,
                                                            double *r, double *c, double *rowcnd, double *colcnd, double *amax, int *info) {
    constexpr int H = W > 16 ? 2 : 1, NC = W / H;
    const int i = threadIdx.x & (W - 1);
    long long b = (long long)blockIdx.x * (256 / W) + threadIdx.x / W;
    const bool live = b < batch, valid = live && i < n;
    if (!live) b = 0;
    const double *a = A + b * stride + i;
    eq_key x[NC], y[NC];                                            // columns 0 .. NC-1 and (H == 2) NC .. W-1
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        x[k] = (valid && k < n) ? eq_abs(a[k * lda]) : 0;
        y[k] = (H == 2 && valid && NC + k < n) ? eq_abs(a[(NC + k) * lda]) : 0;
    }
    eq_key rk = 0;
#pragma unroll
    for (int k = 0; k < NC; ++k) rk = eq_max(rk, eq_max(x[k], y[k]));
    eq_key kmax = valid ? rk : 0, kmin = valid ? rk : ~0ull;
    int z = (valid && rk == 0) ? i : n;
    eq_team_reduce<W>(kmax, kmin, z);
    bool go = eq_row_verdict(kmax, kmin, z, n, live && i == 0, rowcnd + b, amax + b, info + b);
    const double ri = eq_pow2_inv(rk);
    if (valid && kmax < EQ_INF) r[b * n + i] = ri;
    go = go && live;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        x[k] = (go && valid && k < n) ? eq_abs(eq_val(x[k]) * ri) : 0;
        y[k] = (H == 2 && go && valid && NC + k < n) ? eq_abs(eq_val(y[k]) * ri) : 0;
    }
    if (H == 2) {                                                   // the transposing step at offset NC, across the two arrays
        const bool up = (i & NC) != 0;
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            const eq_key keep = up ? y[k] : x[k], send = up ? x[k] : y[k];
            x[k] = eq_max(keep, eq_shfl_xor(send, NC));
        }
    }
    const eq_key ck = eq_col_reduce<NC, NC>(x);                     // lane j: column j
    kmax = (go && valid) ? ck : 0;
    kmin = (go && valid) ? ck : ~0ull;
    z = (go && valid && ck == 0) ? i : n;
    eq_team_reduce<W>(kmax, kmin, z);
    if (!go) return;
    if (eq_col_verdict(kmax, kmin, z, n, i == 0, colcnd + b, info + b) && valid) c[b * n + i] = eq_pow2_inv(ck);
}

// ---- n <= 128: one workgroup per matrix, RP rows x G column groups, 16 columns per thread ----------------------------------------------
template <int RP, int G>
__global__ __launch_bounds__(RP * G) void eq_geequ_wg_kernel(const double *__restrict__ A, long long lda, long long stride, int n, double *r, double *c,
                                                             double *rowcnd, double *colcnd, double *amax, int *info) {
    constexpr int NC = RP / G, RW = RP / 64;
    __shared__ eq_key srow[G][RP], scol[RW][RP], sred[3][16];
    const long long b = blockIdx.x;
    const int t = threadIdx.x, i = t % RP, g = t / RP, j0 = g * NC;
    const bool valid = i < n;
    const double *a = A + b * stride + i;
    eq_key x[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) x[k] = (valid && j0 + k < n) ? eq_abs(a[(long long)(j0 + k) * lda]) : 0;
    eq_key rk = 0;
#pragma unroll
    for (int k = 0; k < NC; ++k) rk = eq_max(rk, x[k]);
    srow[g][i] = rk;
    __syncthreads();
    rk = 0;
#pragma unroll
    for (int k = 0; k < G; ++k) rk = eq_max(rk, srow[k][i]);
    const bool mine = valid && g == 0;                              // one thread per row speaks for it
    eq_key kmax = mine ? rk : 0, kmin = mine ? rk : ~0ull;
    int z = (mine && rk == 0) ? i : n;
    eq_wg_reduce(kmax, kmin, z, sred);
    const bool go = eq_row_verdict(kmax, kmin, z, n, t == 0, rowcnd + b, amax + b, info + b);
    const double ri = eq_pow2_inv(rk);
    if (mine && kmax < EQ_INF) r[b * n + i] = ri;
    if (!go) return;                                                // (the whole workgroup)
#pragma unroll
    for (int k = 0; k < NC; ++k) x[k] = (valid && j0 + k < n) ? eq_abs(eq_val(x[k]) * ri) : 0;
    const eq_key ck = eq_col_reduce<NC, 64>(x);                     // lane l: column j0 + (l & (NC - 1)) over the wave's 64 rows
    const int lane = t & 63;
    if (lane < NC) scol[i / 64][j0 + lane] = ck;
    __syncthreads();
    const bool col = t < n;                                         // thread j: column j
    eq_key cj = 0;
    if (t < RP) {
#pragma unroll
        for (int k = 0; k < RW; ++k) cj = eq_max(cj, scol[k][t]);
    }
    kmax = col ? cj : 0;
    kmin = col ? cj : ~0ull;
    z = (col && cj == 0) ? t : n;
    eq_wg_reduce(kmax, kmin, z, sred);
    if (eq_col_verdict(kmax, kmin, z, n, t == 0, colcnd + b, info + b) && col) c[b * n + t] = eq_pow2_inv(cj);
}

// ---- any n: a matrix over several workgroups (bodies shared by the fixed-size and the ragged kernels) -----------------------------------
// 256 threads: lane = row tile * 64 + lane, wave w takes the columns w, w + 4, ..; rk[i] = the key of row i's maximum
__device__ __forceinline__ void eq_rowmax_body(const double *__restrict__ A, long long lda, int n, int tile, eq_key *rk) {
    __shared__ eq_key s[4][EQ_RT];
    if (tile * EQ_RT >= n) return;                                  // (the whole workgroup: the tile lies outside this matrix)
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, i = tile * EQ_RT + lane;
    eq_key m = 0;
    if (i < n) {
        const double *a = A + i;
        int j = w;
        for (; j + 12 < n; j += 16) {
            const double v0 = a[(long long)j * lda], v1 = a[(long long)(j + 4) * lda], v2 = a[(long long)(j + 8) * lda], v3 = a[(long long)(j + 12) * lda];
            m = eq_max(eq_max(m, eq_max(eq_abs(v0), eq_abs(v1))), eq_max(eq_abs(v2), eq_abs(v3)));
        }
        for (; j < n; j += 4) m = eq_max(m, eq_abs(a[(long long)j * lda]));
    }
    s[w][lane] = m;
    __syncthreads();
    if (w == 0 && i < n) rk[i] = eq_max(eq_max(s[0][lane], s[1][lane]), eq_max(s[2][lane], s[3][lane]));
}
// one workgroup of 256 per matrix
__device__ __forceinline__ void eq_rowfin_body(const eq_key *rk, int n, double *r, double *rowcnd, double *amax, int *info) {
    __shared__ eq_key sred[3][16];
    eq_key kmax = 0, kmin = ~0ull;
    int z = n;
    for (int i = threadIdx.x; i < n; i += 256) {
        const eq_key k = rk[i];
        kmax = eq_max(kmax, k);
        kmin = eq_min(kmin, k);
        if (k == 0 && i < z) z = i;
    }
    eq_wg_reduce(kmax, kmin, z, sred);
    eq_row_verdict(kmax, kmin, z, n, threadIdx.x == 0, rowcnd, amax, info);
    if (kmax >= EQ_INF) return;
    if (threadIdx.x == 0 && z >= n) *info = 0;                      // (the column kernels read it)
    for (int i = threadIdx.x; i < n; i += 256) r[i] = eq_pow2_inv(rk[i]);
}
// 256 threads: wave w takes four columns of the tile, lanes along the rows; ck[j] = the key of column j's scaled maximum
__device__ __forceinline__ void eq_colmax_body(const double *__restrict__ A, long long lda, int n, const double *__restrict__ r, const int *info,
                                               int tile, eq_key *ck) {
    if (tile * EQ_CT >= n || *info != 0) return;
    const int lane = threadIdx.x & 63, j0 = tile * EQ_CT + (int)(threadIdx.x >> 6) * 4;
    if (j0 >= n) return;                                            // (a whole wave; no barrier below)
    eq_key m[4] = {0, 0, 0, 0};
    for (int i = lane; i < n; i += 64) {
        const double ri = r[i];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (j0 + k < n) m[k] = eq_max(m[k], eq_abs(A[i + (long long)(j0 + k) * lda] * ri));
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        for (int o = 32; o > 0; o >>= 1) m[k] = eq_max(m[k], eq_shfl_xor(m[k], o));
        if (lane == 0 && j0 + k < n) ck[j0 + k] = m[k];
    }
}
__device__ __forceinline__ void eq_colfin_body(const eq_key *ck, int n, double *c, double *colcnd, int *info) {
    __shared__ eq_key sred[3][16];
    if (*info != 0) return;                                         // (the whole workgroup: every thread reads the same word)
    eq_key kmax = 0, kmin = ~0ull;
    int z = n;
    for (int j = threadIdx.x; j < n; j += 256) {
        const eq_key k = ck[j];
        kmax = eq_max(kmax, k);
        kmin = eq_min(kmin, k);
        if (k == 0 && j < z) z = j;
    }
    eq_wg_reduce(kmax, kmin, z, sred);
    if (!eq_col_verdict(kmax, kmin, z, n, threadIdx.x == 0, colcnd, info)) return;
    for (int j = threadIdx.x; j < n; j += 256) c[j] = eq_pow2_inv(ck[j]);
}
// workgroup = (tile of EQ_CT columns, matrix), thread = row (blockDim.x rows at a time); q = the matrix's equed
__device__ __forceinline__ void eq_laqge_body(const double *A, long long lda, int n, const double *__restrict__ r, const double *__restrict__ c, int q,
                                              double *out, int tile) {
    const int j0 = tile * EQ_CT;
    if (j0 >= n || (q == 0 && out == A)) return;
    const int jn = n - j0 < EQ_CT ? n - j0 : EQ_CT;
    for (int i = threadIdx.x; i < n; i += (int)blockDim.x) {
        const double ri = (q & 1) ? r[i] : 1.0;
        for (int k = 0; k < jn; ++k) {
            double v = A[i + (long long)(j0 + k) * lda];
            if (q & 1) v = v * ri;
            if (q & 2) v = v * c[j0 + k];
            out[i + (long long)(j0 + k) * lda] = v;
        }
    }
}

// fixed size: blockIdx.y = matrix, the chunk's maxima at b * n
__global__ __launch_bounds__(256) void eq_rowmax_kernel(const double *A, long long lda, long long stride, int n, eq_key *rk) {
    eq_rowmax_body(A + (long long)blockIdx.y * stride, lda, n, (int)blockIdx.x, rk + (long long)blockIdx.y * n);
}
__global__ __launch_bounds__(256) void eq_rowfin_kernel(const eq_key *rk, int n, double *r, double *rowcnd, double *amax, int *info) {
    const long long b = blockIdx.x;
    eq_rowfin_body(rk + b * n, n, r + b * n, rowcnd + b, amax + b, info + b);
}
__global__ __launch_bounds__(256) void eq_colmax_kernel(const double *A, long long lda, long long stride, int n, const double *r, const int *info,
                                                        eq_key *ck) {
    const long long b = blockIdx.y;
    eq_colmax_body(A + b * stride, lda, n, r + b * n, info + b, (int)blockIdx.x, ck + b * n);
}
__global__ __launch_bounds__(256) void eq_colfin_kernel(const eq_key *ck, int n, double *c, double *colcnd, int *info) {
    const long long b = blockIdx.x;
    eq_colfin_body(ck + b * n, n, c + b * n, colcnd + b, info + b);
}
__global__ __launch_bounds__(256) void eq_laqge_tile_kernel(const double *A, long long lda, long long stride, int n, const double *r, const double *c,
                                                            const int *equed, double *out) {
    const long long b = blockIdx.y;
    eq_laqge_body(A + b * stride, lda, n, r + b * n, c + b * n, equed[b], out + b * stride, (int)blockIdx.x);
}

// ragged: blockIdx.y (the finishing kernels: blockIdx.x) = list entry, the chunk's maxima at row[entry] - row0
__global__ __launch_bounds__(256) void eqv_rowmax_kernel(const double *A, BtRagged v, const int *idx, const long long *row, long long row0, eq_key *rk) {
    const bbv_entry e = bbv_fetch(v, idx, blockIdx.y);
    eq_rowmax_body(A + e.off, e.ld, e.n, (int)blockIdx.x, rk + (row[blockIdx.y] - row0));
}
__global__ __launch_bounds__(256) void eqv_rowfin_kernel(const eq_key *rk, BtRagged v, const int *idx, const long long *row, long long row0, double *r,
                                                         double *rowcnd, double *amax, int *info) {
    const bbv_entry e = bbv_fetch(v, idx, blockIdx.x);
    eq_rowfin_body(rk + (row[blockIdx.x] - row0), e.n, r + e.offv, rowcnd + e.b, amax + e.b, info + e.b);
}
__global__ __launch_bounds__(256) void eqv_colmax_kernel(const double *A, BtRagged v, const int *idx, const long long *row, long long row0,
                                                         const double *r, const int *info, eq_key *ck) {
    const bbv_entry e = bbv_fetch(v, idx, blockIdx.y);
    eq_colmax_body(A + e.off, e.ld, e.n, r + e.offv, info + e.b, (int)blockIdx.x, ck + (row[blockIdx.y] - row0));
}
__global__ __launch_bounds__(256) void eqv_colfin_kernel(const eq_key *ck, BtRagged v, const int *idx, const long long *row, long long row0, double *c,
                                                         double *colcnd, int *info) {
    const bbv_entry e = bbv_fetch(v, idx, blockIdx.x);
    eq_colfin_body(ck + (row[blockIdx.x] - row0), e.n, c + e.offv, colcnd + e.b, info + e.b);
}
__global__ __launch_bounds__(256) void eqv_laqge_kernel(const double *A, BtRagged v, const int *idx, const double *r, const double *c, const int *equed,
                                                        double *out) {
    const bbv_entry e = bbv_fetch(v, idx, blockIdx.y);
    eq_laqge_body(A + e.off, e.ld, e.n, r + e.offv, c + e.offv, equed[e.b], out + e.off, (int)blockIdx.x);
}
// the matrices of order 0: dgeequ's quick return.  One thread per matrix
__global__ __launch_bounds__(256) void eqv_empty_kernel(const int *idx, long long count, double *rowcnd, double *colcnd, double *amax, int *info) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const long long b = idx[i];
    rowcnd[b] = 1.0;
    colcnd[b] = 1.0;
    amax[b] = 0.0;
    info[b] = 0;
}

// ---- laqge's decision and the spreads: T lanes per matrix; idx null: matrix = team, its n doubles at team * n ---------------------------
template <int T>
__global__ __launch_bounds__(256) void eq_decide_kernel(int rule, int n, long long count, const int *idx, const int *vn, const long long *voffv,
                                                        const double *r, const double *c, const double *rowcnd, const double *colcnd,
                                                        const double *amax, const int *info, int *equed, double *spread) {
    const int l = threadIdx.x & (T - 1);
    const long long m = (long long)blockIdx.x * (256 / T) + threadIdx.x / T;
    const bool live = m < count;
    long long b = 0, at = 0;
    int nn = 0;
    if (live) {
        b = idx ? idx[m] : m;
        nn = idx ? vn[b] : n;
        at = idx ? voffv[b] : m * n;
    }
    bool rows = false, cols = false;
    if (live && nn > 0 && rule != 0 && info[b] == 0) {
        if (rule == 2) rows = cols = true;
        else {                                                      // dlaqge's rule as mpf_gesvx states it
            const double small = DBL_MIN / DBL_EPSILON, large = 1.0 / small, am = amax[b];
            rows = rowcnd[b] < 0.1 || am < small || am > large;
            cols = colcnd[b] < 0.1;
        }
    }
    eq_key rmax = 0, rmin = ~0ull, cmax = 0, cmin = ~0ull;
    if (spread) {
        if (rows)
            for (int i = l; i < nn; i += T) { const eq_key k = eq_abs(r[at + i]); rmax = eq_max(rmax, k); rmin = eq_min(rmin, k); }
        if (cols)
            for (int i = l; i < nn; i += T) { const eq_key k = eq_abs(c[at + i]); cmax = eq_max(cmax, k); cmin = eq_min(cmin, k); }
        int z = 0;
        eq_team_reduce<T>(rmax, rmin, z);
        eq_team_reduce<T>(cmax, cmin, z);
    }
    if (!live || l != 0) return;
    equed[b] = (rows ? 1 : 0) | (cols ? 2 : 0);
    if (spread) {
        spread[2 * b] = rows ? eq_val(rmax) / eq_val(rmin) : 1.0;
        spread[2 * b + 1] = cols ? eq_val(cmax) / eq_val(cmin) : 1.0;
    }
}

// ---- n <= 128: four elements per thread, every load before the first store (out may be A); total = batch * n * n < 2^31 ----------------------
constexpr int EQ_FE = 4;
__global__ __launch_bounds__(256) void eq_laqge_flat_kernel(const double *A, long long lda, long long stride, unsigned n, unsigned total,
                                                            const double *__restrict__ r, const double *__restrict__ c,
                                                            const int *__restrict__ equed, double *out) {
    const unsigned nn = n * n, e0 = blockIdx.x * (256u * EQ_FE) + threadIdx.x;
    long long at[EQ_FE];
    double v[EQ_FE], ri[EQ_FE], cj[EQ_FE];
    int q[EQ_FE];
#pragma unroll
    for (int k = 0; k < EQ_FE; ++k) {
        const unsigned e = e0 + 256u * k;
        q[k] = -1;                                                  // (past the end)
        if (e < total) {
            const unsigned b = e / nn, rem = e - b * nn, j = rem / n, i = rem - j * n;
            at[k] = (long long)b * stride + i + (long long)j * lda;
            q[k] = equed[b];
            v[k] = A[at[k]];
            ri[k] = r[(long long)b * n + i];                        // (a matrix that is not scaled: whatever is there, not used)
            cj[k] = c[(long long)b * n + j];
        }
    }
#pragma unroll
    for (int k = 0; k < EQ_FE; ++k) {
        if (q[k] < 0 || (q[k] == 0 && out == A)) continue;
        double w = v[k];
        if (q[k] & 1) w = w * ri[k];
        if (q[k] & 2) w = w * cj[k];
        out[at[k]] = w;
    }
}
// V[b] = diag(s[b]) V[b] where equed is null or equed[b] & bit; total = batch * n * nrhs < 2^31
__global__ __launch_bounds__(256) void eq_lascl2_flat_kernel(const double *__restrict__ s, unsigned n, unsigned nrhs, unsigned total, double *V,
                                                             long long ldv, long long stride, const int *__restrict__ equed, int bit) {
    const unsigned e = blockIdx.x * 256u + threadIdx.x;
    if (e >= total) return;
    const unsigned per = n * nrhs, b = e / per, rem = e - b * per, k = rem / n, i = rem - k * n;
    if (equed && !(equed[b] & bit)) return;
    const long long at = (long long)b * stride + i + (long long)k * ldv;
    V[at] = s[(long long)b * n + i] * V[at];
}
// ragged: workgroup = (tile of 4 columns, list entry), thread = row of the matrix's rows of the tall V
__global__ __launch_bounds__(1024) void eq_lascl2_ragged_kernel(const double *__restrict__ s, BtRagged v, const int *idx, int nrhs, double *V,
                                                                long long ldv, const int *equed, int bit) {
    const bbv_entry e = bbv_fetch(v, idx, blockIdx.y);
    if (equed && !(equed[e.b] & bit)) return;
    const int i = threadIdx.x, k0 = (int)blockIdx.x * 4;
    if (i >= e.n) return;
    const double si = s[e.offv + i];
    for (int k = k0; k < k0 + 4 && k < nrhs; ++k) {
        double *p = V + e.offv + i + (long long)k * ldv;
        *p = si * *p;
    }
}

bool eq_small(mpf_ctx *c, const char *who, int n, int64_t batch) {
    const bool ok = n >= 1 && n <= 128 && batch >= 1 && batch <= BT_MAX_LAUNCH;
    if (!ok) c->err = std::string(who) + ": size out of range";
    return ok;
}
bool eq_blocked(mpf_ctx *c, const char *who, int n, int64_t batch) {
    const bool ok = n >= 1 && n <= BB_MAXN && batch >= 1 && batch <= BB_MAX_LAUNCH;
    if (!ok) c->err = std::string(who) + ": size out of range";
    return ok;
}
unsigned eq_threads(int nmax) { return nmax >= 256 ? 256u : (unsigned)((nmax + 63) / 64 * 64); }

} // namespace

// ---- launchers -----------------------------------------------------------------------------------------------------------------------
int launch_geequ_batched(mpf_ctx *c, const double *A, int64_t lda, int64_t stride, int n, int64_t batch, double *r, double *cs, double *rowcnd,
                         double *colcnd, double *amax, int *info) {
    if (!eq_small(c, "launch_geequ_batched", n, batch)) return -1;
    hipStream_t st = c->stream;
    if (n <= 32) {
        const int W = n <= 8 ? 8 : (n <= 16 ? 16 : 32);
        const unsigned g = (unsigned)((batch + 256 / W - 1) / (256 / W));
        if (W == 8) eq_geequ_team_kernel<8><<<g, 256, 0, st>>>(A, lda, stride, n, batch, r, cs, rowcnd, colcnd, amax, info);
        else if (W == 16) eq_geequ_team_kernel<16><<<g, 256, 0, st>>>(A, lda, stride, n, batch, r, cs, rowcnd, colcnd, amax, info);
        else eq_geequ_team_kernel<32><<<g, 256, 0, st>>>(A, lda, stride, n, batch, r, cs, rowcnd, colcnd, amax, info);
    } else if (n <= 64) eq_geequ_wg_kernel<64, 4><<<(unsigned)batch, 256, 0, st>>>(A, lda, stride, n, r, cs, rowcnd, colcnd, amax, info);
    else eq_geequ_wg_kernel<128, 8><<<(unsigned)batch, 1024, 0, st>>>(A, lda, stride, n, r, cs, rowcnd, colcnd, amax, info);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

// rk, ck: n keys per matrix of the launch each (the context's workspace)
int launch_geequ_batched_blocked(mpf_ctx *c, const double *A, int64_t lda, int64_t stride, int n, int64_t batch, double *r, double *cs,
                                 double *rowcnd, double *colcnd, double *amax, int *info, double *rk, double *ck) {
    if (!eq_blocked(c, "launch_geequ_batched_blocked", n, batch)) return -1;
    hipStream_t st = c->stream;
    eq_key *kr = (eq_key *)rk, *kc = (eq_key *)ck;
    eq_rowmax_kernel<<<dim3((unsigned)((n + EQ_RT - 1) / EQ_RT), (unsigned)batch), 256, 0, st>>>(A, lda, stride, n, kr);
    eq_rowfin_kernel<<<(unsigned)batch, 256, 0, st>>>(kr, n, r, rowcnd, amax, info);
    eq_colmax_kernel<<<dim3((unsigned)((n + EQ_CT - 1) / EQ_CT), (unsigned)batch), 256, 0, st>>>(A, lda, stride, n, r, info, kc);
    eq_colfin_kernel<<<(unsigned)batch, 256, 0, st>>>(kc, n, cs, colcnd, info);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

int launch_geequ_vbatched(mpf_ctx *c, const BtRagged &v, const int32_t *idx, const int64_t *row, int64_t row0, int64_t count, int nmax,
                          const double *A, double *r, double *cs, double *rowcnd, double *colcnd, double *amax, int *info, double *rk, double *ck) {
    if (count < 1) return 0;
    if (!eq_blocked(c, "launch_geequ_vbatched", nmax, count)) return -1;
    hipStream_t st = c->stream;
    eq_key *kr = (eq_key *)rk, *kc = (eq_key *)ck;
    const long long *rw = (const long long *)row;
    eqv_rowmax_kernel<<<dim3((unsigned)((nmax + EQ_RT - 1) / EQ_RT), (unsigned)count), 256, 0, st>>>(A, v, idx, rw, row0, kr);
    eqv_rowfin_kernel<<<(unsigned)count, 256, 0, st>>>(kr, v, idx, rw, row0, r, rowcnd, amax, info);
    eqv_colmax_kernel<<<dim3((unsigned)((nmax + EQ_CT - 1) / EQ_CT), (unsigned)count), 256, 0, st>>>(A, v, idx, rw, row0, r, info, kc);
    eqv_colfin_kernel<<<(unsigned)count, 256, 0, st>>>(kc, v, idx, rw, row0, cs, colcnd, info);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

int launch_geequ_vbatched_empty(mpf_ctx *c, const int32_t *idx, int64_t count, double *rowcnd, double *colcnd, double *amax, int *info) {
    if (count < 1) return 0;
    if (count > BT_MAX_LAUNCH) { c->err = "launch_geequ_vbatched_empty: size out of range"; return -1; }
    eqv_empty_kernel<<<(unsigned)((count + 255) / 256), 256, 0, c->stream>>>(idx, count, rowcnd, colcnd, amax, info);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

// equed (and spread, when not null) of `count` matrices: idx null -- matrices 0 .. count-1 of one order n; else the list entries idx[0 ..
// count) of a descriptor (orders 0 included)
int launch_laqge_decide(mpf_ctx *c, int rule, int n, int64_t count, const int32_t *idx, const BtRagged *v, const double *r, const double *cs,
                        const double *rowcnd, const double *colcnd, const double *amax, const int *info, int *equed, double *spread) {
    if (count < 1) return 0;
    if (count > BT_MAX_LAUNCH || rule < 0 || rule > 2) { c->err = "launch_laqge_decide: argument out of range"; return -1; }
    const int *vn = v ? v->n : nullptr;
    const long long *vo = v ? (const long long *)v->offv : nullptr;
    if (!idx && n <= 32) {
        eq_decide_kernel<8><<<(unsigned)((count + 31) / 32), 256, 0, c->stream>>>(rule, n, count, idx, vn, vo, r, cs, rowcnd, colcnd, amax, info, equed, spread);
    } else {
        eq_decide_kernel<64><<<(unsigned)((count + 3) / 4), 256, 0, c->stream>>>(rule, n, count, idx, vn, vo, r, cs, rowcnd, colcnd, amax, info, equed, spread);
    }
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

// batch * n * n < 2^31
int launch_laqge_batched(mpf_ctx *c, const double *A, int64_t lda, int64_t stride, int n, int64_t batch, const double *r, const double *cs,
                         const int *equed, double *out) {
    if (!eq_small(c, "launch_laqge_batched", n, batch) || batch * n * n >= ((int64_t)1 << 31)) { c->err = "launch_laqge_batched: size out of range"; return -1; }
    const unsigned total = (unsigned)(batch * n * n);
    eq_laqge_flat_kernel<<<(total + 256u * EQ_FE - 1u) / (256u * EQ_FE), 256, 0, c->stream>>>(A, lda, stride, (unsigned)n, total, r, cs, equed, out);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

int launch_laqge_batched_blocked(mpf_ctx *c, const double *A, int64_t lda, int64_t stride, int n, int64_t batch, const double *r, const double *cs,
                                 const int *equed, double *out) {
    if (!eq_blocked(c, "launch_laqge_batched_blocked", n, batch)) return -1;
    eq_laqge_tile_kernel<<<dim3((unsigned)((n + EQ_CT - 1) / EQ_CT), (unsigned)batch), eq_threads(n), 0, c->stream>>>(A, lda, stride, n, r, cs, equed, out);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

int launch_laqge_vbatched(mpf_ctx *c, const BtRagged &v, const int32_t *idx, int64_t count, int nmax, const double *A, const double *r,
                          const double *cs, const int *equed, double *out) {
    if (count < 1) return 0;
    if (!eq_blocked(c, "launch_laqge_vbatched", nmax, count)) return -1;
    eqv_laqge_kernel<<<dim3((unsigned)((nmax + EQ_CT - 1) / EQ_CT), (unsigned)count), eq_threads(nmax), 0, c->stream>>>(A, v, idx, r, cs, equed, out);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

// batch * n * nrhs < 2^31
int launch_lascl2_batched(mpf_ctx *c, const double *s, int n, int64_t batch, int nrhs, double *V, int64_t ldv, int64_t stride, const int *equed,
                          int bit) {
    if (n < 1 || nrhs < 1 || batch < 1 || batch * n * nrhs >= ((int64_t)1 << 31)) { c->err = "launch_lascl2_batched: size out of range"; return -1; }
    const unsigned total = (unsigned)(batch * n * nrhs);
    eq_lascl2_flat_kernel<<<(total + 255u) / 256u, 256, 0, c->stream>>>(s, (unsigned)n, (unsigned)nrhs, total, V, ldv, stride, equed, bit);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

int launch_lascl2_vbatched(mpf_ctx *c, const BtRagged &v, const int32_t *idx, int64_t count, int nmax, const double *s, int nrhs, double *V,
                           int64_t ldv, const int *equed, int bit) {
    if (count < 1 || nrhs < 1) return 0;
    if (!eq_blocked(c, "launch_lascl2_vbatched", nmax, count) || nrhs > 4 * 65535) { c->err = "launch_lascl2_vbatched: size out of range"; return -1; }
    eq_lascl2_ragged_kernel<<<dim3((unsigned)((nrhs + 3) / 4), (unsigned)count), (unsigned)((nmax + 63) / 64 * 64), 0, c->stream>>>(s, v, idx, nrhs, V, ldv,
                                                                                                                             equed, bit);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}
