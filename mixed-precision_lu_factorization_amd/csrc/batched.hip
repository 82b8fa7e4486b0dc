// LU of many small matrices (mpf_getrf_batched, mpf_getrs_batched; contracts in include/mpf_c.h, host side in mpf_batched.cpp).
//
// The numeric contract is dpivot.hip's on an n x n panel: idamax with a strict > on |a| (a NaN counts as 0, the first maximum wins,
// an all-zero rest keeps p = j), m = a_ij / a_jj, then per element one update per k in ascending order (contract C3: separate
// multiply and subtract, or one FMA).  Every matrix is factored by the lanes of ONE wave or by ONE workgroup, from registers or LDS:
// every launch is an ordinary launch, nothing waits for another workgroup, and a matrix's bits depend on nothing but the matrix.
//
// In both forms of the factorization rows never move while the matrix is resident: the owner of a row keeps the row's CURRENT
// position (what dgetf2's interchange changes and what breaks a tie, as dtp_select_kernel does) and the rows go to their final
// positions with the store.
//   bt_getrf_wave_kernel<W>     n <= W = 8, 16, 32: 64 / W matrices per wave64, four waves per workgroup; lane = (matrix, row), the
//                               row's W columns in registers (column loops fully unrolled, predicated on n).  The pivot search is a
//                               cross-lane reduction over (key, position) inside the matrix's W lanes; the pivot row is broadcast by
//                               ds_bpermute.  No LDS memory, no barrier.  (One matrix per wave, the pivot row through v_readlane, was
//                               the first form: at n = 8 seven lanes in eight idle and the kernel is bound by instruction issue --
//                               measured 1.88 ms for 2^20 matrices against 0.23 ms with eight per wave.)
//   bt_getrf_wg_kernel<H>       n <= 128: one workgroup per matrix, the matrix in LDS with an odd leading dimension (n | 1: column
//                               walks and row walks are both conflict-free).  Per column step wave 0 finds the pivot and forms the
//                               multipliers, then all waves apply the rank-1 update; two barriers.  (A first form had one barrier and
//                               let every wave repeat the search and every column group the divisions: that fixed cost per wave was
//                               the whole time -- 6.0 ms for 4096 matrices of order 128 against 3.6 ms now.)
//   bt_getrs_kernel<H, TS>      the factors once into LDS, then dgetrs's chains per right-hand-side column, lane = row, b_j by
//                               v_readlane or ds_bpermute -- no barrier after the load.  A team of TS threads per matrix: 8, 16 or 32
//                               lanes of a wave for n <= 32 (columns one after the other), four waves above (a wave per column).
#include "mpf_internal.h"
#include <limits.h>

constexpr int BT_MAXN = 128;   // largest matrix (the workgroup form's LDS: 129 x 128 doubles)
constexpr int BT_T = 256;      // threads per workgroup, every kernel of this file

extern __shared__ __attribute__((aligned(16))) char bt_smem[];

template <bool FUSED>
__device__ __forceinline__ double bt_mulsub(double x, double m, double u) {
    if (FUSED) return __builtin_fma(-m, u, x);
    const double t = m * u; // file is compiled with -ffp-contract=off: stays mul + sub
    return x - t;
}
// search key of an element: |a|'s bit pattern (monotone in |a|), 0 for a NaN
__device__ __forceinline__ unsigned long long bt_key(double a) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(a) & 0x7FFFFFFFFFFFFFFFull;
    return b > 0x7FF0000000000000ull ? 0ull : b;
}
// (k1, r1) beats (k0, r0): larger key, or the same key at an earlier position
__device__ __forceinline__ bool bt_beats(unsigned long long k1, int r1, unsigned long long k0, int r0) {
    return k1 > k0 || (k1 == k0 && r1 < r0);
}
// best (key, position) of the wave, in every lane
__device__ __forceinline__ void bt_wave_best(unsigned long long &key, int &pos) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)key, o), hi = (unsigned)__shfl_xor((int)(unsigned)(key >> 32), o);
        const unsigned long long k1 = ((unsigned long long)hi << 32) | lo;
        const int p1 = __shfl_xor(pos, o);
        if (bt_beats(k1, p1, key, pos)) { key = k1; pos = p1; }
    }
}
// v of a wave-uniform lane, in every lane (v_readlane: through scalar registers, not LDS)
__device__ __forceinline__ double bt_readlane(double v, int lane) {
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)b, lane), hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), lane);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// ---- factorization, wave form ------------------------------------------------------------------------------------------------------
// G = 64 / W matrices per wave: lane = (matrix g, row r).  The reduction's xor steps below W stay inside a matrix's lanes; the pivot
// row differs per matrix, so it is broadcast by ds_bpermute, not through scalar registers.
template <int W, bool FUSED>
__global__ __launch_bounds__(BT_T) void bt_getrf_wave_kernel(double *A, long long lda, long long strideA, int n, long long batch, int *ipiv,
                                                            long long strideP, int *info) {
    constexpr int G = 64 / W;
    const int lane = threadIdx.x & 63, r = lane & (W - 1), g = lane / W;
    const long long b0 = ((long long)blockIdx.x * (BT_T / 64) + (threadIdx.x >> 6)) * G, b = b0 + g;
    if (b0 >= batch) return;                                    // (the whole wave)
    const bool valid = b < batch && r < n;
    double *a = A + (valid ? b : b0) * strideA;
    double x[W];
#pragma unroll
    for (int c = 0; c < W; ++c) x[c] = (valid && c < n) ? a[r + (long long)c * lda] : 0.0;
    int cp = r, mypiv = 0, inf = 0;                             // cp: this row's current position
#pragma unroll
    for (int j = 0; j < W; ++j) {
        if (j < n) {                                            // (uniform)
            const bool open = valid && cp >= j;
            unsigned long long key = open ? bt_key(x[j]) : 0ull;
            int pos = open ? ((cp << 8) | r) : INT_MAX;         // ordered by position; carries the row.  The row at position j is open
#pragma unroll
            for (int o = W / 2; o > 0; o >>= 1) {
                const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)key, o), hi = (unsigned)__shfl_xor((int)(unsigned)(key >> 32), o);
                const unsigned long long k1 = ((unsigned long long)hi << 32) | lo;
                const int p1 = __shfl_xor(pos, o);
                if (bt_beats(k1, p1, key, pos)) { key = k1; pos = p1; }
            }
            const int p = pos >> 8, wl = pos & (W - 1);   // (a matrix past the batch's end has no open row: its lanes compute on zeros)
            if (r == j) mypiv = p + 1;
            if (r == wl) cp = j;
            else if (cp == j) cp = p;                           // dgetf2's interchange: the row at position j goes where the pivot row was
            const int src = (lane & ~(W - 1)) | wl;             // the pivot row's lane
            const double uj = __shfl(x[j], src);
            if (uj == 0.0 && inf == 0) inf = j + 1;
            const bool below = valid && cp > j;
            const double m = x[j] / uj;
            if (below) x[j] = m;
#pragma unroll
            for (int c = j + 1; c < W; ++c) {
                const double uc = __shfl(x[c], src);
                if (below) x[c] = bt_mulsub<FUSED>(x[c], m, uc);
            }
        }
    }
    if (valid) {
#pragma unroll
        for (int c = 0; c < W; ++c)
            if (c < n) a[cp + (long long)c * lda] = x[c];
        ipiv[b * strideP + r] = mypiv;
        if (info && r == 0) info[b] = inf;
    }
}

// ---- the matrix between global memory and LDS: coalesced, 16 bytes per lane where the matrix allows it --------------------------------
// T[r + c * ldl] = a[r + c * lda]; a thread takes the rows 2 i, 2 i + 1 of a column
__device__ __forceinline__ void bt_load_matrix(const double *a, long long lda, int n, double *T, int ldl, int t, int nt) {
    const int half = (n + 1) >> 1;
    const bool vec = (((unsigned long long)a & 15ull) == 0ull) && ((lda & 1) == 0);   // every column starts on 16 bytes
    for (int i = t; i < half * n; i += nt) {
        const int c = i / half, r = (i - c * half) * 2;
        const double *src = a + r + (long long)c * lda;
        if (r + 1 < n) {
            double v0, v1;
            if (vec) { const double2 v = *(const double2 *)src; v0 = v.x; v1 = v.y; }
            else { v0 = src[0]; v1 = src[1]; }
            T[r + c * ldl] = v0;
            T[r + 1 + c * ldl] = v1;
        } else T[r + c * ldl] = src[0];
    }
}

template <int H>
__device__ __forceinline__ double bt_bcast(const double (&x)[H], int j) {   // x of row j (j uniform; rows lane + 64 h), in every lane
    if (H == 1) return bt_readlane(x[0], j);
    return j < 64 ? bt_readlane(x[0], j) : bt_readlane(x[H - 1], j - 64);
}

// ---- factorization, workgroup form --------------------------------------------------------------------------------------------------
// LDS: T[ldl x n] doubles, then rowpos[BT_MAXN] (the rows' positions), inv[BT_MAXN] (the row at each position, for the store),
// piv[BT_MAXN], ctl[4] (the pivot row of the step)
static size_t bt_getrf_wg_lds(int n) { return (size_t)(n | 1) * n * sizeof(double) + (3 * BT_MAXN + 4) * sizeof(int); }

// H = 1: n <= 64, 256 threads (64 rows x 4 column groups; up to four workgroups per CU); H = 2: 1024 threads (128 rows x 8 column
// groups: the one workgroup the LDS leaves room for brings 16 waves).  A column step has two phases and two barriers:
//   A  wave 0 alone, H rows per lane, the rows' positions in its registers: the pivot search on column j, the pivot through
//      v_readlane, the multipliers (one division per row, stored in place);
//   B  every thread: the rank-1 update of the columns right of j, a thread one row and every ncg-th column.
// Nothing is computed twice; while wave 0 is in phase A the other waves wait at the barrier and leave the CU to other workgroups.
template <bool FUSED, int H>
__global__ __launch_bounds__(H == 1 ? 256 : 1024) void bt_getrf_wg_kernel(double *A, long long lda, long long strideA, int n, int *ipiv,
                                                                         long long strideP, int *info) {
    constexpr int NT = H == 1 ? 256 : 1024, rg = 64 * H, ncg = NT / rg;
    const int ldl = n | 1;
    double *T = (double *)bt_smem;
    int *rowpos = (int *)(T + (size_t)ldl * n), *inv = rowpos + BT_MAXN, *piv = inv + BT_MAXN, *ctl = piv + BT_MAXN;
    const int tid = threadIdx.x, lane = tid & 63;
    double *a = A + (long long)blockIdx.x * strideA;
    bt_load_matrix(a, lda, n, T, ldl, tid, NT);
    const int row = tid & (rg - 1), cg = tid / rg;               // phase B: this thread's row and column group
    int cp[H];                                                   // wave 0: the current positions of the rows lane + 64 h
#pragma unroll
    for (int h = 0; h < H; ++h) cp[h] = lane + 64 * h;
    int inf = 0;
    for (int j = 0; j < n; ++j) {
        __syncthreads();                                         // step j - 1's update is in LDS, its rowpos and ctl have been read
        if (tid < 64) {
            double xv[H];
            unsigned long long key = 0ull;
            int best = INT_MAX;
#pragma unroll
            for (int h = 0; h < H; ++h) {
                const int r = lane + 64 * h;
                xv[h] = 0.0;
                if (r < n && cp[h] >= j) {
                    xv[h] = T[r + j * ldl];
                    const unsigned long long k1 = bt_key(xv[h]);
                    const int p1 = (cp[h] << 8) | r;             // ordered by position; carries the row
                    if (bt_beats(k1, p1, key, best)) { key = k1; best = p1; }
                }
            }
            bt_wave_best(key, best);                             // (the row at position j is a candidate: best names a row < n)
            const int p = best >> 8, wr = best & (BT_MAXN - 1);
            const double uj = bt_bcast<H>(xv, wr);
#pragma unroll
            for (int h = 0; h < H; ++h) {
                const int r = lane + 64 * h;
                if (r == wr) cp[h] = j;
                else if (cp[h] == j) cp[h] = p;                  // dgetf2's interchange
                if (r < n) {
                    rowpos[r] = cp[h];
                    if (cp[h] > j) T[r + j * ldl] = xv[h] / uj;
                }
            }
            if (lane == 0) {
                piv[j] = p + 1;
                ctl[0] = wr;
                if (uj == 0.0 && inf == 0) inf = j + 1;
            }
        }
        __syncthreads();
        if (row < n && rowpos[row] > j) {
            const double m = T[row + j * ldl];
            double *xr = T + row;
            const double *ur = T + ctl[0];
            int c = j + 1 + cg;
            for (; c + 3 * ncg < n; c += 4 * ncg) {              // four columns at a time: all eight LDS reads in flight before the first store
                double x[4], u[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) { x[q] = xr[(c + q * ncg) * ldl]; u[q] = ur[(c + q * ncg) * ldl]; }
#pragma unroll
                for (int q = 0; q < 4; ++q) xr[(c + q * ncg) * ldl] = bt_mulsub<FUSED>(x[q], m, u[q]);
            }
            for (; c < n; c += ncg) xr[c * ldl] = bt_mulsub<FUSED>(xr[c * ldl], m, ur[c * ldl]);
        }
    }
    __syncthreads();
    if (tid < n) inv[rowpos[tid]] = tid;                         // the row that stands at each position
    __syncthreads();
    {
        const int half = (n + 1) >> 1;
        const bool vec = (((unsigned long long)a & 15ull) == 0ull) && ((lda & 1) == 0);
        for (int i = tid; i < half * n; i += NT) {
            const int c = i / half, r = (i - c * half) * 2;
            double *dst = a + r + (long long)c * lda;
            const double v0 = T[inv[r] + c * ldl];
            if (r + 1 < n) {
                const double v1 = T[inv[r + 1] + c * ldl];
                if (vec) *(double2 *)dst = make_double2(v0, v1);
                else { dst[0] = v0; dst[1] = v1; }
            } else dst[0] = v0;
        }
    }
    if (tid < n) ipiv[(long long)blockIdx.x * strideP + tid] = piv[tid];
    if (info && tid == 0) info[blockIdx.x] = inf;
}

// ---- solve ----------------------------------------------------------------------------------------------------------------------------
// LDS per matrix: T[ldl x n] doubles, map[n], pv[n] ints, rounded up to 16 bytes
static size_t bt_getrs_lds(int n) { return ((size_t)(n | 1) * n * sizeof(double) + 2 * (size_t)n * sizeof(int) + 15) & ~(size_t)15; }

// b_j of the team's column, in every lane of the team: through scalar registers for a team of whole waves, by ds_bpermute inside a wave
template <int H, int TS>
__device__ __forceinline__ double bt_rhs_bcast(const double (&x)[H], int j) {
    if (TS >= 64) return bt_bcast<H>(x, j);
    return __shfl(x[0], (int)((threadIdx.x & 63 & ~(TS - 1)) | j));
}

// A team of TS threads per matrix, 256 / TS matrices per workgroup, each with its own LDS region: TS = 8, 16, 32 (n <= TS: lane = row,
// the columns of B one after the other) or 256 (four waves, H rows per lane; a wave takes every fourth column of B)
template <int H, int TS>
__global__ __launch_bounds__(BT_T) void bt_getrs_kernel(int trans, const double *LU, long long ldlu, long long strideLU, int n, long long batch,
                                                       const int *ipiv, long long strideP, int nrhs, double *B, long long ldb, long long strideB) {
    static_assert(TS >= 64 || H == 1, "a team inside a wave holds one row per lane");
    constexpr int tthreads = TS, wpm = TS >= 64 ? TS / 64 : 1;
    const int ldl = n | 1;
    const int tid = threadIdx.x, team = tid / tthreads, tt = tid - team * tthreads;
    const long long b = (long long)blockIdx.x * (BT_T / tthreads) + team;
    const bool active = b < batch;
    double *T = (double *)(bt_smem + (size_t)team * (((size_t)ldl * n * sizeof(double) + 2 * (size_t)n * sizeof(int) + 15) & ~(size_t)15));
    int *map = (int *)(T + (size_t)ldl * n), *pv = map + n;
    if (active) {
        bt_load_matrix(LU + b * strideLU, ldlu, n, T, ldl, tt, tthreads);
        if (tt < n) {
            int p = ipiv[b * strideP + tt] - 1;
            if (p < 0 || p >= n) p = tt;                         // (never, for pivots of a factorization: keeps every access in range regardless)
            pv[tt] = p;
        }
    }
    __syncthreads();
    // The interchanges as one map.  trans = 0: they run j = 0 .. n-1 on B before the solves -- the row that starts at tt ends at cpos,
    // so position cpos loads row tt (map[cpos] = tt).  trans = 1: they run j = n-1 .. 0 on the result -- position tt stores to row cpos.
    if (active && tt < n) {
        int cpos = tt;
        if (!trans) {
            for (int j = 0; j < n; ++j) { const int p = pv[j]; cpos = cpos == j ? p : (cpos == p ? j : cpos); }
            map[cpos] = tt;
        } else {
            for (int j = n - 1; j >= 0; --j) { const int p = pv[j]; cpos = cpos == j ? p : (cpos == p ? j : cpos); }
            map[tt] = cpos;
        }
    }
    __syncthreads();
    if (!active) return;
    const int w = tt >> 6, lane = tt & 63;
    double *bb = B + b * strideB;
    for (int k = w; k < nrhs; k += wpm) {
        double *col = bb + (long long)k * ldb;
        double x[H];
#pragma unroll
        for (int h = 0; h < H; ++h) {
            const int r = lane + 64 * h;
            x[h] = r < n ? (trans ? col[r] : col[map[r]]) : 0.0;
        }
        if (!trans) {
            for (int j = 0; j < n; ++j) {                        // L: b_i -= l_ij b_j
                const double xj = bt_rhs_bcast<H, TS>(x, j);
#pragma unroll
                for (int h = 0; h < H; ++h) {
                    const int r = lane + 64 * h;
                    if (r > j && r < n) { const double t = T[r + j * ldl] * xj; x[h] = x[h] - t; }
                }
            }
            for (int j = n - 1; j >= 0; --j) {                   // U: b_j /= u_jj, then b_i -= u_ij b_j
                const double xj = bt_rhs_bcast<H, TS>(x, j) / T[j + j * ldl];
#pragma unroll
                for (int h = 0; h < H; ++h) {
                    const int r = lane + 64 * h;
                    if (r == j) x[h] = xj;
                    else if (r < j) { const double t = T[r + j * ldl] * xj; x[h] = x[h] - t; }
                }
            }
#pragma unroll
            for (int h = 0; h < H; ++h) {
                const int r = lane + 64 * h;
                if (r < n) col[r] = x[h];
            }
        } else {
            for (int j = 0; j < n; ++j) {                        // U^T: b_j /= u_jj, then b_i -= u_ji b_j
                const double xj = bt_rhs_bcast<H, TS>(x, j) / T[j + j * ldl];
#pragma unroll
                for (int h = 0; h < H; ++h) {
                    const int r = lane + 64 * h;
                    if (r == j) x[h] = xj;
                    else if (r > j && r < n) { const double t = T[j + r * ldl] * xj; x[h] = x[h] - t; }
                }
            }
            for (int j = n - 1; j >= 0; --j) {                   // L^T: b_i -= l_ji b_j
                const double xj = bt_rhs_bcast<H, TS>(x, j);
#pragma unroll
                for (int h = 0; h < H; ++h) {
                    const int r = lane + 64 * h;
                    if (r < j) { const double t = T[j + r * ldl] * xj; x[h] = x[h] - t; }
                }
            }
#pragma unroll
            for (int h = 0; h < H; ++h) {
                const int r = lane + 64 * h;
                if (r < n) col[map[r]] = x[h];
            }
        }
    }
}

// ---- launchers: one launch each, batch <= BT_MAX_LAUNCH matrices (the host splits longer batches) -----------------------------------
static int bt_attrs(mpf_ctx *c) {
    if (c->attr_done & ATTR_BATCHED) return 0;
    const void *ks[] = {(const void *)bt_getrf_wg_kernel<false, 1>, (const void *)bt_getrf_wg_kernel<true, 1>,
                        (const void *)bt_getrf_wg_kernel<false, 2>, (const void *)bt_getrf_wg_kernel<true, 2>,
                        (const void *)bt_getrs_kernel<1, 32>, (const void *)bt_getrs_kernel<1, 256>, (const void *)bt_getrs_kernel<2, 256>};
    for (const void *k : ks) MPF_HIP_TRY(c, hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    c->attr_done |= ATTR_BATCHED;
    return 0;
}

int launch_getrf_batched(mpf_ctx *c, double *A, int64_t lda, int64_t strideA, int n, int64_t batch, int *ipiv, int64_t strideP, int *info,
                         int fused) {
    if (n < 1 || batch < 1) return 0;
    if (n > BT_MAXN || batch > BT_MAX_LAUNCH) { c->err = "launch_getrf_batched: size out of range"; return -1; }
    if (n <= 32) {
#define BT_WAVE(W_)                                                                                                                  \
        do {                                                                                                                         \
            const long long per = (BT_T / W_);                                                                                       \
            const unsigned g = (unsigned)((batch + per - 1) / per);                                                                  \
            if (fused) bt_getrf_wave_kernel<W_, true><<<g, BT_T, 0, c->stream>>>(A, lda, strideA, n, batch, ipiv, strideP, info);     \
            else bt_getrf_wave_kernel<W_, false><<<g, BT_T, 0, c->stream>>>(A, lda, strideA, n, batch, ipiv, strideP, info);          \
        } while (0)
        if (n <= 8) BT_WAVE(8);
        else if (n <= 16) BT_WAVE(16);
        else BT_WAVE(32);
#undef BT_WAVE
    } else {
        { const int e = bt_attrs(c); if (e) return e; }
        const size_t lds = bt_getrf_wg_lds(n);
        if (n <= 64) {
            if (fused) bt_getrf_wg_kernel<true, 1><<<(unsigned)batch, 256, lds, c->stream>>>(A, lda, strideA, n, ipiv, strideP, info);
            else bt_getrf_wg_kernel<false, 1><<<(unsigned)batch, 256, lds, c->stream>>>(A, lda, strideA, n, ipiv, strideP, info);
        } else {
            if (fused) bt_getrf_wg_kernel<true, 2><<<(unsigned)batch, 1024, lds, c->stream>>>(A, lda, strideA, n, ipiv, strideP, info);
            else bt_getrf_wg_kernel<false, 2><<<(unsigned)batch, 1024, lds, c->stream>>>(A, lda, strideA, n, ipiv, strideP, info);
        }
    }
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

int launch_getrs_batched(mpf_ctx *c, int trans, const double *LU, int64_t ldlu, int64_t strideLU, int n, int64_t batch, const int *ipiv,
                         int64_t strideP, int nrhs, double *B, int64_t ldb, int64_t strideB) {
    if (n < 1 || batch < 1 || nrhs < 1) return 0;
    if (n > BT_MAXN || batch > BT_MAX_LAUNCH) { c->err = "launch_getrs_batched: size out of range"; return -1; }
    { const int e = bt_attrs(c); if (e) return e; }
#define BT_SOLVE(H_, TS_)                                                                                                                \
    do {                                                                                                                                 \
        const int per_wg = BT_T / TS_;                                                                                                   \
        const unsigned g = (unsigned)((batch + per_wg - 1) / per_wg);                                                                    \
        bt_getrs_kernel<H_, TS_><<<g, BT_T, bt_getrs_lds(n) * per_wg, c->stream>>>(trans, LU, ldlu, strideLU, n, batch, ipiv, strideP,   \
                                                                                    nrhs, B, ldb, strideB);                              \
    } while (0)
    if (n <= 8) BT_SOLVE(1, 8);
    else if (n <= 16) BT_SOLVE(1, 16);
    else if (n <= 32) BT_SOLVE(1, 32);
    else if (n <= 64) BT_SOLVE(1, 256);
    else BT_SOLVE(2, 256);
#undef BT_SOLVE
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}
