// The bodies of the variable-size small-matrix kernels (vbatched.hip): every matrix its own n, offset and leading dimension, taken from
// a class list.  A kernel works out where its matrix lies and calls the body; the arithmetic -- and with it every bit of the result --
// is the body's, and each body restates, statement for statement, the kernel of the same name in batched.hip (bt_getrf_wave_kernel ->
// bt_getrf_wave_body, ...), whose comments say why each form is the way it is.
//
// Why the fixed-size kernels do not call these bodies: they did, in a first form of this change (one body, a bool RG for the ragged
// guards, RG = false folding them away).  Handing the matrix over as pointers changed the fixed-size kernels' register allocation --
// bt_getrf_wave_kernel<32> went from 88 to 146 VGPRs -- and the fixed-size path must not pay for this layer, so batched.hip keeps its
// kernels untouched and the tests compare the two files' results bit for bit (tests/test_gpu_vbatched.py).
//
// Bodies of the wave forms (W lanes of a wave per matrix) take two orders: n, the order of the lane's own matrix, and nw, the number of
// column steps the WAVE runs (wave-uniform, >= n; in a scalar register).  With RG = true the matrices of a wave differ in n: the steps run
// to the largest, every lane executes every cross-lane operation (no __shfl under a per-matrix branch), and a matrix whose n is exhausted
// has no open row: its lanes compute on zeros and store nothing.  RG = false (nw = n: the workgroup forms' whole-workgroup teams)
// compiles every `RG && ...` guard away.
#pragma once
#include "mpf_internal.h"
#include <limits.h>

constexpr int BT_MAXN = 128;   // largest matrix (the workgroup form's LDS: 129 x 128 doubles)
constexpr int BT_T = 256;      // threads per workgroup, every kernel of these files but the 1024-thread workgroup forms

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
// a: the lane's matrix (any readable matrix when !valid); valid: the lane holds row r < n of a matrix; piv, infp: the matrix's pivots
// and its info word (or null), used by valid lanes only.
template <int W, bool FUSED, bool RG>
__device__ __forceinline__ void bt_getrf_wave_body(double *a, long long lda, int n, int nw, bool valid, int *piv, int *infp) {
    const int lane = threadIdx.x & 63, r = lane & (W - 1);
    double x[W];
#pragma unroll
    for (int c = 0; c < W; ++c) x[c] = (valid && c < n) ? a[r + (long long)c * lda] : 0.0;
    int cp = r, mypiv = 0, inf = 0;                             // cp: this row's current position
#pragma unroll
    for (int j = 0; j < W; ++j) {
        if (j < nw) {                                           // (uniform)
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
            const int p = pos >> 8, wl = pos & (W - 1);   // (a matrix past the batch's end, or one of n <= j, has no open row: its lanes compute on zeros)
            if (r == j) mypiv = p + 1;
            if (r == wl) cp = j;
            else if (cp == j) cp = p;                           // dgetf2's interchange: the row at position j goes where the pivot row was
            const int src = (lane & ~(W - 1)) | wl;             // the pivot row's lane
            const double uj = __shfl(x[j], src);
            if ((!RG || j < n) && uj == 0.0 && inf == 0) inf = j + 1;
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
        piv[r] = mypiv;
        if (infp && r == 0) *infp = inf;
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
static inline size_t bt_getrf_wg_lds(int n) { return (size_t)(n | 1) * n * sizeof(double) + (3 * BT_MAXN + 4) * sizeof(int); }

// H = 1: n <= 64, 256 threads (64 rows x 4 column groups; up to four workgroups per CU); H = 2: 1024 threads (128 rows x 8 column
// groups: the one workgroup the LDS leaves room for brings 16 waves).  A column step has two phases and two barriers:
//   A  wave 0 alone, H rows per lane, the rows' positions in its registers: the pivot search on column j, the pivot through
//      v_readlane, the multipliers (one division per row, stored in place);
//   B  every thread: the rank-1 update of the columns right of j, a thread one row and every ncg-th column.
// Nothing is computed twice; while wave 0 is in phase A the other waves wait at the barrier and leave the CU to other workgroups.
// a: the workgroup's matrix, n its order (uniform); pivout, infp: its pivots and its info word (or null).
template <bool FUSED, int H>
__device__ __forceinline__ void bt_getrf_wg_body(double *a, long long lda, int n, int *pivout, int *infp) {
    constexpr int NT = H == 1 ? 256 : 1024, rg = 64 * H, ncg = NT / rg;
    const int ldl = n | 1;
    double *T = (double *)bt_smem;
    int *rowpos = (int *)(T + (size_t)ldl * n), *inv = rowpos + BT_MAXN, *piv = inv + BT_MAXN, *ctl = piv + BT_MAXN;
    const int tid = threadIdx.x, lane = tid & 63;
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
    if (tid < n) pivout[tid] = piv[tid];
    if (infp && tid == 0) *infp = inf;
}

// ---- solve ----------------------------------------------------------------------------------------------------------------------------
// LDS per matrix: T[ldl x n] doubles, map[n], pv[n] ints, rounded up to 16 bytes
static inline size_t bt_getrs_lds(int n) { return ((size_t)(n | 1) * n * sizeof(double) + 2 * (size_t)n * sizeof(int) + 15) & ~(size_t)15; }

// b_j of the team's column, in every lane of the team: through scalar registers for a team of whole waves, by ds_bpermute inside a wave
template <int H, int TS>
__device__ __forceinline__ double bt_rhs_bcast(const double (&x)[H], int j) {
    if (TS >= 64) return bt_bcast<H>(x, j);
    return __shfl(x[0], (int)((threadIdx.x & 63 & ~(TS - 1)) | j));
}

// A team of TS threads per matrix, 256 / TS matrices per workgroup, each with its own LDS region: TS = 8, 16, 32 (n <= TS: lane = row,
// the columns of B one after the other) or 256 (four waves, H rows per lane; a wave takes every fourth column of B).
// lu, piv, bb: the team's factors, pivots and right-hand sides (read only when active); T: the team's LDS region; tt: the thread's index
// in the team.  nw: the steps of the chains (TS < 64 with RG: the largest n among the wave's teams; else n).
template <int H, int TS, bool RG>
__device__ __forceinline__ void bt_getrs_body(int trans, const double *lu, long long ldlu, int n, int nw, bool active, const int *piv, int nrhs,
                                              double *bb, long long ldb, double *T, int tt) {
    static_assert(TS >= 64 || H == 1, "a team inside a wave holds one row per lane");
    constexpr int tthreads = TS, wpm = TS >= 64 ? TS / 64 : 1;
    const int ldl = n | 1;
    int *map = (int *)(T + (size_t)ldl * n), *pv = map + n;
    if (active) {
        bt_load_matrix(lu, ldlu, n, T, ldl, tt, tthreads);
        if (tt < n) {
            int p = piv[tt] - 1;
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
    for (int k = w; k < nrhs; k += wpm) {
        double *col = bb + (long long)k * ldb;
        double x[H];
#pragma unroll
        for (int h = 0; h < H; ++h) {
            const int r = lane + 64 * h;
            x[h] = r < n ? (trans ? col[r] : col[map[r]]) : 0.0;
        }
        if (!trans) {
            for (int j = 0; j < nw; ++j) {                       // L: b_i -= l_ij b_j
                const double xj = bt_rhs_bcast<H, TS>(x, j);
#pragma unroll
                for (int h = 0; h < H; ++h) {
                    const int r = lane + 64 * h;
                    if (r > j && r < n) { const double t = T[r + j * ldl] * xj; x[h] = x[h] - t; }
                }
            }
            for (int j = nw - 1; j >= 0; --j) {                  // U: b_j /= u_jj, then b_i -= u_ij b_j
                const bool mine = !RG || j < n;                  // (a step past the team's n: nothing of the team changes)
                const double xj = bt_rhs_bcast<H, TS>(x, j) / (mine ? T[j + j * ldl] : 1.0);
#pragma unroll
                for (int h = 0; h < H; ++h) {
                    const int r = lane + 64 * h;
                    if (r == j) x[h] = xj;
                    else if (r < j && mine) { const double t = T[r + j * ldl] * xj; x[h] = x[h] - t; }
                }
            }
#pragma unroll
            for (int h = 0; h < H; ++h) {
                const int r = lane + 64 * h;
                if (r < n) col[r] = x[h];
            }
        } else {
            for (int j = 0; j < nw; ++j) {                       // U^T: b_j /= u_jj, then b_i -= u_ji b_j
                const bool mine = !RG || j < n;
                const double xj = bt_rhs_bcast<H, TS>(x, j) / (mine ? T[j + j * ldl] : 1.0);
#pragma unroll
                for (int h = 0; h < H; ++h) {
                    const int r = lane + 64 * h;
                    if (r == j) x[h] = xj;
                    else if (r > j && r < n) { const double t = T[j + r * ldl] * xj; x[h] = x[h] - t; }
                }
            }
            for (int j = nw - 1; j >= 0; --j) {                  // L^T: b_i -= l_ji b_j
                const bool mine = !RG || j < n;
                const double xj = bt_rhs_bcast<H, TS>(x, j);
#pragma unroll
                for (int h = 0; h < H; ++h) {
                    const int r = lane + 64 * h;
                    if (r < j && mine) { const double t = T[j + r * ldl] * xj; x[h] = x[h] - t; }
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

// ---- inverse from the factors -----------------------------------------------------------------------------------------------------
// a, piv: the lane's factors and pivots; o: the matrix's inverse; infp: its info word or null (valid lanes only)
template <int W, bool RG>
__device__ __forceinline__ void bt_getri_wave_body(const double *a, long long ldlu, int n, int nw, bool valid, const int *piv, double *o,
                                                   long long ldinv, int *infp) {
    const int lane = threadIdx.x & 63, r = lane & (W - 1), base = lane & ~(W - 1);
    double lu[W], x[W];
#pragma unroll
    for (int c = 0; c < W; ++c) lu[c] = (valid && c < n) ? a[r + (long long)c * ldlu] : 0.0;   // row r of LU
    int p = r;
    if (valid) {
        p = piv[r] - 1;
        if (p < 0 || p >= n) p = r;                             // (never, for pivots of a factorization: as bt_getrs_kernel)
    }
    int q = r;                                                  // where row r stands after the interchanges: column r of X starts as e_q
    double d = 1.0;                                             // u_rr
#pragma unroll
    for (int j = 0; j < W; ++j) {
        if (j < nw) {                                           // (uniform; a lane past its matrix's n holds p = its own row: no interchange)
            const int pj = __shfl(p, base | j);
            q = q == j ? pj : (q == pj ? j : q);
        }
        if (j == r) d = lu[j];
    }
    int z = (valid && d == 0.0) ? r + 1 : INT_MAX;              // the first zero on U's diagonal, in every lane of the matrix
#pragma unroll
    for (int o2 = W / 2; o2 > 0; o2 >>= 1) { const int z1 = __shfl_xor(z, o2); z = z1 < z ? z1 : z; }
#pragma unroll
    for (int i = 0; i < W; ++i) x[i] = i == q ? 1.0 : 0.0;
    // from here on the lane is column r of X; lane base | i still holds row i of LU
#pragma unroll
    for (int j = 0; j < W; ++j) {                               // L: x_i -= l_ij x_j
        if (j + 1 < nw) {
#pragma unroll
            for (int i = j + 1; i < W; ++i) {
                if (i < nw) {
                    const double l = __shfl(lu[j], base | i);   // (a row past the matrix's n: l = 0; what x[i] becomes there is never
                    const double t = l * x[j];                  //  stored and never read as an x_j: the backward sweep reads 0 instead)
                    x[i] = x[i] - t;
                }
            }
        }
    }
#pragma unroll
    for (int j = W - 1; j >= 0; --j) {                          // U: x_j /= u_jj, then x_i -= u_ij x_j
        if (j < nw) {
            // A step past the matrix's n would divide by the zeros its spare lanes hold.  One select per step keeps it out: there x_j
            // reads as +0, and the u_ij of such a column are +0 in every row (loaded so), so every update subtracts 0 * 0 = +0:
            // x - (+0) = x for every x, -0 included.
            const bool mine = !RG || j < n;
            const double ujj = __shfl(lu[j], base | j);
            if (mine) x[j] = x[j] / ujj;
            const double xj = mine ? x[j] : 0.0;
#pragma unroll
            for (int i = 0; i < j; ++i) {
                const double u = __shfl(lu[j], base | i);
                const double t = u * xj;
                x[i] = x[i] - t;
            }
        }
    }
    if (!valid) return;
    if (z == INT_MAX) {
        double *oc = o + (long long)r * ldinv;
#pragma unroll
        for (int i = 0; i < W; ++i)
            if (i < n) oc[i] = x[i];
    }
    if (infp && r == 0) *infp = z == INT_MAX ? 0 : z;
}

// LDS: T[ldl x n] doubles, then qpos[BT_MAXN] (where each row stands after the interchanges), pv[BT_MAXN], ctl[4] (the first zero of
// U's diagonal)
static inline size_t bt_getri_wg_lds(int n) { return (size_t)(n | 1) * n * sizeof(double) + (2 * BT_MAXN + 4) * sizeof(int); }

// lu, piv: the workgroup's factors and pivots; o: its inverse; infp: its info word or null
template <int H>
__device__ __forceinline__ void bt_getri_wg_body(const double *lu, long long ldlu, int n, const int *piv, double *o, long long ldinv, int *infp) {
    constexpr int NT = H == 1 ? 256 : 1024, NW = NT / 64, CB = 4;
    const int ldl = n | 1;
    double *T = (double *)bt_smem;
    int *qpos = (int *)(T + (size_t)ldl * n), *pv = qpos + BT_MAXN, *ctl = pv + BT_MAXN;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    bt_load_matrix(lu, ldlu, n, T, ldl, tid, NT);
    if (tid < n) {
        int p = piv[tid] - 1;
        if (p < 0 || p >= n) p = tid;                            // (as bt_getrs_kernel: keeps every access in range)
        pv[tid] = p;
    }
    if (tid == 0) ctl[0] = INT_MAX;
    __syncthreads();
    if (tid < n) {
        int cpos = tid;
        for (int j = 0; j < n; ++j) { const int p = pv[j]; cpos = cpos == j ? p : (cpos == p ? j : cpos); }
        qpos[tid] = cpos;
        if (T[tid + tid * ldl] == 0.0) atomicMin(&ctl[0], tid + 1);
    }
    __syncthreads();
    const int z = ctl[0];
    if (infp && tid == 0) *infp = z == INT_MAX ? 0 : z;
    if (z != INT_MAX) return;                                    // (the whole workgroup: nothing is stored)
    for (int kb = w * CB; kb < n; kb += NW * CB) {               // columns kb .. kb + 3 of X (those past n: all zero, not stored)
        double x[CB][H], xj[CB];
        int q0 = n;
#pragma unroll
        for (int c = 0; c < CB; ++c) {
            const int qc = kb + c < n ? qpos[kb + c] : n;
            q0 = qc < q0 ? qc : q0;
#pragma unroll
            for (int h = 0; h < H; ++h) x[c][h] = lane + 64 * h == qc ? 1.0 : 0.0;
        }
        q0 = __builtin_amdgcn_readfirstlane(q0);                 // (the same in every lane: keeps the step counter scalar)
        for (int j = q0; j < n - 1; ++j) {                       // L: x_i -= l_ij x_j; the steps before q0 meet zeros only
#pragma unroll
            for (int c = 0; c < CB; ++c) xj[c] = bt_bcast<H>(x[c], j);
#pragma unroll
            for (int h = 0; h < H; ++h) {
                if (64 * h + 63 > j) {                           // (uniform)
                    const int r = lane + 64 * h;
                    const bool low = r > j && r < n;
                    const double l = low ? T[r + j * ldl] : 0.0;
#pragma unroll
                    for (int c = 0; c < CB; ++c) {               // (selects, not branches: the other lanes' differences are dropped)
                        const double t = l * xj[c];
                        const double v = x[c][h] - t;
                        x[c][h] = low ? v : x[c][h];
                    }
                }
            }
        }
        for (int j = n - 1; j >= 0; --j) {                       // U: x_j /= u_jj, then x_i -= u_ij x_j
            double dv = 1.0;
#pragma unroll
            for (int c = 0; c < CB; ++c) { const double v = bt_bcast<H>(x[c], j); if (lane == c) dv = v; }
            dv = dv / T[j + j * ldl];                            // the four divisions of the step, in lanes 0 .. 3
#pragma unroll
            for (int c = 0; c < CB; ++c) xj[c] = bt_readlane(dv, c);
#pragma unroll
            for (int h = 0; h < H; ++h) {
                if (64 * h <= j) {                               // (uniform)
                    const int r = lane + 64 * h;
                    const bool up = r < j;
                    const double u = up ? T[r + j * ldl] : 0.0;
#pragma unroll
                    for (int c = 0; c < CB; ++c) {
                        const double t = u * xj[c];
                        const double v = x[c][h] - t;
                        x[c][h] = r == j ? xj[c] : (up ? v : x[c][h]);
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < CB; ++c) {
            if (kb + c < n) {
                double *col = o + (long long)(kb + c) * ldinv;
#pragma unroll
                for (int h = 0; h < H; ++h) {
                    const int r = lane + 64 * h;
                    if (r < n) col[r] = x[c][h];
                }
            }
        }
    }
}

// ---- determinant from the factors -------------------------------------------------------------------------------------------------
// mpf_getdet's order on one chunk (n <= 128 < 256): (m_i, e_i) = frexp(u_ii); from p = 1, e = 0: p = p m_i, (p, k) = frexp(p),
// e += k + e_i, i ascending; the one combining step from (1, 0); the sign flips once per ipiv[i] != i + 1.  The chain is serial by
// contract.  TS = 1: a thread per matrix (n <= 32); TS = 64: a wave per matrix, the diagonal and the pivots loaded by lane = row, the
// pivot count and the special cases by ballot, the chain on v_readlane values (every lane runs it; lane 0 stores).
// a, pv: the matrix's factors and pivots (TS = 64: the wave's); mant, expo: where its result goes
template <int TS>
__device__ __forceinline__ void bt_getdet_body(const double *a, long long ldlu, int n, const int *pv, double *mant, int *expo) {
    double p = 1.0;
    int e = 0, flips = 0;
    bool zero = false, bad = false;
    if (TS == 1) {
        for (int i = 0; i < n; ++i) {
            const double u = a[i + (long long)i * ldlu];
            zero |= u == 0.0;
            bad |= !(fabs(u) <= 1.7976931348623157e308);
            flips ^= pv[i] != i + 1 ? 1 : 0;
            int ei;
            const double m = frexp(u, &ei);
            mpf_det_step(p, e, m, ei);
        }
    } else {
        const int lane = threadIdx.x & 63;
        double m[2];
        int ex[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int r = lane + 64 * h;
            const double u = r < n ? a[r + (long long)r * ldlu] : 1.0;
            const bool f = r < n && pv[r] != r + 1;
            zero |= __any(u == 0.0) != 0;
            bad |= __any(!(fabs(u) <= 1.7976931348623157e308)) != 0;
            flips += __popcll(__ballot(f));
            m[h] = frexp(u, &ex[h]);
        }
        for (int i = 0; i < n; ++i) {
            const double mi = bt_bcast<2>(m, i);
            const int ei = i < 64 ? __builtin_amdgcn_readlane(ex[0], i) : __builtin_amdgcn_readlane(ex[1], i - 64);
            mpf_det_step(p, e, mi, ei);
        }
        if (lane != 0) return;
    }
    int k;
    double P = frexp(1.0 * p, &k);                               // the combining step of the one chunk
    int E = k + e;
    if (flips & 1) P = -P;
    if (bad) { P = __builtin_nan(""); E = 0; }
    else if (zero) { P = 0.0; E = 0; }
    *mant = P;
    *expo = E;
}
