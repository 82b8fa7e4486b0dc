// LU of many small matrices (mpf_getrf_batched, mpf_getrs_batched, and from their factors mpf_getri_batched, mpf_getdet_batched;
// contracts in include/mpf_c.h, host side in mpf_batched.cpp).
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

// ---- inverse from the factors -----------------------------------------------------------------------------------------------------
// inv[b] = what bt_getrs_kernel(trans = 0) leaves for B[b] = I, without the identity.  Column k of X starts as e_q, q = the position row
// k reaches under the interchanges j = 0 .. n-1; then x_i -= l_ij x_j (j ascending); then, j descending, x_j /= u_jj and x_i -= u_ij x_j
// for i < j.  Per element that is the solve's chain, so the bits are the solve's.
// Structural zeros: before step q of the forward sweep column k holds +0 above and below its one, so the steps j < q subtract
// l_ij * (+0) = +-0 from +0 (finite l_ij), and +0 - (+-0) = +0: skipping them changes no bit, the signs of zeros included.  The wave
// form does not skip (a lane's column starts where it starts; the step is the wave's), the workgroup form starts a group of four
// columns at the smallest q among them.  Nothing is skipped in the backward sweep.
//   bt_getri_wave_kernel<W>     n <= W = 8, 16, 32: 64 / W matrices per wave64; lane = (matrix, row) for the load of LU -- the row's W
//                               columns in registers -- and lane = (matrix, COLUMN of X) for the sweeps: the column's W rows in registers,
//                               l_ij / u_ij broadcast from the row's lane by ds_bpermute (W^2 broadcasts per matrix for both sweeps),
//                               x_j is the lane's own register, and the division x_j / u_jj is one instruction sequence per step for all
//                               W columns.  (With lane = row for X, as the factorization has it, a step broadcasts row j of X -- 2 W^2
//                               broadcasts -- and every lane repeats the W divisions of the step for the one lane that holds row j: W^2
//                               division sequences per wave against W here; not built for that reason.)  No LDS memory, no barrier.
//   bt_getri_wg_kernel<H>       32 < n <= 128: one workgroup per matrix, LU once into LDS (odd leading dimension), X never: a wave owns
//                               four columns of X at a time, lane = row, H rows per lane; x_j by v_readlane.  The four x_j of a backward
//                               step are gathered into lanes 0 .. 3, divided by u_jj in ONE division sequence and read back by v_readlane
//                               (every lane of the wave repeating the division per column was the larger half of a backward step's
//                               instructions); one LDS read of l_ij / u_ij serves the four columns.  256 threads for n <= 64, 1024 above
//                               (the LDS leaves room for one workgroup per CU there).  No barrier after the pivots are composed.
//                               The updates are selects, not branches: written as `if (r == j) .. else if (r < j) ..` per column the
//                               compiler built a nest of exec-mask branches with a copy of all eight registers on each side --
//                               3.89 ms for 16384 matrices of order 64 and 5.69 ms for 4096 of order 128 against 3.43 and 5.45 ms now.
// Measured on one MI355X, 512 MB of factors per size (tools/batched_inv_probe.py; "before" = an identity batch filled on the device and
// bt_getrs_kernel with nrhs = n, the only route before these kernels): n = 8: 0.445 ms against 1.110 ms; 16: 0.665 / 1.811; 32: 0.800 /
// 4.591; 64: 3.425 / 4.879; 128: 5.452 / 24.385.  Not tried: X in LDS with LU streamed from L2 and a rank-1 update per step; staging
// the wave form's stores through LDS (a lane stores a column: 8-byte stores ldinv apart, where the load of LU is coalesced).
// A zero on U's diagonal: found by the matrix's lanes before any store; the whole team then skips the stores.
template <int W>
__global__ __launch_bounds__(BT_T) void bt_getri_wave_kernel(const double *LU, long long ldlu, long long strideLU, int n, long long batch,
                                                            const int *ipiv, long long strideP, double *inv, long long ldinv,
                                                            long long strideInv, int *info) {
    constexpr int G = 64 / W;
    const int lane = threadIdx.x & 63, r = lane & (W - 1), g = lane / W, base = lane & ~(W - 1);
    const long long b0 = ((long long)blockIdx.x * (BT_T / 64) + (threadIdx.x >> 6)) * G, b = b0 + g;
    if (b0 >= batch) return;                                    // (the whole wave)
    const bool valid = b < batch && r < n;
    const double *a = LU + (valid ? b : b0) * strideLU;
    double lu[W], x[W];
#pragma unroll
    for (int c = 0; c < W; ++c) lu[c] = (valid && c < n) ? a[r + (long long)c * ldlu] : 0.0;   // row r of LU
    int p = r;
    if (valid) {
        p = ipiv[b * strideP + r] - 1;
        if (p < 0 || p >= n) p = r;                             // (never, for pivots of a factorization: as bt_getrs_kernel)
    }
    int q = r;                                                  // where row r stands after the interchanges: column r of X starts as e_q
    double d = 1.0;                                             // u_rr
#pragma unroll
    for (int j = 0; j < W; ++j) {
        if (j < n) {                                            // (uniform)
            const int pj = __shfl(p, base | j);
            q = q == j ? pj : (q == pj ? j : q);
        }
        if (j == r) d = lu[j];
    }
    int z = (valid && d == 0.0) ? r + 1 : INT_MAX;              // the first zero on U's diagonal, in every lane of the matrix
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) { const int z1 = __shfl_xor(z, o); z = z1 < z ? z1 : z; }
#pragma unroll
    for (int i = 0; i < W; ++i) x[i] = i == q ? 1.0 : 0.0;
    // from here on the lane is column r of X; lane base | i still holds row i of LU
#pragma unroll
    for (int j = 0; j < W; ++j) {                               // L: x_i -= l_ij x_j
        if (j + 1 < n) {
#pragma unroll
            for (int i = j + 1; i < W; ++i) {
                if (i < n) {
                    const double l = __shfl(lu[j], base | i);
                    const double t = l * x[j];
                    x[i] = x[i] - t;
                }
            }
        }
    }
#pragma unroll
    for (int j = W - 1; j >= 0; --j) {                          // U: x_j /= u_jj, then x_i -= u_ij x_j
        if (j < n) {
            const double ujj = __shfl(lu[j], base | j);
            x[j] = x[j] / ujj;
#pragma unroll
            for (int i = 0; i < j; ++i) {
                const double u = __shfl(lu[j], base | i);
                const double t = u * x[j];
                x[i] = x[i] - t;
            }
        }
    }
    if (!valid) return;
    if (z == INT_MAX) {
        double *o = inv + b * strideInv + (long long)r * ldinv;
#pragma unroll
        for (int i = 0; i < W; ++i)
            if (i < n) o[i] = x[i];
    }
    if (info && r == 0) info[b] = z == INT_MAX ? 0 : z;
}

// LDS: T[ldl x n] doubles, then qpos[BT_MAXN] (where each row stands after the interchanges), pv[BT_MAXN], ctl[4] (the first zero of
// U's diagonal)
static size_t bt_getri_wg_lds(int n) { return (size_t)(n | 1) * n * sizeof(double) + (2 * BT_MAXN + 4) * sizeof(int); }

template <int H>
__global__ __launch_bounds__(H == 1 ? 256 : 1024) void bt_getri_wg_kernel(const double *LU, long long ldlu, long long strideLU, int n,
                                                                         const int *ipiv, long long strideP, double *inv, long long ldinv,
                                                                         long long strideInv, int *info) {
    constexpr int NT = H == 1 ? 256 : 1024, NW = NT / 64, CB = 4;
    const int ldl = n | 1;
    double *T = (double *)bt_smem;
    int *qpos = (int *)(T + (size_t)ldl * n), *pv = qpos + BT_MAXN, *ctl = pv + BT_MAXN;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long long b = blockIdx.x;
    bt_load_matrix(LU + b * strideLU, ldlu, n, T, ldl, tid, NT);
    if (tid < n) {
        int p = ipiv[b * strideP + tid] - 1;
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
    if (info && tid == 0) info[b] = z == INT_MAX ? 0 : z;
    if (z != INT_MAX) return;                                    // (the whole workgroup: nothing is stored)
    double *o = inv + b * strideInv;
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
template <int TS>
__global__ __launch_bounds__(BT_T) void bt_getdet_kernel(const double *LU, long long ldlu, long long strideLU, int n, long long batch,
                                                        const int *ipiv, long long strideP, double *mant, int *expo) {
    double p = 1.0;
    int e = 0, flips = 0;
    bool zero = false, bad = false;
    long long b;
    if (TS == 1) {
        b = (long long)blockIdx.x * BT_T + threadIdx.x;
        if (b >= batch) return;
        const double *a = LU + b * strideLU;
        const int *pv = ipiv + b * strideP;
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
        b = (long long)blockIdx.x * (BT_T / 64) + (threadIdx.x >> 6);
        if (b >= batch) return;                                  // (the whole wave)
        const double *a = LU + b * strideLU;
        const int *pv = ipiv + b * strideP;
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
    mant[b] = P;
    expo[b] = E;
}

// ---- launchers: one launch each, batch <= BT_MAX_LAUNCH matrices (the host splits longer batches) -----------------------------------
static int bt_attrs(mpf_ctx *c) {
    if (c->attr_done & ATTR_BATCHED) return 0;
    const void *ks[] = {(const void *)bt_getrf_wg_kernel<false, 1>, (const void *)bt_getrf_wg_kernel<true, 1>,
                        (const void *)bt_getrf_wg_kernel<false, 2>, (const void *)bt_getrf_wg_kernel<true, 2>,
                        (const void *)bt_getri_wg_kernel<1>, (const void *)bt_getri_wg_kernel<2>,
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

int launch_getri_batched(mpf_ctx *c, const double *LU, int64_t ldlu, int64_t strideLU, int n, int64_t batch, const int *ipiv, int64_t strideP,
                         double *inv, int64_t ldinv, int64_t strideInv, int *info) {
    if (n < 1 || batch < 1) return 0;
    if (n > BT_MAXN || batch > BT_MAX_LAUNCH) { c->err = "launch_getri_batched: size out of range"; return -1; }
    if (n <= 32) {
#define BT_INV(W_)                                                                                                                   \
        do {                                                                                                                         \
            const long long per = (BT_T / W_);                                                                                       \
            const unsigned g = (unsigned)((batch + per - 1) / per);                                                                  \
            bt_getri_wave_kernel<W_><<<g, BT_T, 0, c->stream>>>(LU, ldlu, strideLU, n, batch, ipiv, strideP, inv, ldinv, strideInv, info); \
        } while (0)
        if (n <= 8) BT_INV(8);
        else if (n <= 16) BT_INV(16);
        else BT_INV(32);
#undef BT_INV
    } else {
        { const int e = bt_attrs(c); if (e) return e; }
        const size_t lds = bt_getri_wg_lds(n);
        if (n <= 64) bt_getri_wg_kernel<1><<<(unsigned)batch, 256, lds, c->stream>>>(LU, ldlu, strideLU, n, ipiv, strideP, inv, ldinv, strideInv, info);
        else bt_getri_wg_kernel<2><<<(unsigned)batch, 1024, lds, c->stream>>>(LU, ldlu, strideLU, n, ipiv, strideP, inv, ldinv, strideInv, info);
    }
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

int launch_getdet_batched(mpf_ctx *c, const double *LU, int64_t ldlu, int64_t strideLU, int n, int64_t batch, const int *ipiv, int64_t strideP,
                          double *mant, int *expo) {
    if (n < 1 || batch < 1) return 0;
    if (n > BT_MAXN || batch > BT_MAX_LAUNCH) { c->err = "launch_getdet_batched: size out of range"; return -1; }
    if (n <= 32) {
        const unsigned g = (unsigned)((batch + BT_T - 1) / BT_T);
        bt_getdet_kernel<1><<<g, BT_T, 0, c->stream>>>(LU, ldlu, strideLU, n, batch, ipiv, strideP, mant, expo);
    } else {
        const unsigned g = (unsigned)((batch + BT_T / 64 - 1) / (BT_T / 64));
        bt_getdet_kernel<64><<<g, BT_T, 0, c->stream>>>(LU, ldlu, strideLU, n, batch, ipiv, strideP, mant, expo);
    }
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}
