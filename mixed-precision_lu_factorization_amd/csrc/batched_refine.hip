// The expert layer for strided batches of one order n <= 128 (mpf_lange_batched, mpf_gecon_batched, mpf_residual_batched,
// mpf_gerfs_batched; contracts in include/mpf_c.h, host side in mpf_batched.cpp, numpy restatement in tests/batched_refine_model.py).
//
// Nothing here is an estimate: || (L U)^-1 || and dgerfs's || |op(A)^-1| g ||_inf are formed EXACTLY, from the columns or rows of the
// inverse that the solve's chains leave in registers; they are reduced on the fly and never stored.  (dlacn2 would take 4 to 11
// single-vector solves per matrix or right-hand side; at these sizes one such solve is bound by the latency of a wave's 2 n-step chain
// and costs about what all n columns cost when they run side by side.)  The shared rules:
//   tree sum   every sum over a row or column index is the halving tree on the terms padded to 128 with +0: v[i] + v[i + 64], then
//              + 32, .. + 1.  The terms are never negative, so adding +0 is exact and the levels above the team's width drop out:
//              lane = index, one add for the second row of a lane, then an xor butterfly inside the team.
//   maxima     order-free, but a NaN among the terms gives NaN (v_max_f64 alone would drop it): br_nanmax.
//   fusion     every multiply-subtract and multiply-add is unfused (the file is compiled with -ffp-contract=off).
// The helpers of batched.hip are copied here (that file and its kernels stay as they are); the chains are bt_getrs_kernel's.
//   br_lange_kernel<H, TS>      the matrix once into LDS (odd leading dimension: row walks and column walks are conflict-free), then
//                               one index per step: lane = the other index, tree or maximum, running maximum.
//   br_gecon_wave_kernel<W, TR> n <= W = 8, 16, 32: bt_getri_wave_kernel without interchanges; lane = (matrix, column of X) for
//                               TR = 0 ('1': the trans = 0 chains from e_k) or (matrix, row of X) for TR = 1 ('I': the trans = 1
//                               chains from e_i); the tree runs over the lane's own registers, the maximum over the matrix's lanes.
//   br_gecon_wg_kernel<H, TR>   32 < n <= 128: bt_getri_wg_kernel without interchanges, four chains per wave at a time; seven
//                               butterfly steps per chain replace the stores.  The forward steps before a chain's one are skipped
//                               (they meet zeros only; for TR = 1 that leaves +0 where 0 / u_jj may be -0: the sign of a zero changes
//                               no other value and is dropped by | |).
//   br_residual_kernel<H, TS>   a team per (matrix, column): lane = row, A streamed from global memory (trans = 1: lane i walks down
//                               column i), x_j by v_readlane or ds_bpermute.  No LDS.
//   br_gerfs_kernel<H, TS>      bt_getrs_kernel's teams: the factors once into LDS; a wave (or the team) per column for the
//                               refinement loop, x, b, r and w in registers; then, when ferr is asked for, g per column into LDS,
//                               a barrier, the n rows of op(A)^-1 shared among the waves (each chain serves every column of the
//                               chunk: lane c keeps column c's running maximum) and one more barrier to combine the waves.  Columns
//                               go in chunks of BR_GC = 8; the chunk changes no bit.  Four waves for n <= 64, sixteen above (the LDS
//                               leaves room for one workgroup per CU there, as in bt_getri_wg_kernel).
#include "mpf_internal.h"
#include <float.h>
#include <limits.h>

constexpr int BR_MAXN = 128;
constexpr int BR_T = 256;      // threads per workgroup (the workgroup form of gecon above n = 64: 1024)
constexpr int BR_GC = 8;       // columns of B per chunk of br_gerfs_kernel (<= the smallest team)

extern __shared__ __attribute__((aligned(16))) char br_smem[];

__device__ __forceinline__ double br_nanmax(double a, double b) { return (b > a || b != b) ? b : a; }   // a NaN on either side stays
__device__ __forceinline__ double br_readlane(double v, int lane) {
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)b, lane), hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), lane);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
template <int H>
__device__ __forceinline__ double br_bcast(const double (&x)[H], int j) {   // x of row j (j uniform; rows lane + 64 h), in every lane
    if (H == 1) return br_readlane(x[0], j);
    return j < 64 ? br_readlane(x[0], j) : br_readlane(x[H - 1], j - 64);
}
// x_j of the team's vector, in every lane of the team
template <int H, int TS>
__device__ __forceinline__ double br_rhs_bcast(const double (&x)[H], int j) {
    if (TS >= 64) return br_bcast<H>(x, j);
    return __shfl(x[0], (int)((threadIdx.x & 63 & ~(TS - 1)) | j));
}
// the tree's levels below the team's width, and the maximum, over the lanes of a team (of a wave for TS >= 64); in every lane
template <int TS>
__device__ __forceinline__ double br_team_sum(double s) {
#pragma unroll
    for (int o = (TS >= 64 ? 64 : TS) / 2; o > 0; o >>= 1) s = s + __shfl_xor(s, o);
    return s;
}
template <int TS>
__device__ __forceinline__ double br_team_max(double m) {
#pragma unroll
    for (int o = (TS >= 64 ? 64 : TS) / 2; o > 0; o >>= 1) m = br_nanmax(m, __shfl_xor(m, o));
    return m;
}
// LDS written by one lane of a wave and read by another
__device__ __forceinline__ void br_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// T[r + c * ldl] = a[r + c * lda] (bt_load_matrix)
__device__ __forceinline__ void br_load_matrix(const double *a, long long lda, int n, double *T, int ldl, int t, int nt) {
    const int half = (n + 1) >> 1;
    const bool vec = (((unsigned long long)a & 15ull) == 0ull) && ((lda & 1) == 0);
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
// rcond from the two norms: 0 for anorm == 0 and for a norm of the inverse that is not finite (or 0: every 1 / u_ii underflowed or met Inf)
__device__ __forceinline__ double br_rcond(double ainvnm, double anorm) {
    if (anorm == 0.0 || ainvnm == 0.0 || !(fabs(ainvnm) <= DBL_MAX)) return 0.0;
    return (1.0 / ainvnm) / anorm;
}

// ---- norms ----------------------------------------------------------------------------------------------------------------------------
static size_t br_lange_lds(int n) { return ((size_t)(n | 1) * n * sizeof(double) + 4 * sizeof(double) + 15) & ~(size_t)15; }

// mode 0: max_j tree_i |a_ij|; 1: max_i tree_j |a_ij|; 2: max |a_ij|.  A team of TS threads per matrix as bt_getrs_kernel has it.
template <int H, int TS>
__global__ __launch_bounds__(BR_T) void br_lange_kernel(int mode, const double *A, long long lda, long long strideA, int n, long long batch,
                                                       double *out) {
    static_assert(TS >= 64 || H == 1, "a team inside a wave holds one row per lane");
    constexpr int NWV = TS >= 64 ? TS / 64 : 1;
    const int ldl = n | 1;
    const int tid = threadIdx.x, team = tid / TS, tt = tid - team * TS;
    const long long b = (long long)blockIdx.x * (BR_T / TS) + team;
    const bool active = b < batch;
    double *T = (double *)(br_smem + (size_t)team * (((size_t)ldl * n * sizeof(double) + 4 * sizeof(double) + 15) & ~(size_t)15));
    double *WM = T + (size_t)ldl * n;
    if (active) br_load_matrix(A + b * strideA, lda, n, T, ldl, tt, TS);
    __syncthreads();
    if (!active) return;
    const int w = tt >> 6, lane = tt & 63;
    double m = 0.0;
    for (int k = w; k < n; k += NWV) {
        double v[H];
#pragma unroll
        for (int h = 0; h < H; ++h) {
            const int r = lane + 64 * h;
            v[h] = r < n ? fabs(mode == 1 ? T[k + r * ldl] : T[r + k * ldl]) : 0.0;
        }
        double s;
        if (mode == 2) s = br_team_max<TS>(H == 1 ? v[0] : br_nanmax(v[0], v[H - 1]));
        else s = br_team_sum<TS>(H == 1 ? v[0] : v[0] + v[H - 1]);
        m = br_nanmax(m, s);
    }
    if (TS >= 64) {
        if (lane == 0) WM[w] = m;
        __syncthreads();
        if (tt == 0) {
            for (int i = 1; i < NWV; ++i) m = br_nanmax(m, WM[i]);
            out[b] = m;
        }
    } else if (tt == 0) out[b] = m;
}

// ---- reciprocal condition number, wave form ---------------------------------------------------------------------------------------
// bt_getri_wave_kernel with q = r (no interchanges).  TR = 0: the lane's registers are column r of (L U)^-1 (L forward, U backward);
// TR = 1: row r of it, as the trans = 1 chains leave it for e_r (U^T forward, L^T backward) -- the coefficient of step (i, j) is then
// lu_ji: register i of the lane that holds row j.
template <int W, bool TR>
__global__ __launch_bounds__(BR_T) void br_gecon_wave_kernel(const double *LU, long long ldlu, long long strideLU, int n, long long batch,
                                                            const double *anorm, double *rcond, double *ainvnm) {
    constexpr int G = 64 / W;
    const int lane = threadIdx.x & 63, r = lane & (W - 1), g = lane / W, base = lane & ~(W - 1);
    const long long b0 = ((long long)blockIdx.x * (BR_T / 64) + (threadIdx.x >> 6)) * G, b = b0 + g;
    if (b0 >= batch) return;                                    // (the whole wave)
    const bool valid = b < batch && r < n;
    const double *a = LU + (valid ? b : b0) * strideLU;
    double lu[W], x[W];
#pragma unroll
    for (int c = 0; c < W; ++c) lu[c] = (valid && c < n) ? a[r + (long long)c * ldlu] : 0.0;   // row r of LU
    double d = 1.0;
#pragma unroll
    for (int j = 0; j < W; ++j)
        if (j == r) d = lu[j];
    int z = (valid && d == 0.0) ? 1 : 0;                        // a zero on U's diagonal, in every lane of the matrix
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) z |= __shfl_xor(z, o);
#pragma unroll
    for (int i = 0; i < W; ++i) x[i] = i == r ? 1.0 : 0.0;
    if (!TR) {
#pragma unroll
        for (int j = 0; j < W; ++j) {                           // L: x_i -= l_ij x_j
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
        for (int j = W - 1; j >= 0; --j) {                      // U: x_j /= u_jj, then x_i -= u_ij x_j
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
    } else {
#pragma unroll
        for (int j = 0; j < W; ++j) {                           // U^T: x_j /= u_jj, then x_i -= u_ji x_j
            if (j < n) {
                const double ujj = __shfl(lu[j], base | j);
                x[j] = x[j] / ujj;
#pragma unroll
                for (int i = j + 1; i < W; ++i) {
                    if (i < n) {
                        const double u = __shfl(lu[i], base | j);
                        const double t = u * x[j];
                        x[i] = x[i] - t;
                    }
                }
            }
        }
#pragma unroll
        for (int j = W - 1; j >= 1; --j) {                      // L^T: x_i -= l_ji x_j
            if (j < n) {
#pragma unroll
                for (int i = 0; i < j; ++i) {
                    const double l = __shfl(lu[i], base | j);
                    const double t = l * x[j];
                    x[i] = x[i] - t;
                }
            }
        }
    }
    // the tree over the lane's own registers (the levels above W add +0), then the maximum over the matrix's lanes
#pragma unroll
    for (int i = 0; i < W; ++i) x[i] = i < n ? fabs(x[i]) : 0.0;
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) {
#pragma unroll
        for (int i = 0; i < o; ++i) x[i] = x[i] + x[i + o];
    }
    double m = valid ? x[0] : 0.0;
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) m = br_nanmax(m, __shfl_xor(m, o));
    if (valid && r == 0) {
        if (z) m = __longlong_as_double(0x7FF0000000000000ll);  // no inverse: +Inf, rcond 0
        rcond[b] = z ? 0.0 : br_rcond(m, anorm[b]);
        if (ainvnm) ainvnm[b] = m;
    }
}

// ---- reciprocal condition number, workgroup form ------------------------------------------------------------------------------------
// LDS: T[ldl x n] doubles, WM[16] (the waves' maxima), ctl[4] (a zero on U's diagonal)
static size_t br_gecon_wg_lds(int n) { return (size_t)(n | 1) * n * sizeof(double) + 16 * sizeof(double) + 4 * sizeof(int); }

template <int H, bool TR>
__global__ __launch_bounds__(H == 1 ? 256 : 1024) void br_gecon_wg_kernel(const double *LU, long long ldlu, long long strideLU, int n,
                                                                         const double *anorm, double *rcond, double *ainvnm) {
    constexpr int NT = H == 1 ? 256 : 1024, NW = NT / 64, CB = 4;
    const int ldl = n | 1;
    double *T = (double *)br_smem, *WM = T + (size_t)ldl * n;
    int *ctl = (int *)(WM + 16);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long long b = blockIdx.x;
    br_load_matrix(LU + b * strideLU, ldlu, n, T, ldl, tid, NT);
    if (tid == 0) ctl[0] = 0;
    __syncthreads();
    if (tid < n && T[tid + tid * ldl] == 0.0) ctl[0] = 1;       // (every writer stores the same value)
    __syncthreads();
    if (ctl[0]) {                                                // (the whole workgroup) no inverse: +Inf, rcond 0, before any arithmetic
        if (tid == 0) {
            rcond[b] = 0.0;
            if (ainvnm) ainvnm[b] = __longlong_as_double(0x7FF0000000000000ll);
        }
        return;
    }
    double wm = 0.0;
    for (int kb = w * CB; kb < n; kb += NW * CB) {               // chains kb .. kb + 3 (those past n: all zero, not counted)
        double x[CB][H], xj[CB];
#pragma unroll
        for (int c = 0; c < CB; ++c) {
#pragma unroll
            for (int h = 0; h < H; ++h) x[c][h] = (lane + 64 * h == kb + c && kb + c < n) ? 1.0 : 0.0;
        }
        if (!TR) {
            for (int j = kb; j < n - 1; ++j) {                   // L: x_i -= l_ij x_j; the steps before kb meet zeros only
#pragma unroll
                for (int c = 0; c < CB; ++c) xj[c] = br_bcast<H>(x[c], j);
#pragma unroll
                for (int h = 0; h < H; ++h) {
                    if (64 * h + 63 > j) {                       // (uniform)
                        const int r = lane + 64 * h;
                        const bool low = r > j && r < n;
                        const double l = low ? T[r + j * ldl] : 0.0;
#pragma unroll
                        for (int c = 0; c < CB; ++c) {           // (selects, not branches, as bt_getri_wg_kernel)
                            const double t = l * xj[c];
                            const double v = x[c][h] - t;
                            x[c][h] = low ? v : x[c][h];
                        }
                    }
                }
            }
            for (int j = n - 1; j >= 0; --j) {                   // U: x_j /= u_jj, then x_i -= u_ij x_j
                double dv = 1.0;
#pragma unroll
                for (int c = 0; c < CB; ++c) { const double v = br_bcast<H>(x[c], j); if (lane == c) dv = v; }
                dv = dv / T[j + j * ldl];                        // the four divisions of the step, in lanes 0 .. 3
#pragma unroll
                for (int c = 0; c < CB; ++c) xj[c] = br_readlane(dv, c);
#pragma unroll
                for (int h = 0; h < H; ++h) {
                    if (64 * h <= j) {                           // (uniform)
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
        } else {
            for (int j = kb; j < n; ++j) {                       // U^T: x_j /= u_jj, then x_i -= u_ji x_j; the steps before kb meet zeros only
                double dv = 1.0;
#pragma unroll
                for (int c = 0; c < CB; ++c) { const double v = br_bcast<H>(x[c], j); if (lane == c) dv = v; }
                dv = dv / T[j + j * ldl];
#pragma unroll
                for (int c = 0; c < CB; ++c) xj[c] = br_readlane(dv, c);
#pragma unroll
                for (int h = 0; h < H; ++h) {
                    if (64 * h + 63 >= j) {                      // (uniform)
                        const int r = lane + 64 * h;
                        const bool low = r > j && r < n;
                        const double u = low ? T[j + r * ldl] : 0.0;
#pragma unroll
                        for (int c = 0; c < CB; ++c) {
                            const double t = u * xj[c];
                            const double v = x[c][h] - t;
                            x[c][h] = r == j ? xj[c] : (low ? v : x[c][h]);
                        }
                    }
                }
            }
            for (int j = n - 1; j >= 1; --j) {                   // L^T: x_i -= l_ji x_j
#pragma unroll
                for (int c = 0; c < CB; ++c) xj[c] = br_bcast<H>(x[c], j);
#pragma unroll
                for (int h = 0; h < H; ++h) {
                    if (64 * h < j) {                            // (uniform)
                        const int r = lane + 64 * h;
                        const bool up = r < j;
                        const double l = up ? T[j + r * ldl] : 0.0;
#pragma unroll
                        for (int c = 0; c < CB; ++c) {
                            const double t = l * xj[c];
                            const double v = x[c][h] - t;
                            x[c][h] = up ? v : x[c][h];
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < CB; ++c) {                           // the tree: the lane's second row, then the butterfly
            double s = fabs(x[c][0]);
            if (H == 2) s = s + fabs(x[c][H - 1]);
            s = br_team_sum<64>(s);
            if (kb + c < n) wm = br_nanmax(wm, s);
        }
    }
    if (lane == 0) WM[w] = wm;
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < NW; ++i) wm = br_nanmax(wm, WM[i]);
        rcond[b] = br_rcond(wm, anorm[b]);
        if (ainvnm) ainvnm[b] = wm;
    }
}

// ---- the step operator ----------------------------------------------------------------------------------------------------------------
// r_i = b_i - sum_j op(A)_ij x_j and w_i = |b_i| + sum_j |op(A)_ij| |x_j|, j ascending, every product rounded before it is added;
// lane = row (rows lane + 64 h), x in the team's registers.  Rows >= n keep r = w = 0 (x and bv are 0 there).
template <int H, int TS>
__device__ __forceinline__ void br_resid(int trans, const double *a, long long lda, int n, int lane, const double (&x)[H],
                                         const double (&bv)[H], double (&r)[H], double (&w)[H]) {
#pragma unroll
    for (int h = 0; h < H; ++h) { r[h] = bv[h]; w[h] = fabs(bv[h]); }
    constexpr int PF = 8;                                        // columns of op(A) in flight before the first of them is used (with four the
                                                                 // 1024-thread kernel needs no scratch, and measured slower: 2.46 against 2.03 ms)
    for (int j0 = 0; j0 < n; j0 += PF) {
        double av[PF][H];
#pragma unroll
        for (int u = 0; u < PF; ++u) {
#pragma unroll
            for (int h = 0; h < H; ++h) {
                const int row = lane + 64 * h, j = j0 + u;
                av[u][h] = (row < n && j < n) ? (trans ? a[j + (long long)row * lda] : a[row + (long long)j * lda]) : 0.0;
            }
        }
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int j = j0 + u;
            if (j < n) {                                         // (uniform)
                const double xj = br_rhs_bcast<H, TS>(x, j), axj = fabs(xj);
#pragma unroll
                for (int h = 0; h < H; ++h) {
                    if (lane + 64 * h < n) {
                        const double t = av[u][h] * xj;
                        r[h] = r[h] - t;
                        const double v = fabs(av[u][h]) * axj;
                        w[h] = w[h] + v;
                    }
                }
            }
        }
    }
}

// a team of TS threads (8, 16, 32 lanes of a wave, or one wave with H rows per lane) per (matrix, column)
template <int H, int TS>
__global__ __launch_bounds__(BR_T) void br_residual_kernel(int trans, const double *A, long long lda, long long strideA, int n, long long units,
                                                          int nrhs, const double *X, long long ldx, long long strideX, const double *B,
                                                          long long ldb, long long strideB, double *R, long long ldr, long long strideR,
                                                          double *Wo) {
    static_assert(TS <= 64, "a team is part of one wave");
    const int tid = threadIdx.x, team = tid / TS, lane = tid - team * TS;
    const long long u = (long long)blockIdx.x * (BR_T / TS) + team;
    if (u >= units) return;                                      // (whole teams)
    const long long b = u / nrhs;
    const int k = (int)(u - b * nrhs);
    const double *xc = X + b * strideX + (long long)k * ldx, *bc = B + b * strideB + (long long)k * ldb;
    double x[H], bv[H], r[H], w[H];
#pragma unroll
    for (int h = 0; h < H; ++h) {
        const int row = lane + 64 * h;
        x[h] = row < n ? xc[row] : 0.0;
        bv[h] = row < n ? bc[row] : 0.0;
    }
    br_resid<H, TS>(trans, A + b * strideA, lda, n, lane, x, bv, r, w);
#pragma unroll
    for (int h = 0; h < H; ++h) {
        const int row = lane + 64 * h;
        if (row < n) {
            R[b * strideR + (long long)k * ldr + row] = r[h];
            if (Wo) Wo[b * strideR + (long long)k * ldr + row] = w[h];
        }
    }
}

// ---- refinement and bound -------------------------------------------------------------------------------------------------------------
// bt_getrs_kernel's chains on the team's vector, lane = row, without the interchanges (the caller applies them as a map)
template <int H, int TS>
__device__ __forceinline__ void br_chain(int trans, const double *T, int ldl, int n, int lane, double (&x)[H]) {
    if (!trans) {
        for (int j = 0; j < n; ++j) {                            // L: b_i -= l_ij b_j
            const double xj = br_rhs_bcast<H, TS>(x, j);
#pragma unroll
            for (int h = 0; h < H; ++h) {
                const int r = lane + 64 * h;
                if (r > j && r < n) { const double t = T[r + j * ldl] * xj; x[h] = x[h] - t; }
            }
        }
        for (int j = n - 1; j >= 0; --j) {                       // U: b_j /= u_jj, then b_i -= u_ij b_j
            const double xj = br_rhs_bcast<H, TS>(x, j) / T[j + j * ldl];
#pragma unroll
            for (int h = 0; h < H; ++h) {
                const int r = lane + 64 * h;
                if (r == j) x[h] = xj;
                else if (r < j) { const double t = T[r + j * ldl] * xj; x[h] = x[h] - t; }
            }
        }
    } else {
        for (int j = 0; j < n; ++j) {                            // U^T: b_j /= u_jj, then b_i -= u_ji b_j
            const double xj = br_rhs_bcast<H, TS>(x, j) / T[j + j * ldl];
#pragma unroll
            for (int h = 0; h < H; ++h) {
                const int r = lane + 64 * h;
                if (r == j) x[h] = xj;
                else if (r > j && r < n) { const double t = T[j + r * ldl] * xj; x[h] = x[h] - t; }
            }
        }
        for (int j = n - 1; j >= 0; --j) {                       // L^T: b_i -= l_ji b_j
            const double xj = br_rhs_bcast<H, TS>(x, j);
#pragma unroll
            for (int h = 0; h < H; ++h) {
                const int r = lane + 64 * h;
                if (r < j) { const double t = T[j + r * ldl] * xj; x[h] = x[h] - t; }
            }
        }
    }
}

// LDS per team: T[ldl x n], G[BR_GC x n] (g per column of the chunk), S[waves x n] (a wave's vector on its way through an interchange
// map), XM[BR_GC] (max |x| per column), FM[waves x BR_GC] (the waves' maxima), then pv, map0, map1 [n] ints; rounded up to 16 bytes
__host__ __device__ inline size_t br_gerfs_lds(int n, int waves) {
    return (((size_t)(n | 1) * n + (size_t)BR_GC * n + (size_t)waves * n + BR_GC + (size_t)waves * BR_GC) * sizeof(double) +
            3 * (size_t)n * sizeof(int) + 15) & ~(size_t)15;
}

template <int H, int TS>
__global__ __launch_bounds__(TS >= 64 ? TS : 64) void br_gerfs_kernel(int trans, const double *A, long long lda, long long strideA, const double *LU,
                                                       long long ldlu, long long strideLU, int n, long long batch, const int *ipiv,
                                                       long long strideP, int nrhs, const double *B, long long ldb, long long strideB,
                                                       double *X, long long ldx, long long strideX, int itmax, double *ferr, double *berr,
                                                       int *iters) {
    static_assert(TS >= 64 || H == 1, "a team inside a wave holds one row per lane");
    static_assert(TS >= BR_GC, "lane c of a team keeps column c's maximum");
    constexpr int NWV = TS >= 64 ? TS / 64 : 1, TPW = TS >= 64 ? 1 : 64 / TS;   // waves per team; teams per workgroup: a team of whole
                                                                                 // waves is a workgroup, smaller teams share ONE wave (the LDS
                                                                                 // per wave decides how many waves a CU holds, not the workgroup)
    const int ldl = n | 1;
    const int tid = threadIdx.x, team = tid / TS, tt = tid - team * TS;
    const long long b = (long long)blockIdx.x * TPW + team;
    const bool active = b < batch;
    double *T = (double *)(br_smem + (size_t)team * br_gerfs_lds(n, NWV));
    double *G = T + (size_t)ldl * n, *S = G + (size_t)BR_GC * n, *XM = S + (size_t)NWV * n, *FM = XM + BR_GC;
    int *pv = (int *)(FM + NWV * BR_GC), *map0 = pv + n, *map1 = map0 + n;
    if (active) {
        br_load_matrix(LU + b * strideLU, ldlu, n, T, ldl, tt, TS);
        if (tt < n) {
            int p = ipiv[b * strideP + tt] - 1;
            if (p < 0 || p >= n) p = tt;                         // (as bt_getrs_kernel: keeps every access in range)
            pv[tt] = p;
        }
    }
    __syncthreads();
    // both interchange maps of bt_getrs_kernel: trans = 0 loads position q from row map0[q]; trans = 1 stores position q to row map1[q]
    if (active && tt < n) {
        int cpos = tt;
        for (int j = 0; j < n; ++j) { const int p = pv[j]; cpos = cpos == j ? p : (cpos == p ? j : cpos); }
        map0[cpos] = tt;
        cpos = tt;
        for (int j = n - 1; j >= 0; --j) { const int p = pv[j]; cpos = cpos == j ? p : (cpos == p ? j : cpos); }
        map1[tt] = cpos;
    }
    __syncthreads();
    if (!active) return;                                         // (whole teams; for TS = 256 the whole workgroup)
    const int w = tt >> 6, lane = tt & 63;
    double *Sw = S + (size_t)w * n;
    const double *a = A + b * strideA, *bb = B + b * strideB;
    double *xx = X + b * strideX;
    const double eps = 0x1p-53, nz = (double)(n + 1), safe1 = nz * DBL_MIN, safe2 = safe1 / eps, nzeps = nz * eps;
    for (int c0 = 0; c0 < nrhs; c0 += BR_GC) {
        const int nc = nrhs - c0 < BR_GC ? nrhs - c0 : BR_GC;
        for (int c = w; c < nc; c += NWV) {
            const long long k = c0 + c;
            double x[H], bv[H], r[H], wv[H];
#pragma unroll
            for (int h = 0; h < H; ++h) {
                const int row = lane + 64 * h;
                x[h] = row < n ? xx[k * ldx + row] : 0.0;
                bv[h] = row < n ? bb[k * ldb + row] : 0.0;
            }
            double lst = 3.0, be_out = 0.0;
            int it = 0, count = 1;
            bool act = true;
            for (;;) {
                br_resid<H, TS>(trans, a, lda, n, lane, x, bv, r, wv);
                double q = 0.0;
#pragma unroll
                for (int h = 0; h < H; ++h) {
                    if (lane + 64 * h < n) {
                        const double ar = fabs(r[h]);
                        q = br_nanmax(q, wv[h] > safe2 ? ar / wv[h] : (ar + safe1) / (wv[h] + safe1));
                    }
                }
                const double be = br_team_max<TS>(q);
                if (act) be_out = be;
                const bool go = act && be > eps && 2.0 * be <= lst && count <= itmax;   // (false for a NaN: the column stops)
                act = go;
                if (!__any(go)) break;                           // (teams of one wave stay in step; a stopped team's x no longer changes)
                double d[H];
                if (!trans) {
#pragma unroll
                    for (int h = 0; h < H; ++h) { const int row = lane + 64 * h; if (row < n) Sw[row] = r[h]; }
                    br_wave_sync();
#pragma unroll
                    for (int h = 0; h < H; ++h) { const int row = lane + 64 * h; d[h] = row < n ? Sw[map0[row]] : 0.0; }
                    br_wave_sync();
                    br_chain<H, TS>(0, T, ldl, n, lane, d);
                } else {
#pragma unroll
                    for (int h = 0; h < H; ++h) d[h] = r[h];
                    br_chain<H, TS>(1, T, ldl, n, lane, d);
#pragma unroll
                    for (int h = 0; h < H; ++h) { const int row = lane + 64 * h; if (row < n) Sw[map1[row]] = d[h]; }
                    br_wave_sync();
#pragma unroll
                    for (int h = 0; h < H; ++h) { const int row = lane + 64 * h; d[h] = row < n ? Sw[row] : 0.0; }
                    br_wave_sync();
                }
                if (go) {
#pragma unroll
                    for (int h = 0; h < H; ++h) x[h] = x[h] + d[h];
                    lst = be;
                    it = count;
                }
                ++count;
            }
            double xm = 0.0;
#pragma unroll
            for (int h = 0; h < H; ++h) {
                const int row = lane + 64 * h;
                if (row < n) {
                    xx[k * ldx + row] = x[h];
                    xm = br_nanmax(xm, fabs(x[h]));
                    if (ferr) {                                  // g_i = |r_i| + nz eps w_i (+ safe1 where w_i <= safe2)
                        const double t = nzeps * wv[h];
                        double g = fabs(r[h]) + t;
                        if (!(wv[h] > safe2)) g = g + safe1;
                        G[(size_t)c * n + row] = g;
                    }
                }
            }
            xm = br_team_max<TS>(xm);
            if (lane == 0) {
                berr[b * nrhs + k] = be_out;
                if (iters) iters[b * nrhs + k] = it;
                if (ferr) XM[c] = xm;
            }
        }
        if (!ferr) continue;
        if (TS >= 64) __syncthreads(); else br_wave_sync();
        // f_i = tree_k |y_k| g_k for every row i of op(A)^-1: y = the chain of 1 - trans on e_i, interchanges included
        double fm = 0.0;                                         // lane c: max_i f_i of column c0 + c, over this wave's rows
        for (int i = w; i < n; i += NWV) {
            double y[H];
            if (trans) {                                         // the trans = 0 chain: e_i goes through map0 first
#pragma unroll
                for (int h = 0; h < H; ++h) { const int row = lane + 64 * h; y[h] = (row < n && map0[row] == i) ? 1.0 : 0.0; }
                br_chain<H, TS>(0, T, ldl, n, lane, y);
            } else {                                             // the trans = 1 chain: its result goes through map1
#pragma unroll
                for (int h = 0; h < H; ++h) y[h] = lane + 64 * h == i ? 1.0 : 0.0;
                br_chain<H, TS>(1, T, ldl, n, lane, y);
#pragma unroll
                for (int h = 0; h < H; ++h) { const int row = lane + 64 * h; if (row < n) Sw[map1[row]] = y[h]; }
                br_wave_sync();
#pragma unroll
                for (int h = 0; h < H; ++h) { const int row = lane + 64 * h; y[h] = row < n ? Sw[row] : 0.0; }
                br_wave_sync();
            }
#pragma unroll
            for (int h = 0; h < H; ++h) y[h] = fabs(y[h]);
            for (int c = 0; c < nc; ++c) {
                double t[H];
#pragma unroll
                for (int h = 0; h < H; ++h) { const int row = lane + 64 * h; t[h] = row < n ? y[h] * G[(size_t)c * n + row] : 0.0; }
                const double s = br_team_sum<TS>(H == 1 ? t[0] : t[0] + t[H - 1]);
                if (lane == c) fm = br_nanmax(fm, s);
            }
        }
        if (TS >= 64) {
            if (lane < nc) FM[w * BR_GC + lane] = fm;
            __syncthreads();
            if (tt < nc) {
                for (int i = 1; i < NWV; ++i) fm = br_nanmax(fm, FM[i * BR_GC + tt]);
                const double xm = XM[tt];
                ferr[b * nrhs + c0 + tt] = xm != 0.0 ? fm / xm : fm;
            }
            __syncthreads();                                     // the next chunk rewrites G, XM and FM
        } else {
            if (tt < nc) {
                const double xm = XM[tt];
                ferr[b * nrhs + c0 + tt] = xm != 0.0 ? fm / xm : fm;
            }
            br_wave_sync();
        }
    }
}

// ---- launchers: one launch each, batch <= BT_MAX_LAUNCH matrices (the host splits longer batches) -----------------------------------
static int br_attrs(mpf_ctx *c) {
    if (c->attr_done & ATTR_BATCHED_REFINE) return 0;
    const void *ks[] = {(const void *)br_lange_kernel<1, 32>, (const void *)br_lange_kernel<1, 256>, (const void *)br_lange_kernel<2, 256>,
                        (const void *)br_gecon_wg_kernel<1, false>, (const void *)br_gecon_wg_kernel<1, true>,
                        (const void *)br_gecon_wg_kernel<2, false>, (const void *)br_gecon_wg_kernel<2, true>,
                        (const void *)br_gerfs_kernel<1, 8>, (const void *)br_gerfs_kernel<1, 16>, (const void *)br_gerfs_kernel<1, 32>,
                        (const void *)br_gerfs_kernel<1, 256>, (const void *)br_gerfs_kernel<2, 1024>};
    for (const void *k : ks) MPF_HIP_TRY(c, hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    c->attr_done |= ATTR_BATCHED_REFINE;
    return 0;
}

int launch_lange_batched(mpf_ctx *c, int mode, const double *A, int64_t lda, int64_t strideA, int n, int64_t batch, double *out) {
    if (n < 1 || batch < 1) return 0;
    if (n > BR_MAXN || batch > BT_MAX_LAUNCH || mode < 0 || mode > 2) { c->err = "launch_lange_batched: argument out of range"; return -1; }
    { const int e = br_attrs(c); if (e) return e; }
#define BR_NORM(H_, TS_)                                                                                                                 \
    do {                                                                                                                                 \
        const int per_wg = BR_T / TS_;                                                                                                   \
        const unsigned g = (unsigned)((batch + per_wg - 1) / per_wg);                                                                    \
        br_lange_kernel<H_, TS_><<<g, BR_T, br_lange_lds(n) * per_wg, c->stream>>>(mode, A, lda, strideA, n, batch, out);                \
    } while (0)
    if (n <= 8) BR_NORM(1, 8);
    else if (n <= 16) BR_NORM(1, 16);
    else if (n <= 32) BR_NORM(1, 32);
    else if (n <= 64) BR_NORM(1, 256);
    else BR_NORM(2, 256);
#undef BR_NORM
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

int launch_gecon_batched(mpf_ctx *c, int inf, const double *LU, int64_t ldlu, int64_t strideLU, int n, int64_t batch, const double *anorm,
                         double *rcond, double *ainvnm) {
    if (n < 1 || batch < 1) return 0;
    if (n > BR_MAXN || batch > BT_MAX_LAUNCH) { c->err = "launch_gecon_batched: size out of range"; return -1; }
    if (n <= 32) {
#define BR_CON(W_)                                                                                                                   \
        do {                                                                                                                         \
            const long long per = (BR_T / W_);                                                                                       \
            const unsigned g = (unsigned)((batch + per - 1) / per);                                                                  \
            if (inf) br_gecon_wave_kernel<W_, true><<<g, BR_T, 0, c->stream>>>(LU, ldlu, strideLU, n, batch, anorm, rcond, ainvnm);    \
            else br_gecon_wave_kernel<W_, false><<<g, BR_T, 0, c->stream>>>(LU, ldlu, strideLU, n, batch, anorm, rcond, ainvnm);       \
        } while (0)
        if (n <= 8) BR_CON(8);
        else if (n <= 16) BR_CON(16);
        else BR_CON(32);
#undef BR_CON
    } else {
        { const int e = br_attrs(c); if (e) return e; }
        const size_t lds = br_gecon_wg_lds(n);
        if (n <= 64) {
            if (inf) br_gecon_wg_kernel<1, true><<<(unsigned)batch, 256, lds, c->stream>>>(LU, ldlu, strideLU, n, anorm, rcond, ainvnm);
            else br_gecon_wg_kernel<1, false><<<(unsigned)batch, 256, lds, c->stream>>>(LU, ldlu, strideLU, n, anorm, rcond, ainvnm);
        } else {
            if (inf) br_gecon_wg_kernel<2, true><<<(unsigned)batch, 1024, lds, c->stream>>>(LU, ldlu, strideLU, n, anorm, rcond, ainvnm);
            else br_gecon_wg_kernel<2, false><<<(unsigned)batch, 1024, lds, c->stream>>>(LU, ldlu, strideLU, n, anorm, rcond, ainvnm);
        }
    }
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

int launch_residual_batched(mpf_ctx *c, int trans, const double *A, int64_t lda, int64_t strideA, int n, int64_t batch, int nrhs,
                            const double *X, int64_t ldx, int64_t strideX, const double *B, int64_t ldb, int64_t strideB, double *R,
                            int64_t ldr, int64_t strideR, double *W) {
    if (n < 1 || batch < 1 || nrhs < 1) return 0;
    const int64_t units = batch * nrhs;
    if (n > BR_MAXN || units > BR_MAX_UNITS) { c->err = "launch_residual_batched: size out of range"; return -1; }
#define BR_RES(H_, TS_)                                                                                                                  \
    do {                                                                                                                                 \
        const int per_wg = BR_T / TS_;                                                                                                   \
        const unsigned g = (unsigned)((units + per_wg - 1) / per_wg);                                                                    \
        br_residual_kernel<H_, TS_><<<g, BR_T, 0, c->stream>>>(trans, A, lda, strideA, n, units, nrhs, X, ldx, strideX, B, ldb, strideB, \
                                                               R, ldr, strideR, W);                                                      \
    } while (0)
    if (n <= 8) BR_RES(1, 8);
    else if (n <= 16) BR_RES(1, 16);
    else if (n <= 32) BR_RES(1, 32);
    else if (n <= 64) BR_RES(1, 64);
    else BR_RES(2, 64);
#undef BR_RES
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

int launch_gerfs_batched(mpf_ctx *c, int trans, const double *A, int64_t lda, int64_t strideA, const double *LU, int64_t ldlu,
                         int64_t strideLU, int n, int64_t batch, const int *ipiv, int64_t strideP, int nrhs, const double *B, int64_t ldb,
                         int64_t strideB, double *X, int64_t ldx, int64_t strideX, int itmax, double *ferr, double *berr, int *iters) {
    if (n < 1 || batch < 1 || nrhs < 1) return 0;
    if (n > BR_MAXN || batch > BT_MAX_LAUNCH) { c->err = "launch_gerfs_batched: size out of range"; return -1; }
    { const int e = br_attrs(c); if (e) return e; }
#define BR_RFS(H_, TS_)                                                                                                                  \
    do {                                                                                                                                 \
        const int per_wg = TS_ >= 64 ? 1 : 64 / TS_, nt = TS_ >= 64 ? TS_ : 64;                                                          \
        const unsigned g = (unsigned)((batch + per_wg - 1) / per_wg);                                                                    \
        br_gerfs_kernel<H_, TS_><<<g, nt, br_gerfs_lds(n, TS_ >= 64 ? TS_ / 64 : 1) * per_wg, c->stream>>>(                            \
            trans, A, lda, strideA, LU, ldlu, strideLU, n, batch, ipiv, strideP, nrhs, B, ldb, strideB, X, ldx, strideX, itmax, ferr,    \
            berr, iters);                                                                                                                \
    } while (0)
    if (n <= 8) BR_RFS(1, 8);
    else if (n <= 16) BR_RFS(1, 16);
    else if (n <= 32) BR_RFS(1, 32);
    else if (n <= 64) BR_RFS(1, 256);
    else BR_RFS(2, 1024);                                        // (one workgroup per CU fits beside 129 KB of factors: sixteen waves share the bound's chains)
#undef BR_RFS
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}
