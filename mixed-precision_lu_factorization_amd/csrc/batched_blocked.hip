// Blocked LU of many matrices of order up to 1024 (mpf_getrf_batched_blocked, mpf_getrs_batched_blocked; contracts in
// include/mpf_c.h, host side in mpf_batched.cpp), and from its factors the inverse and the determinant
// (mpf_getri_batched_blocked, mpf_getdet_batched_blocked; bb_getri_kernel and bb_getdet_kernel below).
//
// The numeric contract is batched.hip's, unchanged: mpf_dgetf2_piv on the whole n x n matrix.  Per element that is one update per k in
// ascending order (contract C3), and for fused = 1 the update is c = fma(-l_ik, u_kj, c) -- the chain of v_mfma_f64_16x16x4_f64
// (contract C5).  A right-looking blocked loop applies exactly those updates in exactly that order whatever the panel width, so the
// width (8, 16 or 32) is a performance choice.  Per panel step three ordinary launches, each ONE grid over the whole batch:
//   bb_panel_kernel<NB>      one workgroup per matrix, thread = row of A[j0:n, j0:j0+nb], the row's nb columns in registers (column loops
//                            fully unrolled).  Rows never move while resident (batched.hip): a thread keeps its row's CURRENT position.
//                            Pivot search: wave reduction over (|x| bits with NaN -> 0, position), the waves' bests combined through
//                            LDS by every thread; the pivot row is broadcast through LDS; one division per row; rank-1 update fused or
//                            not.  Two barriers per column, everything they guard double-buffered.  Writes ipiv (1-based, global), info
//                            (the first panel's launch initialises it) and the rows at their final positions.
//   bb_rowblk_kernel<NB>     grid (column chunks, batch), thread = one column left or right of the panel: the panel's nb interchanges as
//                            ONE map (simulated once per workgroup on an index array in LDS), every load before the first store; right
//                            of the panel then the forward substitution with the panel's unit-lower tile from LDS, k ascending.
//   bb_update_mfma_kernel<NB>  grid (64 x 64 tiles of C, batch), four waves of 32 x 32: C into the accumulators, nb / 4
//                            v_mfma_f64_16x16x4_f64 with k ascending, the negation on the L operand (the instruction's NEG bit).  The
//                            MFMA's row index is C's column (trailing_f64.hip): a lane's 16-lane group walks 16 consecutive rows of C.
//                            Operands straight from global memory (K = nb: every operand element is used by two MFMAs of the wave).
//   bb_update_valu_kernel<NB, FUSED>  the same tiling on the VALU: the unfused contract (rounded product, rounded difference); its fused
//                            instantiation is the MFMA kernel's cross-check (probe library, option batched_blocked_valu).
// A trailing matrix exists only behind a FULL panel, so K = nb always: no operand is padded along k.  Rows and columns past the matrix
// are predicated loads of zeros whose results are never stored; an element inside the matrix never sees them.
//   bb_getrs_kernel<CT>      one workgroup per (matrix, tile of CT right-hand-side columns), thread = row, the row's CT values in
//                            registers.  The sweeps go in blocks of 32: a thread loads its 32 factor elements of the block first (all
//                            in flight), the block's wave solves the 32 x 32 diagonal block with v_readlane broadcasts and publishes the
//                            32 x CT results in LDS, one barrier, then every other row applies the 32 steps in the contract's order.
//                            trans = 1 reads the same blocks transposed.  The interchanges are one composed map (bt_getrs_kernel).
#include "mpf_internal.h"
#include <limits.h>

typedef double bb_d4 __attribute__((ext_vector_type(4)));

template <bool FUSED>
__device__ __forceinline__ double bb_mulsub(double x, double m, double u) {
    if (FUSED) return __builtin_fma(-m, u, x);
    const double t = m * u; // -ffp-contract=off: stays mul + sub
    return x - t;
}
// search key of an element: |a|'s bit pattern (monotone in |a|), 0 for a NaN
__device__ __forceinline__ unsigned long long bb_key(double a) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(a) & 0x7FFFFFFFFFFFFFFFull;
    return b > 0x7FF0000000000000ull ? 0ull : b;
}
__device__ __forceinline__ bool bb_beats(unsigned long long k1, int r1, unsigned long long k0, int r0) {
    return k1 > k0 || (k1 == k0 && r1 < r0);
}
__device__ __forceinline__ double bb_readlane(double v, int lane) {
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)b, lane), hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), lane);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// ---- panel ------------------------------------------------------------------------------------------------------------------------------
// blockDim.x = the panel's rows n - j0 rounded up to whole waves (<= 1024); blockIdx.x = matrix
template <int NB, bool FUSED>
__global__ __launch_bounds__(1024) void bb_panel_kernel(double *A, long long lda, long long strideA, int n, int j0, int *ipiv,
                                                        long long strideP, int *info) {
    __shared__ unsigned long long skey[2][16];
    __shared__ int spos[2][16];
    __shared__ double urow[2][NB];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, nw = (int)(blockDim.x >> 6);
    const int rows = n - j0, jc = rows < NB ? rows : NB;
    double *a = A + (long long)blockIdx.x * strideA + j0 + (long long)j0 * lda;
    const bool valid = t < rows;
    double x[NB];
#pragma unroll
    for (int c = 0; c < NB; ++c) x[c] = (valid && c < jc) ? a[t + (long long)c * lda] : 0.0;
    int cp = t, inf = 0;                                            // cp: this row's current position (local to the panel)
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        if (j < jc) {                                               // (uniform)
            const bool open = valid && cp >= j;
            unsigned long long key = open ? bb_key(x[j]) : 0ull;
            int pos = open ? ((cp << 10) | t) : INT_MAX;            // ordered by position; carries the row.  The row at position j is open
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)key, o), hi = (unsigned)__shfl_xor((int)(unsigned)(key >> 32), o);
                const unsigned long long k1 = ((unsigned long long)hi << 32) | lo;
                const int p1 = __shfl_xor(pos, o);
                if (bb_beats(k1, p1, key, pos)) { key = k1; pos = p1; }
            }
            if (lane == 0) { skey[j & 1][w] = key; spos[j & 1][w] = pos; }
            __syncthreads();
            key = skey[j & 1][0];
            pos = spos[j & 1][0];
            for (int i = 1; i < nw; ++i) {
                const unsigned long long k1 = skey[j & 1][i];
                const int p1 = spos[j & 1][i];
                if (bb_beats(k1, p1, key, pos)) { key = k1; pos = p1; }
            }
            const int p = pos >> 10, wr = pos & 1023;
            if (t == wr) {
#pragma unroll
                for (int c = j; c < NB; ++c) urow[j & 1][c] = x[c];
            }
            __syncthreads();
            if (t == wr) cp = j;
            else if (cp == j) cp = p;                               // dgetf2's interchange: the row at position j goes where the pivot row was
            const double uj = urow[j & 1][j];
            if (t == 0) ipiv[(long long)blockIdx.x * strideP + j0 + j] = j0 + p + 1;
            if (uj == 0.0 && inf == 0) inf = j0 + j + 1;
            if (valid && cp > j) {
                const double m = x[j] / uj;
                x[j] = m;
#pragma unroll
                for (int c = j + 1; c < NB; ++c) x[c] = bb_mulsub<FUSED>(x[c], m, urow[j & 1][c]);
            }
        }
    }
    if (valid) {
#pragma unroll
        for (int c = 0; c < NB; ++c)
            if (c < jc) a[cp + (long long)c * lda] = x[c];
    }
    if (info && t == 0) {
        if (j0 == 0) info[blockIdx.x] = inf;
        else if (inf != 0 && info[blockIdx.x] == 0) info[blockIdx.x] = inf;
    }
}

// ---- row block: interchanges outside the panel, then U12 = L11^-1 A12 ---------------------------------------------------------------
constexpr int BB_RT = 256;   // threads = columns per workgroup
template <int NB, bool FUSED>
__global__ __launch_bounds__(BB_RT) void bb_rowblk_kernel(double *A, long long lda, long long strideA, int n, int j0, const int *ipiv,
                                                          long long strideP) {
    __shared__ double Ls[NB * NB];
    __shared__ int perm[BB_MAXN];
    __shared__ int pv[NB];
    const int tid = threadIdx.x;
    const int rows = n - j0, jc = rows < NB ? rows : NB;
    double *a = A + (long long)blockIdx.y * strideA;
    for (int i = tid; i < rows; i += BB_RT) perm[i] = i;
    if (tid < jc) {
        int p = ipiv[(long long)blockIdx.y * strideP + j0 + tid] - 1 - j0;
        if (p < tid || p >= rows) p = tid;                          // (never, for the panel kernel's pivots: keeps every access in range regardless)
        pv[tid] = p;
    }
    for (int i = tid; i < NB * NB; i += BB_RT) {
        const int r = i % NB, k = i / NB;
        Ls[i] = (r < jc && k < r) ? a[(j0 + r) + (long long)(j0 + k) * lda] : 0.0;
    }
    __syncthreads();
    if (tid == 0)
        for (int k = 0; k < jc; ++k) { const int p = pv[k], v = perm[k]; perm[k] = perm[p]; perm[p] = v; }
    __syncthreads();
    const int ci = (int)blockIdx.x * BB_RT + tid;
    if (ci >= n - jc) return;
    const bool right = ci >= j0;
    double *col = a + j0 + (long long)(right ? ci + jc : ci) * lda;  // the column from the panel's first row on
    double y[NB], z[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        y[k] = 0.0;
        z[k] = 0.0;
        if (k < jc) {
            y[k] = col[perm[k]];                                    // position k receives the row that stands there after the interchanges
            const int pk = pv[k];
            if (pk >= jc) z[k] = col[perm[pk]];                     // ... and so does every position below the block that one of them touched
        }
    }
#pragma unroll
    for (int k = 0; k < NB; ++k)
        if (k < jc && pv[k] >= jc) col[pv[k]] = z[k];
    if (right) {                                                    // (then jc == NB: columns right of the panel exist only behind a full panel)
#pragma unroll
        for (int k = 0; k < NB; ++k)
#pragma unroll
            for (int i = k + 1; i < NB; ++i) y[i] = bb_mulsub<FUSED>(y[i], Ls[i + k * NB], y[k]);
    }
#pragma unroll
    for (int k = 0; k < NB; ++k)
        if (k < jc) col[k] = y[k];
}

// ---- trailing update: C -= L U, K = NB ----------------------------------------------------------------------------------------------------
// blockIdx.x = 64 x 64 tile of the m x m trailing matrix (m = n - j0 - NB), blockIdx.y = matrix
constexpr int BB_UT = 64;
template <int NB>
__global__ __launch_bounds__(256) void bb_update_mfma_kernel(double *A, long long lda, long long strideA, int n, int j0) {
    const int j1 = j0 + NB, m = n - j1, tiles = (m + BB_UT - 1) / BB_UT;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, lj = lane & 15, lk = lane >> 4;
    const int r0 = ((int)blockIdx.x % tiles) * BB_UT + (w & 1) * 32, c0 = ((int)blockIdx.x / tiles) * BB_UT + (w >> 1) * 32;
    if (r0 >= m || c0 >= m) return;                                 // (the whole wave; the kernel has no barrier)
    double *a = A + (long long)blockIdx.y * strideA;
    const double *Lp = a + j1 + (long long)j0 * lda;                // l_ik = Lp[i + k lda]
    const double *Up = a + j0 + (long long)j1 * lda;                // u_kj = Up[k + j lda]
    double *Cp = a + j1 + (long long)j1 * lda;
    bb_d4 acc[2][2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {                        // register rr of tile (mt, nt) is C[r0 + 16 mt + lj, c0 + 16 nt + lk + 4 rr]
                const int r = r0 + 16 * mt + lj, c = c0 + 16 * nt + lk + 4 * rr;
                acc[mt][nt][rr] = (r < m && c < m) ? Cp[r + (long long)c * lda] : 0.0;
            }
#pragma unroll
    for (int k0 = 0; k0 < NB; k0 += 4) {
        double lf[2], uf[2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const int r = r0 + 16 * mt + lj;
            lf[mt] = r < m ? Lp[r + (long long)(k0 + lk) * lda] : 0.0;
        }
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const int c = c0 + 16 * nt + lj;
            uf[nt] = c < m ? Up[(k0 + lk) + (long long)c * lda] : 0.0;
        }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
                acc[mt][nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(uf[nt], lf[mt], acc[mt][nt], 0, 0, 2 /* -L */);
    }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int r = r0 + 16 * mt + lj, c = c0 + 16 * nt + lk + 4 * rr;
                if (r < m && c < m) Cp[r + (long long)c * lda] = acc[mt][nt][rr];
            }
}

// the same tiles on the VALU: thread = (row of the tile, group of 16 columns), the row's NB multipliers in registers
template <int NB, bool FUSED>
__global__ __launch_bounds__(256) void bb_update_valu_kernel(double *A, long long lda, long long strideA, int n, int j0) {
    const int j1 = j0 + NB, m = n - j1, tiles = (m + BB_UT - 1) / BB_UT;
    const int r = ((int)blockIdx.x % tiles) * BB_UT + (int)(threadIdx.x & 63);
    const int c0 = ((int)blockIdx.x / tiles) * BB_UT + (int)(threadIdx.x >> 6) * 16;
    if (r >= m) return;
    double *a = A + (long long)blockIdx.y * strideA;
    const double *Lp = a + j1 + (long long)j0 * lda;
    const double *Up = a + j0 + (long long)j1 * lda;
    double *Cp = a + j1 + (long long)j1 * lda;
    double l[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) l[k] = Lp[r + (long long)k * lda];
    for (int q = 0; q < 16; ++q) {
        const int c = c0 + q;
        if (c >= m) break;
        const double *u = Up + (long long)c * lda;
        double v = Cp[r + (long long)c * lda];
#pragma unroll
        for (int k = 0; k < NB; ++k) v = bb_mulsub<FUSED>(v, l[k], u[k]);
        Cp[r + (long long)c * lda] = v;
    }
}

// ---- solve ---------------------------------------------------------------------------------------------------------------------------------
// One sweep over the blocks of 32.  ASC: L (trans = 0) and U^T; descending: U and L^T.  DIV: the sweep divides by the diagonal (U, U^T).
// TR: the factor element of (row t, step j) is LU[j, t] instead of LU[t, j].  ph counts the blocks of both sweeps: xs is double-buffered.
template <int CT, bool ASC, bool DIV, bool TR>
__device__ __forceinline__ void bb_sweep(const double *T, long long ld, int n, int t, bool valid, double (&x)[CT], double (*xs)[32][CT], int &ph) {
    const int nblk = (n + 31) >> 5;
    for (int s = 0; s < nblk; ++s, ++ph) {
        const int kb = ASC ? s : nblk - 1 - s, r0 = kb * 32, buf = ph & 1;
        const bool part = valid && (ASC ? t >= r0 : t < r0 + 32);
        double l[32];
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            const int c = r0 + j;
            l[j] = (part && c < n) ? (TR ? T[c + (long long)t * ld] : T[t + (long long)c * ld]) : 0.0;
        }
        if ((t >> 6) == (kb >> 1)) {                                // the block's wave: the 32 x 32 diagonal block
            const int rr = t - r0, base = (kb & 1) * 32;
            const bool mine = valid && rr >= 0 && rr < 32;
#pragma unroll
            for (int jj = 0; jj < 32; ++jj) {
                const int j = ASC ? jj : 31 - jj;
                if (r0 + j < n) {                                   // (uniform)
                    double d = 1.0;
                    if (DIV) d = T[(r0 + j) + (long long)(r0 + j) * ld];
                    const bool upd = mine && (ASC ? rr > j : rr < j);
#pragma unroll
                    for (int c = 0; c < CT; ++c) {
                        double xj = bb_readlane(x[c], base + j);
                        if (DIV) xj = xj / d;
                        const double p = l[j] * xj;
                        const double v = x[c] - p;
                        x[c] = (DIV && mine && rr == j) ? xj : (upd ? v : x[c]);
                    }
                }
            }
            if (mine) {
#pragma unroll
                for (int c = 0; c < CT; ++c) xs[buf][rr][c] = x[c];
            }
        }
        __syncthreads();
        if (valid && (ASC ? t >= r0 + 32 : t < r0)) {
#pragma unroll
            for (int jj = 0; jj < 32; ++jj) {
                const int j = ASC ? jj : 31 - jj;
                if (r0 + j < n) {
#pragma unroll
                    for (int c = 0; c < CT; ++c) {
                        const double p = l[j] * xs[buf][j][c];
                        x[c] = x[c] - p;
                    }
                }
            }
        }
    }
}

// blockDim.x = n rounded up to whole waves; blockIdx.x = tile of CT columns of B, blockIdx.y = matrix
template <int CT>
__global__ __launch_bounds__(1024) void bb_getrs_kernel(int trans, const double *LU, long long ldlu, long long strideLU, int n, const int *ipiv,
                                                        long long strideP, int nrhs, double *B, long long ldb, long long strideB) {
    __shared__ int pv[BB_MAXN], map[BB_MAXN];
    __shared__ double xs[2][32][CT];
    const int t = threadIdx.x;
    const long long b = blockIdx.y;
    const int c0 = (int)blockIdx.x * CT, nc = nrhs - c0 < CT ? nrhs - c0 : CT;
    const double *T = LU + b * strideLU;
    const bool valid = t < n;
    if (valid) {
        int p = ipiv[b * strideP + t] - 1;
        if (p < 0 || p >= n) p = t;                                 // (as bt_getrs_kernel: keeps every access in range)
        pv[t] = p;
    }
    __syncthreads();
    if (valid) {                                                    // the interchanges as one map (bt_getrs_kernel)
        int cpos = t;
        if (!trans) {
            for (int j = 0; j < n; ++j) { const int p = pv[j]; cpos = cpos == j ? p : (cpos == p ? j : cpos); }
            map[cpos] = t;
        } else {
            for (int j = n - 1; j >= 0; --j) { const int p = pv[j]; cpos = cpos == j ? p : (cpos == p ? j : cpos); }
            map[t] = cpos;
        }
    }
    __syncthreads();
    double *bb = B + b * strideB + (long long)c0 * ldb;
    double x[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) x[c] = (valid && c < nc) ? bb[(trans ? t : map[t]) + (long long)c * ldb] : 0.0;
    int ph = 0;
    if (!trans) {
        bb_sweep<CT, true, false, false>(T, ldlu, n, t, valid, x, xs, ph);    // L: b_i -= l_ij b_j
        bb_sweep<CT, false, true, false>(T, ldlu, n, t, valid, x, xs, ph);    // U: b_j /= u_jj, then b_i -= u_ij b_j
    } else {
        bb_sweep<CT, true, true, true>(T, ldlu, n, t, valid, x, xs, ph);      // U^T: b_j /= u_jj, then b_i -= u_ji b_j
        bb_sweep<CT, false, false, true>(T, ldlu, n, t, valid, x, xs, ph);    // L^T: b_i -= l_ji b_j
    }
    if (valid) {
#pragma unroll
        for (int c = 0; c < CT; ++c)
            if (c < nc) bb[(trans ? map[t] : t) + (long long)c * ldb] = x[c];
    }
}

// ---- inverse ----------------------------------------------------------------------------------------------------------------------------
// inv(A) = inv(U) inv(L) P: column k of the result is column q(k) of inv(L) taken through the backward sweep, so the interchanges are
// no arithmetic -- the workgroup that owns columns q .. q + CT - 1 of inv(L) stores them at columns k(q) = map[q], bb_getrs_kernel's
// composed map.  One workgroup per (matrix, tile of CT consecutive q), thread = row, the row's CT values in registers, both sweeps in
// blocks of 32 rows as bb_sweep has them.  What differs from the solve:
//   - the tile's columns start as e_q, never read; the forward sweep starts at the block that holds the tile's smallest q (the steps
//     before it subtract l * (+0) from +0);
//   - the 32 x 32 diagonal block is solved with lane = COLUMN: the block's rows go through LDS (xs, with the block's factor rows in
//     ds), lane c of the block's wave takes column c in groups of BB_IG rows -- the terms of the rows already solved first, then the
//     group's triangle -- with the factor elements as LDS broadcasts: one division per (row, column) instead of one per (row, column,
//     lane), 496 multiply-subtract pairs per column instead of 32 x 32 selects;
//   - the rows outside the block then apply its 32 steps in the chain's order, the factor elements BB_IG at a time.
// Rows past n inside the last block publish zeros that the solve never writes back, and columns past n of the factors read as zero,
// so the 32 steps of a block need no bound checks: x - 0 * 0 = x.  A zero on U's diagonal is found by every workgroup of the matrix
// before its first store; such a workgroup returns, the tile-0 workgroup writes info.
constexpr int BB_IG = 8;    // rows per register group of the diagonal solve
constexpr int BB_UG = 16;   // factor elements per load group of the update
template <int CT, bool ASC>
__device__ __forceinline__ void bb_inv_sweep(const double *T, long long ld, int n, int t, bool valid, int kb0, double (&x)[CT],
                                             double (*xs)[32][CT + 1], double (*ds)[32][33], int &ph) {
    const int nblk = (n + 31) >> 5, lane = t & 63;
    for (int s = ASC ? kb0 : 0; s < nblk; ++s, ++ph) {
        const int kb = ASC ? s : nblk - 1 - s, r0 = kb * 32, buf = ph & 1, rr = t - r0;
        const int cnt = n - r0 < 32 ? n - r0 : 32;
        const bool mine = rr >= 0 && rr < 32;                       // (rows past n included: they publish zeros)
        const bool part = valid && (ASC ? t >= r0 + 32 : t < r0);
        if (mine) {
#pragma unroll
            for (int c = 0; c < CT; ++c) xs[buf][rr][c] = x[c];
#pragma unroll 16
            for (int j = 0; j < 32; ++j) ds[buf][rr][j] = (valid && j < cnt) ? T[t + (long long)(r0 + j) * ld] : 0.0;
        }
        __syncthreads();
        if ((t >> 6) == (kb >> 1) && lane < CT) {                   // the block's wave, lane = column
#pragma unroll 1
            for (int gg = 0; gg < 32 / BB_IG; ++gg) {
                const int i0 = (ASC ? gg : 32 / BB_IG - 1 - gg) * BB_IG;
                if (i0 < cnt) {                                     // (uniform)
                    double y[BB_IG];
#pragma unroll
                    for (int i = 0; i < BB_IG; ++i) y[i] = xs[buf][i0 + i][lane];
                    if (ASC) {
#pragma unroll 2
                        for (int j = 0; j < i0; ++j) {              // (j < i0 < cnt)
                            const double xj = xs[buf][j][lane];
#pragma unroll
                            for (int i = 0; i < BB_IG; ++i) { const double p = ds[buf][i0 + i][j] * xj; y[i] = y[i] - p; }
                        }
#pragma unroll
                        for (int j = 0; j < BB_IG; ++j)
#pragma unroll
                            for (int i = j + 1; i < BB_IG; ++i) { const double p = ds[buf][i0 + i][i0 + j] * y[j]; y[i] = y[i] - p; }
                    } else {
#pragma unroll 2
                        for (int j = cnt - 1; j >= i0 + BB_IG; --j) {
                            const double xj = xs[buf][j][lane];
#pragma unroll
                            for (int i = 0; i < BB_IG; ++i) { const double p = ds[buf][i0 + i][j] * xj; y[i] = y[i] - p; }
                        }
#pragma unroll
                        for (int j = BB_IG - 1; j >= 0; --j) {
                            if (i0 + j < cnt) {                     // (uniform)
                                y[j] = y[j] / ds[buf][i0 + j][i0 + j];
#pragma unroll
                                for (int i = 0; i < j; ++i) { const double p = ds[buf][i0 + i][i0 + j] * y[j]; y[i] = y[i] - p; }
                            }
                        }
                    }
#pragma unroll
                    for (int i = 0; i < BB_IG; ++i)
                        if (i0 + i < cnt) xs[buf][i0 + i][lane] = y[i];
                }
            }
        }
        __syncthreads();
        if (part) {
#pragma unroll 1
            for (int g = 0; g < 32 / BB_UG; ++g) {
                const int j0 = (ASC ? g : 32 / BB_UG - 1 - g) * BB_UG;
                double l[BB_UG];
#pragma unroll
                for (int j = 0; j < BB_UG; ++j) l[j] = j0 + j < cnt ? T[t + (long long)(r0 + j0 + j) * ld] : 0.0;
#pragma unroll
                for (int jj = 0; jj < BB_UG; ++jj) {
                    const int j = ASC ? jj : BB_UG - 1 - jj;
#pragma unroll
                    for (int c = 0; c < CT; ++c) { const double p = l[j] * xs[buf][j0 + j][c]; x[c] = x[c] - p; }
                }
            }
        } else if (mine && valid) {
#pragma unroll
            for (int c = 0; c < CT; ++c) x[c] = xs[buf][rr][c];
        }
    }
}

// blockDim.x = n rounded up to whole waves; blockIdx.x = tile of CT columns of inv(L), blockIdx.y = matrix
template <int CT>
__global__ __launch_bounds__(1024) void bb_getri_kernel(const double *LU, long long ldlu, long long strideLU, int n, const int *ipiv,
                                                        long long strideP, double *inv, long long ldinv, long long strideInv, int *info) {
    __shared__ int pv[BB_MAXN], map[BB_MAXN];
    __shared__ double xs[2][32][CT + 1], ds[2][32][33];
    __shared__ int zfirst;
    const int t = threadIdx.x;
    const long long b = blockIdx.y;
    const int q0 = (int)blockIdx.x * CT;
    const double *T = LU + b * strideLU;
    const bool valid = t < n;
    if (t == 0) zfirst = INT_MAX;
    if (valid) {
        int p = ipiv[b * strideP + t] - 1;
        if (p < 0 || p >= n) p = t;                                 // (as bb_getrs_kernel: keeps every access in range)
        pv[t] = p;
    }
    __syncthreads();
    if (valid) {
        int cpos = t;
        for (int j = 0; j < n; ++j) { const int p = pv[j]; cpos = cpos == j ? p : (cpos == p ? j : cpos); }
        map[cpos] = t;                                              // position cpos holds row t: column t of the result starts as e_cpos
        if (T[t + (long long)t * ldlu] == 0.0) atomicMin(&zfirst, t + 1);
    }
    __syncthreads();
    const int z = zfirst;
    if (info && blockIdx.x == 0 && t == 0) info[b] = z == INT_MAX ? 0 : z;
    if (z != INT_MAX) return;                                       // (the whole workgroup: nothing is stored)
    double x[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) x[c] = (valid && t == q0 + c) ? 1.0 : 0.0;   // (columns past n: zeros, never stored)
    int ph = 0;
    bb_inv_sweep<CT, true>(T, ldlu, n, t, valid, q0 >> 5, x, xs, ds, ph);     // L from the tile's first block: x_i -= l_ij x_j
    bb_inv_sweep<CT, false>(T, ldlu, n, t, valid, 0, x, xs, ds, ph);          // U in full: x_i -= u_ij x_j, then x_i /= u_ii
    if (valid) {
        double *o = inv + b * strideInv;
#pragma unroll
        for (int c = 0; c < CT; ++c)
            if (q0 + c < n) o[t + (long long)map[q0 + c] * ldinv] = x[c];
    }
}

// ---- determinant -----------------------------------------------------------------------------------------------------------------------
// mpf_getdet's order for n <= 1024: up to four chunks of 256 consecutive diagonal entries.  One workgroup per matrix: thread = diagonal
// entry for the loads ((m_i, e_i) = frexp(u_ii) into LDS, the pivot count and the special cases by LDS atomics), thread = chunk for the
// serial chains, thread 0 for the combining chain.  Reads n of the matrix's n^2 doubles.
__global__ __launch_bounds__(256) void bb_getdet_kernel(const double *LU, long long ldlu, long long strideLU, int n, const int *ipiv,
                                                        long long strideP, double *mant, int *expo) {
    constexpr int DCH = 256;
    __shared__ double sm[BB_MAXN], cp[BB_MAXN / DCH];
    __shared__ int se[BB_MAXN], ce[BB_MAXN / DCH];
    __shared__ int s_zero, s_bad, s_flips;
    const int t = threadIdx.x, nch = (n + DCH - 1) / DCH;
    const long long b = blockIdx.x;
    const double *a = LU + b * strideLU;
    const int *pvt = ipiv + b * strideP;
    if (t == 0) { s_zero = 0; s_bad = 0; s_flips = 0; }
    __syncthreads();
    int zero = 0, bad = 0, flips = 0;
    for (int i = t; i < n; i += 256) {
        const double u = a[i + (long long)i * ldlu];
        zero |= u == 0.0;
        bad |= !(fabs(u) <= 1.7976931348623157e308);
        flips ^= pvt[i] != i + 1 ? 1 : 0;
        int ei;
        sm[i] = frexp(u, &ei);
        se[i] = ei;
    }
    if (zero) atomicOr(&s_zero, 1);
    if (bad) atomicOr(&s_bad, 1);
    if (flips) atomicXor(&s_flips, 1);
    __syncthreads();
    if (t < nch) {
        const int i1 = (t + 1) * DCH < n ? (t + 1) * DCH : n;
        double p = 1.0;
        int e = 0;
        for (int i = t * DCH; i < i1; ++i) mpf_det_step(p, e, sm[i], se[i]);
        cp[t] = p;
        ce[t] = e;
    }
    __syncthreads();
    if (t != 0) return;
    double P = 1.0;
    int E = 0;
    for (int ch = 0; ch < nch; ++ch) mpf_det_step(P, E, cp[ch], ce[ch]);
    if (s_flips) P = -P;
    if (s_bad) { P = __builtin_nan(""); E = 0; }
    else if (s_zero) { P = 0.0; E = 0; }
    mant[b] = P;
    expo[b] = E;
}

// ---- launchers: batch <= BB_MAX_LAUNCH matrices (the host splits longer batches) ---------------------------------------------------------
template <int NB>
static void bb_factor_loop(mpf_ctx *c, double *A, int64_t lda, int64_t strideA, int n, int64_t batch, int *ipiv, int64_t strideP, int *info,
                           bool fused, bool valu, int stages) {
    const unsigned nbat = (unsigned)batch;
    for (int j0 = 0; j0 < n; j0 += NB) {
        const int rows = n - j0, jc = rows < NB ? rows : NB, m = rows - jc;
        if (stages & 1) {
            const unsigned th = (unsigned)((rows + 63) / 64 * 64);
            if (fused) bb_panel_kernel<NB, true><<<nbat, th, 0, c->stream>>>(A, lda, strideA, n, j0, ipiv, strideP, info);
            else bb_panel_kernel<NB, false><<<nbat, th, 0, c->stream>>>(A, lda, strideA, n, j0, ipiv, strideP, info);
        }
        if (n - jc > 0 && (stages & 2)) {
            const dim3 g((unsigned)((n - jc + BB_RT - 1) / BB_RT), nbat);
            if (fused) bb_rowblk_kernel<NB, true><<<g, BB_RT, 0, c->stream>>>(A, lda, strideA, n, j0, ipiv, strideP);
            else bb_rowblk_kernel<NB, false><<<g, BB_RT, 0, c->stream>>>(A, lda, strideA, n, j0, ipiv, strideP);
        }
        if (m > 0 && (stages & 4)) {
            const unsigned tiles = (unsigned)((m + BB_UT - 1) / BB_UT);
            const dim3 g(tiles * tiles, nbat);
            if (!fused) bb_update_valu_kernel<NB, false><<<g, 256, 0, c->stream>>>(A, lda, strideA, n, j0);
            else if (valu) bb_update_valu_kernel<NB, true><<<g, 256, 0, c->stream>>>(A, lda, strideA, n, j0);
            else bb_update_mfma_kernel<NB><<<g, 256, 0, c->stream>>>(A, lda, strideA, n, j0);
        }
    }
}

int launch_getrf_batched_blocked(mpf_ctx *c, double *A, int64_t lda, int64_t strideA, int n, int64_t batch, int *ipiv, int64_t strideP,
                                 int *info, int fused, int nb, int valu, int stages) {
    if (n < 1 || batch < 1) return 0;
    if (n > BB_MAXN || batch > BB_MAX_LAUNCH) { c->err = "launch_getrf_batched_blocked: size out of range"; return -1; }
    // automatic: 32 was the fastest width at every measured n from 24 to 1024 but n = 48 (16: 3 - 6 % faster); DESIGN 4.21
    if (nb != 8 && nb != 16 && nb != 32) nb = 32;
    if (nb == 8) bb_factor_loop<8>(c, A, lda, strideA, n, batch, ipiv, strideP, info, fused != 0, valu != 0, stages);
    else if (nb == 16) bb_factor_loop<16>(c, A, lda, strideA, n, batch, ipiv, strideP, info, fused != 0, valu != 0, stages);
    else bb_factor_loop<32>(c, A, lda, strideA, n, batch, ipiv, strideP, info, fused != 0, valu != 0, stages);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

int launch_getrs_batched_blocked(mpf_ctx *c, int trans, const double *LU, int64_t ldlu, int64_t strideLU, int n, int64_t batch,
                                 const int *ipiv, int64_t strideP, int nrhs, double *B, int64_t ldb, int64_t strideB) {
    if (n < 1 || batch < 1 || nrhs < 1) return 0;
    if (n > BB_MAXN || batch > BB_MAX_LAUNCH) { c->err = "launch_getrs_batched_blocked: size out of range"; return -1; }
    const unsigned th = (unsigned)((n + 63) / 64 * 64);
    // the column tiles of one matrix are a grid's first dimension; a tile of one column below four right-hand sides
    if (nrhs < 4) {
        const dim3 g((unsigned)nrhs, (unsigned)batch);
        bb_getrs_kernel<1><<<g, th, 0, c->stream>>>(trans, LU, ldlu, strideLU, n, ipiv, strideP, nrhs, B, ldb, strideB);
    } else {
        const dim3 g((unsigned)((nrhs + 7) / 8), (unsigned)batch);
        bb_getrs_kernel<8><<<g, th, 0, c->stream>>>(trans, LU, ldlu, strideLU, n, ipiv, strideP, nrhs, B, ldb, strideB);
    }
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

int launch_getri_batched_blocked(mpf_ctx *c, const double *LU, int64_t ldlu, int64_t strideLU, int n, int64_t batch, const int *ipiv,
                                 int64_t strideP, double *inv, int64_t ldinv, int64_t strideInv, int *info, int ct) {
    if (n < 1 || batch < 1) return 0;
    if (n > BB_MAXN || batch > BB_MAX_LAUNCH) { c->err = "launch_getri_batched_blocked: size out of range"; return -1; }
    const unsigned th = (unsigned)((n + 63) / 64 * 64);
    if (ct != 8 && ct != 16) ct = 16;                              // automatic
    const dim3 g((unsigned)((n + ct - 1) / ct), (unsigned)batch);
    if (ct == 8) bb_getri_kernel<8><<<g, th, 0, c->stream>>>(LU, ldlu, strideLU, n, ipiv, strideP, inv, ldinv, strideInv, info);
    else bb_getri_kernel<16><<<g, th, 0, c->stream>>>(LU, ldlu, strideLU, n, ipiv, strideP, inv, ldinv, strideInv, info);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

int launch_getdet_batched_blocked(mpf_ctx *c, const double *LU, int64_t ldlu, int64_t strideLU, int n, int64_t batch, const int *ipiv,
                                  int64_t strideP, double *mant, int *expo) {
    if (n < 1 || batch < 1) return 0;
    if (n > BB_MAXN || batch > BB_MAX_LAUNCH) { c->err = "launch_getdet_batched_blocked: size out of range"; return -1; }
    bb_getdet_kernel<<<(unsigned)batch, 256, 0, c->stream>>>(LU, ldlu, strideLU, n, ipiv, strideP, mant, expo);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}
