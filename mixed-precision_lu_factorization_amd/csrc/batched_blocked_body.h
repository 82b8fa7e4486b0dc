// The blocked batched kernels' bodies as __device__ functions of (matrix base, leading dimension, n, the matrix's pivots, the matrix's
// info entry, the work item): the one copy of the arithmetic of the blocked family.  Three files wrap it: batched_blocked.hip (one order
// per call: base = A + b stride), vbatched_blocked.hip (ragged lists: base from the descriptor) and batched_refine_blocked.hip (the two
// sweeps).  A matrix's bits are therefore the same whichever entry it came through (DESIGN 4.23 has the resource table and the times
// that allowed the sharing).
//
// The numeric contract is batched.hip's, unchanged: mpf_dgetf2_piv on the whole n x n matrix.  Per element that is one update per k in
// ascending order (contract C3), and for fused = 1 the update is c = fma(-l_ik, u_kj, c) -- the chain of v_mfma_f64_16x16x4_f64
// (contract C5).  A right-looking blocked loop applies exactly those updates in exactly that order whatever the panel width, so the
// width (8, 16 or 32) is a performance choice.  Per panel step three ordinary launches, each ONE grid over the whole batch:
//   bb_panel_body<NB>        one workgroup per matrix, thread = row of A[j0:n, j0:j0+nb], the row's nb columns in registers (column loops
//                            fully unrolled).  Rows never move while resident (batched.hip): a thread keeps its row's CURRENT position.
//                            Pivot search: wave reduction over (|x| bits with NaN -> 0, position), the waves' bests combined through
//                            LDS by every thread; the pivot row is broadcast through LDS; one division per row; rank-1 update fused or
//                            not.  Two barriers per column, everything they guard double-buffered.  Writes ipiv (1-based, global), info
//                            (the first panel's launch initialises it) and the rows at their final positions.
//   bb_rowblk_body<NB>       workgroup = (column chunk, matrix), thread = one column left or right of the panel: the panel's nb
//                            interchanges as ONE map (simulated once per workgroup on an index array in LDS), every load before the first
//                            store; right of the panel then the forward substitution with the panel's unit-lower tile from LDS, k ascending.
//   bb_update_mfma_body<NB>  workgroup = (64 x 64 tile of C, matrix), four waves of 32 x 32: C into the accumulators, nb / 4
//                            v_mfma_f64_16x16x4_f64 with k ascending, the negation on the L operand (the instruction's NEG bit).  The
//                            MFMA's row index is C's column (trailing_f64.hip): a lane's 16-lane group walks 16 consecutive rows of C.
//                            Operands straight from global memory (K = nb: every operand element is used by two MFMAs of the wave).
//   bb_update_valu_body<NB, FUSED>  the same tiling on the VALU: the unfused contract (rounded product, rounded difference); its fused
//                            instantiation is the MFMA kernel's cross-check (probe library, option batched_blocked_valu).
// A trailing matrix exists only behind a FULL panel, so K = nb always: no operand is padded along k.  Rows and columns past the matrix
// are predicated loads of zeros whose results are never stored; an element inside the matrix never sees them.
//   bb_getrs_body<CT>        one workgroup per (matrix, tile of CT right-hand-side columns), thread = row, the row's CT values in
//                            registers.  The sweeps go in blocks of 32: a thread loads its 32 factor elements of the block first (all
//                            in flight), the block's wave solves the 32 x 32 diagonal block with v_readlane broadcasts and publishes the
//                            32 x CT results in LDS, one barrier, then every other row applies the 32 steps in the contract's order.
//                            trans = 1 reads the same blocks transposed.  The interchanges are one composed map (bt_getrs_kernel).
//
// Where a workgroup stands in its launch is the caller's business.  A ragged launch is sized for the largest matrix of its list, so:
//   - a body takes the work item's coordinates (column chunk, C tile, right-hand-side tile, inverse tile) as arguments and leaves as a
//     whole, before its first barrier, when its matrix is exhausted (n <= j0) or the item lies outside its own matrix (uniform scalar
//     compares that never hold in a fixed-size launch);
//   - threads past the matrix's own rows stay in every barrier and reduction as valid = false; nw comes from blockDim, and the surplus
//     waves publish the neutral key (0, INT_MAX) like the surplus lanes of a fixed-size launch's last wave;
//   - every "rows and columns past the matrix read as zero" is a predicated load against the matrix's own n: in a packed descriptor the
//     next matrix starts at the very next double.
#pragma once
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

constexpr int BB_RT = 256;   // row block: threads = columns per workgroup
constexpr int BB_UT = 64;    // trailing update: tile of C
constexpr int BB_IG = 8;     // inverse: rows per register group of the diagonal solve
constexpr int BB_UG = 16;    // inverse: factor elements per load group of the update

// The ragged launches' fetch (vbatched_blocked.hip, vbatched_refine.hip): entry i of a list ordered by n is matrix b = idx[i]; its order,
// matrix offset, leading dimension and vector offset come from the descriptor's arrays
struct bbv_entry { int b, n; long long off, ld, offv; };
__device__ __forceinline__ bbv_entry bbv_fetch(const BtRagged &v, const int *idx, unsigned i) {
    bbv_entry e;
    e.b = idx[i];
    e.n = v.n[e.b];
    e.off = v.off[e.b];
    e.ld = v.ld[e.b];
    e.offv = v.offv[e.b];
    return e;
}

// ---- panel (bb_panel_kernel) ----------------------------------------------------------------------------------------------------------
// A: the matrix; ipiv: the matrix's pivots; info: the matrix's entry or null.  blockDim.x >= n - j0 in whole waves (<= 1024)
template <int NB, bool FUSED>
__device__ __forceinline__ void bb_panel_body(double *A, long long lda, int n, int j0, int *ipiv, int *info) {
    __shared__ unsigned long long skey[2][16];
    __shared__ int spos[2][16];
    __shared__ double urow[2][NB];
    if (n <= j0) return;                                            // (the whole workgroup: the matrix is exhausted)
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, nw = (int)(blockDim.x >> 6);
    const int rows = n - j0, jc = rows < NB ? rows : NB;
    double *a = A + j0 + (long long)j0 * lda;
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
            if (t == 0) ipiv[j0 + j] = j0 + p + 1;
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
        if (j0 == 0) *info = inf;
        else if (inf != 0 && *info == 0) *info = inf;
    }
}

// ---- row block (bb_rowblk_kernel): interchanges outside the panel, then U12 = L11^-1 A12 ------------------------------------------------
// chunk: which BB_RT columns of the matrix's n - jc columns outside the panel this workgroup takes.  blockDim.x = BB_RT
template <int NB, bool FUSED>
__device__ __forceinline__ void bb_rowblk_body(double *a, long long lda, int n, int j0, const int *ipiv, int chunk) {
    __shared__ double Ls[NB * NB];
    __shared__ int perm[BB_MAXN];
    __shared__ int pv[NB];
    if (n <= j0) return;                                            // (the whole workgroup: the matrix is exhausted)
    const int tid = threadIdx.x;
    const int rows = n - j0, jc = rows < NB ? rows : NB;
    if (chunk * BB_RT >= n - jc) return;                            // (the whole workgroup: the chunk lies outside this matrix)
    for (int i = tid; i < rows; i += BB_RT) perm[i] = i;
    if (tid < jc) {
        int p = ipiv[j0 + tid] - 1 - j0;
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
    const int ci = chunk * BB_RT + tid;
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

// ---- trailing update (bb_update_mfma_kernel, bb_update_valu_kernel): C -= L U, K = NB ---------------------------------------------------
// tile: which 64 x 64 tile of the matrix's own m x m trailing matrix (m = n - j0 - NB).  A matrix without a full panel at j0 has
// m <= 0 and no trailing matrix: nothing runs for it, whatever the launch's m is.  blockDim.x = 256; no barrier
template <int NB>
__device__ __forceinline__ void bb_update_mfma_body(double *a, long long lda, int n, int j0, int tile) {
    const int j1 = j0 + NB, m = n - j1;
    if (m <= 0) return;
    const int tiles = (m + BB_UT - 1) / BB_UT;
    if (tile >= tiles * tiles) return;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, lj = lane & 15, lk = lane >> 4;
    const int r0 = (tile % tiles) * BB_UT + (w & 1) * 32, c0 = (tile / tiles) * BB_UT + (w >> 1) * 32;
    if (r0 >= m || c0 >= m) return;                                 // (the whole wave; the kernel has no barrier)
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
__device__ __forceinline__ void bb_update_valu_body(double *a, long long lda, int n, int j0, int tile) {
    const int j1 = j0 + NB, m = n - j1;
    if (m <= 0) return;
    const int tiles = (m + BB_UT - 1) / BB_UT;
    if (tile >= tiles * tiles) return;
    const int r = (tile % tiles) * BB_UT + (int)(threadIdx.x & 63);
    const int c0 = (tile / tiles) * BB_UT + (int)(threadIdx.x >> 6) * 16;
    if (r >= m) return;
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

// ---- solve (bb_sweep, bb_getrs_kernel) --------------------------------------------------------------------------------------------------
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

// T: the matrix's factors; ipiv: its pivots; B: its first right-hand-side row (row 0 of the matrix, column 0 of B); tile: which CT
// columns of B.  blockDim.x >= n in whole waves
template <int CT>
__device__ __forceinline__ void bb_getrs_body(int trans, const double *T, long long ldlu, int n, const int *ipiv, int nrhs, double *B,
                                              long long ldb, int tile) {
    __shared__ int pv[BB_MAXN], map[BB_MAXN];
    __shared__ double xs[2][32][CT];
    const int t = threadIdx.x;
    const int c0 = tile * CT, nc = nrhs - c0 < CT ? nrhs - c0 : CT;
    if (n < 1 || nc < 1) return;                                    // (the whole workgroup)
    const bool valid = t < n;
    if (valid) {
        int p = ipiv[t] - 1;
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
    double *bb = B + (long long)c0 * ldb;
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

// ---- inverse (bb_inv_sweep, bb_getri_kernel) --------------------------------------------------------------------------------------------
// inv(A) = inv(U) inv(L) P: column k of the result is column q(k) of inv(L) taken through the backward sweep, so the interchanges are
// no arithmetic -- the workgroup that owns columns q .. q + CT - 1 of inv(L) stores them at columns k(q) = map[q], bb_getrs_body's
// composed map.  One workgroup per (matrix, tile of CT consecutive q), thread = row, the row's CT values in registers, both sweeps in
// blocks of 32 rows as bb_sweep has them.  What differs from the solve:
//   - the tile's columns start as e_q, never read; the forward sweep starts at the block that holds the tile's smallest q (the steps
//     before it subtract l * (+0) from +0);
//   - the 32 x 32 diagonal block is solved with lane = COLUMN: the block's rows go through LDS (xs, with the block's factor rows in
//     ds), lane c of the block's wave takes column c in groups of BB_IG rows -- the terms of the rows already solved first, then the
//     group's triangle -- with the factor elements as LDS broadcasts: one division per (row, column) instead of one per (row, column,
//     lane), 496 multiply-subtract pairs per column instead of 32 x 32 selects;
//   - the rows outside the block then apply its 32 steps in the chain's order, the factor elements BB_UG at a time.
// Rows past n inside the last block publish zeros that the solve never writes back, and columns past n of the factors read as zero,
// so the 32 steps of a block need no bound checks: x - 0 * 0 = x.  A zero on U's diagonal is found by every workgroup of the matrix
// before its first store; such a workgroup returns, the tile-0 workgroup writes info.
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

// T: the matrix's factors; ipiv: its pivots; o: its inverse; info: its entry or null; tile: which CT columns of inv(L).
// blockDim.x >= n in whole waves
template <int CT>
__device__ __forceinline__ void bb_getri_body(const double *T, long long ldlu, int n, const int *ipiv, double *o, long long ldinv, int *info,
                                              int tile) {
    __shared__ int pv[BB_MAXN], map[BB_MAXN];
    __shared__ double xs[2][32][CT + 1], ds[2][32][33];
    __shared__ int zfirst;
    const int t = threadIdx.x;
    const int q0 = tile * CT;
    if (q0 >= n) return;                                            // (the whole workgroup: the tile lies outside this matrix)
    const bool valid = t < n;
    if (t == 0) zfirst = INT_MAX;
    if (valid) {
        int p = ipiv[t] - 1;
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
    if (info && tile == 0 && t == 0) *info = z == INT_MAX ? 0 : z;
    if (z != INT_MAX) return;                                       // (the whole workgroup: nothing is stored)
    double x[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) x[c] = (valid && t == q0 + c) ? 1.0 : 0.0;   // (columns past n: zeros, never stored)
    int ph = 0;
    bb_inv_sweep<CT, true>(T, ldlu, n, t, valid, q0 >> 5, x, xs, ds, ph);     // L from the tile's first block: x_i -= l_ij x_j
    bb_inv_sweep<CT, false>(T, ldlu, n, t, valid, 0, x, xs, ds, ph);          // U in full: x_i -= u_ij x_j, then x_i /= u_ii
    if (valid) {
#pragma unroll
        for (int c = 0; c < CT; ++c)
            if (q0 + c < n) o[t + (long long)map[q0 + c] * ldinv] = x[c];
    }
}

// ---- determinant (bb_getdet_kernel) ----------------------------------------------------------------------------------------------------
// mpf_getdet's order for n <= 1024: up to four chunks of 256 consecutive diagonal entries.  One workgroup per matrix: thread = diagonal
// entry for the loads ((m_i, e_i) = frexp(u_ii) into LDS, the pivot count and the special cases by LDS atomics), thread = chunk for the
// serial chains, thread 0 for the combining chain.  Reads n of the matrix's n^2 doubles.
// a: the matrix's factors; pvt: its pivots; mant, expo: its entries.  blockDim.x = 256
__device__ __forceinline__ void bb_getdet_body(const double *a, long long ldlu, int n, const int *pvt, double *mant, int *expo) {
    constexpr int DCH = 256;
    __shared__ double sm[BB_MAXN], cp[BB_MAXN / DCH];
    __shared__ int se[BB_MAXN], ce[BB_MAXN / DCH];
    __shared__ int s_zero, s_bad, s_flips;
    const int t = threadIdx.x, nch = (n + DCH - 1) / DCH;
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
    *mant = P;
    *expo = E;
}
