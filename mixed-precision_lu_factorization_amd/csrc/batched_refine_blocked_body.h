// The bodies of the blocked batched expert kernels, one copy for the two files that launch them: batched_refine_blocked.hip (strided
// batches of one order: base = A + b stride, slots at b) and vbatched_refine.hip (ragged lists: base and slots from the descriptor).
// As in batched_blocked_body.h a body takes the matrix's base pointer(s), leading dimension(s) and n, its pivots, its right-hand-side
// and solution columns, its output slots and its work item (the tile) as arguments; nothing in here reads blockIdx or gridDim.
// blockDim.x is the launch's: >= n in whole waves, <= 1024.  A block sized for a LARGER matrix (the ragged launch) changes no bit:
//   rows >= n      hold +0 terms and +0 maxima.  Every term of a tree and every candidate of a maximum is >= +0, so the padding is
//                  exact (the tree padded to any power of two >= n is the tree padded to 1024; tests/test_vbatched_refine_cpu.py shows
//                  it on the model for every block size).  In rb_chain_body a row t >= n writes red[cc][t], t < blockDim.x <= 1024:
//                  inside the 1024 entries, and outside the positions map[] uses, which are a permutation of 0 .. n-1.
//   nw             = blockDim.x >> 6 only says how many waves share the columns of a round and how many per-wave maxima are combined;
//                  the maxima are order-free (rb_nanmax) and the extra waves bring +0.
// The account of every scheme is in batched_refine_blocked.hip's header.  Compiled with -ffp-contract=off like every kernel file.
#pragma once
#include "batched_blocked_body.h"
#include <float.h>

constexpr int RB_RC = 2;       // columns per round of rb_chain_body's tree (LDS: RB_RC x 1024 doubles, inside the sweeps' ds)
constexpr int RB_PF = 8;       // elements of a row of op(A) in flight in the residual
constexpr int RB_CT = 16;      // chains per workgroup of rb_chain_body as both files launch it: a matrix has ceil(n / RB_CT) tiles

__device__ __forceinline__ double rb_nanmax(double a, double b) { return (b > a || b != b) ? b : a; }   // a NaN on either side stays
__device__ __forceinline__ double rb_wave_max(double m) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = rb_nanmax(m, __shfl_xor(m, o));
    return m;
}
__device__ __forceinline__ double rb_wave_sum(double s) {       // the tree's levels 32 .. 1
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o);
    return s;
}
// the tree's levels 512 .. 64 for one lane: s[m] is the term of index lane + 64 m
__device__ __forceinline__ double rb_tree16(double (&s)[16]) {
#pragma unroll
    for (int h = 8; h > 0; h >>= 1) {
#pragma unroll
        for (int i = 0; i < h; ++i) s[i] = s[i] + s[i + h];
    }
    return s[0];
}
// br_rcond: 0 for anorm == 0 and for a norm of the inverse that is not finite (or 0)
__device__ __forceinline__ double rb_rcond(double ainvnm, double anorm) {
    if (anorm == 0.0 || ainvnm == 0.0 || !(fabs(ainvnm) <= DBL_MAX)) return 0.0;
    return (1.0 / ainvnm) / anorm;
}
// the maximum of one value per thread over the workgroup, in thread 0 (WM: 16 doubles of LDS; a barrier inside)
__device__ __forceinline__ double rb_block_max(double m, double *WM) {
    const int t = threadIdx.x, nw = (int)(blockDim.x >> 6);
    m = rb_wave_max(m);
    if ((t & 63) == 0) WM[t >> 6] = m;
    __syncthreads();
    if (t == 0)
        for (int i = 1; i < nw; ++i) m = rb_nanmax(m, WM[i]);
    return m;
}

// ---- norms ----------------------------------------------------------------------------------------------------------------------------
// mode 0: max_j tree_i |a_ij|; 1: max_i tree_j |a_ij|; 2: max |a_ij|.  a: the matrix; out: its slot.  One workgroup per matrix
__device__ __forceinline__ void rb_lange_body(int mode, const double *a, long long lda, int n, double *out) {
    __shared__ double WM[16];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, nw = (int)(blockDim.x >> 6);
    const bool valid = t < n;
    double m = 0.0;
    if (mode == 0) {
        for (int j = w; j < n; j += nw) {
            const double *col = a + (long long)j * lda;
            double s[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) { const int r = lane + 64 * i; s[i] = r < n ? fabs(col[r]) : 0.0; }
            m = rb_nanmax(m, rb_wave_sum(rb_tree16(s)));
        }
    } else if (mode == 2) {
        if (valid)
            for (int j = 0; j < n; ++j) m = rb_nanmax(m, fabs(a[t + (long long)j * lda]));
    } else {
        // the columns in bit-reversed order: position Q holds column rev(Q), so neighbours Q, Q + 1 are columns j, j + P / 2 and the
        // pairwise tree over Q is the halving tree over j (P: the power of two the row is padded to, >= 16)
        int bits = 4;
        while ((1 << bits) < n) ++bits;
        const int lg = bits - 4, groups = 1 << lg;
        double st[6], tot = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) st[k] = 0.0;
        for (int g = 0; g < groups; ++g) {
            double v[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int j = (int)(__brev((unsigned)(g * 16 + q)) >> (32 - bits));
                v[q] = (valid && j < n) ? fabs(a[t + (long long)j * lda]) : 0.0;
            }
#pragma unroll
            for (int h = 1; h < 16; h <<= 1) {
#pragma unroll
                for (int i = 0; i < 16; i += 2 * h) v[i] = v[i] + v[i + h];
            }
            double s = v[0];
            bool carry = true;
#pragma unroll
            for (int k = 0; k < 6; ++k) {                         // (g, lg uniform) the stack of a pairwise sum: level k is taken when bit k of g is set
                if (carry && k < lg) {
                    if ((g >> k) & 1) s = st[k] + s;
                    else { st[k] = s; carry = false; }
                }
            }
            tot = s;                                             // (after the last group: every level was taken)
        }
        m = valid ? tot : 0.0;
    }
    m = rb_block_max(m, WM);
    if (t == 0) *out = m;
}

// ---- chains from unit vectors, reduced ----------------------------------------------------------------------------------------------------
// bb_inv_sweep (batched_blocked_body.h) for the two sweeps of the trans = 1 chain as well: the scheme, the groups and the order of
// every element's steps are that function's.  ASC: the sweep runs down the rows (L, U^T), else up (U, L^T); DIV: it divides by the
// diagonal (U, U^T); TR: the factor element of (row t, step j) is LU[j, t] -- a thread then reads 32 (its block) or BB_UG consecutive
// doubles of its own column.  <CT, true, false, false> and <CT, false, true, false> are bb_inv_sweep<CT, true> and <CT, false>.
template <int CT, bool ASC, bool DIV, bool TR>
__device__ __forceinline__ void rb_inv_sweep(const double *T, long long ld, int n, int t, bool valid, int kb0, double (&x)[CT],
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
            for (int j = 0; j < 32; ++j)
                ds[buf][rr][j] = (valid && j < cnt) ? (TR ? T[(r0 + j) + (long long)t * ld] : T[t + (long long)(r0 + j) * ld]) : 0.0;
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
                        for (int j = 0; j < BB_IG; ++j) {
                            if (!DIV || i0 + j < cnt) {             // (uniform; rows past the matrix have no diagonal to divide by)
                                if (DIV) y[j] = y[j] / ds[buf][i0 + j][i0 + j];
#pragma unroll
                                for (int i = j + 1; i < BB_IG; ++i) { const double p = ds[buf][i0 + i][i0 + j] * y[j]; y[i] = y[i] - p; }
                            }
                        }
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
                                if (DIV) y[j] = y[j] / ds[buf][i0 + j][i0 + j];
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
                for (int j = 0; j < BB_UG; ++j)
                    l[j] = j0 + j < cnt ? (TR ? T[(r0 + j0 + j) + (long long)t * ld] : T[t + (long long)(r0 + j0 + j) * ld]) : 0.0;
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

// T: the matrix's factors; ipiv: its pivots (TR && WGT only); tile: which CT unit vectors; part: the matrix's tile maxima, `tiles`
// of them per column.  WGT = 0: part[tile] = max over the tile's columns of tree_t |x_t|; a zero on U's diagonal: +Inf before any
// arithmetic.  WGT = 1: part[k * tiles + tile] = max over the tile's columns of tree_p |y_p| g_p, g = G + k * n: G is the matrix's
// nrhs columns of g, n apart.  The tree's terms go through the sweeps' LDS (ds: RB_RC columns of up to 1024 terms), so the kernels
// keep bb_getri_kernel's footprint and its workgroups per CU.
template <int CT, bool TR, bool WGT>
__device__ __forceinline__ void rb_chain_body(const double *T, long long ldlu, int n, const int *ipiv, const double *G, int nrhs, double *part,
                                              int tiles, int tile) {
    static_assert(CT % RB_RC == 0, "the tree takes RB_RC columns per round");
    static_assert(RB_RC * BB_MAXN <= 2 * 32 * 33, "the tree's terms fit the sweeps' ds");
    __shared__ double xs[2][32][CT + 1], ds[2][32][33];
    __shared__ int map[(TR && WGT) ? BB_MAXN : 1];
    __shared__ double WM[16];
    __shared__ int zflag;
    double(*red)[BB_MAXN] = (double(*)[BB_MAXN]) & ds[0][0][0];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, nw = (int)(blockDim.x >> 6);
    const int q0 = tile * CT;
    const bool valid = t < n;
    if (!WGT) {
        if (t == 0) zflag = 0;
        __syncthreads();
        if (valid && T[t + (long long)t * ldlu] == 0.0) zflag = 1;   // (every writer stores the same value)
        __syncthreads();
        if (zflag) {                                                // (the whole workgroup) no inverse: +Inf, rcond 0
            if (t == 0) part[tile] = __longlong_as_double(0x7FF0000000000000ll);
            return;
        }
    }
    if (TR && WGT) {                                                // the trans = 1 chain's interchanges: its row t ends at row map[t] (bb_getrs_kernel)
        int *pv = (int *)&ds[0][0][0];
        if (valid) {
            int p = ipiv[t] - 1;
            if (p < 0 || p >= n) p = t;                             // (as bb_getrs_kernel: keeps every access in range)
            pv[t] = p;
        }
        __syncthreads();
        if (valid) {
            int cpos = t;
            for (int j = n - 1; j >= 0; --j) { const int p = pv[j]; cpos = cpos == j ? p : (cpos == p ? j : cpos); }
            map[t] = cpos;
        }
        __syncthreads();
    }
    double x[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) x[c] = (valid && t == q0 + c) ? 1.0 : 0.0;   // (columns past n: zeros, never counted)
    int ph = 0;
    if (TR) {
        // U^T from the tile's first block (the steps before it divide and subtract zeros; the bound keeps them: its factors may hold a
        // zero on the diagonal, which no skipped step may hide), then L^T in full
        rb_inv_sweep<CT, true, true, true>(T, ldlu, n, t, valid, WGT ? 0 : q0 >> 5, x, xs, ds, ph);
        rb_inv_sweep<CT, false, false, true>(T, ldlu, n, t, valid, 0, x, xs, ds, ph);
    } else {
        bb_inv_sweep<CT, true>(T, ldlu, n, t, valid, q0 >> 5, x, xs, ds, ph);    // L from the tile's first block
        bb_inv_sweep<CT, false>(T, ldlu, n, t, valid, 0, x, xs, ds, ph);         // U in full
    }
    const int pos = (TR && WGT && valid) ? map[t] : t;             // where this row's term enters the tree
    const int nk = WGT ? nrhs : 1, nred = nw < RB_RC ? nw : RB_RC;
    for (int k = 0; k < nk; ++k) {
        double g = 1.0;
        if (WGT) g = valid ? G[(long long)k * n + pos] : 0.0;
        double wm = 0.0;
#pragma unroll
        for (int c0 = 0; c0 < CT; c0 += RB_RC) {
            __syncthreads();                                        // the sweeps, or the round before, have read this LDS
#pragma unroll
            for (int cc = 0; cc < RB_RC; ++cc) {
                double v = valid ? fabs(x[c0 + cc]) : 0.0;
                if (WGT) v = v * g;                                 // rounded before the sum
                red[cc][pos] = v;
            }
            __syncthreads();
            for (int cc = w; cc < RB_RC; cc += nw) {               // (whole waves) wave w takes column c0 + w (+ nw ..)
                double s[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) s[i] = i < nw ? red[cc][lane + 64 * i] : 0.0;
                const double sum = rb_wave_sum(rb_tree16(s));
                if (q0 + c0 + cc < n) wm = rb_nanmax(wm, sum);
            }
        }
        __syncthreads();                                            // (WM of the column before has been read)
        if (w < nred && lane == 0) WM[w] = wm;
        __syncthreads();
        if (t == 0) {
            for (int i = 1; i < nred; ++i) wm = rb_nanmax(wm, WM[i]);
            part[(long long)k * tiles + tile] = wm;
        }
    }
}

// the maximum over a matrix's `tiles` tile maxima (order-free), then rcond
__device__ __forceinline__ void rb_gecon_fin_body(const double *part, int tiles, double anorm, double *rcond, double *ainvnm) {
    double m = 0.0;
    for (int i = 0; i < tiles; ++i) m = rb_nanmax(m, part[i]);
    *rcond = rb_rcond(m, anorm);
    if (ainvnm) *ainvnm = m;
}

// the same for one (matrix, column) of the bound
__device__ __forceinline__ void rb_ferr_fin_body(const double *part, int tiles, double xm, double *ferr) {
    double fm = 0.0;
    for (int i = 0; i < tiles; ++i) fm = rb_nanmax(fm, part[i]);
    *ferr = xm != 0.0 ? fm / xm : fm;
}

// ---- the step operator ----------------------------------------------------------------------------------------------------------------
// r_i = b_i - sum_j op(A)_ij x_j and w_i = |b_i| + sum_j |op(A)_ij| |x_j|, j ascending, every product rounded before it is added;
// thread = row, S[j * CT + c] = x_j of column c (LDS).  Rows >= n keep r = w = 0.
template <int CT>
__device__ __forceinline__ void rb_resid(int trans, const double *a, long long lda, int n, int t, bool valid, const double *S,
                                         const double *bcol, long long ldb, int nc, double (&r)[CT], double (&w)[CT]) {
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        const double bv = (valid && c < nc) ? bcol[t + (long long)c * ldb] : 0.0;
        r[c] = bv;
        w[c] = fabs(bv);
    }
    if (!valid) return;
    for (int j0 = 0; j0 < n; j0 += RB_PF) {
        double av[RB_PF];
#pragma unroll
        for (int u = 0; u < RB_PF; ++u) {
            const int j = j0 + u;
            av[u] = j < n ? (trans ? a[j + (long long)t * lda] : a[t + (long long)j * lda]) : 0.0;
        }
#pragma unroll
        for (int u = 0; u < RB_PF; ++u) {
            const int j = j0 + u;
            if (j < n) {                                            // (uniform)
                const double aa = fabs(av[u]);
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    const double xj = S[j * CT + c];
                    const double p = av[u] * xj;
                    r[c] = r[c] - p;
                    const double v = aa * fabs(xj);
                    w[c] = w[c] + v;
                }
            }
        }
    }
}

// a: the matrix; X, B, R, Wo (or null): row 0 of the matrix, column 0 of the operand; tile: which CT columns
template <int CT>
__device__ __forceinline__ void rb_residual_body(int trans, const double *a, long long lda, int n, int nrhs, const double *X, long long ldx,
                                                 const double *B, long long ldb, double *R, long long ldr, double *Wo, int tile) {
    __shared__ double S[BB_MAXN * CT];
    const int t = threadIdx.x;
    const int c0 = tile * CT, nc = nrhs - c0 < CT ? nrhs - c0 : CT;
    const bool valid = t < n;
    if (valid) {
#pragma unroll
        for (int c = 0; c < CT; ++c) S[t * CT + c] = c < nc ? X[(long long)(c0 + c) * ldx + t] : 0.0;
    }
    __syncthreads();
    double r[CT], w[CT];
    rb_resid<CT>(trans, a, lda, n, t, valid, S, B + (long long)c0 * ldb, ldb, nc, r, w);
    if (valid) {
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            if (c < nc) {
                const long long o = (long long)(c0 + c) * ldr + t;
                R[o] = r[c];
                if (Wo) Wo[o] = w[c];
            }
        }
    }
}

// ---- refinement -------------------------------------------------------------------------------------------------------------------------
// a, T: the matrix and its factors; ipiv: its pivots; B, X: row 0 of the matrix, column 0 of the operand; berr, iters (or null), XMout
// (or null): the matrix's nrhs slots; Gout (when the bound is asked for): the matrix's nrhs columns of g, n apart; tile: which CT columns
template <int CT>
__device__ __forceinline__ void rb_gerfs_body(int trans, const double *a, long long lda, const double *T, long long ldlu, int n, const int *ipiv,
                                              int nrhs, const double *B, long long ldb, double *X, long long ldx, int itmax, double *berr,
                                              int *iters, double *Gout, double *XMout, int tile) {
    __shared__ double S[BB_MAXN * CT];
    __shared__ double xs[2][32][CT];
    __shared__ int pv[BB_MAXN], map[BB_MAXN];
    __shared__ double WM[16][CT];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, nw = (int)(blockDim.x >> 6);
    const int c0 = tile * CT, nc = nrhs - c0 < CT ? nrhs - c0 : CT;
    const double *bcol = B + (long long)c0 * ldb;
    double *xcol = X + (long long)c0 * ldx;
    const bool valid = t < n;
    if (valid) {
        int p = ipiv[t] - 1;
        if (p < 0 || p >= n) p = t;                                 // (as bb_getrs_kernel: keeps every access in range)
        pv[t] = p;
    }
    __syncthreads();
    if (valid) {                                                    // the interchanges as one map (bb_getrs_kernel)
        int cpos = t;
        if (!trans) {
            for (int j = 0; j < n; ++j) { const int p = pv[j]; cpos = cpos == j ? p : (cpos == p ? j : cpos); }
            map[cpos] = t;
        } else {
            for (int j = n - 1; j >= 0; --j) { const int p = pv[j]; cpos = cpos == j ? p : (cpos == p ? j : cpos); }
            map[t] = cpos;
        }
    }
    const double eps = 0x1p-53, nz = (double)(n + 1), safe1 = nz * DBL_MIN, safe2 = safe1 / eps, nzeps = nz * eps;
    double x[CT], gq[CT], lst[CT], be_out[CT];
    int it[CT];
    bool act[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        x[c] = (valid && c < nc) ? xcol[t + (long long)c * ldx] : 0.0;
        gq[c] = 0.0;
        lst[c] = 3.0;
        be_out[c] = 0.0;
        it[c] = 0;
        act[c] = c < nc;
    }
    int count = 1;
    for (;;) {
        __syncthreads();                                            // S (and the map, the first time) is free
        if (valid) {
#pragma unroll
            for (int c = 0; c < CT; ++c) S[t * CT + c] = x[c];
        }
        __syncthreads();
        double r[CT], wv[CT];
        rb_resid<CT>(trans, a, lda, n, t, valid, S, bcol, ldb, nc, r, wv);
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            double q = 0.0;
            if (valid) {
                const double ar = fabs(r[c]);
                q = wv[c] > safe2 ? ar / wv[c] : (ar + safe1) / (wv[c] + safe1);
                const double p = nzeps * wv[c];                     // g_i = |r_i| + nz eps w_i (+ safe1 where w_i <= safe2): of the last
                double g = ar + p;                                  // residual, so only g stays live through the sweeps
                if (!(wv[c] > safe2)) g = g + safe1;
                gq[c] = g;
            }
            q = rb_wave_max(q);
            if (lane == 0) WM[w][c] = q;
        }
        __syncthreads();
        bool any = false, go[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            double be = WM[0][c];
            for (int i = 1; i < nw; ++i) be = rb_nanmax(be, WM[i][c]);
            if (act[c]) be_out[c] = be;
            go[c] = act[c] && be > eps && 2.0 * be <= lst[c] && count <= itmax;   // (false for a NaN: the column stops)
            act[c] = go[c];
            any = any || go[c];
        }
        if (!any) break;                                            // (the whole workgroup: be is the same in every thread)
        double d[CT];
        int ph = 0;
        if (!trans) {
            __syncthreads();                                        // S has been read by the residual
            if (valid) {
#pragma unroll
                for (int c = 0; c < CT; ++c) S[t * CT + c] = r[c];
            }
            __syncthreads();
#pragma unroll
            for (int c = 0; c < CT; ++c) d[c] = valid ? S[map[t] * CT + c] : 0.0;
            bb_sweep<CT, true, false, false>(T, ldlu, n, t, valid, d, xs, ph);    // L: b_i -= l_ij b_j
            bb_sweep<CT, false, true, false>(T, ldlu, n, t, valid, d, xs, ph);    // U: b_j /= u_jj, then b_i -= u_ij b_j
        } else {
#pragma unroll
            for (int c = 0; c < CT; ++c) d[c] = r[c];
            bb_sweep<CT, true, true, true>(T, ldlu, n, t, valid, d, xs, ph);      // U^T: b_j /= u_jj, then b_i -= u_ji b_j
            bb_sweep<CT, false, false, true>(T, ldlu, n, t, valid, d, xs, ph);    // L^T: b_i -= l_ji b_j
            if (valid) {                                            // (the sweeps' barriers lie between the residual's reads and this)
#pragma unroll
                for (int c = 0; c < CT; ++c) S[map[t] * CT + c] = d[c];
            }
            __syncthreads();
#pragma unroll
            for (int c = 0; c < CT; ++c) d[c] = valid ? S[t * CT + c] : 0.0;
        }
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            if (go[c]) {
                x[c] = x[c] + d[c];
                lst[c] = be_out[c];
                it[c] = count;
            }
        }
        ++count;
    }
    __syncthreads();                                                // WM has been read
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        double xm = 0.0;
        if (valid && c < nc) {
            xcol[t + (long long)c * ldx] = x[c];
            xm = fabs(x[c]);
            if (Gout) Gout[(long long)(c0 + c) * n + t] = gq[c];
        }
        xm = rb_wave_max(xm);
        if (lane == 0) WM[w][c] = xm;
    }
    __syncthreads();
    if (t < nc) {
        double xm = WM[0][t];
        for (int i = 1; i < nw; ++i) xm = rb_nanmax(xm, WM[i][t]);
        const int u = c0 + t;
        double be = 0.0;
        int its = 0;
#pragma unroll
        for (int c = 0; c < CT; ++c)
            if (c == t) { be = be_out[c]; its = it[c]; }
        berr[u] = be;
        if (iters) iters[u] = its;
        if (XMout) XMout[u] = xm;
    }
}
