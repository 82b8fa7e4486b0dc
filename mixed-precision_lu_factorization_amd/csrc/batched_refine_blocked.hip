// The expert layer for strided batches of one order n <= 1024 (mpf_lange_batched_blocked, mpf_gecon_batched_blocked,
// mpf_residual_batched_blocked, mpf_gerfs_batched_blocked; contracts in include/mpf_c.h, host side in mpf_batched.cpp, numpy restatement
// in tests/batched_refine_blocked_model.py).
//
// The contract is batched_refine.hip's with the larger limit, and so are the bits for n <= 128: nothing is an estimate, the norms of
// the inverse are formed exactly from chains that are reduced on the fly and never stored.  The shared rules:
//   tree sum   the halving tree on the terms padded with +0 to 1024 (the same as any power of two >= n): v[i] + v[i + 512], + 256, ..
//              + 1.  The terms are never negative, so the padding is exact.  With thread = index the levels 512 .. 64 pair WAVES: lane l
//              of wave w holds index 64 w + l, so those levels are a halving tree over w for every lane (through LDS), and the levels
//              32 .. 1 are an xor butterfly inside one wave.
//   maxima     order-free, a NaN stays: rb_nanmax.
//   fusion     every multiply-subtract and multiply-add is unfused (the file is compiled with -ffp-contract=off).
// The chains are batched_blocked_body.h's: bb_sweep (mpf_getrs_batched_blocked's) and bb_inv_sweep (mpf_getri_batched_blocked's, the
// trans = 0 chains from unit vectors), the same functions that batched_blocked.hip's and vbatched_blocked.hip's kernels call.
//   rb_lange_kernel            one workgroup per matrix.  '1': a wave per column, lane l takes rows l + 64 m (coalesced), the tree over m
//                              in registers, then the butterfly.  'I': thread = row (coalesced along every column); the row's tree runs
//                              over the columns in BIT-REVERSED order, where the halving tree is the pairwise tree of neighbours: sixteen
//                              columns at a time in registers, the levels above on a six-entry stack.  'M': thread = row.
//   rb_chain_kernel<CT, TR, WGT>  one workgroup per (matrix, tile of CT = 16 unit vectors), thread = row.  TR = 0: the trans = 0 chains
//                              from e_q by bb_inv_sweep (the forward sweep starts at the tile's block).  TR = 1: the trans = 1 chains by
//                              rb_inv_sweep, bb_inv_sweep's scheme with the factor read transposed and the division in the forward
//                              sweep (bb_sweep gives the same bits at twice the time: eight chains per workgroup and a division per
//                              lane and step).  Then, instead of a store, a tree over the row index per column -- its terms go through
//                              the sweeps' own LDS, two columns a round -- and the tile's maximum.
//                              WGT = 0 (gecon): |x|.  WGT = 1 (ferr): |y_k| g_k for every right-hand-side column, the chains formed
//                              once; for TR = 1 the chain's result goes through its interchanges, so the term of row t enters the tree at
//                              position map[t].  For TR = 0 the interchanges only say WHICH e_i a chain belongs to, and the maximum over
//                              all i does not ask.  The tile maxima go to a partial array; rb_gecon_fin_kernel / rb_ferr_fin_kernel
//                              take the maximum over the tiles (order-free) and finish.
//   rb_residual_kernel<CT>     one workgroup per (matrix, tile of CT columns), thread = row, x of the tile in LDS, j ascending.
//                              trans = 1: a thread reads its own column of A eight consecutive doubles at a time (whole 64-byte
//                              segments, every byte fetched is used; DESIGN 4.25 says why no LDS stage).
//   rb_gerfs_kernel<CT>        the fused form: one workgroup per (matrix, tile of CT columns) runs residual, berr, rule, the two sweeps
//                              on a copy of r, x += dx, masked per column until every column of the tile has stopped; the last r and w
//                              leave as g for the bound, max |x| beside them.
#include "batched_blocked_body.h"
#include <float.h>

constexpr int RB_RC = 2;       // columns per round of rb_chain_kernel's tree (LDS: RB_RC x 1024 doubles, inside the sweeps' ds)
constexpr int RB_PF = 8;       // elements of a row of op(A) in flight in the residual

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
// mode 0: max_j tree_i |a_ij|; 1: max_i tree_j |a_ij|; 2: max |a_ij|.  blockDim.x >= n in whole waves; blockIdx.x = matrix
__global__ __launch_bounds__(1024) void rb_lange_kernel(int mode, const double *A, long long lda, long long strideA, int n, double *out) {
    __shared__ double WM[16];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, nw = (int)(blockDim.x >> 6);
    const long long b = blockIdx.x;
    const double *a = A + b * strideA;
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
    if (t == 0) out[b] = m;
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

// blockDim.x = n rounded up to whole waves; blockIdx.x = tile of CT unit vectors, blockIdx.y = matrix.
// WGT = 0: part[b * tiles + tile] = max over the tile's columns of tree_t |x_t|; a zero on U's diagonal: +Inf before any arithmetic.
// WGT = 1: part[(b * nrhs + k) * tiles + tile] = max over the tile's columns of tree_p |y_p| g_p, g = G + (b * nrhs + k) * n.
// The tree's terms go through the sweeps' LDS (ds: RB_RC columns of up to 1024 terms), so the kernel keeps bb_getri_kernel's footprint
// and its workgroups per CU.
template <int CT, bool TR, bool WGT>
__global__ __launch_bounds__(1024) void rb_chain_kernel(const double *LU, long long ldlu, long long strideLU, int n, const int *ipiv,
                                                        long long strideP, const double *G, int nrhs, double *part) {
    static_assert(CT % RB_RC == 0, "the tree takes RB_RC columns per round");
    static_assert(RB_RC * BB_MAXN <= 2 * 32 * 33, "the tree's terms fit the sweeps' ds");
    __shared__ double xs[2][32][CT + 1], ds[2][32][33];
    __shared__ int map[(TR && WGT) ? BB_MAXN : 1];
    __shared__ double WM[16];
    __shared__ int zflag;
    double(*red)[BB_MAXN] = (double(*)[BB_MAXN]) & ds[0][0][0];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, nw = (int)(blockDim.x >> 6);
    const long long b = blockIdx.y;
    const int tiles = (int)gridDim.x, q0 = (int)blockIdx.x * CT;
    const double *T = LU + b * strideLU;
    const bool valid = t < n;
    if (!WGT) {
        if (t == 0) zflag = 0;
        __syncthreads();
        if (valid && T[t + (long long)t * ldlu] == 0.0) zflag = 1;   // (every writer stores the same value)
        __syncthreads();
        if (zflag) {                                                // (the whole workgroup) no inverse: +Inf, rcond 0
            if (t == 0) part[b * tiles + blockIdx.x] = __longlong_as_double(0x7FF0000000000000ll);
            return;
        }
    }
    if (TR && WGT) {                                                // the trans = 1 chain's interchanges: its row t ends at row map[t] (bb_getrs_kernel)
        int *pv = (int *)&ds[0][0][0];
        if (valid) {
            int p = ipiv[b * strideP + t] - 1;
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
        if (WGT) g = valid ? G[(b * nrhs + k) * n + pos] : 0.0;
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
            part[(WGT ? b * nrhs + k : b) * tiles + blockIdx.x] = wm;
        }
    }
}

__global__ __launch_bounds__(256) void rb_gecon_fin_kernel(const double *part, int tiles, long long batch, const double *anorm, double *rcond,
                                                           double *ainvnm) {
    const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
    if (b >= batch) return;
    double m = 0.0;
    for (int i = 0; i < tiles; ++i) m = rb_nanmax(m, part[b * tiles + i]);
    rcond[b] = rb_rcond(m, anorm[b]);
    if (ainvnm) ainvnm[b] = m;
}

__global__ __launch_bounds__(256) void rb_ferr_fin_kernel(const double *part, int tiles, long long units, const double *xmax, double *ferr) {
    const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
    if (u >= units) return;
    double fm = 0.0;
    for (int i = 0; i < tiles; ++i) fm = rb_nanmax(fm, part[u * tiles + i]);
    const double xm = xmax[u];
    ferr[u] = xm != 0.0 ? fm / xm : fm;
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

// blockDim.x = n rounded up to whole waves; blockIdx.x = tile of CT columns, blockIdx.y = matrix
template <int CT>
__global__ __launch_bounds__(1024) void rb_residual_kernel(int trans, const double *A, long long lda, long long strideA, int n, int nrhs,
                                                           const double *X, long long ldx, long long strideX, const double *B, long long ldb,
                                                           long long strideB, double *R, long long ldr, long long strideR, double *Wo) {
    __shared__ double S[BB_MAXN * CT];
    const int t = threadIdx.x;
    const long long b = blockIdx.y;
    const int c0 = (int)blockIdx.x * CT, nc = nrhs - c0 < CT ? nrhs - c0 : CT;
    const bool valid = t < n;
    if (valid) {
#pragma unroll
        for (int c = 0; c < CT; ++c) S[t * CT + c] = c < nc ? X[b * strideX + (long long)(c0 + c) * ldx + t] : 0.0;
    }
    __syncthreads();
    double r[CT], w[CT];
    rb_resid<CT>(trans, A + b * strideA, lda, n, t, valid, S, B + b * strideB + (long long)c0 * ldb, ldb, nc, r, w);
    if (valid) {
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            if (c < nc) {
                const long long o = b * strideR + (long long)(c0 + c) * ldr + t;
                R[o] = r[c];
                if (Wo) Wo[o] = w[c];
            }
        }
    }
}

// ---- refinement -------------------------------------------------------------------------------------------------------------------------
// blockDim.x = n rounded up to whole waves; blockIdx.x = tile of CT columns, blockIdx.y = matrix.  Gout (when the bound is asked for):
// g of column (b, k) at (b * nrhs + k) * n; XMout: max |x| of the column at b * nrhs + k.
template <int CT>
__global__ __launch_bounds__(1024) void rb_gerfs_kernel(int trans, const double *A, long long lda, long long strideA, const double *LU,
                                                        long long ldlu, long long strideLU, int n, const int *ipiv, long long strideP, int nrhs,
                                                        const double *B, long long ldb, long long strideB, double *X, long long ldx,
                                                        long long strideX, int itmax, double *berr, int *iters, double *Gout, double *XMout) {
    __shared__ double S[BB_MAXN * CT];
    __shared__ double xs[2][32][CT];
    __shared__ int pv[BB_MAXN], map[BB_MAXN];
    __shared__ double WM[16][CT];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, nw = (int)(blockDim.x >> 6);
    const long long b = blockIdx.y;
    const int c0 = (int)blockIdx.x * CT, nc = nrhs - c0 < CT ? nrhs - c0 : CT;
    const double *T = LU + b * strideLU, *a = A + b * strideA, *bcol = B + b * strideB + (long long)c0 * ldb;
    double *xcol = X + b * strideX + (long long)c0 * ldx;
    const bool valid = t < n;
    if (valid) {
        int p = ipiv[b * strideP + t] - 1;
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
            if (Gout) Gout[(b * nrhs + c0 + c) * n + t] = gq[c];
        }
        xm = rb_wave_max(xm);
        if (lane == 0) WM[w][c] = xm;
    }
    __syncthreads();
    if (t < nc) {
        double xm = WM[0][t];
        for (int i = 1; i < nw; ++i) xm = rb_nanmax(xm, WM[i][t]);
        const long long u = b * nrhs + c0 + t;
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

// ---- launchers: batch <= BB_MAX_LAUNCH matrices (the host splits longer batches) ---------------------------------------------------------
static unsigned rb_threads(int n) { return (unsigned)((n + 63) / 64 * 64); }

int launch_lange_batched_blocked(mpf_ctx *c, int mode, const double *A, int64_t lda, int64_t strideA, int n, int64_t batch, double *out) {
    if (n < 1 || batch < 1) return 0;
    if (n > BB_MAXN || batch > BB_MAX_LAUNCH || mode < 0 || mode > 2) { c->err = "launch_lange_batched_blocked: argument out of range"; return -1; }
    unsigned th = rb_threads(n);
    if (mode == 0 && th < 256) th = 256;                            // (a wave per column: more waves than the rows need)
    rb_lange_kernel<<<(unsigned)batch, th, 0, c->stream>>>(mode, A, lda, strideA, n, out);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

int launch_gecon_batched_blocked(mpf_ctx *c, int inf, const double *LU, int64_t ldlu, int64_t strideLU, int n, int64_t batch,
                                 const double *anorm, double *rcond, double *ainvnm) {
    if (n < 1 || batch < 1) return 0;
    if (n > BB_MAXN || batch > BB_MAX_LAUNCH) { c->err = "launch_gecon_batched_blocked: size out of range"; return -1; }
    const int ct = 16, tiles = (n + ct - 1) / ct;
    MPF_HIP_TRY(c, c->rb_part.grow(batch * tiles));
    const dim3 g((unsigned)tiles, (unsigned)batch);
    if (inf) rb_chain_kernel<16, true, false><<<g, rb_threads(n), 0, c->stream>>>(LU, ldlu, strideLU, n, nullptr, 0, nullptr, 0, c->rb_part);
    else rb_chain_kernel<16, false, false><<<g, rb_threads(n), 0, c->stream>>>(LU, ldlu, strideLU, n, nullptr, 0, nullptr, 0, c->rb_part);
    rb_gecon_fin_kernel<<<(unsigned)((batch + 255) / 256), 256, 0, c->stream>>>(c->rb_part, tiles, batch, anorm, rcond, ainvnm);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

int launch_residual_batched_blocked(mpf_ctx *c, int trans, const double *A, int64_t lda, int64_t strideA, int n, int64_t batch, int nrhs,
                                    const double *X, int64_t ldx, int64_t strideX, const double *B, int64_t ldb, int64_t strideB, double *R,
                                    int64_t ldr, int64_t strideR, double *W) {
    if (n < 1 || batch < 1 || nrhs < 1) return 0;
    if (n > BB_MAXN || batch > BB_MAX_LAUNCH) { c->err = "launch_residual_batched_blocked: size out of range"; return -1; }
    // the column tiles of one matrix are a grid's first dimension; a tile of one column below four right-hand sides
    if (nrhs < 4) {
        const dim3 g((unsigned)nrhs, (unsigned)batch);
        rb_residual_kernel<1><<<g, rb_threads(n), 0, c->stream>>>(trans, A, lda, strideA, n, nrhs, X, ldx, strideX, B, ldb, strideB, R, ldr,
                                                                  strideR, W);
    } else {
        const dim3 g((unsigned)((nrhs + 3) / 4), (unsigned)batch);
        rb_residual_kernel<4><<<g, rb_threads(n), 0, c->stream>>>(trans, A, lda, strideA, n, nrhs, X, ldx, strideX, B, ldb, strideB, R, ldr,
                                                                  strideR, W);
    }
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

int launch_gerfs_batched_blocked(mpf_ctx *c, int trans, const double *A, int64_t lda, int64_t strideA, const double *LU, int64_t ldlu,
                                 int64_t strideLU, int n, int64_t batch, const int *ipiv, int64_t strideP, int nrhs, const double *B,
                                 int64_t ldb, int64_t strideB, double *X, int64_t ldx, int64_t strideX, int itmax, double *ferr, double *berr,
                                 int *iters) {
    if (n < 1 || batch < 1 || nrhs < 1) return 0;
    if (n > BB_MAXN || batch > BB_MAX_LAUNCH) { c->err = "launch_gerfs_batched_blocked: size out of range"; return -1; }
    const int64_t units = batch * nrhs;
    // the other trans's chains, 16 per workgroup: trans = 1 wants the trans = 0 chains, trans = 0 the trans = 1 chains
    const int ct = 16, tiles = (n + ct - 1) / ct;
    double *G = nullptr, *XM = nullptr;
    if (ferr) {
        MPF_HIP_TRY(c, c->rb_g.grow(units * n));
        MPF_HIP_TRY(c, c->rb_xm.grow(units));
        MPF_HIP_TRY(c, c->rb_part.grow(units * tiles));
        G = c->rb_g;
        XM = c->rb_xm;
    }
    const unsigned th = rb_threads(n);
    if (nrhs < 4) {
        const dim3 g((unsigned)nrhs, (unsigned)batch);
        rb_gerfs_kernel<1><<<g, th, 0, c->stream>>>(trans, A, lda, strideA, LU, ldlu, strideLU, n, ipiv, strideP, nrhs, B, ldb, strideB, X, ldx,
                                                    strideX, itmax, berr, iters, G, XM);
    } else {
        const dim3 g((unsigned)((nrhs + 3) / 4), (unsigned)batch);
        rb_gerfs_kernel<4><<<g, th, 0, c->stream>>>(trans, A, lda, strideA, LU, ldlu, strideLU, n, ipiv, strideP, nrhs, B, ldb, strideB, X, ldx,
                                                    strideX, itmax, berr, iters, G, XM);
    }
    if (ferr) {
        const dim3 g((unsigned)tiles, (unsigned)batch);
        if (trans) rb_chain_kernel<16, false, true><<<g, th, 0, c->stream>>>(LU, ldlu, strideLU, n, ipiv, strideP, G, nrhs, c->rb_part);
        else rb_chain_kernel<16, true, true><<<g, th, 0, c->stream>>>(LU, ldlu, strideLU, n, ipiv, strideP, G, nrhs, c->rb_part);
        rb_ferr_fin_kernel<<<(unsigned)((units + 255) / 256), 256, 0, c->stream>>>(c->rb_part, tiles, units, XM, ferr);
    }
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}
