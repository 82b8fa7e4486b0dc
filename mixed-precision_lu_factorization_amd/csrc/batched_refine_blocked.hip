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
// The arithmetic is batched_refine_blocked_body.h's, shared with the ragged kernels of vbatched_refine.hip.  What is here
// is where a workgroup stands in a strided launch: its matrix (blockIdx.y, for the norms blockIdx.x), the bases b * stride, its tile.
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
#include "batched_refine_blocked_body.h"

// ---- norms ----------------------------------------------------------------------------------------------------------------------------
// blockDim.x >= n in whole waves; blockIdx.x = matrix
__global__ __launch_bounds__(1024) void rb_lange_kernel(int mode, const double *A, long long lda, long long strideA, int n, double *out) {
    const long long b = blockIdx.x;
    rb_lange_body(mode, A + b * strideA, lda, n, out + b);
}

// ---- chains from unit vectors, reduced ----------------------------------------------------------------------------------------------------
// blockDim.x = n rounded up to whole waves; blockIdx.x = tile of CT unit vectors, blockIdx.y = matrix.
// WGT = 0: part[b * tiles + tile]; WGT = 1: part[(b * nrhs + k) * tiles + tile], g = G + (b * nrhs + k) * n.
template <int CT, bool TR, bool WGT>
__global__ __launch_bounds__(1024) void rb_chain_kernel(const double *LU, long long ldlu, long long strideLU, int n, const int *ipiv,
                                                        long long strideP, const double *G, int nrhs, double *part) {
    const long long b = blockIdx.y;
    const int tiles = (int)gridDim.x;
    rb_chain_body<CT, TR, WGT>(LU + b * strideLU, ldlu, n, (TR && WGT) ? ipiv + b * strideP : nullptr, WGT ? G + b * nrhs * n : nullptr, nrhs,
                               part + (WGT ? b * nrhs : b) * tiles, tiles, (int)blockIdx.x);
}

__global__ __launch_bounds__(256) void rb_gecon_fin_kernel(const double *part, int tiles, long long batch, const double *anorm, double *rcond,
                                                           double *ainvnm) {
    const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
    if (b >= batch) return;
    rb_gecon_fin_body(part + b * tiles, tiles, anorm[b], rcond + b, ainvnm ? ainvnm + b : nullptr);
}

__global__ __launch_bounds__(256) void rb_ferr_fin_kernel(const double *part, int tiles, long long units, const double *xmax, double *ferr) {
    const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
    if (u >= units) return;
    rb_ferr_fin_body(part + u * tiles, tiles, xmax[u], ferr + u);
}

// ---- the step operator ----------------------------------------------------------------------------------------------------------------
// blockDim.x = n rounded up to whole waves; blockIdx.x = tile of CT columns, blockIdx.y = matrix
template <int CT>
__global__ __launch_bounds__(1024) void rb_residual_kernel(int trans, const double *A, long long lda, long long strideA, int n, int nrhs,
                                                           const double *X, long long ldx, long long strideX, const double *B, long long ldb,
                                                           long long strideB, double *R, long long ldr, long long strideR, double *Wo) {
    const long long b = blockIdx.y;
    rb_residual_body<CT>(trans, A + b * strideA, lda, n, nrhs, X + b * strideX, ldx, B + b * strideB, ldb, R + b * strideR, ldr,
                         Wo ? Wo + b * strideR : nullptr, (int)blockIdx.x);
}

// ---- refinement -------------------------------------------------------------------------------------------------------------------------
// blockDim.x = n rounded up to whole waves; blockIdx.x = tile of CT columns, blockIdx.y = matrix.  Gout (when the bound is asked for):
// g of column (b, k) at (b * nrhs + k) * n; XMout: max |x| of the column at b * nrhs + k.
template <int CT>
__global__ __launch_bounds__(1024) void rb_gerfs_kernel(int trans, const double *A, long long lda, long long strideA, const double *LU,
                                                        long long ldlu, long long strideLU, int n, const int *ipiv, long long strideP, int nrhs,
                                                        const double *B, long long ldb, long long strideB, double *X, long long ldx,
                                                        long long strideX, int itmax, double *berr, int *iters, double *Gout, double *XMout) {
    const long long b = blockIdx.y;
    rb_gerfs_body<CT>(trans, A + b * strideA, lda, LU + b * strideLU, ldlu, n, ipiv + b * strideP, nrhs, B + b * strideB, ldb,
                      X + b * strideX, ldx, itmax, berr + b * nrhs, iters ? iters + b * nrhs : nullptr, Gout ? Gout + b * nrhs * n : nullptr,
                      XMout ? XMout + b * nrhs : nullptr, (int)blockIdx.x);
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
