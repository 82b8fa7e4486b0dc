// The expert layer for many matrices of DIFFERENT orders up to 1024: norms, exact reciprocal condition numbers, the residual step
// operator and dgerfs's refinement with berr and an exact ferr on a descriptor of either kind (mpf_lange_vbatched, mpf_gecon_vbatched,
// mpf_residual_vbatched, mpf_gerfs_vbatched; contracts in include/mpf_c.h, host side in mpf_batched.cpp, the launch groups in
// vbatch_plan.h: refine_chunks).
//
// The arithmetic is batched_refine_blocked_body.h's: the very bodies that batched_refine_blocked.hip's fixed-size kernels call, so a
// matrix's bits are those of the fixed-size blocked expert entry on that matrix alone (and, for n <= 128, of the small expert entry).
// What is here is vbatched_blocked.hip's fetch (bbv_fetch, batched_blocked_body.h): a workgroup takes entry i = blockIdx.y (the norms:
// blockIdx.x) of a list ordered by n, reads b = idx[i], then n[b], off[b], ld[b], offv[b], and calls the body with its own tile
// blockIdx.x.  Grids and blocks are sized for the largest matrix of the launch; a workgroup whose tile lies outside its own matrix
// leaves as a whole before its first barrier, and every load in the bodies is predicated on the matrix's own n.  Every launch is an
// ordinary launch; nothing waits for another workgroup.
//   vectors     X, B, R, W are tall total_n x nrhs matrices, matrix b's rows at offv[b] (mpf_getrs_vbatched's B); the pivots at offv[b].
//   outputs     per matrix at b, per column at b * nrhs + c.
//   workspace   laid out by LIST POSITION inside the launch's chunk, from the plan's prefix sums (row[i], tile[i]: orders and tiles of
//               the entries before i): the tile maxima of entry i at (tile[i] - tile0) * nk, nk per-column groups of the matrix's OWN
//               ceil(n / 16) tiles; g at (row[i] - row0) * nrhs, nrhs columns n apart; max |x| at i * nrhs.  The finishing kernels read
//               a matrix's own tiles only, and every tile inside a matrix is written by its workgroup, so no slot that is read stays
//               unwritten.
#include "batched_refine_blocked_body.h"
#include "vbatch_plan.h"

static_assert(RB_CT == vbatch::REFINE_CT, "the plan counts a matrix's tiles by the chain kernel's tile");

namespace {

// blockDim.x = the launch's largest n rounded up to whole waves (at least 256 for the '1' norm); blockIdx.x = list entry
__global__ __launch_bounds__(1024) void rbv_lange_kernel(int mode, const double *A, BtRagged v, const int *idx, double *out) {
    const bbv_entry e = bbv_fetch(v, idx, blockIdx.x);
    rb_lange_body(mode, A + e.off, e.ld, e.n, out + e.b);
}

// blockDim.x = the launch's largest n rounded up to whole waves; blockIdx.x = tile of CT unit vectors, blockIdx.y = list entry;
// row, tile: the plan's prefix sums from this launch's first entry on, row0 / tile0 their values there
template <int CT, bool TR, bool WGT>
__global__ __launch_bounds__(1024) void rbv_chain_kernel(const double *LU, BtRagged v, const int *idx, const int *ipiv, const long long *row,
                                                         const long long *tile, long long row0, long long tile0, const double *G, int nrhs,
                                                         double *part) {
    const bbv_entry e = bbv_fetch(v, idx, blockIdx.y);
    if ((int)blockIdx.x * CT >= e.n) return;                        // (the whole workgroup: the tile lies outside this matrix)
    const int tiles = (e.n + CT - 1) / CT;
    const long long nk = WGT ? nrhs : 1;
    rb_chain_body<CT, TR, WGT>(LU + e.off, e.ld, e.n, (TR && WGT) ? ipiv + e.offv : nullptr, WGT ? G + (row[blockIdx.y] - row0) * nrhs : nullptr, nrhs,
                               part + (tile[blockIdx.y] - tile0) * nk, tiles, (int)blockIdx.x);
}

__global__ __launch_bounds__(256) void rbv_gecon_fin_kernel(const double *part, BtRagged v, const int *idx, const long long *tile, long long tile0,
                                                            long long count, const double *anorm, double *rcond, double *ainvnm) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int b = idx[i], n = v.n[b];
    rb_gecon_fin_body(part + (tile[i] - tile0), (n + RB_CT - 1) / RB_CT, anorm[b], rcond + b, ainvnm ? ainvnm + b : nullptr);
}

// one thread per (list entry, column)
__global__ __launch_bounds__(256) void rbv_ferr_fin_kernel(const double *part, BtRagged v, const int *idx, const long long *tile, long long tile0,
                                                           long long count, int nrhs, const double *xmax, double *ferr) {
    const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
    if (u >= count * nrhs) return;
    const long long i = u / nrhs, k = u % nrhs;
    const int b = idx[i], n = v.n[b], tiles = (n + RB_CT - 1) / RB_CT;
    rb_ferr_fin_body(part + (tile[i] - tile0) * nrhs + k * tiles, tiles, xmax[u], ferr + (long long)b * nrhs + k);
}

// blockDim.x as above; blockIdx.x = tile of CT columns, blockIdx.y = list entry
template <int CT>
__global__ __launch_bounds__(1024) void rbv_residual_kernel(int trans, const double *A, BtRagged v, const int *idx, int nrhs, const double *X,
                                                            long long ldx, const double *B, long long ldb, double *R, long long ldr, double *Wo) {
    const bbv_entry e = bbv_fetch(v, idx, blockIdx.y);
    rb_residual_body<CT>(trans, A + e.off, e.ld, e.n, nrhs, X + e.offv, ldx, B + e.offv, ldb, R + e.offv, ldr, Wo ? Wo + e.offv : nullptr,
                         (int)blockIdx.x);
}

template <int CT>
__global__ __launch_bounds__(1024) void rbv_gerfs_kernel(int trans, const double *A, const double *LU, BtRagged v, const int *idx, const int *ipiv,
                                                         int nrhs, const double *B, long long ldb, double *X, long long ldx, int itmax, double *berr,
                                                         int *iters, const long long *row, long long row0, double *Gout, double *XMout) {
    const bbv_entry e = bbv_fetch(v, idx, blockIdx.y);
    const long long u0 = (long long)e.b * nrhs;
    rb_gerfs_body<CT>(trans, A + e.off, e.ld, LU + e.off, e.ld, e.n, ipiv + e.offv, nrhs, B + e.offv, ldb, X + e.offv, ldx, itmax, berr + u0,
                      iters ? iters + u0 : nullptr, Gout ? Gout + (row[blockIdx.y] - row0) * nrhs : nullptr,
                      XMout ? XMout + (long long)blockIdx.y * nrhs : nullptr, (int)blockIdx.x);
}

// the matrices of order 0: whichever outputs are given.  norm 0; rcond 1 and ainvnm 0 (dgecon's quick return); berr = ferr = 0 and
// iters = 0 for each of their columns.  One thread per matrix
__global__ __launch_bounds__(256) void rbv_empty_kernel(const int *idx, long long count, int nrhs, double *norm, double *rcond, double *ainvnm,
                                                        double *berr, double *ferr, int *iters) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const long long b = idx[i];
    if (norm) norm[b] = 0.0;
    if (rcond) rcond[b] = 1.0;
    if (ainvnm) ainvnm[b] = 0.0;
    for (int k = 0; k < nrhs; ++k) {
        if (berr) berr[b * nrhs + k] = 0.0;
        if (ferr) ferr[b * nrhs + k] = 0.0;
        if (iters) iters[b * nrhs + k] = 0;
    }
}

bool rbv_range(mpf_ctx *c, const char *who, int64_t count, int nmax) {
    const bool ok = count <= BB_MAX_LAUNCH && nmax >= 1 && nmax <= BB_MAXN;
    if (!ok) c->err = std::string(who) + ": size out of range";
    return ok;
}
unsigned rbv_threads(int nmax) { return (unsigned)((nmax + 63) / 64 * 64); }

} // namespace

// ---- launchers: count <= BB_MAX_LAUNCH entries of a list ordered by n, nmax the largest order among them ----------------------------------
int launch_lange_vbatched(mpf_ctx *c, const BtRagged &v, const int32_t *idx, int64_t count, int nmax, int mode, const double *A, double *out) {
    if (count < 1) return 0;
    if (!rbv_range(c, "launch_lange_vbatched", count, nmax) || mode < 0 || mode > 2) { c->err = "launch_lange_vbatched: argument out of range"; return -1; }
    unsigned th = rbv_threads(nmax);
    if (mode == 0 && th < 256) th = 256;                            // launch_lange_batched_blocked's rule, per launch
    rbv_lange_kernel<<<(unsigned)count, th, 0, c->stream>>>(mode, A, v, idx, out);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

int launch_gecon_vbatched(mpf_ctx *c, const BtRagged &v, const int32_t *idx, const RbvWork &w, int64_t count, int nmax, int inf, const double *LU,
                          const double *anorm, double *rcond, double *ainvnm) {
    if (count < 1) return 0;
    if (!rbv_range(c, "launch_gecon_vbatched", count, nmax)) return -1;
    const dim3 g((unsigned)((nmax + RB_CT - 1) / RB_CT), (unsigned)count);
    const long long *row = (const long long *)w.row, *tile = (const long long *)w.tile;
    if (inf) rbv_chain_kernel<RB_CT, true, false><<<g, rbv_threads(nmax), 0, c->stream>>>(LU, v, idx, nullptr, row, tile, w.row0, w.tile0, nullptr, 0, w.part);
    else rbv_chain_kernel<RB_CT, false, false><<<g, rbv_threads(nmax), 0, c->stream>>>(LU, v, idx, nullptr, row, tile, w.row0, w.tile0, nullptr, 0, w.part);
    rbv_gecon_fin_kernel<<<(unsigned)((count + 255) / 256), 256, 0, c->stream>>>(w.part, v, idx, tile, w.tile0, count, anorm, rcond, ainvnm);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

int launch_residual_vbatched(mpf_ctx *c, const BtRagged &v, const int32_t *idx, int64_t count, int nmax, int trans, const double *A, int nrhs,
                             const double *X, int64_t ldx, const double *B, int64_t ldb, double *R, int64_t ldr, double *W) {
    if (count < 1 || nrhs < 1) return 0;
    if (!rbv_range(c, "launch_residual_vbatched", count, nmax)) return -1;
    // launch_residual_batched_blocked's tiles: one column below four right-hand sides, four from there
    if (nrhs < 4) {
        const dim3 g((unsigned)nrhs, (unsigned)count);
        rbv_residual_kernel<1><<<g, rbv_threads(nmax), 0, c->stream>>>(trans, A, v, idx, nrhs, X, ldx, B, ldb, R, ldr, W);
    } else {
        const dim3 g((unsigned)((nrhs + 3) / 4), (unsigned)count);
        rbv_residual_kernel<4><<<g, rbv_threads(nmax), 0, c->stream>>>(trans, A, v, idx, nrhs, X, ldx, B, ldb, R, ldr, W);
    }
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

// ferr != null: w.g holds nrhs doubles per row of the chunk, w.xm nrhs per entry, w.part nrhs per tile of the chunk
int launch_gerfs_vbatched(mpf_ctx *c, const BtRagged &v, const int32_t *idx, const RbvWork &w, int64_t count, int nmax, int trans, const double *A,
                          const double *LU, const int *ipiv, int nrhs, const double *B, int64_t ldb, double *X, int64_t ldx, int itmax,
                          double *ferr, double *berr, int *iters) {
    if (count < 1 || nrhs < 1) return 0;
    if (!rbv_range(c, "launch_gerfs_vbatched", count, nmax)) return -1;
    const unsigned th = rbv_threads(nmax);
    const long long *row = (const long long *)w.row, *tile = (const long long *)w.tile;
    double *G = ferr ? w.g : nullptr, *XM = ferr ? w.xm : nullptr;
    if (nrhs < 4) {
        const dim3 g((unsigned)nrhs, (unsigned)count);
        rbv_gerfs_kernel<1><<<g, th, 0, c->stream>>>(trans, A, LU, v, idx, ipiv, nrhs, B, ldb, X, ldx, itmax, berr, iters, row, w.row0, G, XM);
    } else {
        const dim3 g((unsigned)((nrhs + 3) / 4), (unsigned)count);
        rbv_gerfs_kernel<4><<<g, th, 0, c->stream>>>(trans, A, LU, v, idx, ipiv, nrhs, B, ldb, X, ldx, itmax, berr, iters, row, w.row0, G, XM);
    }
    if (ferr) {
        // the other trans's chains, 16 per workgroup: trans = 1 wants the trans = 0 chains, trans = 0 the trans = 1 chains
        const dim3 g((unsigned)((nmax + RB_CT - 1) / RB_CT), (unsigned)count);
        if (trans) rbv_chain_kernel<RB_CT, false, true><<<g, th, 0, c->stream>>>(LU, v, idx, ipiv, row, tile, w.row0, w.tile0, G, nrhs, w.part);
        else rbv_chain_kernel<RB_CT, true, true><<<g, th, 0, c->stream>>>(LU, v, idx, ipiv, row, tile, w.row0, w.tile0, G, nrhs, w.part);
        const int64_t units = count * nrhs;
        rbv_ferr_fin_kernel<<<(unsigned)((units + 255) / 256), 256, 0, c->stream>>>(w.part, v, idx, tile, w.tile0, count, nrhs, XM, ferr);
    }
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

int launch_refine_vbatched_empty(mpf_ctx *c, const int32_t *idx, int64_t count, int nrhs, double *norm, double *rcond, double *ainvnm,
                                 double *berr, double *ferr, int *iters) {
    if (count < 1) return 0;
    if (count > BT_MAX_LAUNCH) { c->err = "launch_refine_vbatched_empty: size out of range"; return -1; }
    rbv_empty_kernel<<<(unsigned)((count + 255) / 256), 256, 0, c->stream>>>(idx, count, nrhs, norm, rcond, ainvnm, berr, ferr, iters);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}
