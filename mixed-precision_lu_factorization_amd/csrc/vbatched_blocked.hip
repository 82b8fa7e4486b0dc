// Blocked LU, solve, inverse and determinant of many matrices of DIFFERENT orders up to 1024: the large list of a descriptor made by
// mpf_vbatch_create_blocked (contracts in include/mpf_c.h, descriptor and host side in mpf_batched.cpp, the host plan and the per-step
// schedule in vbatch_plan.h).
//
// The arithmetic is batched_blocked_body.h's: the very bodies that batched_blocked.hip's fixed-size kernels call, so a matrix's bits
// are those of the fixed-size blocked entry on that matrix alone.  What is new here is vbatched.hip's fetch: a workgroup
// takes entry i = blockIdx.y (the panel and the determinant: blockIdx.x) of a list ordered by n, reads the matrix's index b = idx[i],
// then n[b], off[b], ld[b] and offv[b], and calls the body with its own work item blockIdx.x.  Grids and blocks are sized for the
// largest matrix of the launch; a body leaves as a whole when its item lies outside its own matrix.  The factorization launches each
// panel step only over the suffix of the list whose matrices are still active (n > j0).  Every launch is an ordinary launch; nothing
// waits for another workgroup.
#include "batched_blocked_body.h"

namespace {

// (bbv_fetch: batched_blocked_body.h, shared with vbatched_refine.hip)
// blockDim.x = the launch's largest row count n - j0 rounded up to whole waves (<= 1024); blockIdx.x = list entry
template <int NB, bool FUSED>
__global__ __launch_bounds__(1024) void bbv_panel_kernel(double *A, BtRagged v, const int *idx, int j0, int *ipiv, int *info) {
    const bbv_entry e = bbv_fetch(v, idx, blockIdx.x);
    bb_panel_body<NB, FUSED>(A + e.off, e.ld, e.n, j0, ipiv + e.offv, info ? info + e.b : nullptr);
}

// blockIdx.x = column chunk, blockIdx.y = list entry
template <int NB, bool FUSED>
__global__ __launch_bounds__(BB_RT) void bbv_rowblk_kernel(double *A, BtRagged v, const int *idx, int j0, const int *ipiv) {
    const bbv_entry e = bbv_fetch(v, idx, blockIdx.y);
    bb_rowblk_body<NB, FUSED>(A + e.off, e.ld, e.n, j0, ipiv + e.offv, (int)blockIdx.x);
}

// blockIdx.x = 64 x 64 tile of C, blockIdx.y = list entry
template <int NB>
__global__ __launch_bounds__(256) void bbv_update_mfma_kernel(double *A, BtRagged v, const int *idx, int j0) {
    const bbv_entry e = bbv_fetch(v, idx, blockIdx.y);
    bb_update_mfma_body<NB>(A + e.off, e.ld, e.n, j0, (int)blockIdx.x);
}

template <int NB, bool FUSED>
__global__ __launch_bounds__(256) void bbv_update_valu_kernel(double *A, BtRagged v, const int *idx, int j0) {
    const bbv_entry e = bbv_fetch(v, idx, blockIdx.y);
    bb_update_valu_body<NB, FUSED>(A + e.off, e.ld, e.n, j0, (int)blockIdx.x);
}

// blockDim.x = the list's largest n rounded up to whole waves; blockIdx.x = tile of CT columns of B, blockIdx.y = list entry
template <int CT>
__global__ __launch_bounds__(1024) void bbv_getrs_kernel(int trans, const double *LU, BtRagged v, const int *idx, const int *ipiv, int nrhs,
                                                         double *B, long long ldb) {
    const bbv_entry e = bbv_fetch(v, idx, blockIdx.y);
    bb_getrs_body<CT>(trans, LU + e.off, e.ld, e.n, ipiv + e.offv, nrhs, B + e.offv, ldb, (int)blockIdx.x);
}

// blockDim.x as above; blockIdx.x = tile of CT columns of inv(L), blockIdx.y = list entry
template <int CT>
__global__ __launch_bounds__(1024) void bbv_getri_kernel(const double *LU, BtRagged v, const int *idx, const int *ipiv, double *inv, int *info) {
    const bbv_entry e = bbv_fetch(v, idx, blockIdx.y);
    bb_getri_body<CT>(LU + e.off, e.ld, e.n, ipiv + e.offv, inv + e.off, e.ld, info ? info + e.b : nullptr, (int)blockIdx.x);
}

__global__ __launch_bounds__(256) void bbv_getdet_kernel(const double *LU, BtRagged v, const int *idx, const int *ipiv, double *mant, int *expo) {
    const bbv_entry e = bbv_fetch(v, idx, blockIdx.x);
    bb_getdet_body(LU + e.off, e.ld, e.n, ipiv + e.offv, mant + e.b, expo + e.b);
}

bool bbv_range(mpf_ctx *c, const char *who, int64_t count, int nmax) {
    const bool ok = count <= BB_MAX_LAUNCH && nmax >= 1 && nmax <= BB_MAXN;
    if (!ok) c->err = std::string(who) + ": size out of range";
    return ok;
}

template <int NB>
void bbv_factor_step(mpf_ctx *c, const BtRagged &v, const int32_t *idx, unsigned count, int nmax, int j0, double *A, int *ipiv, int *info,
                     bool fused, bool valu, int stages) {
    const int rows = nmax - j0, jc = rows < NB ? rows : NB, m = rows - jc;
    if (stages & 1) {
        const unsigned th = (unsigned)((rows + 63) / 64 * 64);
        if (fused) bbv_panel_kernel<NB, true><<<count, th, 0, c->stream>>>(A, v, idx, j0, ipiv, info);
        else bbv_panel_kernel<NB, false><<<count, th, 0, c->stream>>>(A, v, idx, j0, ipiv, info);
    }
    // the largest matrix has the most columns outside its panel, and the largest trailing matrix
    if (nmax - jc > 0 && (stages & 2)) {
        const dim3 g((unsigned)((nmax - jc + BB_RT - 1) / BB_RT), count);
        if (fused) bbv_rowblk_kernel<NB, true><<<g, BB_RT, 0, c->stream>>>(A, v, idx, j0, ipiv);
        else bbv_rowblk_kernel<NB, false><<<g, BB_RT, 0, c->stream>>>(A, v, idx, j0, ipiv);
    }
    if (m > 0 && (stages & 4)) {
        const unsigned tiles = (unsigned)((m + BB_UT - 1) / BB_UT);
        const dim3 g(tiles * tiles, count);
        if (!fused) bbv_update_valu_kernel<NB, false><<<g, 256, 0, c->stream>>>(A, v, idx, j0);
        else if (valu) bbv_update_valu_kernel<NB, true><<<g, 256, 0, c->stream>>>(A, v, idx, j0);
        else bbv_update_mfma_kernel<NB><<<g, 256, 0, c->stream>>>(A, v, idx, j0);
    }
}

} // namespace

// launch_getrf_batched_blocked's rule: 8, 16 or 32, anything else automatic (32)
int vbatched_blocked_nb(int nb) { return nb == 8 || nb == 16 ? nb : 32; }

// ---- launchers: count <= BB_MAX_LAUNCH entries of a list ordered by n (the host splits longer groups) -----------------------------------
// One panel step (vbatch_plan.h: factor_steps) over the entries still active at j0: idx points at the first of them, nmax is the
// largest order among them (> j0), nb the resolved panel width.
int launch_getrf_vbatched_blocked_step(mpf_ctx *c, const BtRagged &v, const int32_t *idx, int64_t count, int nmax, int j0, int nb, double *A,
                                       int *ipiv, int *info, int fused, int valu, int stages) {
    if (count < 1) return 0;
    if (!bbv_range(c, "launch_getrf_vbatched_blocked_step", count, nmax) || j0 < 0 || j0 >= nmax || j0 % nb != 0) {
        c->err = "launch_getrf_vbatched_blocked_step: size out of range";
        return -1;
    }
    if (nb == 8) bbv_factor_step<8>(c, v, idx, (unsigned)count, nmax, j0, A, ipiv, info, fused != 0, valu != 0, stages);
    else if (nb == 16) bbv_factor_step<16>(c, v, idx, (unsigned)count, nmax, j0, A, ipiv, info, fused != 0, valu != 0, stages);
    else if (nb == 32) bbv_factor_step<32>(c, v, idx, (unsigned)count, nmax, j0, A, ipiv, info, fused != 0, valu != 0, stages);
    else { c->err = "launch_getrf_vbatched_blocked_step: panel width must be 8, 16 or 32"; return -1; }
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

int launch_getrs_vbatched_blocked(mpf_ctx *c, const BtRagged &v, const int32_t *idx, int64_t count, int nmax, int trans, const double *LU,
                                  const int *ipiv, int nrhs, double *B, int64_t ldb) {
    if (count < 1 || nrhs < 1) return 0;
    if (!bbv_range(c, "launch_getrs_vbatched_blocked", count, nmax)) return -1;
    const unsigned th = (unsigned)((nmax + 63) / 64 * 64);
    // launch_getrs_batched_blocked's tiles: one column below four right-hand sides, eight from there
    if (nrhs < 4) {
        const dim3 g((unsigned)nrhs, (unsigned)count);
        bbv_getrs_kernel<1><<<g, th, 0, c->stream>>>(trans, LU, v, idx, ipiv, nrhs, B, ldb);
    } else {
        const dim3 g((unsigned)((nrhs + 7) / 8), (unsigned)count);
        bbv_getrs_kernel<8><<<g, th, 0, c->stream>>>(trans, LU, v, idx, ipiv, nrhs, B, ldb);
    }
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

int launch_getri_vbatched_blocked(mpf_ctx *c, const BtRagged &v, const int32_t *idx, int64_t count, int nmax, const double *LU,
                                  const int *ipiv, double *inv, int *info, int ct) {
    if (count < 1) return 0;
    if (!bbv_range(c, "launch_getri_vbatched_blocked", count, nmax)) return -1;
    const unsigned th = (unsigned)((nmax + 63) / 64 * 64);
    if (ct != 8 && ct != 16) ct = 16;                              // automatic
    const dim3 g((unsigned)((nmax + ct - 1) / ct), (unsigned)count);
    if (ct == 8) bbv_getri_kernel<8><<<g, th, 0, c->stream>>>(LU, v, idx, ipiv, inv, info);
    else bbv_getri_kernel<16><<<g, th, 0, c->stream>>>(LU, v, idx, ipiv, inv, info);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

int launch_getdet_vbatched_blocked(mpf_ctx *c, const BtRagged &v, const int32_t *idx, int64_t count, const double *LU, const int *ipiv,
                                   double *mant, int *expo) {
    if (count < 1) return 0;
    if (count > BB_MAX_LAUNCH) { c->err = "launch_getdet_vbatched_blocked: size out of range"; return -1; }
    bbv_getdet_kernel<<<(unsigned)count, 256, 0, c->stream>>>(LU, v, idx, ipiv, mant, expo);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}
