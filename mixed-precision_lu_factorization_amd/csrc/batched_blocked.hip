// Blocked LU of many matrices of one order up to 1024 (mpf_getrf_batched_blocked, mpf_getrs_batched_blocked; contracts in
// include/mpf_c.h, host side in mpf_batched.cpp), and from its factors the inverse and the determinant
// (mpf_getri_batched_blocked, mpf_getdet_batched_blocked).
//
// The arithmetic and the account of every scheme are batched_blocked_body.h's, shared with the ragged kernels of vbatched_blocked.hip
// and the expert kernels of batched_refine_blocked.hip.  What is here is where a workgroup stands in a strided launch:
// each kernel finds matrix b's base, pivots and info entry from the strides and calls the body of its name with blockIdx.x as the work
// item; then the launchers, the panel loop and the form choice.
#include "batched_blocked_body.h"

// blockDim.x = the panel's rows n - j0 rounded up to whole waves (<= 1024); blockIdx.x = matrix
template <int NB, bool FUSED>
__global__ __launch_bounds__(1024) void bb_panel_kernel(double *A, long long lda, long long strideA, int n, int j0, int *ipiv,
                                                        long long strideP, int *info) {
    const long long b = blockIdx.x;
    bb_panel_body<NB, FUSED>(A + b * strideA, lda, n, j0, ipiv + b * strideP, info ? info + b : nullptr);
}

// blockIdx.x = chunk of BB_RT columns outside the panel, blockIdx.y = matrix
template <int NB, bool FUSED>
__global__ __launch_bounds__(BB_RT) void bb_rowblk_kernel(double *A, long long lda, long long strideA, int n, int j0, const int *ipiv,
                                                          long long strideP) {
    const long long b = blockIdx.y;
    bb_rowblk_body<NB, FUSED>(A + b * strideA, lda, n, j0, ipiv + b * strideP, (int)blockIdx.x);
}

// blockIdx.x = 64 x 64 tile of the m x m trailing matrix (m = n - j0 - NB), blockIdx.y = matrix
template <int NB>
__global__ __launch_bounds__(256) void bb_update_mfma_kernel(double *A, long long lda, long long strideA, int n, int j0) {
    bb_update_mfma_body<NB>(A + (long long)blockIdx.y * strideA, lda, n, j0, (int)blockIdx.x);
}

template <int NB, bool FUSED>
__global__ __launch_bounds__(256) void bb_update_valu_kernel(double *A, long long lda, long long strideA, int n, int j0) {
    bb_update_valu_body<NB, FUSED>(A + (long long)blockIdx.y * strideA, lda, n, j0, (int)blockIdx.x);
}

// blockDim.x = n rounded up to whole waves; blockIdx.x = tile of CT columns of B, blockIdx.y = matrix
template <int CT>
__global__ __launch_bounds__(1024) void bb_getrs_kernel(int trans, const double *LU, long long ldlu, long long strideLU, int n, const int *ipiv,
                                                        long long strideP, int nrhs, double *B, long long ldb, long long strideB) {
    const long long b = blockIdx.y;
    bb_getrs_body<CT>(trans, LU + b * strideLU, ldlu, n, ipiv + b * strideP, nrhs, B + b * strideB, ldb, (int)blockIdx.x);
}

// blockDim.x = n rounded up to whole waves; blockIdx.x = tile of CT columns of inv(L), blockIdx.y = matrix
template <int CT>
__global__ __launch_bounds__(1024) void bb_getri_kernel(const double *LU, long long ldlu, long long strideLU, int n, const int *ipiv,
                                                        long long strideP, double *inv, long long ldinv, long long strideInv, int *info) {
    const long long b = blockIdx.y;
    bb_getri_body<CT>(LU + b * strideLU, ldlu, n, ipiv + b * strideP, inv + b * strideInv, ldinv, info ? info + b : nullptr, (int)blockIdx.x);
}

// blockIdx.x = matrix
__global__ __launch_bounds__(256) void bb_getdet_kernel(const double *LU, long long ldlu, long long strideLU, int n, const int *ipiv,
                                                        long long strideP, double *mant, int *expo) {
    const long long b = blockIdx.x;
    bb_getdet_body(LU + b * strideLU, ldlu, n, ipiv + b * strideP, mant + b, expo + b);
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
