// LU of many small matrices (no reference counterpart; LAPACK dgetrf / dgetrs per matrix of a strided batch):
//   mpf_getrf_batched   mpf_dgetf2_piv's pivots and bits for every n x n matrix of the batch, n <= 128
//   mpf_getrs_batched   dgetrs with those factors, in place on the right-hand sides
//   mpf_getri_batched   the inverse from those factors, out of place: the solve's bits on an identity that is never formed
//   mpf_getdet_batched  the determinant from those factors as mant 2^expo, mpf_getdet's order per matrix
// The argument checks, the chunks of a batch longer than one grid and the error text; kernels and form choice in batched.hip; the
// contracts are in include/mpf_c.h.
#include "mpf_internal.h"

namespace {
constexpr int32_t BATCHED_MAXN = 128;

// what both entry points ask of a strided batch of `rows` x `cols` column-major matrices
int check_strided(mpf_ctx *c, const char *who, const char *what, int64_t ld, int64_t stride, int64_t rows, int64_t cols, int64_t batch) {
    if (ld < rows) { c->err = std::string(who) + ": leading dimension of " + what + " < n"; return -1; }
    if (batch > 1 && stride < ld * cols) { c->err = std::string(who) + ": stride of " + what + " is smaller than one matrix"; return -1; }
    return 0;
}
int check_sizes(mpf_ctx *c, const char *who, int32_t n, int64_t batch, int64_t strideP) {
    if (n < 0 || batch < 0) { c->err = std::string(who) + ": n and batch must not be negative"; return -1; }
    if (n > BATCHED_MAXN) {
        c->err = std::string(who) + ": n > 128 is not a small matrix: factor it with mpf_factor_dev (and solve with mpf_getrs)";
        return -1;
    }
    if (batch > 1 && strideP < n) { c->err = std::string(who) + ": stride of ipiv < n"; return -1; }
    return 0;
}
} // namespace

extern "C" {

int mpf_getrf_batched(mpf_ctx *c, double *d_A, int64_t lda, int64_t strideA, int32_t n, int64_t batch, int32_t *d_ipiv, int64_t strideP,
                      int32_t *d_info, int32_t fused) {
    if (!c) return -1;
    int rc = check_sizes(c, "getrf_batched", n, batch, strideP);
    if (rc) return rc;
    if (n == 0 || batch == 0) return 0;
    rc = check_strided(c, "getrf_batched", "A", lda, strideA, n, n, batch);
    if (rc) return rc;
    if (!d_A || !d_ipiv) { c->err = "getrf_batched: null pointer"; return -1; }
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    for (int64_t b0 = 0; b0 < batch; b0 += BT_MAX_LAUNCH) {
        const int64_t nb = batch - b0 < BT_MAX_LAUNCH ? batch - b0 : BT_MAX_LAUNCH;
        rc = launch_getrf_batched(c, d_A + b0 * strideA, lda, strideA, n, nb, d_ipiv + b0 * strideP, strideP, d_info ? d_info + b0 : nullptr,
                                  fused != 0);
        if (rc) return rc;
    }
    return 0;
}

int mpf_getrs_batched(mpf_ctx *c, int32_t trans, const double *d_LU, int64_t ldlu, int64_t strideLU, int32_t n, int64_t batch,
                      const int32_t *d_ipiv, int64_t strideP, int32_t nrhs, double *d_B, int64_t ldb, int64_t strideB) {
    if (!c) return -1;
    int rc = check_sizes(c, "getrs_batched", n, batch, strideP);
    if (rc) return rc;
    if (nrhs < 0) { c->err = "getrs_batched: nrhs must not be negative"; return -1; }
    if (trans != 0 && trans != 1) { c->err = "getrs_batched: trans must be 0 or 1"; return -1; }
    if (n == 0 || batch == 0 || nrhs == 0) return 0;
    rc = check_strided(c, "getrs_batched", "LU", ldlu, strideLU, n, n, batch);
    if (!rc) rc = check_strided(c, "getrs_batched", "B", ldb, strideB, n, nrhs, batch);
    if (rc) return rc;
    if (!d_LU || !d_ipiv || !d_B) { c->err = "getrs_batched: null pointer"; return -1; }
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    for (int64_t b0 = 0; b0 < batch; b0 += BT_MAX_LAUNCH) {
        const int64_t nb = batch - b0 < BT_MAX_LAUNCH ? batch - b0 : BT_MAX_LAUNCH;
        rc = launch_getrs_batched(c, trans, d_LU + b0 * strideLU, ldlu, strideLU, n, nb, d_ipiv + b0 * strideP, strideP, nrhs,
                                  d_B + b0 * strideB, ldb, strideB);
        if (rc) return rc;
    }
    return 0;
}

int mpf_getri_batched(mpf_ctx *c, const double *d_LU, int64_t ldlu, int64_t strideLU, int32_t n, int64_t batch, const int32_t *d_ipiv,
                      int64_t strideP, double *d_inv, int64_t ldinv, int64_t strideInv, int32_t *d_info) {
    if (!c) return -1;
    int rc = check_sizes(c, "getri_batched", n, batch, strideP);
    if (rc) return rc;
    if (n == 0 || batch == 0) return 0;
    rc = check_strided(c, "getri_batched", "LU", ldlu, strideLU, n, n, batch);
    if (!rc) rc = check_strided(c, "getri_batched", "inv", ldinv, strideInv, n, n, batch);
    if (rc) return rc;
    if (!d_LU || !d_ipiv || !d_inv) { c->err = "getri_batched: null pointer"; return -1; }
    {   // the factors are still being read while the result is stored (mpf_getri's rule, on the address ranges of the two batches)
        const uintptr_t a0 = (uintptr_t)d_LU, a1 = a0 + (size_t)((batch - 1) * strideLU + (n - 1) * ldlu + n) * sizeof(double);
        const uintptr_t b0 = (uintptr_t)d_inv, b1 = b0 + (size_t)((batch - 1) * strideInv + (n - 1) * ldinv + n) * sizeof(double);
        if (a0 < b1 && b0 < a1) { c->err = "getri_batched: d_inv overlaps d_LU (the inverse is formed out of place)"; return -1; }
    }
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    for (int64_t b0 = 0; b0 < batch; b0 += BT_MAX_LAUNCH) {
        const int64_t nb = batch - b0 < BT_MAX_LAUNCH ? batch - b0 : BT_MAX_LAUNCH;
        rc = launch_getri_batched(c, d_LU + b0 * strideLU, ldlu, strideLU, n, nb, d_ipiv + b0 * strideP, strideP, d_inv + b0 * strideInv,
                                  ldinv, strideInv, d_info ? d_info + b0 : nullptr);
        if (rc) return rc;
    }
    return 0;
}

int mpf_getdet_batched(mpf_ctx *c, const double *d_LU, int64_t ldlu, int64_t strideLU, int32_t n, int64_t batch, const int32_t *d_ipiv,
                       int64_t strideP, double *d_mant, int32_t *d_expo) {
    if (!c) return -1;
    int rc = check_sizes(c, "getdet_batched", n, batch, strideP);
    if (rc) return rc;
    if (n == 0 || batch == 0) return 0;
    rc = check_strided(c, "getdet_batched", "LU", ldlu, strideLU, n, n, batch);
    if (rc) return rc;
    if (!d_LU || !d_ipiv || !d_mant || !d_expo) { c->err = "getdet_batched: null pointer"; return -1; }
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    for (int64_t b0 = 0; b0 < batch; b0 += BT_MAX_LAUNCH) {
        const int64_t nb = batch - b0 < BT_MAX_LAUNCH ? batch - b0 : BT_MAX_LAUNCH;
        rc = launch_getdet_batched(c, d_LU + b0 * strideLU, ldlu, strideLU, n, nb, d_ipiv + b0 * strideP, strideP, d_mant + b0, d_expo + b0);
        if (rc) return rc;
    }
    return 0;
}

} // extern "C"
