// LU of many small matrices (no reference counterpart; LAPACK dgetrf / dgetrs per matrix of a strided batch):
//   mpf_getrf_batched   mpf_dgetf2_piv's pivots and bits for every n x n matrix of the batch, n <= 128
//   mpf_getrs_batched   dgetrs with those factors, in place on the right-hand sides
//   mpf_getri_batched   the inverse from those factors, out of place: the solve's bits on an identity that is never formed
//   mpf_getdet_batched  the determinant from those factors as mant 2^expo, mpf_getdet's order per matrix
//   mpf_lange_batched, mpf_gecon_batched, mpf_residual_batched, mpf_gerfs_batched   the expert layer on those batches: a norm and an
//                       exact reciprocal condition number per matrix, the residual step operator, dgerfs's refinement with berr and
//                       an exact ferr per matrix and column (kernels in batched_refine.hip)
// The argument checks, the chunks of a batch longer than one grid and the error text; kernels and form choice in batched.hip; the
// contracts are in include/mpf_c.h.
//   mpf_getrf_batched_blocked, mpf_getrs_batched_blocked   the first two for one n <= 1024: the same bits from a right-looking blocked
//                       loop (batched_blocked.hip), three launches per panel step for the whole batch
//   mpf_getri_batched_blocked, mpf_getdet_batched_blocked   the other two for one n <= 1024: one launch each, no workspace
//   mpf_lange_batched_blocked, mpf_gecon_batched_blocked, mpf_residual_batched_blocked, mpf_gerfs_batched_blocked   the expert layer for
//                       one n <= 1024 (batched_refine_blocked.hip): the small layer's arguments, rules and, for n <= 128, bits
// The same four for matrices of different orders (mpf_*_vbatched) on a descriptor, mpf_vbatch: the host plan of vbatch_plan.h (checks,
// prefix sums, size classes) uploaded once; each call then launches one ragged kernel of vbatched.hip per class that is not empty.
// A descriptor from mpf_vbatch_create_blocked (orders up to 1024) also has the plan's large list: its matrices take the ragged blocked
// kernels of vbatched_blocked.hip, launch group by launch group, the factorization panel step by panel step over the active suffix.
#include "mpf_internal.h"
#include "vbatch_plan.h"
#include <memory>

// n, off, ld, offV by matrix and the class lists, on the host (the plan) and on the device
struct mpf_vbatch {
    mpf_ctx *ctx = nullptr;
    vbatch::Plan plan;
    Buf<int32_t> d_n, d_list;
    Buf<int64_t> d_off, d_ld, d_offv;
};

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
// the same for the blocked entry points: n <= 1024
int check_sizes_blocked(mpf_ctx *c, const char *who, int32_t n, int64_t batch, int64_t strideP, const char *then = "solve with mpf_getrs") {
    if (n < 0 || batch < 0) { c->err = std::string(who) + ": n and batch must not be negative"; return -1; }
    if (n > BB_MAXN) {
        c->err = std::string(who) + ": n > 1024 is not a batch-sized matrix: factor it with mpf_factor_dev (and " + then + ")";
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

// ---- the expert layer, n <= 128 (kernels in batched_refine.hip) ---------------------------------------------------------------------------
// check_sizes' rules with the message that names where larger matrices go
static int check_sizes_refine(mpf_ctx *c, const char *who, int32_t n, int64_t batch, const char *use) {
    if (n < 0 || batch < 0) { c->err = std::string(who) + ": n and batch must not be negative"; return -1; }
    if (n > BATCHED_MAXN) { c->err = std::string(who) + ": n > 128 is not a small matrix: use " + use + " on one matrix at a time"; return -1; }
    return 0;
}

int mpf_lange_batched(mpf_ctx *c, char norm, const double *d_A, int64_t lda, int64_t strideA, int32_t n, int64_t batch, double *d_out) {
    if (!c) return -1;
    int rc = check_sizes_refine(c, "lange_batched", n, batch, "mpf_lange (and mpf_gecon / mpf_gerfs)");
    if (rc) return rc;
    int mode;
    if (norm == '1' || norm == 'O' || norm == 'o') mode = 0;
    else if (norm == 'I' || norm == 'i') mode = 1;
    else if (norm == 'M' || norm == 'm') mode = 2;
    else { c->err = "lange_batched: norm must be '1', 'O', 'I' or 'M'"; return -1; }
    if (n == 0 || batch == 0) return 0;
    rc = check_strided(c, "lange_batched", "A", lda, strideA, n, n, batch);
    if (rc) return rc;
    if (!d_A || !d_out) { c->err = "lange_batched: null pointer"; return -1; }
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    for (int64_t b0 = 0; b0 < batch; b0 += BT_MAX_LAUNCH) {
        const int64_t nb = batch - b0 < BT_MAX_LAUNCH ? batch - b0 : BT_MAX_LAUNCH;
        rc = launch_lange_batched(c, mode, d_A + b0 * strideA, lda, strideA, n, nb, d_out + b0);
        if (rc) return rc;
    }
    return 0;
}

int mpf_gecon_batched(mpf_ctx *c, char norm, const double *d_LU, int64_t ldlu, int64_t strideLU, int32_t n, int64_t batch,
                      const double *d_anorm, double *d_rcond, double *d_ainvnm) {
    if (!c) return -1;
    int rc = check_sizes_refine(c, "gecon_batched", n, batch, "mpf_gecon (and mpf_gerfs)");
    if (rc) return rc;
    const bool one = norm == '1' || norm == 'O' || norm == 'o';
    if (!one && norm != 'I' && norm != 'i') { c->err = "gecon_batched: norm must be '1', 'O' or 'I'"; return -1; }
    if (n == 0 || batch == 0) return 0;
    rc = check_strided(c, "gecon_batched", "LU", ldlu, strideLU, n, n, batch);
    if (rc) return rc;
    if (!d_LU || !d_anorm || !d_rcond) { c->err = "gecon_batched: null pointer"; return -1; }
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    for (int64_t b0 = 0; b0 < batch; b0 += BT_MAX_LAUNCH) {
        const int64_t nb = batch - b0 < BT_MAX_LAUNCH ? batch - b0 : BT_MAX_LAUNCH;
        rc = launch_gecon_batched(c, one ? 0 : 1, d_LU + b0 * strideLU, ldlu, strideLU, n, nb, d_anorm + b0, d_rcond + b0,
                                  d_ainvnm ? d_ainvnm + b0 : nullptr);
        if (rc) return rc;
    }
    return 0;
}

int mpf_residual_batched(mpf_ctx *c, int32_t trans, const double *d_A, int64_t lda, int64_t strideA, int32_t n, int64_t batch, int32_t nrhs,
                         const double *d_X, int64_t ldx, int64_t strideX, const double *d_B, int64_t ldb, int64_t strideB, double *d_R,
                         int64_t ldr, int64_t strideR, double *d_W) {
    if (!c) return -1;
    int rc = check_sizes_refine(c, "residual_batched", n, batch, "mpf_gerfs (and mpf_gecon)");
    if (rc) return rc;
    if (nrhs < 0) { c->err = "residual_batched: nrhs must not be negative"; return -1; }
    if (trans != 0 && trans != 1) { c->err = "residual_batched: trans must be 0 or 1"; return -1; }
    if (n == 0 || batch == 0 || nrhs == 0) return 0;
    rc = check_strided(c, "residual_batched", "A", lda, strideA, n, n, batch);
    if (!rc) rc = check_strided(c, "residual_batched", "X", ldx, strideX, n, nrhs, batch);
    if (!rc) rc = check_strided(c, "residual_batched", "B", ldb, strideB, n, nrhs, batch);
    if (!rc) rc = check_strided(c, "residual_batched", "R", ldr, strideR, n, nrhs, batch);
    if (rc) return rc;
    if (!d_A || !d_X || !d_B || !d_R) { c->err = "residual_batched: null pointer"; return -1; }
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    int64_t step = BR_MAX_UNITS / nrhs;
    if (step > BT_MAX_LAUNCH) step = BT_MAX_LAUNCH;
    for (int64_t b0 = 0; b0 < batch; b0 += step) {
        const int64_t nb = batch - b0 < step ? batch - b0 : step;
        rc = launch_residual_batched(c, trans, d_A + b0 * strideA, lda, strideA, n, nb, nrhs, d_X + b0 * strideX, ldx, strideX,
                                     d_B + b0 * strideB, ldb, strideB, d_R + b0 * strideR, ldr, strideR, d_W ? d_W + b0 * strideR : nullptr);
        if (rc) return rc;
    }
    return 0;
}

int mpf_gerfs_batched(mpf_ctx *c, int32_t trans, const double *d_A, int64_t lda, int64_t strideA, const double *d_LU, int64_t ldlu,
                      int64_t strideLU, int32_t n, int64_t batch, const int32_t *d_ipiv, int64_t strideP, int32_t nrhs, const double *d_B,
                      int64_t ldb, int64_t strideB, double *d_X, int64_t ldx, int64_t strideX, int32_t itmax, double *d_ferr, double *d_berr,
                      int32_t *d_iters) {
    if (!c) return -1;
    int rc = check_sizes_refine(c, "gerfs_batched", n, batch, "mpf_gerfs (and mpf_gecon)");
    if (rc) return rc;
    if (batch > 1 && strideP < n) { c->err = "gerfs_batched: stride of ipiv < n"; return -1; }
    if (nrhs < 0) { c->err = "gerfs_batched: nrhs must not be negative"; return -1; }
    if (trans != 0 && trans != 1) { c->err = "gerfs_batched: trans must be 0 or 1"; return -1; }
    if (n == 0 || batch == 0 || nrhs == 0) return 0;
    rc = check_strided(c, "gerfs_batched", "A", lda, strideA, n, n, batch);
    if (!rc) rc = check_strided(c, "gerfs_batched", "LU", ldlu, strideLU, n, n, batch);
    if (!rc) rc = check_strided(c, "gerfs_batched", "B", ldb, strideB, n, nrhs, batch);
    if (!rc) rc = check_strided(c, "gerfs_batched", "X", ldx, strideX, n, nrhs, batch);
    if (rc) return rc;
    if (!d_A || !d_LU || !d_ipiv || !d_B || !d_X || !d_berr) { c->err = "gerfs_batched: null pointer"; return -1; }
    const int it = itmax <= 0 ? 5 : (itmax > 31 ? 31 : itmax);   // mpf_gerfs's rule
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    for (int64_t b0 = 0; b0 < batch; b0 += BT_MAX_LAUNCH) {
        const int64_t nb = batch - b0 < BT_MAX_LAUNCH ? batch - b0 : BT_MAX_LAUNCH;
        rc = launch_gerfs_batched(c, trans, d_A + b0 * strideA, lda, strideA, d_LU + b0 * strideLU, ldlu, strideLU, n, nb,
                                  d_ipiv + b0 * strideP, strideP, nrhs, d_B + b0 * strideB, ldb, strideB, d_X + b0 * strideX, ldx, strideX, it,
                                  d_ferr ? d_ferr + b0 * nrhs : nullptr, d_berr + b0 * nrhs, d_iters ? d_iters + b0 * nrhs : nullptr);
        if (rc) return rc;
    }
    return 0;
}

// ---- blocked: one n <= 1024 per call ------------------------------------------------------------------------------------------------------
// The checks are check_sizes' and check_strided's with the larger limit; n below option batched_blocked_min_n (and <= 128) goes to the
// entry points above, whose bits are the same by contract.
int mpf_getrf_batched_blocked(mpf_ctx *c, double *d_A, int64_t lda, int64_t strideA, int32_t n, int64_t batch, int32_t *d_ipiv,
                              int64_t strideP, int32_t *d_info, int32_t fused) {
    if (!c) return -1;
    int rc = check_sizes_blocked(c, "getrf_batched_blocked", n, batch, strideP);
    if (rc) return rc;
    if (n == 0 || batch == 0) return 0;
    rc = check_strided(c, "getrf_batched_blocked", "A", lda, strideA, n, n, batch);
    if (rc) return rc;
    if (!d_A || !d_ipiv) { c->err = "getrf_batched_blocked: null pointer"; return -1; }
    if (n <= BATCHED_MAXN && n < c->tune.batched_blocked_min_n) return mpf_getrf_batched(c, d_A, lda, strideA, n, batch, d_ipiv, strideP, d_info, fused);
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    int valu = 0, stages = 7;
#ifdef MPF_PROBE
    valu = c->tune.batched_blocked_valu;
    stages = c->tune.batched_blocked_stages;
#endif
    for (int64_t b0 = 0; b0 < batch; b0 += BB_MAX_LAUNCH) {
        const int64_t nb = batch - b0 < BB_MAX_LAUNCH ? batch - b0 : BB_MAX_LAUNCH;
        rc = launch_getrf_batched_blocked(c, d_A + b0 * strideA, lda, strideA, n, nb, d_ipiv + b0 * strideP, strideP,
                                          d_info ? d_info + b0 : nullptr, fused != 0, c->tune.batched_blocked_nb, valu, stages);
        if (rc) return rc;
    }
    return 0;
}

int mpf_getrs_batched_blocked(mpf_ctx *c, int32_t trans, const double *d_LU, int64_t ldlu, int64_t strideLU, int32_t n, int64_t batch,
                              const int32_t *d_ipiv, int64_t strideP, int32_t nrhs, double *d_B, int64_t ldb, int64_t strideB) {
    if (!c) return -1;
    int rc = check_sizes_blocked(c, "getrs_batched_blocked", n, batch, strideP);
    if (rc) return rc;
    if (nrhs < 0) { c->err = "getrs_batched_blocked: nrhs must not be negative"; return -1; }
    if (trans != 0 && trans != 1) { c->err = "getrs_batched_blocked: trans must be 0 or 1"; return -1; }
    if (n == 0 || batch == 0 || nrhs == 0) return 0;
    rc = check_strided(c, "getrs_batched_blocked", "LU", ldlu, strideLU, n, n, batch);
    if (!rc) rc = check_strided(c, "getrs_batched_blocked", "B", ldb, strideB, n, nrhs, batch);
    if (rc) return rc;
    if (!d_LU || !d_ipiv || !d_B) { c->err = "getrs_batched_blocked: null pointer"; return -1; }
    if (n <= BATCHED_MAXN && n < c->tune.batched_blocked_min_n)
        return mpf_getrs_batched(c, trans, d_LU, ldlu, strideLU, n, batch, d_ipiv, strideP, nrhs, d_B, ldb, strideB);
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    for (int64_t b0 = 0; b0 < batch; b0 += BB_MAX_LAUNCH) {
        const int64_t nb = batch - b0 < BB_MAX_LAUNCH ? batch - b0 : BB_MAX_LAUNCH;
        rc = launch_getrs_batched_blocked(c, trans, d_LU + b0 * strideLU, ldlu, strideLU, n, nb, d_ipiv + b0 * strideP, strideP, nrhs,
                                          d_B + b0 * strideB, ldb, strideB);
        if (rc) return rc;
    }
    return 0;
}

// mpf_getri_batched's checks with the larger limit.  The kernels need no flag buffer: every workgroup reads its matrix's diagonal and
// knows the first zero before its first store, whether or not d_info is given.
int mpf_getri_batched_blocked(mpf_ctx *c, const double *d_LU, int64_t ldlu, int64_t strideLU, int32_t n, int64_t batch,
                              const int32_t *d_ipiv, int64_t strideP, double *d_inv, int64_t ldinv, int64_t strideInv, int32_t *d_info) {
    if (!c) return -1;
    int rc = check_sizes_blocked(c, "getri_batched_blocked", n, batch, strideP, "invert with mpf_getri");
    if (rc) return rc;
    if (n == 0 || batch == 0) return 0;
    rc = check_strided(c, "getri_batched_blocked", "LU", ldlu, strideLU, n, n, batch);
    if (!rc) rc = check_strided(c, "getri_batched_blocked", "inv", ldinv, strideInv, n, n, batch);
    if (rc) return rc;
    if (!d_LU || !d_ipiv || !d_inv) { c->err = "getri_batched_blocked: null pointer"; return -1; }
    {   // mpf_getri_batched's rule and text
        const uintptr_t a0 = (uintptr_t)d_LU, a1 = a0 + (size_t)((batch - 1) * strideLU + (n - 1) * ldlu + n) * sizeof(double);
        const uintptr_t b0 = (uintptr_t)d_inv, b1 = b0 + (size_t)((batch - 1) * strideInv + (n - 1) * ldinv + n) * sizeof(double);
        if (a0 < b1 && b0 < a1) { c->err = "getri_batched_blocked: d_inv overlaps d_LU (the inverse is formed out of place)"; return -1; }
    }
    if (n <= BATCHED_MAXN && n < c->tune.batched_blocked_min_n)
        return mpf_getri_batched(c, d_LU, ldlu, strideLU, n, batch, d_ipiv, strideP, d_inv, ldinv, strideInv, d_info);
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    for (int64_t b0 = 0; b0 < batch; b0 += BB_MAX_LAUNCH) {
        const int64_t nb = batch - b0 < BB_MAX_LAUNCH ? batch - b0 : BB_MAX_LAUNCH;
        rc = launch_getri_batched_blocked(c, d_LU + b0 * strideLU, ldlu, strideLU, n, nb, d_ipiv + b0 * strideP, strideP,
                                          d_inv + b0 * strideInv, ldinv, strideInv, d_info ? d_info + b0 : nullptr,
                                          c->tune.batched_blocked_inv_ct);
        if (rc) return rc;
    }
    return 0;
}

int mpf_getdet_batched_blocked(mpf_ctx *c, const double *d_LU, int64_t ldlu, int64_t strideLU, int32_t n, int64_t batch,
                               const int32_t *d_ipiv, int64_t strideP, double *d_mant, int32_t *d_expo) {
    if (!c) return -1;
    int rc = check_sizes_blocked(c, "getdet_batched_blocked", n, batch, strideP, "take the determinant with mpf_getdet");
    if (rc) return rc;
    if (n == 0 || batch == 0) return 0;
    rc = check_strided(c, "getdet_batched_blocked", "LU", ldlu, strideLU, n, n, batch);
    if (rc) return rc;
    if (!d_LU || !d_ipiv || !d_mant || !d_expo) { c->err = "getdet_batched_blocked: null pointer"; return -1; }
    if (n <= BATCHED_MAXN && n < c->tune.batched_blocked_min_n)
        return mpf_getdet_batched(c, d_LU, ldlu, strideLU, n, batch, d_ipiv, strideP, d_mant, d_expo);
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    for (int64_t b0 = 0; b0 < batch; b0 += BB_MAX_LAUNCH) {
        const int64_t nb = batch - b0 < BB_MAX_LAUNCH ? batch - b0 : BB_MAX_LAUNCH;
        rc = launch_getdet_batched_blocked(c, d_LU + b0 * strideLU, ldlu, strideLU, n, nb, d_ipiv + b0 * strideP, strideP, d_mant + b0,
                                           d_expo + b0);
        if (rc) return rc;
    }
    return 0;
}

// ---- the expert layer, one n <= 1024 per call (kernels in batched_refine_blocked.hip) ---------------------------------------------------
// The checks of the n <= 128 entries in their order with the larger limit; n below option batched_blocked_min_n (and <= 128) goes to
// those entries, whose bits are the same by contract.
static int check_sizes_refine_blocked(mpf_ctx *c, const char *who, int32_t n, int64_t batch) {
    if (n < 0 || batch < 0) { c->err = std::string(who) + ": n and batch must not be negative"; return -1; }
    if (n > BB_MAXN) {
        c->err = std::string(who) + ": n > 1024 is not a batch-sized matrix: use mpf_lange, mpf_gecon / mpf_gerfs on one matrix at a time";
        return -1;
    }
    return 0;
}

int mpf_lange_batched_blocked(mpf_ctx *c, char norm, const double *d_A, int64_t lda, int64_t strideA, int32_t n, int64_t batch, double *d_out) {
    if (!c) return -1;
    int rc = check_sizes_refine_blocked(c, "lange_batched_blocked", n, batch);
    if (rc) return rc;
    int mode;
    if (norm == '1' || norm == 'O' || norm == 'o') mode = 0;
    else if (norm == 'I' || norm == 'i') mode = 1;
    else if (norm == 'M' || norm == 'm') mode = 2;
    else { c->err = "lange_batched_blocked: norm must be '1', 'O', 'I' or 'M'"; return -1; }
    if (n == 0 || batch == 0) return 0;
    rc = check_strided(c, "lange_batched_blocked", "A", lda, strideA, n, n, batch);
    if (rc) return rc;
    if (!d_A || !d_out) { c->err = "lange_batched_blocked: null pointer"; return -1; }
    if (n <= BATCHED_MAXN && n < c->tune.batched_blocked_min_n) return mpf_lange_batched(c, norm, d_A, lda, strideA, n, batch, d_out);
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    for (int64_t b0 = 0; b0 < batch; b0 += BB_MAX_LAUNCH) {
        const int64_t nb = batch - b0 < BB_MAX_LAUNCH ? batch - b0 : BB_MAX_LAUNCH;
        rc = launch_lange_batched_blocked(c, mode, d_A + b0 * strideA, lda, strideA, n, nb, d_out + b0);
        if (rc) return rc;
    }
    return 0;
}

int mpf_gecon_batched_blocked(mpf_ctx *c, char norm, const double *d_LU, int64_t ldlu, int64_t strideLU, int32_t n, int64_t batch,
                              const double *d_anorm, double *d_rcond, double *d_ainvnm) {
    if (!c) return -1;
    int rc = check_sizes_refine_blocked(c, "gecon_batched_blocked", n, batch);
    if (rc) return rc;
    const bool one = norm == '1' || norm == 'O' || norm == 'o';
    if (!one && norm != 'I' && norm != 'i') { c->err = "gecon_batched_blocked: norm must be '1', 'O' or 'I'"; return -1; }
    if (n == 0 || batch == 0) return 0;
    rc = check_strided(c, "gecon_batched_blocked", "LU", ldlu, strideLU, n, n, batch);
    if (rc) return rc;
    if (!d_LU || !d_anorm || !d_rcond) { c->err = "gecon_batched_blocked: null pointer"; return -1; }
    if (n <= BATCHED_MAXN && n < c->tune.batched_blocked_min_n)
        return mpf_gecon_batched(c, norm, d_LU, ldlu, strideLU, n, batch, d_anorm, d_rcond, d_ainvnm);
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    for (int64_t b0 = 0; b0 < batch; b0 += BB_MAX_LAUNCH) {
        const int64_t nb = batch - b0 < BB_MAX_LAUNCH ? batch - b0 : BB_MAX_LAUNCH;
        rc = launch_gecon_batched_blocked(c, one ? 0 : 1, d_LU + b0 * strideLU, ldlu, strideLU, n, nb, d_anorm + b0, d_rcond + b0,
                                          d_ainvnm ? d_ainvnm + b0 : nullptr);
        if (rc) return rc;
    }
    return 0;
}

int mpf_residual_batched_blocked(mpf_ctx *c, int32_t trans, const double *d_A, int64_t lda, int64_t strideA, int32_t n, int64_t batch,
                                 int32_t nrhs, const double *d_X, int64_t ldx, int64_t strideX, const double *d_B, int64_t ldb, int64_t strideB,
                                 double *d_R, int64_t ldr, int64_t strideR, double *d_W) {
    if (!c) return -1;
    int rc = check_sizes_refine_blocked(c, "residual_batched_blocked", n, batch);
    if (rc) return rc;
    if (nrhs < 0) { c->err = "residual_batched_blocked: nrhs must not be negative"; return -1; }
    if (trans != 0 && trans != 1) { c->err = "residual_batched_blocked: trans must be 0 or 1"; return -1; }
    if (n == 0 || batch == 0 || nrhs == 0) return 0;
    rc = check_strided(c, "residual_batched_blocked", "A", lda, strideA, n, n, batch);
    if (!rc) rc = check_strided(c, "residual_batched_blocked", "X", ldx, strideX, n, nrhs, batch);
    if (!rc) rc = check_strided(c, "residual_batched_blocked", "B", ldb, strideB, n, nrhs, batch);
    if (!rc) rc = check_strided(c, "residual_batched_blocked", "R", ldr, strideR, n, nrhs, batch);
    if (rc) return rc;
    if (!d_A || !d_X || !d_B || !d_R) { c->err = "residual_batched_blocked: null pointer"; return -1; }
    if (n <= BATCHED_MAXN && n < c->tune.batched_blocked_min_n)
        return mpf_residual_batched(c, trans, d_A, lda, strideA, n, batch, nrhs, d_X, ldx, strideX, d_B, ldb, strideB, d_R, ldr, strideR, d_W);
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    for (int64_t b0 = 0; b0 < batch; b0 += BB_MAX_LAUNCH) {
        const int64_t nb = batch - b0 < BB_MAX_LAUNCH ? batch - b0 : BB_MAX_LAUNCH;
        rc = launch_residual_batched_blocked(c, trans, d_A + b0 * strideA, lda, strideA, n, nb, nrhs, d_X + b0 * strideX, ldx, strideX,
                                             d_B + b0 * strideB, ldb, strideB, d_R + b0 * strideR, ldr, strideR,
                                             d_W ? d_W + b0 * strideR : nullptr);
        if (rc) return rc;
    }
    return 0;
}

int mpf_gerfs_batched_blocked(mpf_ctx *c, int32_t trans, const double *d_A, int64_t lda, int64_t strideA, const double *d_LU, int64_t ldlu,
                              int64_t strideLU, int32_t n, int64_t batch, const int32_t *d_ipiv, int64_t strideP, int32_t nrhs,
                              const double *d_B, int64_t ldb, int64_t strideB, double *d_X, int64_t ldx, int64_t strideX, int32_t itmax,
                              double *d_ferr, double *d_berr, int32_t *d_iters) {
    if (!c) return -1;
    int rc = check_sizes_refine_blocked(c, "gerfs_batched_blocked", n, batch);
    if (rc) return rc;
    if (batch > 1 && strideP < n) { c->err = "gerfs_batched_blocked: stride of ipiv < n"; return -1; }
    if (nrhs < 0) { c->err = "gerfs_batched_blocked: nrhs must not be negative"; return -1; }
    if (trans != 0 && trans != 1) { c->err = "gerfs_batched_blocked: trans must be 0 or 1"; return -1; }
    if (n == 0 || batch == 0 || nrhs == 0) return 0;
    rc = check_strided(c, "gerfs_batched_blocked", "A", lda, strideA, n, n, batch);
    if (!rc) rc = check_strided(c, "gerfs_batched_blocked", "LU", ldlu, strideLU, n, n, batch);
    if (!rc) rc = check_strided(c, "gerfs_batched_blocked", "B", ldb, strideB, n, nrhs, batch);
    if (!rc) rc = check_strided(c, "gerfs_batched_blocked", "X", ldx, strideX, n, nrhs, batch);
    if (rc) return rc;
    if (!d_A || !d_LU || !d_ipiv || !d_B || !d_X || !d_berr) { c->err = "gerfs_batched_blocked: null pointer"; return -1; }
    if (n <= BATCHED_MAXN && n < c->tune.batched_blocked_min_n)
        return mpf_gerfs_batched(c, trans, d_A, lda, strideA, d_LU, ldlu, strideLU, n, batch, d_ipiv, strideP, nrhs, d_B, ldb, strideB, d_X,
                                 ldx, strideX, itmax, d_ferr, d_berr, d_iters);
    const int it = itmax <= 0 ? 5 : (itmax > 31 ? 31 : itmax);   // mpf_gerfs's rule
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    // with the bound, a chunk is also as many matrices as keep its workspace (n + 1 doubles per column, one per column and tile of
    // 16 chains) within 256 MB; a matrix's results do not depend on the chunk
    int64_t step = BB_MAX_LAUNCH;
    if (d_ferr) {
        const int64_t fit = ((int64_t)1 << 25) / ((int64_t)nrhs * (n + 1 + (n + 15) / 16));
        step = fit < 1 ? 1 : (fit < step ? fit : step);
    }
    for (int64_t b0 = 0; b0 < batch; b0 += step) {
        const int64_t nb = batch - b0 < step ? batch - b0 : step;
        rc = launch_gerfs_batched_blocked(c, trans, d_A + b0 * strideA, lda, strideA, d_LU + b0 * strideLU, ldlu, strideLU, n, nb,
                                          d_ipiv + b0 * strideP, strideP, nrhs, d_B + b0 * strideB, ldb, strideB, d_X + b0 * strideX, ldx,
                                          strideX, it, d_ferr ? d_ferr + b0 * nrhs : nullptr, d_berr + b0 * nrhs,
                                          d_iters ? d_iters + b0 * nrhs : nullptr);
        if (rc) return rc;
    }
    return 0;
}

} // extern "C"

// ---- variable sizes -------------------------------------------------------------------------------------------------------------------
namespace {
// both creators: the plan with the limit and forwarding threshold in force, then the upload
int vb_create(mpf_ctx *c, const char *who, int maxn, int min_n, int64_t batch, const int32_t *n, const int64_t *ld, const int64_t *off,
              mpf_vbatch **out) {
    if (!c) return -1;
    if (!out) { c->err = std::string(who) + ": null pointer (out)"; return -1; }
    *out = nullptr;
    std::unique_ptr<mpf_vbatch> vb(new mpf_vbatch);
    vb->ctx = c;
    if (vbatch::plan(batch, n, ld, off, vb->plan, c->err, maxn, min_n)) return -1;
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    if (batch > 0) {
        const vbatch::Plan &p = vb->plan;
        MPF_HIP_TRY(c, vb->d_n.grow(batch));
        MPF_HIP_TRY(c, vb->d_list.grow(batch));
        MPF_HIP_TRY(c, vb->d_off.grow(batch));
        MPF_HIP_TRY(c, vb->d_ld.grow(batch));
        MPF_HIP_TRY(c, vb->d_offv.grow(batch));
        // synchronous copies: complete before any later launch on any stream, and the plan's vectors need not be pinned
        MPF_HIP_TRY(c, hipMemcpy(vb->d_n.get(), p.n.data(), (size_t)batch * sizeof(int32_t), hipMemcpyHostToDevice));
        MPF_HIP_TRY(c, hipMemcpy(vb->d_list.get(), p.list.data(), (size_t)batch * sizeof(int32_t), hipMemcpyHostToDevice));
        MPF_HIP_TRY(c, hipMemcpy(vb->d_off.get(), p.off.data(), (size_t)batch * sizeof(int64_t), hipMemcpyHostToDevice));
        MPF_HIP_TRY(c, hipMemcpy(vb->d_ld.get(), p.ld.data(), (size_t)batch * sizeof(int64_t), hipMemcpyHostToDevice));
        MPF_HIP_TRY(c, hipMemcpy(vb->d_offv.get(), p.offv.data(), (size_t)batch * sizeof(int64_t), hipMemcpyHostToDevice));
    }
    *out = vb.release();
    return 0;
}
} // namespace

extern "C" {

int mpf_vbatch_create(mpf_ctx *c, int64_t batch, const int32_t *n, const int64_t *ld, const int64_t *off, mpf_vbatch **out) {
    return vb_create(c, "vbatch_create", vbatch::MAXN, vbatch::MAXN + 1, batch, n, ld, off, out);
}

// the forwarding threshold is read here, once, and kept in the descriptor's plan
int mpf_vbatch_create_blocked(mpf_ctx *c, int64_t batch, const int32_t *n, const int64_t *ld, const int64_t *off, mpf_vbatch **out) {
    if (!c) return -1;
    return vb_create(c, "vbatch_create_blocked", vbatch::MAXN_BLOCKED, c->tune.batched_blocked_min_n, batch, n, ld, off, out);
}

void mpf_vbatch_destroy(mpf_vbatch *vb) {
    if (!vb) return;
    if (vb->ctx) {   // launches that read the descriptor's device arrays may still be in flight
        (void)hipSetDevice(vb->ctx->device);
        (void)hipStreamSynchronize(vb->ctx->stream);
    }
    delete vb;
}

int mpf_vbatch_info(const mpf_vbatch *vb, int64_t *batch, int64_t *total_n, int64_t *extent) {
    if (!vb) return -1;
    if (batch) *batch = vb->plan.batch;
    if (total_n) *total_n = vb->plan.total_n;
    if (extent) *extent = vb->plan.extent;
    return 0;
}

int mpf_vbatch_offsets(const mpf_vbatch *vb, int64_t *offM, int64_t *offV) {
    if (!vb) return -1;
    if (offM) std::copy(vb->plan.off.begin(), vb->plan.off.end(), offM);
    if (offV) std::copy(vb->plan.offv.begin(), vb->plan.offv.end(), offV);
    return 0;
}

} // extern "C"

namespace {
// what every vbatched entry point asks first
int vb_enter(mpf_ctx *c, const mpf_vbatch *vb, const char *who) {
    if (!vb) { c->err = std::string(who) + ": null pointer (descriptor)"; return -1; }
    if (vb->ctx != c) { c->err = std::string(who) + ": the descriptor belongs to another context"; return -1; }
    return 0;
}
// f(list + i0, count, top, nmax) for every chunk of every class that is not empty
template <class F>
int vb_classes(const mpf_vbatch *vb, F f) {
    const vbatch::Plan &p = vb->plan;
    for (int k = 0; k < vbatch::NCLASS; ++k)
        for (int64_t i0 = 0; i0 < p.count[k]; i0 += BT_MAX_LAUNCH) {
            const int64_t nb = p.count[k] - i0 < BT_MAX_LAUNCH ? p.count[k] - i0 : BT_MAX_LAUNCH;
            const int rc = f(vb->d_list.get() + p.start[k] + i0, nb, vbatch::CLASS_TOP[k], p.nmax[k]);
            if (rc) return rc;
        }
    return 0;
}
// the matrices of order 0: info = 0, determinant (0.5, 1)
int vb_empty(mpf_ctx *c, const mpf_vbatch *vb, int32_t *info, double *mant, int32_t *expo) {
    for (int64_t i0 = 0; i0 < vb->plan.zeros; i0 += BT_MAX_LAUNCH) {
        const int64_t nb = vb->plan.zeros - i0 < BT_MAX_LAUNCH ? vb->plan.zeros - i0 : BT_MAX_LAUNCH;
        const int rc = launch_vbatched_empty(c, vb->d_list.get() + i0, nb, info, mant, expo);
        if (rc) return rc;
    }
    return 0;
}
// f(device list + first, count, nmax, host orders of those entries) for every chunk of every launch group of the large list
template <class F>
int vb_large(const mpf_vbatch *vb, F f) {
    const vbatch::Plan &p = vb->plan;
    std::vector<int32_t> ns;
    for (int g = 0; g < vbatch::NGROUP; ++g)
        for (int64_t i0 = 0; i0 < p.gcount[g]; i0 += BB_MAX_LAUNCH) {
            const int64_t nb = p.gcount[g] - i0 < BB_MAX_LAUNCH ? p.gcount[g] - i0 : BB_MAX_LAUNCH, at = p.gstart[g] + i0;
            ns.resize((size_t)nb);
            for (int64_t i = 0; i < nb; ++i) ns[(size_t)i] = p.n[(size_t)p.list[(size_t)(at + i)]];
            const int rc = f(vb->d_list.get() + at, nb, (int)ns.back(), ns.data());
            if (rc) return rc;
        }
    return 0;
}
BtRagged vb_arrays(const mpf_vbatch *vb) { return BtRagged{vb->d_n.get(), vb->d_off.get(), vb->d_ld.get(), vb->d_offv.get()}; }
} // namespace

extern "C" {

int mpf_getrf_vbatched(mpf_ctx *c, const mpf_vbatch *vb, double *d_A, int32_t *d_ipiv, int32_t *d_info, int32_t fused) {
    if (!c) return -1;
    int rc = vb_enter(c, vb, "getrf_vbatched");
    if (rc) return rc;
    if (vb->plan.batch == 0) return 0;
    if (vb->plan.total_n > 0 && (!d_A || !d_ipiv)) { c->err = "getrf_vbatched: null pointer"; return -1; }
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    rc = vb_empty(c, vb, d_info, nullptr, nullptr);
    if (rc) return rc;
    const BtRagged v = vb_arrays(vb);
    rc = vb_classes(vb, [&](const int32_t *idx, int64_t count, int top, int nmax) {
        return launch_getrf_vbatched(c, v, idx, count, top, nmax, d_A, d_ipiv, d_info, fused != 0);
    });
    if (rc || vb->plan.large_count == 0) return rc;
    int valu = 0, stages = 7;
#ifdef MPF_PROBE
    valu = c->tune.batched_blocked_valu;
    stages = c->tune.batched_blocked_stages;
#endif
    const int nb = vbatched_blocked_nb(c->tune.batched_blocked_nb);
    return vb_large(vb, [&](const int32_t *idx, int64_t count, int nmax, const int32_t *ns) {
        for (const vbatch::Step &s : vbatch::factor_steps(ns, count, nb)) {   // nmax - s.j0 == s.rows
            const int e = launch_getrf_vbatched_blocked_step(c, v, idx + s.first, count - s.first, nmax, s.j0, nb, d_A, d_ipiv, d_info,
                                                             fused != 0, valu, stages);
            if (e) return e;
        }
        return 0;
    });
}

int mpf_getrs_vbatched(mpf_ctx *c, const mpf_vbatch *vb, int32_t trans, const double *d_LU, const int32_t *d_ipiv, int32_t nrhs, double *d_B,
                       int64_t ldb) {
    if (!c) return -1;
    int rc = vb_enter(c, vb, "getrs_vbatched");
    if (rc) return rc;
    if (nrhs < 0) { c->err = "getrs_vbatched: nrhs must not be negative"; return -1; }
    if (trans != 0 && trans != 1) { c->err = "getrs_vbatched: trans must be 0 or 1"; return -1; }
    if (vb->plan.batch == 0 || vb->plan.total_n == 0 || nrhs == 0) return 0;
    if (ldb < vb->plan.total_n) { c->err = "getrs_vbatched: leading dimension of B < total_n"; return -1; }
    if (!d_LU || !d_ipiv || !d_B) { c->err = "getrs_vbatched: null pointer"; return -1; }
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    const BtRagged v = vb_arrays(vb);
    rc = vb_classes(vb, [&](const int32_t *idx, int64_t count, int top, int nmax) {
        return launch_getrs_vbatched(c, v, idx, count, top, nmax, trans, d_LU, d_ipiv, nrhs, d_B, ldb);
    });
    if (rc) return rc;
    return vb_large(vb, [&](const int32_t *idx, int64_t count, int nmax, const int32_t *) {
        return launch_getrs_vbatched_blocked(c, v, idx, count, nmax, trans, d_LU, d_ipiv, nrhs, d_B, ldb);
    });
}

int mpf_getri_vbatched(mpf_ctx *c, const mpf_vbatch *vb, const double *d_LU, const int32_t *d_ipiv, double *d_inv, int32_t *d_info) {
    if (!c) return -1;
    int rc = vb_enter(c, vb, "getri_vbatched");
    if (rc) return rc;
    if (vb->plan.batch == 0) return 0;
    if (vb->plan.total_n > 0) {
        if (!d_LU || !d_ipiv || !d_inv) { c->err = "getri_vbatched: null pointer"; return -1; }
        // the factors are still being read while the result is stored (mpf_getri_batched's rule, on the two operands' extents)
        const uintptr_t a0 = (uintptr_t)d_LU, a1 = a0 + (size_t)vb->plan.extent * sizeof(double);
        const uintptr_t b0 = (uintptr_t)d_inv, b1 = b0 + (size_t)vb->plan.extent * sizeof(double);
        if (a0 < b1 && b0 < a1) { c->err = "getri_vbatched: d_inv overlaps d_LU (the inverse is formed out of place)"; return -1; }
    }
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    rc = vb_empty(c, vb, d_info, nullptr, nullptr);
    if (rc) return rc;
    const BtRagged v = vb_arrays(vb);
    rc = vb_classes(vb, [&](const int32_t *idx, int64_t count, int top, int nmax) {
        return launch_getri_vbatched(c, v, idx, count, top, nmax, d_LU, d_ipiv, d_inv, d_info);
    });
    if (rc) return rc;
    return vb_large(vb, [&](const int32_t *idx, int64_t count, int nmax, const int32_t *) {
        return launch_getri_vbatched_blocked(c, v, idx, count, nmax, d_LU, d_ipiv, d_inv, d_info, c->tune.batched_blocked_inv_ct);
    });
}

int mpf_getdet_vbatched(mpf_ctx *c, const mpf_vbatch *vb, const double *d_LU, const int32_t *d_ipiv, double *d_mant, int32_t *d_expo) {
    if (!c) return -1;
    int rc = vb_enter(c, vb, "getdet_vbatched");
    if (rc) return rc;
    if (vb->plan.batch == 0) return 0;
    if (!d_mant || !d_expo || (vb->plan.total_n > 0 && (!d_LU || !d_ipiv))) { c->err = "getdet_vbatched: null pointer"; return -1; }
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    rc = vb_empty(c, vb, nullptr, d_mant, d_expo);
    if (rc) return rc;
    const BtRagged v = vb_arrays(vb);
    rc = vb_classes(vb, [&](const int32_t *idx, int64_t count, int top, int nmax) {
        return launch_getdet_vbatched(c, v, idx, count, top, d_LU, d_ipiv, d_mant, d_expo);
    });
    if (rc) return rc;
    return vb_large(vb, [&](const int32_t *idx, int64_t count, int, const int32_t *) {
        return launch_getdet_vbatched_blocked(c, v, idx, count, d_LU, d_ipiv, d_mant, d_expo);
    });
}

} // extern "C"
