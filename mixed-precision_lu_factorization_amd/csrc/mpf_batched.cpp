// The host side of the batched layer (no reference counterpart; LAPACK per matrix of a batch; contracts in include/mpf_c.h).
// Strided batches, one order per call: every operator has ONE host body, <operator>_strided, for its two entries mpf_<operator>_batched
// (n <= 128; batched.hip, batched_refine.hip) and mpf_<operator>_batched_blocked (n <= 1024; batched_blocked.hip,
// batched_refine_blocked.hip; equilibration for both: batched_equil.hip).  An entry is a !c test and one call that passes its name, its
// family's limit and the text that says where a larger matrix goes (the three equilibration bodies take no such text: their six entries
// share ONE_GEEQU).  A body reads: the checks in the contract's order (sizes, pivot stride, nrhs / trans / norm, `return 0` on the empty
// cases, strided operands, null pointers, getri's out-of-place test; rules and texts are batch_args.h's), hipSetDevice, then one launch
// per chunk -- the small launcher and chunk step for a small entry and for a blocked one below option batched_blocked_min_n (the same
// bits by contract), the blocked ones otherwise.  Operators: getrf, getrs, getri, getdet; the expert layer lange, gecon, residual, gerfs;
// the equilibration geequ, laqge, lascl2.
// Matrices of different orders (mpf_*_vbatched) on a descriptor, mpf_vbatch: the host plan of vbatch_plan.h uploaded once.  Three walks
// over three different lists stay apart, each cut with batch_args::chunks: vb_classes (orders <= 128 of the factor, solve, inverse and
// determinant entries: one ragged kernel of vbatched.hip per class that is not empty), vb_large (a blocked descriptor's large list:
// vbatched_blocked.hip, launch group by launch group, the factorization panel step by panel step over the active suffix) and
// vb_refine_chunks (expert layer and equilibration on either kind: every order >= 1, vbatched_refine.hip / batched_equil.hip, launch
// groups of the whole ordered list; vbatch_plan.h: refine_chunks).  The matrices of order 0 get their outputs from kernels of their own
// (vb_zeros).
#include "mpf_internal.h"
#include "batch_args.h"
#include "vbatch_plan.h"
#include <memory>

// n, off, ld, offV by matrix and the class lists, on the host (the plan) and on the device
struct mpf_vbatch {
    mpf_ctx *ctx = nullptr;
    vbatch::Plan plan;
    Buf<int32_t> d_n, d_list;
    Buf<int64_t> d_off, d_ld, d_offv;
    Buf<int64_t> d_lrow, d_ltile;   // the plan's prefix sums by list position (the expert layer's workspace layout), batch + 1 each
};

namespace {
namespace ba = batch_args;

// where check_sizes' message sends a matrix that is too large for the family
const char *const THEN_GETRS = "factor it with mpf_factor_dev (and solve with mpf_getrs)";
const char *const THEN_GETRI = "factor it with mpf_factor_dev (and invert with mpf_getri)";
const char *const THEN_GETDET = "factor it with mpf_factor_dev (and take the determinant with mpf_getdet)";
const char *const ONE_LANGE = "use mpf_lange (and mpf_gecon / mpf_gerfs) on one matrix at a time";
const char *const ONE_GECON = "use mpf_gecon (and mpf_gerfs) on one matrix at a time";
const char *const ONE_GERFS = "use mpf_gerfs (and mpf_gecon) on one matrix at a time";
const char *const ONE_AT_A_TIME = "use mpf_lange, mpf_gecon / mpf_gerfs on one matrix at a time";
const char *const ONE_GEEQU = "equilibrate it with mpf_geequ (or mpf_gesvx) and factor it with mpf_factor_dev";

bool forwards_to_small(const mpf_ctx *c, int32_t n) { return ba::forwards_to_small(n, c->tune.batched_blocked_min_n); }
// whether a body launches the small kernels: every call of a small entry, and a blocked entry's that forwards
bool takes_small(const mpf_ctx *c, int32_t limit, int32_t n) { return limit == ba::SMALL_MAXN || forwards_to_small(c, n); }
int null_pointer(mpf_ctx *c, const char *who) { c->err = std::string(who) + ": null pointer"; return -1; }
// an optional per-matrix output of a chunk
template <class T>
T *opt(T *p, int64_t at) { return p ? p + at : nullptr; }
// getri's rule: the factors are still being read while the result is stored (mpf_getri's rule, on the address ranges of the two batches)
int check_out_of_place(mpf_ctx *c, const char *who, const double *d_LU, int64_t na, const double *d_inv, int64_t nb) {
    if (!ba::ranges_overlap((uintptr_t)d_LU, na, (uintptr_t)d_inv, nb)) return 0;
    c->err = std::string(who) + ": d_inv overlaps d_LU (the inverse is formed out of place)";
    return -1;
}
// the blocked factorization's update form and pipeline depth: switches of the probe library only
struct FactorForm { int valu, stages; };
FactorForm factor_form(const mpf_ctx *c) {
#ifdef MPF_PROBE
    return {c->tune.batched_blocked_valu, c->tune.batched_blocked_stages};
#else
    return {0, 7};
#endif
}

// ---- strided batches: one body per operator ------------------------------------------------------------------------------------------------
int getrf_strided(mpf_ctx *c, const char *who, int32_t limit, const char *tail, double *d_A, int64_t lda, int64_t strideA, int32_t n,
                  int64_t batch, int32_t *d_ipiv, int64_t strideP, int32_t *d_info, int32_t fused) {
    int rc = ba::check_sizes(c->err, who, limit, n, batch, tail);
    if (!rc) rc = ba::check_pivot_stride(c->err, who, n, batch, strideP);
    if (rc) return rc;
    if (n == 0 || batch == 0) return 0;
    rc = ba::check_strided(c->err, who, "A", lda, strideA, n, n, batch);
    if (rc) return rc;
    if (!d_A || !d_ipiv) return null_pointer(c, who);
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    if (takes_small(c, limit, n))
        return ba::chunks(batch, BT_MAX_LAUNCH, [&](int64_t b0, int64_t nb) {
            return launch_getrf_batched(c, d_A + b0 * strideA, lda, strideA, n, nb, d_ipiv + b0 * strideP, strideP, opt(d_info, b0), fused != 0);
        });
    const FactorForm f = factor_form(c);
    return ba::chunks(batch, BB_MAX_LAUNCH, [&](int64_t b0, int64_t nb) {
        return launch_getrf_batched_blocked(c, d_A + b0 * strideA, lda, strideA, n, nb, d_ipiv + b0 * strideP, strideP, opt(d_info, b0),
                                            fused != 0, c->tune.batched_blocked_nb, f.valu, f.stages);
    });
}

int getrs_strided(mpf_ctx *c, const char *who, int32_t limit, const char *tail, int32_t trans, const double *d_LU, int64_t ldlu,
                  int64_t strideLU, int32_t n, int64_t batch, const int32_t *d_ipiv, int64_t strideP, int32_t nrhs, double *d_B, int64_t ldb,
                  int64_t strideB) {
    int rc = ba::check_sizes(c->err, who, limit, n, batch, tail);
    if (!rc) rc = ba::check_pivot_stride(c->err, who, n, batch, strideP);
    if (!rc) rc = ba::check_nrhs_trans(c->err, who, nrhs, trans);
    if (rc) return rc;
    if (n == 0 || batch == 0 || nrhs == 0) return 0;
    rc = ba::check_strided(c->err, who, "LU", ldlu, strideLU, n, n, batch);
    if (!rc) rc = ba::check_strided(c->err, who, "B", ldb, strideB, n, nrhs, batch);
    if (rc) return rc;
    if (!d_LU || !d_ipiv || !d_B) return null_pointer(c, who);
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    const bool small = takes_small(c, limit, n);
    const auto launch = small ? launch_getrs_batched : launch_getrs_batched_blocked;
    return ba::chunks(batch, small ? BT_MAX_LAUNCH : BB_MAX_LAUNCH, [&](int64_t b0, int64_t nb) {
        return launch(c, trans, d_LU + b0 * strideLU, ldlu, strideLU, n, nb, d_ipiv + b0 * strideP, strideP, nrhs, d_B + b0 * strideB, ldb, strideB);
    });
}

// The blocked kernels need no flag buffer: every workgroup reads its matrix's diagonal and knows the first zero before its first store,
// whether or not d_info is given.
int getri_strided(mpf_ctx *c, const char *who, int32_t limit, const char *tail, const double *d_LU, int64_t ldlu, int64_t strideLU, int32_t n,
                  int64_t batch, const int32_t *d_ipiv, int64_t strideP, double *d_inv, int64_t ldinv, int64_t strideInv, int32_t *d_info) {
    int rc = ba::check_sizes(c->err, who, limit, n, batch, tail);
    if (!rc) rc = ba::check_pivot_stride(c->err, who, n, batch, strideP);
    if (rc) return rc;
    if (n == 0 || batch == 0) return 0;
    rc = ba::check_strided(c->err, who, "LU", ldlu, strideLU, n, n, batch);
    if (!rc) rc = ba::check_strided(c->err, who, "inv", ldinv, strideInv, n, n, batch);
    if (rc) return rc;
    if (!d_LU || !d_ipiv || !d_inv) return null_pointer(c, who);
    rc = check_out_of_place(c, who, d_LU, ba::extent(n, batch, ldlu, strideLU), d_inv, ba::extent(n, batch, ldinv, strideInv));
    if (rc) return rc;
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    if (takes_small(c, limit, n))
        return ba::chunks(batch, BT_MAX_LAUNCH, [&](int64_t b0, int64_t nb) {
            return launch_getri_batched(c, d_LU + b0 * strideLU, ldlu, strideLU, n, nb, d_ipiv + b0 * strideP, strideP, d_inv + b0 * strideInv,
                                        ldinv, strideInv, opt(d_info, b0));
        });
    return ba::chunks(batch, BB_MAX_LAUNCH, [&](int64_t b0, int64_t nb) {
        return launch_getri_batched_blocked(c, d_LU + b0 * strideLU, ldlu, strideLU, n, nb, d_ipiv + b0 * strideP, strideP,
                                            d_inv + b0 * strideInv, ldinv, strideInv, opt(d_info, b0), c->tune.batched_blocked_inv_ct);
    });
}

int getdet_strided(mpf_ctx *c, const char *who, int32_t limit, const char *tail, const double *d_LU, int64_t ldlu, int64_t strideLU, int32_t n,
                   int64_t batch, const int32_t *d_ipiv, int64_t strideP, double *d_mant, int32_t *d_expo) {
    int rc = ba::check_sizes(c->err, who, limit, n, batch, tail);
    if (!rc) rc = ba::check_pivot_stride(c->err, who, n, batch, strideP);
    if (rc) return rc;
    if (n == 0 || batch == 0) return 0;
    rc = ba::check_strided(c->err, who, "LU", ldlu, strideLU, n, n, batch);
    if (rc) return rc;
    if (!d_LU || !d_ipiv || !d_mant || !d_expo) return null_pointer(c, who);
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    const bool small = takes_small(c, limit, n);
    const auto launch = small ? launch_getdet_batched : launch_getdet_batched_blocked;
    return ba::chunks(batch, small ? BT_MAX_LAUNCH : BB_MAX_LAUNCH, [&](int64_t b0, int64_t nb) {
        return launch(c, d_LU + b0 * strideLU, ldlu, strideLU, n, nb, d_ipiv + b0 * strideP, strideP, d_mant + b0, d_expo + b0);
    });
}

// the expert layer
int lange_strided(mpf_ctx *c, const char *who, int32_t limit, const char *tail, char norm, const double *d_A, int64_t lda, int64_t strideA,
                  int32_t n, int64_t batch, double *d_out) {
    int rc = ba::check_sizes(c->err, who, limit, n, batch, tail);
    if (rc) return rc;
    const int mode = ba::lange_mode(c->err, who, norm);
    if (mode < 0) return -1;
    if (n == 0 || batch == 0) return 0;
    rc = ba::check_strided(c->err, who, "A", lda, strideA, n, n, batch);
    if (rc) return rc;
    if (!d_A || !d_out) return null_pointer(c, who);
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    const bool small = takes_small(c, limit, n);
    const auto launch = small ? launch_lange_batched : launch_lange_batched_blocked;
    return ba::chunks(batch, small ? BT_MAX_LAUNCH : BB_MAX_LAUNCH, [&](int64_t b0, int64_t nb) {
        return launch(c, mode, d_A + b0 * strideA, lda, strideA, n, nb, d_out + b0);
    });
}

int gecon_strided(mpf_ctx *c, const char *who, int32_t limit, const char *tail, char norm, const double *d_LU, int64_t ldlu, int64_t strideLU,
                  int32_t n, int64_t batch, const double *d_anorm, double *d_rcond, double *d_ainvnm) {
    int rc = ba::check_sizes(c->err, who, limit, n, batch, tail);
    if (rc) return rc;
    const int inf = ba::gecon_mode(c->err, who, norm);
    if (inf < 0) return -1;
    if (n == 0 || batch == 0) return 0;
    rc = ba::check_strided(c->err, who, "LU", ldlu, strideLU, n, n, batch);
    if (rc) return rc;
    if (!d_LU || !d_anorm || !d_rcond) return null_pointer(c, who);
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    const bool small = takes_small(c, limit, n);
    const auto launch = small ? launch_gecon_batched : launch_gecon_batched_blocked;
    return ba::chunks(batch, small ? BT_MAX_LAUNCH : BB_MAX_LAUNCH, [&](int64_t b0, int64_t nb) {
        return launch(c, inf, d_LU + b0 * strideLU, ldlu, strideLU, n, nb, d_anorm + b0, d_rcond + b0, opt(d_ainvnm, b0));
    });
}

int residual_strided(mpf_ctx *c, const char *who, int32_t limit, const char *tail, int32_t trans, const double *d_A, int64_t lda,
                     int64_t strideA, int32_t n, int64_t batch, int32_t nrhs, const double *d_X, int64_t ldx, int64_t strideX, const double *d_B,
                     int64_t ldb, int64_t strideB, double *d_R, int64_t ldr, int64_t strideR, double *d_W) {
    int rc = ba::check_sizes(c->err, who, limit, n, batch, tail);
    if (!rc) rc = ba::check_nrhs_trans(c->err, who, nrhs, trans);
    if (rc) return rc;
    if (n == 0 || batch == 0 || nrhs == 0) return 0;
    rc = ba::check_strided(c->err, who, "A", lda, strideA, n, n, batch);
    if (!rc) rc = ba::check_strided(c->err, who, "X", ldx, strideX, n, nrhs, batch);
    if (!rc) rc = ba::check_strided(c->err, who, "B", ldb, strideB, n, nrhs, batch);
    if (!rc) rc = ba::check_strided(c->err, who, "R", ldr, strideR, n, nrhs, batch);
    if (rc) return rc;
    if (!d_A || !d_X || !d_B || !d_R) return null_pointer(c, who);
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    const bool small = takes_small(c, limit, n);
    const auto launch = small ? launch_residual_batched : launch_residual_batched_blocked;
    return ba::chunks(batch, small ? ba::residual_step(BR_MAX_UNITS, BT_MAX_LAUNCH, nrhs) : BB_MAX_LAUNCH, [&](int64_t b0, int64_t nb) {
        return launch(c, trans, d_A + b0 * strideA, lda, strideA, n, nb, nrhs, d_X + b0 * strideX, ldx, strideX, d_B + b0 * strideB, ldb, strideB,
                      d_R + b0 * strideR, ldr, strideR, opt(d_W, b0 * strideR));
    });
}

int gerfs_strided(mpf_ctx *c, const char *who, int32_t limit, const char *tail, int32_t trans, const double *d_A, int64_t lda, int64_t strideA,
                  const double *d_LU, int64_t ldlu, int64_t strideLU, int32_t n, int64_t batch, const int32_t *d_ipiv, int64_t strideP,
                  int32_t nrhs, const double *d_B, int64_t ldb, int64_t strideB, double *d_X, int64_t ldx, int64_t strideX, int32_t itmax,
                  double *d_ferr, double *d_berr, int32_t *d_iters) {
    int rc = ba::check_sizes(c->err, who, limit, n, batch, tail);
    if (!rc) rc = ba::check_pivot_stride(c->err, who, n, batch, strideP);
    if (!rc) rc = ba::check_nrhs_trans(c->err, who, nrhs, trans);
    if (rc) return rc;
    if (n == 0 || batch == 0 || nrhs == 0) return 0;
    rc = ba::check_strided(c->err, who, "A", lda, strideA, n, n, batch);
    if (!rc) rc = ba::check_strided(c->err, who, "LU", ldlu, strideLU, n, n, batch);
    if (!rc) rc = ba::check_strided(c->err, who, "B", ldb, strideB, n, nrhs, batch);
    if (!rc) rc = ba::check_strided(c->err, who, "X", ldx, strideX, n, nrhs, batch);
    if (rc) return rc;
    if (!d_A || !d_LU || !d_ipiv || !d_B || !d_X || !d_berr) return null_pointer(c, who);
    const int it = ba::clamp_itmax(itmax);
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    const bool small = takes_small(c, limit, n);
    const auto launch = small ? launch_gerfs_batched : launch_gerfs_batched_blocked;
    const int64_t step = small ? BT_MAX_LAUNCH : (d_ferr ? ba::ferr_step(BB_MAX_LAUNCH, n, nrhs) : BB_MAX_LAUNCH);
    return ba::chunks(batch, step, [&](int64_t b0, int64_t nb) {
        return launch(c, trans, d_A + b0 * strideA, lda, strideA, d_LU + b0 * strideLU, ldlu, strideLU, n, nb, d_ipiv + b0 * strideP, strideP, nrhs,
                      d_B + b0 * strideB, ldb, strideB, d_X + b0 * strideX, ldx, strideX, it, opt(d_ferr, b0 * nrhs),
                      d_berr + b0 * nrhs, opt(d_iters, b0 * nrhs));
    });
}

// equilibration
int geequ_strided(mpf_ctx *c, const char *who, int32_t limit, const double *d_A, int64_t lda, int64_t strideA, int32_t n, int64_t batch,
                  double *d_r, double *d_c, double *d_rowcnd, double *d_colcnd, double *d_amax, int32_t *d_info) {
    int rc = ba::check_sizes(c->err, who, limit, n, batch, ONE_GEEQU);
    if (rc) return rc;
    if (n == 0 || batch == 0) return 0;
    rc = ba::check_strided(c->err, who, "A", lda, strideA, n, n, batch);
    if (rc) return rc;
    if (!d_A || !d_r || !d_c || !d_rowcnd || !d_colcnd || !d_amax || !d_info) return null_pointer(c, who);
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    if (takes_small(c, limit, n))
        return ba::chunks(batch, BT_MAX_LAUNCH, [&](int64_t b0, int64_t nb) {
            return launch_geequ_batched(c, d_A + b0 * strideA, lda, strideA, n, nb, d_r + b0 * n, d_c + b0 * n, d_rowcnd + b0, d_colcnd + b0,
                                        d_amax + b0, d_info + b0);
        });
    const int64_t step = batch < BB_MAX_LAUNCH ? batch : BB_MAX_LAUNCH;
    MPF_HIP_TRY(c, c->rb_g.grow(step * n));                         // (once, before the first launch that uses them)
    MPF_HIP_TRY(c, c->rb_part.grow(step * n));
    return ba::chunks(batch, BB_MAX_LAUNCH, [&](int64_t b0, int64_t nb) {
        return launch_geequ_batched_blocked(c, d_A + b0 * strideA, lda, strideA, n, nb, d_r + b0 * n, d_c + b0 * n, d_rowcnd + b0,
                                            d_colcnd + b0, d_amax + b0, d_info + b0, c->rb_g.get(), c->rb_part.get());
    });
}

int laqge_strided(mpf_ctx *c, const char *who, int32_t limit, int32_t rule, const double *d_A, int64_t lda, int64_t strideA, int32_t n,
                  int64_t batch, const double *d_r, const double *d_c, const double *d_rowcnd, const double *d_colcnd, const double *d_amax,
                  const int32_t *d_info, double *d_out, int32_t *d_equed, double *d_spread) {
    int rc = ba::check_sizes(c->err, who, limit, n, batch, ONE_GEEQU);
    if (rc) return rc;
    if (rule < 0 || rule > 2) { c->err = std::string(who) + ": rule must be 0, 1 or 2"; return -1; }
    if (n == 0 || batch == 0) return 0;
    rc = ba::check_strided(c->err, who, "A", lda, strideA, n, n, batch);
    if (rc) return rc;
    if (!d_A || !d_r || !d_c || !d_rowcnd || !d_colcnd || !d_amax || !d_info || !d_out || !d_equed) return null_pointer(c, who);
    const int64_t ext = ba::extent(n, batch, lda, strideA);
    if (d_out != d_A && ba::ranges_overlap((uintptr_t)d_A, ext, (uintptr_t)d_out, ext)) {
        c->err = std::string(who) + ": d_out overlaps d_A (in place is d_out == d_A)";
        return -1;
    }
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    rc = ba::chunks(batch, BT_MAX_LAUNCH, [&](int64_t b0, int64_t nb) {
        return launch_laqge_decide(c, rule, n, nb, nullptr, nullptr, d_r + b0 * n, d_c + b0 * n, d_rowcnd + b0, d_colcnd + b0, d_amax + b0,
                                   d_info + b0, d_equed + b0, opt(d_spread, 2 * b0));
    });
    if (rc) return rc;
    if (takes_small(c, limit, n))
        return ba::chunks(batch, ba::elements_step(BT_MAX_LAUNCH, (int64_t)n * n), [&](int64_t b0, int64_t nb) {
            return launch_laqge_batched(c, d_A + b0 * strideA, lda, strideA, n, nb, d_r + b0 * n, d_c + b0 * n, d_equed + b0, d_out + b0 * strideA);
        });
    return ba::chunks(batch, BB_MAX_LAUNCH, [&](int64_t b0, int64_t nb) {
        return launch_laqge_batched_blocked(c, d_A + b0 * strideA, lda, strideA, n, nb, d_r + b0 * n, d_c + b0 * n, d_equed + b0,
                                            d_out + b0 * strideA);
    });
}

// elementwise whatever n: one kernel for both entries
int lascl2_strided(mpf_ctx *c, const char *who, int32_t limit, const double *d_s, int32_t n, int64_t batch, int32_t nrhs, double *d_V,
                   int64_t ldv, int64_t strideV, const int32_t *d_equed, int32_t bit) {
    int rc = ba::check_sizes(c->err, who, limit, n, batch, ONE_GEEQU);
    if (rc) return rc;
    if (nrhs < 0) { c->err = std::string(who) + ": nrhs must not be negative"; return -1; }
    if (n == 0 || batch == 0 || nrhs == 0) return 0;
    rc = ba::check_strided(c->err, who, "V", ldv, strideV, n, nrhs, batch);
    if (rc) return rc;
    if (!d_s || !d_V) return null_pointer(c, who);
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    const int32_t kc = (int32_t)ba::elements_step(nrhs, n);        // columns per launch: n kc < 2^31
    for (int32_t k0 = 0; k0 < nrhs; k0 += kc) {
        const int32_t nk = nrhs - k0 < kc ? nrhs - k0 : kc;
        rc = ba::chunks(batch, ba::elements_step(BT_MAX_LAUNCH, (int64_t)n * nk), [&](int64_t b0, int64_t nb) {
            return launch_lascl2_batched(c, d_s + b0 * n, n, nb, nk, d_V + b0 * strideV + (int64_t)k0 * ldv, ldv, strideV, opt(d_equed, b0), bit);
        });
        if (rc) return rc;
    }
    return 0;
}
} // namespace

// ---- the entries of the strided batches: the name, the limit, where a larger matrix goes -------------------------------------------------
extern "C" {

int mpf_getrf_batched(mpf_ctx *c, double *d_A, int64_t lda, int64_t strideA, int32_t n, int64_t batch, int32_t *d_ipiv, int64_t strideP,
                      int32_t *d_info, int32_t fused) {
    if (!c) return -1;
    return getrf_strided(c, "getrf_batched", ba::SMALL_MAXN, THEN_GETRS, d_A, lda, strideA, n, batch, d_ipiv, strideP, d_info, fused);
}
int mpf_getrf_batched_blocked(mpf_ctx *c, double *d_A, int64_t lda, int64_t strideA, int32_t n, int64_t batch, int32_t *d_ipiv,
                              int64_t strideP, int32_t *d_info, int32_t fused) {
    if (!c) return -1;
    return getrf_strided(c, "getrf_batched_blocked", ba::BLOCKED_MAXN, THEN_GETRS, d_A, lda, strideA, n, batch, d_ipiv, strideP, d_info, fused);
}
int mpf_getrs_batched(mpf_ctx *c, int32_t trans, const double *d_LU, int64_t ldlu, int64_t strideLU, int32_t n, int64_t batch,
                      const int32_t *d_ipiv, int64_t strideP, int32_t nrhs, double *d_B, int64_t ldb, int64_t strideB) {
    if (!c) return -1;
    return getrs_strided(c, "getrs_batched", ba::SMALL_MAXN, THEN_GETRS, trans, d_LU, ldlu, strideLU, n, batch, d_ipiv, strideP, nrhs, d_B, ldb,
                         strideB);
}
int mpf_getrs_batched_blocked(mpf_ctx *c, int32_t trans, const double *d_LU, int64_t ldlu, int64_t strideLU, int32_t n, int64_t batch,
                              const int32_t *d_ipiv, int64_t strideP, int32_t nrhs, double *d_B, int64_t ldb, int64_t strideB) {
    if (!c) return -1;
    return getrs_strided(c, "getrs_batched_blocked", ba::BLOCKED_MAXN, THEN_GETRS, trans, d_LU, ldlu, strideLU, n, batch, d_ipiv, strideP, nrhs,
                         d_B, ldb, strideB);
}
int mpf_getri_batched(mpf_ctx *c, const double *d_LU, int64_t ldlu, int64_t strideLU, int32_t n, int64_t batch, const int32_t *d_ipiv,
                      int64_t strideP, double *d_inv, int64_t ldinv, int64_t strideInv, int32_t *d_info) {
    if (!c) return -1;
    return getri_strided(c, "getri_batched", ba::SMALL_MAXN, THEN_GETRS, d_LU, ldlu, strideLU, n, batch, d_ipiv, strideP, d_inv, ldinv, strideInv,
                         d_info);
}
int mpf_getri_batched_blocked(mpf_ctx *c, const double *d_LU, int64_t ldlu, int64_t strideLU, int32_t n, int64_t batch,
                              const int32_t *d_ipiv, int64_t strideP, double *d_inv, int64_t ldinv, int64_t strideInv, int32_t *d_info) {
    if (!c) return -1;
    return getri_strided(c, "getri_batched_blocked", ba::BLOCKED_MAXN, THEN_GETRI, d_LU, ldlu, strideLU, n, batch, d_ipiv, strideP, d_inv, ldinv,
                         strideInv, d_info);
}
int mpf_getdet_batched(mpf_ctx *c, const double *d_LU, int64_t ldlu, int64_t strideLU, int32_t n, int64_t batch, const int32_t *d_ipiv,
                       int64_t strideP, double *d_mant, int32_t *d_expo) {
    if (!c) return -1;
    return getdet_strided(c, "getdet_batched", ba::SMALL_MAXN, THEN_GETRS, d_LU, ldlu, strideLU, n, batch, d_ipiv, strideP, d_mant, d_expo);
}
int mpf_getdet_batched_blocked(mpf_ctx *c, const double *d_LU, int64_t ldlu, int64_t strideLU, int32_t n, int64_t batch,
                               const int32_t *d_ipiv, int64_t strideP, double *d_mant, int32_t *d_expo) {
    if (!c) return -1;
    return getdet_strided(c, "getdet_batched_blocked", ba::BLOCKED_MAXN, THEN_GETDET, d_LU, ldlu, strideLU, n, batch, d_ipiv, strideP, d_mant, d_expo);
}
int mpf_lange_batched(mpf_ctx *c, char norm, const double *d_A, int64_t lda, int64_t strideA, int32_t n, int64_t batch, double *d_out) {
    if (!c) return -1;
    return lange_strided(c, "lange_batched", ba::SMALL_MAXN, ONE_LANGE, norm, d_A, lda, strideA, n, batch, d_out);
}
int mpf_lange_batched_blocked(mpf_ctx *c, char norm, const double *d_A, int64_t lda, int64_t strideA, int32_t n, int64_t batch, double *d_out) {
    if (!c) return -1;
    return lange_strided(c, "lange_batched_blocked", ba::BLOCKED_MAXN, ONE_AT_A_TIME, norm, d_A, lda, strideA, n, batch, d_out);
}
int mpf_gecon_batched(mpf_ctx *c, char norm, const double *d_LU, int64_t ldlu, int64_t strideLU, int32_t n, int64_t batch,
                      const double *d_anorm, double *d_rcond, double *d_ainvnm) {
    if (!c) return -1;
    return gecon_strided(c, "gecon_batched", ba::SMALL_MAXN, ONE_GECON, norm, d_LU, ldlu, strideLU, n, batch, d_anorm, d_rcond, d_ainvnm);
}
int mpf_gecon_batched_blocked(mpf_ctx *c, char norm, const double *d_LU, int64_t ldlu, int64_t strideLU, int32_t n, int64_t batch,
                              const double *d_anorm, double *d_rcond, double *d_ainvnm) {
    if (!c) return -1;
    return gecon_strided(c, "gecon_batched_blocked", ba::BLOCKED_MAXN, ONE_AT_A_TIME, norm, d_LU, ldlu, strideLU, n, batch, d_anorm, d_rcond,
                         d_ainvnm);
}
int mpf_residual_batched(mpf_ctx *c, int32_t trans, const double *d_A, int64_t lda, int64_t strideA, int32_t n, int64_t batch, int32_t nrhs,
                         const double *d_X, int64_t ldx, int64_t strideX, const double *d_B, int64_t ldb, int64_t strideB, double *d_R,
                         int64_t ldr, int64_t strideR, double *d_W) {
    if (!c) return -1;
    return residual_strided(c, "residual_batched", ba::SMALL_MAXN, ONE_GERFS, trans, d_A, lda, strideA, n, batch, nrhs, d_X, ldx, strideX, d_B, ldb,
                            strideB, d_R, ldr, strideR, d_W);
}
int mpf_residual_batched_blocked(mpf_ctx *c, int32_t trans, const double *d_A, int64_t lda, int64_t strideA, int32_t n, int64_t batch,
                                 int32_t nrhs, const double *d_X, int64_t ldx, int64_t strideX, const double *d_B, int64_t ldb, int64_t strideB,
                                 double *d_R, int64_t ldr, int64_t strideR, double *d_W) {
    if (!c) return -1;
    return residual_strided(c, "residual_batched_blocked", ba::BLOCKED_MAXN, ONE_AT_A_TIME, trans, d_A, lda, strideA, n, batch, nrhs, d_X, ldx,
                            strideX, d_B, ldb, strideB, d_R, ldr, strideR, d_W);
}
int mpf_gerfs_batched(mpf_ctx *c, int32_t trans, const double *d_A, int64_t lda, int64_t strideA, const double *d_LU, int64_t ldlu,
                      int64_t strideLU, int32_t n, int64_t batch, const int32_t *d_ipiv, int64_t strideP, int32_t nrhs, const double *d_B,
                      int64_t ldb, int64_t strideB, double *d_X, int64_t ldx, int64_t strideX, int32_t itmax, double *d_ferr, double *d_berr,
                      int32_t *d_iters) {
    if (!c) return -1;
    return gerfs_strided(c, "gerfs_batched", ba::SMALL_MAXN, ONE_GERFS, trans, d_A, lda, strideA, d_LU, ldlu, strideLU, n, batch, d_ipiv, strideP,
                         nrhs, d_B, ldb, strideB, d_X, ldx, strideX, itmax, d_ferr, d_berr, d_iters);
}
int mpf_gerfs_batched_blocked(mpf_ctx *c, int32_t trans, const double *d_A, int64_t lda, int64_t strideA, const double *d_LU, int64_t ldlu,
                              int64_t strideLU, int32_t n, int64_t batch, const int32_t *d_ipiv, int64_t strideP, int32_t nrhs,
                              const double *d_B, int64_t ldb, int64_t strideB, double *d_X, int64_t ldx, int64_t strideX, int32_t itmax,
                              double *d_ferr, double *d_berr, int32_t *d_iters) {
    if (!c) return -1;
    return gerfs_strided(c, "gerfs_batched_blocked", ba::BLOCKED_MAXN, ONE_AT_A_TIME, trans, d_A, lda, strideA, d_LU, ldlu, strideLU, n, batch,
                         d_ipiv, strideP, nrhs, d_B, ldb, strideB, d_X, ldx, strideX, itmax, d_ferr, d_berr, d_iters);
}
int mpf_geequ_batched(mpf_ctx *c, const double *d_A, int64_t lda, int64_t strideA, int32_t n, int64_t batch, double *d_r, double *d_c,
                      double *d_rowcnd, double *d_colcnd, double *d_amax, int32_t *d_info) {
    if (!c) return -1;
    return geequ_strided(c, "geequ_batched", ba::SMALL_MAXN, d_A, lda, strideA, n, batch, d_r, d_c, d_rowcnd, d_colcnd, d_amax, d_info);
}
int mpf_geequ_batched_blocked(mpf_ctx *c, const double *d_A, int64_t lda, int64_t strideA, int32_t n, int64_t batch, double *d_r, double *d_c,
                              double *d_rowcnd, double *d_colcnd, double *d_amax, int32_t *d_info) {
    if (!c) return -1;
    return geequ_strided(c, "geequ_batched_blocked", ba::BLOCKED_MAXN, d_A, lda, strideA, n, batch, d_r, d_c, d_rowcnd, d_colcnd, d_amax, d_info);
}
int mpf_laqge_batched(mpf_ctx *c, int32_t rule, const double *d_A, int64_t lda, int64_t strideA, int32_t n, int64_t batch, const double *d_r,
                      const double *d_c, const double *d_rowcnd, const double *d_colcnd, const double *d_amax, const int32_t *d_info,
                      double *d_out, int32_t *d_equed, double *d_spread) {
    if (!c) return -1;
    return laqge_strided(c, "laqge_batched", ba::SMALL_MAXN, rule, d_A, lda, strideA, n, batch, d_r, d_c, d_rowcnd, d_colcnd, d_amax, d_info,
                         d_out, d_equed, d_spread);
}
int mpf_laqge_batched_blocked(mpf_ctx *c, int32_t rule, const double *d_A, int64_t lda, int64_t strideA, int32_t n, int64_t batch,
                              const double *d_r, const double *d_c, const double *d_rowcnd, const double *d_colcnd, const double *d_amax,
                              const int32_t *d_info, double *d_out, int32_t *d_equed, double *d_spread) {
    if (!c) return -1;
    return laqge_strided(c, "laqge_batched_blocked", ba::BLOCKED_MAXN, rule, d_A, lda, strideA, n, batch, d_r, d_c, d_rowcnd, d_colcnd, d_amax,
                         d_info, d_out, d_equed, d_spread);
}
int mpf_lascl2_batched(mpf_ctx *c, const double *d_s, int32_t n, int64_t batch, int32_t nrhs, double *d_V, int64_t ldv, int64_t strideV,
                       const int32_t *d_equed, int32_t bit) {
    if (!c) return -1;
    return lascl2_strided(c, "lascl2_batched", ba::SMALL_MAXN, d_s, n, batch, nrhs, d_V, ldv, strideV, d_equed, bit);
}
int mpf_lascl2_batched_blocked(mpf_ctx *c, const double *d_s, int32_t n, int64_t batch, int32_t nrhs, double *d_V, int64_t ldv, int64_t strideV,
                               const int32_t *d_equed, int32_t bit) {
    if (!c) return -1;
    return lascl2_strided(c, "lascl2_batched_blocked", ba::BLOCKED_MAXN, d_s, n, batch, nrhs, d_V, ldv, strideV, d_equed, bit);
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
        MPF_HIP_TRY(c, vb->d_lrow.grow(batch + 1));
        MPF_HIP_TRY(c, vb->d_ltile.grow(batch + 1));
        MPF_HIP_TRY(c, hipMemcpy(vb->d_lrow.get(), p.lrow.data(), (size_t)(batch + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
        MPF_HIP_TRY(c, hipMemcpy(vb->d_ltile.get(), p.ltile.data(), (size_t)(batch + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
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
    if (!c) return -1;
    if (!vb) { c->err = std::string(who) + ": null pointer (descriptor)"; return -1; }
    if (vb->ctx != c) { c->err = std::string(who) + ": the descriptor belongs to another context"; return -1; }
    return 0;
}
// a tall operand (right-hand sides, solutions) has a row for every row of every matrix
int vb_check_ld(mpf_ctx *c, const mpf_vbatch *vb, const char *who, const char *what, int64_t ld) {
    if (ld >= vb->plan.total_n) return 0;
    c->err = std::string(who) + ": leading dimension of " + what + " < total_n";
    return -1;
}
// f(list + i0, count, top, nmax) for every chunk of every class that is not empty
template <class F>
int vb_classes(const mpf_vbatch *vb, F f) {
    const vbatch::Plan &p = vb->plan;
    for (int k = 0; k < vbatch::NCLASS; ++k) {
        const int rc = ba::chunks(p.count[k], BT_MAX_LAUNCH, [&](int64_t i0, int64_t nb) {
            return f(vb->d_list.get() + p.start[k] + i0, nb, vbatch::CLASS_TOP[k], p.nmax[k]);
        });
        if (rc) return rc;
    }
    return 0;
}
// f(device list + first, count) for every chunk of the matrices of order 0, list[0 .. zeros)
template <class F>
int vb_zeros(const mpf_vbatch *vb, F f) {
    return ba::chunks(vb->plan.zeros, BT_MAX_LAUNCH, [&](int64_t i0, int64_t nb) { return f(vb->d_list.get() + i0, nb); });
}
// their outputs from the factor layer: info = 0, determinant (0.5, 1)
int vb_empty(mpf_ctx *c, const mpf_vbatch *vb, int32_t *info, double *mant, int32_t *expo) {
    return vb_zeros(vb, [&](const int32_t *idx, int64_t nb) { return launch_vbatched_empty(c, idx, nb, info, mant, expo); });
}
// ... and from the expert layer
int vb_refine_empty(mpf_ctx *c, const mpf_vbatch *vb, int nrhs, double *norm, double *rcond, double *ainvnm, double *berr, double *ferr,
                    int32_t *iters) {
    return vb_zeros(vb, [&](const int32_t *idx, int64_t nb) {
        return launch_refine_vbatched_empty(c, idx, nb, nrhs, norm, rcond, ainvnm, berr, ferr, iters);
    });
}
// f(device list + first, count, nmax, host orders of those entries) for every chunk of every launch group of the large list
template <class F>
int vb_large(const mpf_vbatch *vb, F f) {
    const vbatch::Plan &p = vb->plan;
    std::vector<int32_t> ns;
    for (int g = 0; g < vbatch::NGROUP; ++g) {
        const int rc = ba::chunks(p.gcount[g], BB_MAX_LAUNCH, [&](int64_t i0, int64_t nb) {
            const int64_t at = p.gstart[g] + i0;
            ns.resize((size_t)nb);
            for (int64_t i = 0; i < nb; ++i) ns[(size_t)i] = p.n[(size_t)p.list[(size_t)(at + i)]];
            return f(vb->d_list.get() + at, nb, (int)ns.back(), ns.data());
        });
        if (rc) return rc;
    }
    return 0;
}
// The expert layer's launch groups over every matrix of order >= 1, list[zeros .. batch) (vbatch_plan.h: refine_chunks; limit > 0: the
// refinement's workspace cut): f(device list + first, count, nmax, the chunk's workspace frame, its rows and tiles)
constexpr int64_t RBV_WORK_LIMIT = (int64_t)1 << 25;   // doubles (256 MB): batch_args::ferr_step's
struct RbvNeed { int64_t rows = 0, tiles = 0, count = 0; };
std::vector<vbatch::Chunk> vb_refine_chunks(const mpf_vbatch *vb, int64_t nrhs, int64_t limit, RbvNeed *need) {
    const vbatch::Plan &p = vb->plan;
    std::vector<vbatch::Chunk> ch = vbatch::refine_chunks(p.ln.data() + p.zeros, p.batch - p.zeros, BB_MAX_LAUNCH, nrhs, limit);
    for (vbatch::Chunk &k : ch) {
        k.first += p.zeros;                                          // (a list position from here on)
        if (!need) continue;
        const size_t a = (size_t)k.first, e = (size_t)(k.first + k.count);
        need->rows = std::max(need->rows, p.lrow[e] - p.lrow[a]);
        need->tiles = std::max(need->tiles, p.ltile[e] - p.ltile[a]);
        need->count = std::max(need->count, k.count);
    }
    return ch;
}
RbvWork vb_work(mpf_ctx *c, const mpf_vbatch *vb, const vbatch::Chunk &k) {
    const vbatch::Plan &p = vb->plan;
    return RbvWork{vb->d_lrow.get() + k.first, vb->d_ltile.get() + k.first, p.lrow[(size_t)k.first], p.ltile[(size_t)k.first],
                   c->rb_part.get(), c->rb_g.get(), c->rb_xm.get()};
}
BtRagged vb_arrays(const mpf_vbatch *vb) { return BtRagged{vb->d_n.get(), vb->d_off.get(), vb->d_ld.get(), vb->d_offv.get()}; }
} // namespace

extern "C" {

int mpf_getrf_vbatched(mpf_ctx *c, const mpf_vbatch *vb, double *d_A, int32_t *d_ipiv, int32_t *d_info, int32_t fused) {
    const char *who = "getrf_vbatched";
    int rc = vb_enter(c, vb, who);
    if (rc) return rc;
    if (vb->plan.batch == 0) return 0;
    if (vb->plan.total_n > 0 && (!d_A || !d_ipiv)) return null_pointer(c, who);
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    rc = vb_empty(c, vb, d_info, nullptr, nullptr);
    if (rc) return rc;
    const BtRagged v = vb_arrays(vb);
    rc = vb_classes(vb, [&](const int32_t *idx, int64_t count, int top, int nmax) {
        return launch_getrf_vbatched(c, v, idx, count, top, nmax, d_A, d_ipiv, d_info, fused != 0);
    });
    if (rc || vb->plan.large_count == 0) return rc;
    const FactorForm f = factor_form(c);
    const int nb = vbatched_blocked_nb(c->tune.batched_blocked_nb);
    return vb_large(vb, [&](const int32_t *idx, int64_t count, int nmax, const int32_t *ns) {
        for (const vbatch::Step &s : vbatch::factor_steps(ns, count, nb)) {   // nmax - s.j0 == s.rows
            const int e = launch_getrf_vbatched_blocked_step(c, v, idx + s.first, count - s.first, nmax, s.j0, nb, d_A, d_ipiv, d_info,
                                                             fused != 0, f.valu, f.stages);
            if (e) return e;
        }
        return 0;
    });
}

int mpf_getrs_vbatched(mpf_ctx *c, const mpf_vbatch *vb, int32_t trans, const double *d_LU, const int32_t *d_ipiv, int32_t nrhs, double *d_B,
                       int64_t ldb) {
    const char *who = "getrs_vbatched";
    int rc = vb_enter(c, vb, who);
    if (!rc) rc = ba::check_nrhs_trans(c->err, who, nrhs, trans);
    if (rc) return rc;
    if (vb->plan.batch == 0 || vb->plan.total_n == 0 || nrhs == 0) return 0;
    rc = vb_check_ld(c, vb, who, "B", ldb);
    if (rc) return rc;
    if (!d_LU || !d_ipiv || !d_B) return null_pointer(c, who);
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
    const char *who = "getri_vbatched";
    int rc = vb_enter(c, vb, who);
    if (rc) return rc;
    if (vb->plan.batch == 0) return 0;
    if (vb->plan.total_n > 0) {
        if (!d_LU || !d_ipiv || !d_inv) return null_pointer(c, who);
        // mpf_getri_batched's rule, on the two operands' extents
        rc = check_out_of_place(c, who, d_LU, vb->plan.extent, d_inv, vb->plan.extent);
        if (rc) return rc;
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
    const char *who = "getdet_vbatched";
    int rc = vb_enter(c, vb, who);
    if (rc) return rc;
    if (vb->plan.batch == 0) return 0;
    if (!d_mant || !d_expo || (vb->plan.total_n > 0 && (!d_LU || !d_ipiv))) return null_pointer(c, who);
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

// ---- the expert layer on a descriptor of either kind (kernels in vbatched_refine.hip) -----------------------------------------------------
// Every matrix of order >= 1 takes the ragged blocked expert kernels, whose bits for n <= 128 are the small expert entries' by contract:
// the descriptor's classes and batched_blocked_min_n play no part.
int mpf_lange_vbatched(mpf_ctx *c, const mpf_vbatch *vb, char norm, const double *d_A, double *d_out) {
    const char *who = "lange_vbatched";
    int rc = vb_enter(c, vb, who);
    if (rc) return rc;
    const int mode = ba::lange_mode(c->err, who, norm);
    if (mode < 0) return -1;
    if (vb->plan.batch == 0) return 0;
    if (!d_out || (vb->plan.total_n > 0 && !d_A)) return null_pointer(c, who);
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    rc = vb_refine_empty(c, vb, 0, d_out, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (rc) return rc;
    const BtRagged v = vb_arrays(vb);
    for (const vbatch::Chunk &k : vb_refine_chunks(vb, 0, 0, nullptr)) {
        rc = launch_lange_vbatched(c, v, vb->d_list.get() + k.first, k.count, k.nmax, mode, d_A, d_out);
        if (rc) return rc;
    }
    return 0;
}

int mpf_gecon_vbatched(mpf_ctx *c, const mpf_vbatch *vb, char norm, const double *d_LU, const double *d_anorm, double *d_rcond,
                       double *d_ainvnm) {
    const char *who = "gecon_vbatched";
    int rc = vb_enter(c, vb, who);
    if (rc) return rc;
    const int inf = ba::gecon_mode(c->err, who, norm);
    if (inf < 0) return -1;
    if (vb->plan.batch == 0) return 0;
    if (!d_rcond || (vb->plan.total_n > 0 && (!d_LU || !d_anorm))) return null_pointer(c, who);
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    rc = vb_refine_empty(c, vb, 0, nullptr, d_rcond, d_ainvnm, nullptr, nullptr, nullptr);
    if (rc) return rc;
    RbvNeed need;
    const std::vector<vbatch::Chunk> chunks = vb_refine_chunks(vb, 0, 0, &need);
    MPF_HIP_TRY(c, c->rb_part.grow(need.tiles));                    // (once, before the first launch that uses it)
    const BtRagged v = vb_arrays(vb);
    for (const vbatch::Chunk &k : chunks) {
        rc = launch_gecon_vbatched(c, v, vb->d_list.get() + k.first, vb_work(c, vb, k), k.count, k.nmax, inf, d_LU, d_anorm, d_rcond, d_ainvnm);
        if (rc) return rc;
    }
    return 0;
}

int mpf_residual_vbatched(mpf_ctx *c, const mpf_vbatch *vb, int32_t trans, const double *d_A, int32_t nrhs, const double *d_X, int64_t ldx,
                          const double *d_B, int64_t ldb, double *d_R, int64_t ldr, double *d_W) {
    const char *who = "residual_vbatched";
    int rc = vb_enter(c, vb, who);
    if (!rc) rc = ba::check_nrhs_trans(c->err, who, nrhs, trans);
    if (rc) return rc;
    if (vb->plan.batch == 0 || vb->plan.total_n == 0 || nrhs == 0) return 0;
    rc = vb_check_ld(c, vb, who, "X", ldx);
    if (!rc) rc = vb_check_ld(c, vb, who, "B", ldb);
    if (!rc) rc = vb_check_ld(c, vb, who, "R", ldr);
    if (rc) return rc;
    if (!d_A || !d_X || !d_B || !d_R) return null_pointer(c, who);
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    const BtRagged v = vb_arrays(vb);
    for (const vbatch::Chunk &k : vb_refine_chunks(vb, 0, 0, nullptr)) {
        rc = launch_residual_vbatched(c, v, vb->d_list.get() + k.first, k.count, k.nmax, trans, d_A, nrhs, d_X, ldx, d_B, ldb, d_R, ldr, d_W);
        if (rc) return rc;
    }
    return 0;
}

int mpf_gerfs_vbatched(mpf_ctx *c, const mpf_vbatch *vb, int32_t trans, const double *d_A, const double *d_LU, const int32_t *d_ipiv,
                       int32_t nrhs, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t itmax, double *d_ferr, double *d_berr,
                       int32_t *d_iters) {
    const char *who = "gerfs_vbatched";
    int rc = vb_enter(c, vb, who);
    if (!rc) rc = ba::check_nrhs_trans(c->err, who, nrhs, trans);
    if (rc) return rc;
    if (vb->plan.batch == 0 || nrhs == 0) return 0;
    if (!d_berr) return null_pointer(c, who);
    if (vb->plan.total_n > 0) {
        rc = vb_check_ld(c, vb, who, "B", ldb);
        if (!rc) rc = vb_check_ld(c, vb, who, "X", ldx);
        if (rc) return rc;
        if (!d_A || !d_LU || !d_ipiv || !d_B || !d_X) return null_pointer(c, who);
    }
    const int it = ba::clamp_itmax(itmax);
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    rc = vb_refine_empty(c, vb, nrhs, nullptr, nullptr, nullptr, d_berr, d_ferr, d_iters);
    if (rc) return rc;
    RbvNeed need;
    const std::vector<vbatch::Chunk> chunks = vb_refine_chunks(vb, nrhs, d_ferr ? RBV_WORK_LIMIT : 0, &need);
    if (d_ferr) {                                                   // (once, before the first launch that uses them)
        MPF_HIP_TRY(c, c->rb_g.grow(need.rows * nrhs));
        MPF_HIP_TRY(c, c->rb_xm.grow(need.count * nrhs));
        MPF_HIP_TRY(c, c->rb_part.grow(need.tiles * nrhs));
    }
    const BtRagged v = vb_arrays(vb);
    for (const vbatch::Chunk &k : chunks) {
        rc = launch_gerfs_vbatched(c, v, vb->d_list.get() + k.first, vb_work(c, vb, k), k.count, k.nmax, trans, d_A, d_LU, d_ipiv, nrhs, d_B,
                                   ldb, d_X, ldx, it, d_ferr, d_berr, d_iters);
        if (rc) return rc;
    }
    return 0;
}

// ---- equilibration on a descriptor of either kind (kernels in batched_equil.hip) ------------------------------------------------------------
// Every matrix of order >= 1 takes the ragged kernels, launch group by launch group of the whole ordered list (refine_chunks), the
// maxima of a chunk in the context's workspace by list position; the decision of laqge runs over the whole list, orders 0 included.
int mpf_geequ_vbatched(mpf_ctx *c, const mpf_vbatch *vb, const double *d_A, double *d_r, double *d_c, double *d_rowcnd, double *d_colcnd,
                       double *d_amax, int32_t *d_info) {
    const char *who = "geequ_vbatched";
    int rc = vb_enter(c, vb, who);
    if (rc) return rc;
    if (vb->plan.batch == 0) return 0;
    if (!d_rowcnd || !d_colcnd || !d_amax || !d_info || (vb->plan.total_n > 0 && (!d_A || !d_r || !d_c))) return null_pointer(c, who);
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    rc = vb_zeros(vb, [&](const int32_t *idx, int64_t nb) { return launch_geequ_vbatched_empty(c, idx, nb, d_rowcnd, d_colcnd, d_amax, d_info); });
    if (rc) return rc;
    RbvNeed need;
    const std::vector<vbatch::Chunk> chunks = vb_refine_chunks(vb, 0, 0, &need);
    MPF_HIP_TRY(c, c->rb_g.grow(need.rows));                        // (once, before the first launch that uses them)
    MPF_HIP_TRY(c, c->rb_part.grow(need.rows));
    const BtRagged v = vb_arrays(vb);
    for (const vbatch::Chunk &k : chunks) {
        rc = launch_geequ_vbatched(c, v, vb->d_list.get() + k.first, vb->d_lrow.get() + k.first, vb->plan.lrow[(size_t)k.first], k.count, k.nmax, d_A,
                                   d_r, d_c, d_rowcnd, d_colcnd, d_amax, d_info, c->rb_g.get(), c->rb_part.get());
        if (rc) return rc;
    }
    return 0;
}

int mpf_laqge_vbatched(mpf_ctx *c, const mpf_vbatch *vb, int32_t rule, const double *d_A, const double *d_r, const double *d_c,
                       const double *d_rowcnd, const double *d_colcnd, const double *d_amax, const int32_t *d_info, double *d_out,
                       int32_t *d_equed, double *d_spread) {
    const char *who = "laqge_vbatched";
    int rc = vb_enter(c, vb, who);
    if (rc) return rc;
    if (rule < 0 || rule > 2) { c->err = "laqge_vbatched: rule must be 0, 1 or 2"; return -1; }
    if (vb->plan.batch == 0) return 0;
    if (!d_rowcnd || !d_colcnd || !d_amax || !d_info || !d_equed || (vb->plan.total_n > 0 && (!d_A || !d_r || !d_c || !d_out)))
        return null_pointer(c, who);
    if (vb->plan.total_n > 0 && d_out != d_A && ba::ranges_overlap((uintptr_t)d_A, vb->plan.extent, (uintptr_t)d_out, vb->plan.extent)) {
        c->err = "laqge_vbatched: d_out overlaps d_A (in place is d_out == d_A)";
        return -1;
    }
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    const BtRagged v = vb_arrays(vb);
    rc = ba::chunks(vb->plan.batch, BT_MAX_LAUNCH, [&](int64_t i0, int64_t nb) {
        return launch_laqge_decide(c, rule, 0, nb, vb->d_list.get() + i0, &v, d_r, d_c, d_rowcnd, d_colcnd, d_amax, d_info, d_equed, d_spread);
    });
    if (rc) return rc;
    for (const vbatch::Chunk &k : vb_refine_chunks(vb, 0, 0, nullptr)) {
        rc = launch_laqge_vbatched(c, v, vb->d_list.get() + k.first, k.count, k.nmax, d_A, d_r, d_c, d_equed, d_out);
        if (rc) return rc;
    }
    return 0;
}

int mpf_lascl2_vbatched(mpf_ctx *c, const mpf_vbatch *vb, const double *d_s, int32_t nrhs, double *d_V, int64_t ldv, const int32_t *d_equed,
                        int32_t bit) {
    const char *who = "lascl2_vbatched";
    int rc = vb_enter(c, vb, who);
    if (rc) return rc;
    if (nrhs < 0) { c->err = "lascl2_vbatched: nrhs must not be negative"; return -1; }
    if (vb->plan.batch == 0 || vb->plan.total_n == 0 || nrhs == 0) return 0;
    rc = vb_check_ld(c, vb, who, "V", ldv);
    if (rc) return rc;
    if (!d_s || !d_V) return null_pointer(c, who);
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    const BtRagged v = vb_arrays(vb);
    constexpr int32_t KC = 1 << 16;                                 // columns per launch (a grid dimension of four columns each)
    for (int32_t k0 = 0; k0 < nrhs; k0 += KC)
        for (const vbatch::Chunk &k : vb_refine_chunks(vb, 0, 0, nullptr)) {
            rc = launch_lascl2_vbatched(c, v, vb->d_list.get() + k.first, k.count, k.nmax, d_s, nrhs - k0 < KC ? nrhs - k0 : KC,
                                        d_V + (int64_t)k0 * ldv, ldv, d_equed, bit);
            if (rc) return rc;
        }
    return 0;
}

} // extern "C"
