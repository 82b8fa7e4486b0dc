// Expert solve driver (no reference counterpart; LAPACK dgetrs('T') / dlange / dgeequ / dgecon / dgesvx analogues):
//   mpf_solve_ir_trans   A^T X = B with the factors of A and fp64 refinement on A^T
//   mpf_lange            matrix norms ('1', 'I', 'M', 'F')
//   mpf_geequ            power-of-two equilibration factors
//   mpf_gecon            reciprocal condition number of the factors (dlacn2 on the device's solves)
//   mpf_gesvx            equilibrate, factor, estimate rcond, refine against the original matrix, fall back to fp64
//   mpf_gesvx_block      the same steps for many right-hand sides: blocked refinement and dgerfs's bounds on the scaled factors
//   mpf_gerpvgrw         reciprocal pivot growth of the factors (dla_gerpvgrw)
//   mpf_gesvxx_block     the same steps with the extra-precise refinement and its bounds (dgesvxx's shape), berr and pivot growth
// Kernels in solve_ext.hip; the device only ever hands scalars back to the host.
#include "solve_common.h"
#include <cfloat>

namespace {
// the context's expert-driver vectors, `len` doubles each: 0 .. 2 dlacn2 (x, sign(x), isgn; 0 also the norms' scratch),
// 3 solve scratch, 4 / 5 refinement residual / correction, 6 / 7 row / column scale factors; then 16 scalars
enum { V_X = 0, V_XS = 1, V_ISGN = 2, V_TMP = 3, V_RES = 4, V_COR = 5, V_R = 6, V_C = 7, V_COUNT = 8 };
struct Ext {
    double *base = nullptr;
    int64_t len = 0;
    double *v(int i) const { return base + (int64_t)i * len; }
    double *scal() const { return base + (int64_t)V_COUNT * len; }
};
int ext_vectors(mpf_ctx *c, int64_t len, Ext &e) {
    MPF_HIP_TRY(c, c->ext_vec.grow(V_COUNT * len + 16));
    e.base = c->ext_vec;
    e.len = len;
    return 0;
}

int lange_core(mpf_ctx *c, const Ext &e, const double *A, int64_t lda, int64_t M, int64_t N, char norm, double &out) {
    double *v = e.v(V_X), *s = e.scal();
    int rc;
    switch (norm) {
    case '1': case 'O': case 'o': rc = launch_col_abs_sums(c, A, lda, M, N, v); if (!rc) rc = launch_vec_max(c, v, N, s); break;
    case 'I': case 'i': rc = launch_row_abs_sums(c, A, lda, M, N, v); if (!rc) rc = launch_vec_max(c, v, M, s); break;
    case 'M': case 'm': rc = launch_col_max_abs(c, A, lda, M, N, nullptr, v); if (!rc) rc = launch_vec_max(c, v, N, s); break;
    case 'F': case 'f': case 'E': case 'e': rc = launch_col_sumsq(c, A, lda, M, N, v); if (!rc) rc = launch_vec_sum(c, v, N, s); break;
    default: c->err = "lange: norm must be '1', 'O', 'I', 'M' or 'F'"; return -1;
    }
    if (rc) return rc;
    rc = read_scalars(c, s, &out, 1);
    if (!rc && (norm == 'F' || norm == 'f' || norm == 'E' || norm == 'e')) out = std::sqrt(out);
    return rc;
}

// dgeequ's bookkeeping on power-of-two factors; returns info (0, i + 1 for a zero row, N + j + 1 for a zero column) or < 0
int geequ_core(mpf_ctx *c, const Ext &e, const double *A, int64_t lda, int64_t N, double *r, double *cs, double &rowcnd, double &colcnd,
               double &amax) {
    const double smlnum = DBL_MIN, bignum = 1.0 / smlnum;
    double st[3];
    double *m = e.v(V_X), *s = e.scal();
    int rc = launch_row_max_abs(c, A, lda, N, N, m);
    if (!rc) rc = launch_pow2_scale(c, m, N, r, s);
    if (!rc) rc = read_scalars(c, s, st, 3);
    if (rc) return rc;
    amax = st[1];
    rowcnd = colcnd = 0;
    if (st[2] > 0) return (int)st[2];
    rowcnd = std::max(st[0], smlnum) / std::min(st[1], bignum);
    rc = launch_col_max_abs(c, A, lda, N, N, r, m);
    if (!rc) rc = launch_pow2_scale(c, m, N, cs, s);
    if (!rc) rc = read_scalars(c, s, st, 3);
    if (rc) return rc;
    if (st[2] > 0) return (int)(N + (int64_t)st[2]);
    colcnd = std::max(st[0], smlnum) / std::min(st[1], bignum);
    return 0;
}

// x <- (L U)^-1 x (t = false) or (L U)^-T x (t = true), in place, no P; the factors are prepared (launch_trsv_prepare)
int lu_apply(mpf_ctx *c, const double *LU, int64_t ld, int64_t N, bool t, double *x) {
    if (!t) {
        int rc = launch_trsv_lower_unit(c, LU, ld, x, N);
        return rc ? rc : launch_trsv_upper(c, LU, ld, x, N);
    }
    int rc = launch_trsv_upper_t(c, LU, ld, x, N);
    return rc ? rc : launch_trsv_lower_unit_t(c, LU, ld, x, N);
}

// dlacn2 / dgecon on prepared factors: ainvnm = estimate of ||(L U)^-1||_1 (onenorm) or ||(L U)^-1||_inf
int gecon_core(mpf_ctx *c, const Ext &e, const double *LU, int64_t ld, int64_t N, bool onenorm, double &ainvnm, mpf_gecon_stats &st) {
    double *x = e.v(V_X), *xs = e.v(V_XS), *isgn = e.v(V_ISGN), *s = e.scal();
    const size_t vb = (size_t)N * sizeof(double);
    auto apply = [&](bool transposed_product) {   // dlacn2's KASE 1 (B x) or 2 (B^T x), B = (L U)^-1 ('1') or (L U)^-T ('I')
        const bool t = transposed_product == onenorm;
        (t ? st.solves_t : st.solves)++;
        return lu_apply(c, LU, ld, N, t, x);
    };
    Lacn2Col col;   // dlacn2's decisions (solve_rules.h); the products and their reductions are formed here
    double sc[3];
    int rc = launch_lacn2_fill(c, x, N, 0, 0);
    if (!rc) rc = apply(false);
    if (rc) return rc;
    if (N == 1) {
        rc = launch_dasum(c, x, 1, s);
        if (!rc) rc = read_scalars(c, s, sc, 1);
        col.first_product(sc[0], N);
        ainvnm = col.est;
        st.iterations = col.iter;
        return rc;
    }
    rc = launch_lacn2_sign(c, x, nullptr, N, xs, s);
    if (!rc) rc = read_scalars(c, s, sc, 2);
    if (rc) return rc;
    col.first_product(sc[0], N);
    MPF_HIP_TRY(c, hipMemcpyAsync(isgn, xs, vb, hipMemcpyDeviceToDevice, c->stream));
    MPF_HIP_TRY(c, hipMemcpyAsync(x, xs, vb, hipMemcpyDeviceToDevice, c->stream));
    rc = apply(true);
    if (!rc) rc = launch_idamax(c, x, N, s);
    if (!rc) rc = read_scalars(c, s, sc, 2);
    if (rc) return rc;
    col.first_transposed((int64_t)sc[1]);
    for (;;) {
        rc = launch_lacn2_fill(c, x, N, 1, col.j);
        if (!rc) rc = apply(false);
        if (!rc) rc = launch_lacn2_sign(c, x, isgn, N, xs, s);
        if (!rc) rc = read_scalars(c, s, sc, 2);
        if (rc) return rc;
        if (!col.product(sc[0], sc[1] == 0)) break;
        MPF_HIP_TRY(c, hipMemcpyAsync(isgn, xs, vb, hipMemcpyDeviceToDevice, c->stream));
        MPF_HIP_TRY(c, hipMemcpyAsync(x, xs, vb, hipMemcpyDeviceToDevice, c->stream));
        rc = apply(true);
        const int64_t jlast = col.j;
        if (!rc) rc = launch_idamax(c, x, N, s);
        if (rc) return rc;
        MPF_HIP_TRY(c, hipMemcpyAsync(s + 2, x + jlast, sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        rc = read_scalars(c, s, sc, 3);
        if (rc) return rc;
        if (!col.transposed((int64_t)sc[1], sc[0], sc[2])) break;
    }
    st.iterations = col.iter;
    // final stage: the alternating test vector
    rc = launch_lacn2_fill(c, x, N, 2, 0);
    if (!rc) rc = apply(false);
    if (!rc) rc = launch_dasum(c, x, N, s);
    if (!rc) rc = read_scalars(c, s, sc, 1);
    if (rc) return rc;
    col.final_stage(sc[0], N);
    ainvnm = col.est;
    return 0;
}
// dla_gerpvgrw: min(1, min_j amax_j / umax_j) of A (scaled by r / cs where given) against the factors' U, through V_X and one scalar
int gerpvgrw_core(mpf_ctx *c, const Ext &e, const double *A, int64_t lda, const double *LU, int64_t ldlu, int64_t N, const double *r,
                  const double *cs, double &out) {
    int rc = launch_pivot_growth_cols(c, A, lda, LU, ldlu, N, r, cs, e.v(V_X));
    if (!rc) rc = launch_vec_min1(c, e.v(V_X), N, e.scal());
    return rc ? rc : read_scalars(c, e.scal(), &out, 1);
}

// rcond from anorm and the factors; checks U's diagonal first.  The factors must be prepared.
int gecon_full(mpf_ctx *c, const Ext &e, const double *LU, int64_t ld, int64_t N, bool onenorm, double anorm, double &rcond, mpf_gecon_stats &st) {
    rcond = 0;
    if (anorm == 0) return 0;
    double z = 0;
    int rc = launch_diag_zero(c, LU, ld, N, e.scal());
    if (!rc) rc = read_scalars(c, e.scal(), &z, 1);
    if (rc || z != 0) return rc;
    double ainvnm = 0;
    rc = gecon_core(c, e, LU, ld, N, onenorm, ainvnm, st);
    if (rc) return rc;
    st.ainvnm = ainvnm;
    if (ainvnm != 0 && std::isfinite(ainvnm) && std::isfinite(anorm)) {
        rcond = (1.0 / ainvnm) / anorm;
        if (!std::isfinite(rcond)) rcond = 0;
    }
    return 0;
}

// the refinement scratch among the expert driver's vectors, or wherever else it lives (solve_ir_columns): residual, correction,
// factor_solve's temporary, one scalar
struct IrScratch { double *r, *d, *tmp, *s; };
IrScratch ir_scratch(const Ext &e) { return {e.v(V_RES), e.v(V_COR), e.v(V_TMP), e.scal()}; }

// refinement against the original op(A) (refine_vector: mpf_solve_ir's rules), x0 and the corrections through factor_solve
int refine_on_factors(mpf_ctx *c, const IrScratch &w, const double *A, int64_t lda, const double *LU, int64_t ld, int64_t N, bool trans,
                      const double *pre, const double *post, const double *b, double *x, int32_t max_iter, double tol, mpf_ir_stats &st) {
    return refine_vector(c, N, b, x, max_iter, tol, st, w.r, w.d,
                         [&](const double *v, double &out) { return vec_norm2(c, v, N, w.s, out); },
                         [&](const double *rhs, double *out) { return factor_solve(c, LU, ld, N, trans, pre, post, w.tmp, rhs, out); },
                         [&](const double *xx, double *r) { return trans ? launch_residual_t(c, A, lda, xx, b, r, N) : launch_residual(c, A, lda, xx, b, r, N); });
}

// Steps 1 .. 6 of the expert drivers (mpf_gesvx, mpf_gesvx_block, mpf_gesvxx_block): equilibrate, factor d_work, rcond, the kappa_max
// gate, one refinement attempt on the low-precision factors and, where that does not stand, fp64 factors of the same equilibrated
// matrix and a second attempt.  Everything up to the gate depends on A alone, so the drivers take the same decisions and leave the
// same factors.  `refine(pre, post, ir, stands)` runs one attempt on the factors in d_work (prepared by solve_setup), fills `ir` and
// says whether the attempt stands (the plain drivers: ir.converged); ir's ms_total is set here.  Fills `gs` except ms_total;
// pre / post are the scale vectors of the preconditioner (null where equed says none), valid while `e`, d_r and d_c are.
template <class Refine>
int gesvx_steps(mpf_ctx *c, const Ext &e, const double *d_A, int64_t lda, int64_t N, int32_t nb, double *d_work, int32_t *d_ipiv, bool tr,
                int32_t equilibrate, int32_t try_fp16, double kappa_max, double *d_r, double *d_c, mpf_gesvx_stats &gs, const double *&pre,
                const double *&post, Refine refine_attempt) {
    double *r = d_r ? d_r : e.v(V_R), *cs = d_c ? d_c : e.v(V_C);
    int rc;

    // ---- 1. equilibration and the scaled copy -------------------------------------------------------------------------
    auto t0 = std::chrono::steady_clock::now();
    if (equilibrate) {
        const int info = geequ_core(c, e, d_A, lda, N, r, cs, gs.rowcnd, gs.colcnd, gs.amax);
        if (info < 0) return info;
        if (info == 0) {
            if (equilibrate == 2) gs.equed = 3;
            else {   // dlaqge's rule
                const double small = DBL_MIN / DBL_EPSILON, large = 1.0 / small;
                const bool rows = gs.rowcnd < 0.1 || gs.amax < small || gs.amax > large;
                const bool cols = gs.colcnd < 0.1;
                gs.equed = (rows ? 1 : 0) | (cols ? 2 : 0);
            }
        }
    }
    auto scaled_copy = [&]() {
        return launch_scaled_copy(c, d_A, lda, (gs.equed & 1) ? r : nullptr, (gs.equed & 2) ? cs : nullptr, d_work, N, N, N);
    };
    rc = scaled_copy();
    if (rc) return rc;
    if (try_fp16 && gs.equed) {
        // headroom of the fp16 operands: max |Dr A Dc| into [2^13, 2^14) by one global power of two, folded into Dr
        double mx = 0;
        rc = lange_core(c, e, d_work, N, N, N, 'M', mx);
        if (rc) return rc;
        if (mx > 0 && std::isfinite(mx)) {
            const int ex = std::ilogb(mx);
            const double s = std::ldexp(1.0, 13 - ex);
            if (s != 1.0) {
                if (gs.equed & 1) rc = launch_vscale(c, r, nullptr, s, r, N);
                else {
                    std::vector<double> sv((size_t)N, s);
                    MPF_HIP_TRY(c, hipMemcpyAsync(r, sv.data(), (size_t)N * sizeof(double), hipMemcpyHostToDevice, c->stream));
                    MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));   // `sv` is a host temporary
                    gs.equed |= 1;
                }
                if (!rc) rc = scaled_copy();
                if (rc) return rc;
            }
        }
    }
    rc = lange_core(c, e, d_work, N, N, N, tr ? 'I' : '1', gs.anorm);
    if (rc) return rc;
    gs.ms_equilibrate = ms_since(t0);
    pre = tr ? ((gs.equed & 2) ? cs : nullptr) : ((gs.equed & 1) ? r : nullptr);
    post = tr ? ((gs.equed & 1) ? r : nullptr) : ((gs.equed & 2) ? cs : nullptr);

    // factor d_work (already the scaled copy) in `mode`, prepare the solves, rcond of the factors
    auto factor_and_rcond = [&](int mode, double &rcond) -> int {
        auto t1 = std::chrono::steady_clock::now();
        int r2 = upload_identity_ipiv(c, d_ipiv, N);
        if (r2) return r2;
        mpf_opts o{};
        o.trailing = mode;
        r2 = mpf_factor_dev(c, d_work, N, N, nb, d_ipiv, &o);
        if (r2 < 0) return r2;
        gs.info = r2;
        gs.ms_factor += ms_since(t1);
        t1 = std::chrono::steady_clock::now();
        mpf_gecon_stats gst{};
        r2 = solve_setup(c, d_work, N, d_ipiv, N);
        if (!r2) r2 = gecon_full(c, e, d_work, N, N, !tr, gs.anorm, rcond, gst);
        if (r2) return r2;
        gs.ms_gecon += ms_since(t1);
        return 0;
    };
    auto refine = [&](mpf_ir_stats &ir, bool &stands) -> int {
        const auto t1 = std::chrono::steady_clock::now();
        int r2 = refine_attempt(pre, post, ir, stands);
        if (!r2) MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));
        ir.ms_total = ms_since(t1);
        gs.ms_ir += ir.ms_total;
        return r2;
    };

    bool done = false;
    if (try_fp16) {
        const int mode = try_fp16 == 2 ? MPF_TRAIL_FP16X3 : MPF_TRAIL_FP16;
        gs.kappa_max = kappa_max > 0 ? kappa_max : (mode == MPF_TRAIL_FP16 ? 1e4 : 1e6);
        rc = factor_and_rcond(mode, gs.rcond_lowp);
        if (rc) return rc;
        if (!(gs.rcond_lowp > 0) || 1.0 / gs.rcond_lowp > gs.kappa_max) gs.skipped_by_rcond = 1;
        else {
            bool stands = false;
            rc = refine(gs.ir_lowp, stands);
            if (!rc) rc = solve_check_waits(c);   // (the fp64 attempt's set-up clears the give-up flag)
            if (rc) return rc;
            if (stands) { gs.path = 1; gs.rcond = gs.rcond_lowp; gs.ir_final = gs.ir_lowp; done = true; }
        }
        if (!done) { rc = scaled_copy(); if (rc) return rc; }   // the low-precision factors overwrote the copy
    }
    if (!done) {
        bool stands = false;   // (the last attempt: whatever it says, its answer is returned)
        rc = factor_and_rcond(MPF_TRAIL_FP64, gs.rcond);
        if (!rc) rc = refine(gs.ir_final, stands);
        if (rc) return rc;
        gs.path = 2;
    }
    return 0;
}
} // namespace

int factor_solve(mpf_ctx *c, const double *LU, int64_t ld, int64_t N, bool trans, const double *pre, const double *post, double *tmp,
                 const double *rhs, double *out) {
    int rc;
    if (!trans) {
        const double *src = rhs;
        if (pre) { rc = launch_vscale(c, rhs, pre, 1.0, tmp, N); if (rc) return rc; src = tmp; }
        rc = launch_gather_rows(c, src, c->perm_buf, out, N);
        if (!rc) rc = lu_apply(c, LU, ld, N, false, out);
    } else {
        rc = launch_vscale(c, rhs, pre, 1.0, tmp, N);
        if (!rc) rc = lu_apply(c, LU, ld, N, true, tmp);
        if (!rc) rc = launch_scatter_rows(c, tmp, c->perm_buf, out, N);
    }
    if (!rc && post) rc = launch_vscale(c, out, post, 1.0, out, N);
    return rc;
}

// One refinement per column on factors prepared once.  The plain solve keeps its scratch in solve_buf (residual, correction, the
// scalar: mpf_solve_ir allocates nothing else); the transposed one needs factor_solve's temporary and takes the expert driver's vectors.
int solve_ir_columns(mpf_ctx *c, bool trans, const double *d_A, int64_t lda, const double *d_LU, int64_t ldlu, const int32_t *d_ipiv,
                     int64_t N, int32_t nrhs, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t max_iter, double tol,
                     mpf_ir_stats *stats) {
    if (max_iter > 31) max_iter = 31;
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    hipEventRecord(c->ev0, c->stream);
    Ext e;
    int rc = trans ? ext_vectors(c, N, e) : 0;
    if (!rc) rc = solve_setup(c, d_LU, ldlu, d_ipiv, N);
    if (rc) return rc;
    const IrScratch w = trans ? ir_scratch(e) : IrScratch{c->solve_buf, c->solve_buf + c->solve_n, nullptr, c->solve_buf + 4 * c->solve_n};
    for (int j = 0; j < nrhs; ++j) {
        mpf_ir_stats st{};
        hipEvent_t e0 = nullptr;
        if (j > 0) { hipEventCreate(&e0); hipEventRecord(e0, c->stream); }
        rc = refine_on_factors(c, w, d_A, lda, d_LU, ldlu, N, trans, nullptr, nullptr, d_B + (int64_t)j * ldb, d_X + (int64_t)j * ldx, max_iter, tol, st);
        if (rc) { if (e0) hipEventDestroy(e0); return rc; }
        hipEventRecord(c->ev1, c->stream);
        MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));
        float ms = 0;
        hipEventElapsedTime(&ms, j > 0 ? e0 : c->ev0, c->ev1);   // the first right-hand side carries the set-up
        if (e0) hipEventDestroy(e0);
        st.ms_total = ms;
        if (stats) stats[j] = st;
    }
    return solve_check_waits(c);
}

extern "C" {

int mpf_solve_ir_trans(mpf_ctx *c, const double *d_A, int64_t lda, const double *d_LU, int64_t ldlu, const int32_t *d_ipiv,
                       int64_t N, int32_t nrhs, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t max_iter,
                       double tol, mpf_ir_stats *stats) {
    if (!c || !d_A || !d_LU || !d_ipiv || !d_B || !d_X) return -1;
    if (N <= 0 || nrhs < 0) { c->err = "solve_ir_trans: N must be positive, nrhs >= 0"; return -1; }
    if (lda < N || ldlu < N) { c->err = "solve_ir_trans: lda / ldlu < N"; return -1; }
    if (nrhs > 1 && (ldb < N || ldx < N)) { c->err = "solve_ir_trans: ldb / ldx < N"; return -1; }
    return solve_ir_columns(c, true, d_A, lda, d_LU, ldlu, d_ipiv, N, nrhs, d_B, ldb, d_X, ldx, max_iter, tol, stats);
}

int mpf_lange(mpf_ctx *c, const double *d_A, int64_t lda, int64_t M, int64_t N, char norm, double *out) {
    if (!c || !out) return -1;
    if (M < 0 || N < 0 || (M > 0 && N > 0 && (!d_A || lda < M))) { c->err = "lange: bad M / N / lda"; return -1; }
    if (M == 0 || N == 0) { *out = 0; return 0; }
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    Ext e;
    int rc = ext_vectors(c, std::max(M, N), e);
    return rc ? rc : lange_core(c, e, d_A, lda, M, N, norm, *out);
}

int mpf_geequ(mpf_ctx *c, const double *d_A, int64_t lda, int64_t N, double *d_r, double *d_c, double *rowcnd, double *colcnd,
              double *amax) {
    if (!c || !d_A || !d_r || !d_c) return -1;
    if (N <= 0 || lda < N) { c->err = "geequ: bad N / lda"; return -1; }
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    Ext e;
    int rc = ext_vectors(c, N, e);
    if (rc) return rc;
    double rc_ = 0, cc_ = 0, am = 0;
    const int info = geequ_core(c, e, d_A, lda, N, d_r, d_c, rc_, cc_, am);
    if (info < 0) return info;
    if (rowcnd) *rowcnd = rc_;
    if (colcnd) *colcnd = cc_;
    if (amax) *amax = am;
    return info;
}

int mpf_gecon(mpf_ctx *c, const double *d_LU, int64_t ldlu, int64_t N, char norm, double anorm, double *rcond, mpf_gecon_stats *stats) {
    if (!c || !d_LU || !rcond) return -1;
    if (N <= 0 || ldlu < N) { c->err = "gecon: bad N / ldlu"; return -1; }
    const bool one = norm == '1' || norm == 'O' || norm == 'o';
    if (!one && norm != 'I' && norm != 'i') { c->err = "gecon: norm must be '1', 'O' or 'I'"; return -1; }
    if (!(anorm >= 0)) { c->err = "gecon: anorm must be >= 0"; return -1; }
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    const auto t0 = std::chrono::steady_clock::now();
    mpf_gecon_stats st{};
    Ext e;
    int rc = mpf_ensure_solve_buf(c, N);
    if (!rc) rc = ext_vectors(c, N, e);
    if (rc) return rc;
    MPF_HIP_TRY(c, hipMemsetAsync(&c->ws->flags[0], 0, sizeof(int), c->stream));
    if (anorm > 0) { rc = launch_trsv_prepare(c, d_LU, ldlu, N); if (rc) return rc; }
    rc = gecon_full(c, e, d_LU, ldlu, N, one, anorm, *rcond, st);
    if (rc) return rc;
    MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));
    st.ms_total = ms_since(t0);
    if (stats) *stats = st;
    return solve_check_waits(c);
}

int mpf_gesvx(mpf_ctx *c, const double *d_A, int64_t lda, int64_t N, int32_t nb, double *d_work, int32_t *d_ipiv,
              const double *d_b, double *d_x, int32_t trans, int32_t equilibrate, int32_t try_fp16, double kappa_max,
              int32_t max_iter, double tol, double *d_r, double *d_c, mpf_gesvx_stats *stats) {
    if (!c || !d_A || !d_work || !d_ipiv || !d_b || !d_x) return -1;
    if (N <= 0 || lda < N) { c->err = "gesvx: bad N / lda"; return -1; }
    if (trans < 0 || trans > 1 || equilibrate < 0 || equilibrate > 2 || try_fp16 < 0 || try_fp16 > 2) {
        c->err = "gesvx: trans must be 0 / 1, equilibrate 0 / 1 / 2, try_fp16 0 / 1 / 2";
        return -1;
    }
    if (max_iter > 31) max_iter = 31;
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    const auto t_all = std::chrono::steady_clock::now();
    mpf_gesvx_stats gs{};
    Ext e;
    int rc = ext_vectors(c, N, e);
    if (rc) return rc;
    const bool tr = trans == 1;
    const double *pre = nullptr, *post = nullptr;
    rc = gesvx_steps(c, e, d_A, lda, N, nb, d_work, d_ipiv, tr, equilibrate, try_fp16, kappa_max, d_r, d_c, gs, pre, post,
                     [&](const double *pr, const double *po, mpf_ir_stats &ir, bool &stands) {
                         int r2 = refine_on_factors(c, ir_scratch(e), d_A, lda, d_work, N, N, tr, pr, po, d_b, d_x, max_iter, tol, ir);
                         stands = ir.converged != 0;
                         return r2;
                     });
    if (rc) return rc;
    MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));
    gs.ms_total = ms_since(t_all);
    if (stats) *stats = gs;
    rc = solve_check_waits(c);
    if (rc) return rc;
    return gs.ir_final.converged ? 0 : 1;
}

int mpf_gesvx_block(mpf_ctx *c, const double *d_A, int64_t lda, int64_t N, int32_t nb, double *d_work, int32_t *d_ipiv, int32_t nrhs,
                    const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t trans, int32_t equilibrate, int32_t try_fp16,
                    double kappa_max, int32_t max_iter, double tol, int32_t itmax, double *d_r, double *d_c, double *ferr, double *berr,
                    mpf_gesvx_stats *stats, mpf_ir_stats *ir, mpf_gerfs_stats *rfs) {
    if (!c) return -1;
    if (N <= 0 || nrhs < 0) { c->err = "gesvx_block: N must be positive, nrhs >= 0"; return -1; }
    if (lda < N || ldb < N || ldx < N) { c->err = "gesvx_block: leading dimension < N"; return -1; }
    if (trans < 0 || trans > 1 || equilibrate < 0 || equilibrate > 2 || try_fp16 < 0 || try_fp16 > 2) {
        c->err = "gesvx_block: trans must be 0 / 1, equilibrate 0 / 1 / 2, try_fp16 0 / 1 / 2";
        return -1;
    }
    if ((ferr == nullptr) != (berr == nullptr)) { c->err = "gesvx_block: ferr and berr go together (both, or both NULL)"; return -1; }
    if (nrhs == 0) return 0;
    if (!d_A || !d_work || !d_ipiv || !d_B || !d_X) { c->err = "gesvx_block: null pointer"; return -1; }
    if (max_iter > 31) max_iter = 31;
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    const auto t_all = std::chrono::steady_clock::now();
    mpf_gesvx_stats gs{};
    Ext e;
    int rc = ext_vectors(c, N, e);
    if (rc) return rc;
    const bool tr = trans == 1;
    const double *pre = nullptr, *post = nullptr;
    std::vector<mpf_ir_stats> cols((size_t)nrhs);
    const BlkRhs rhs{nrhs, d_B, ldb, d_X, ldx};
    // one attempt: all columns on the factors in d_work; the attempt's summary is its worst column
    rc = gesvx_steps(c, e, d_A, lda, N, nb, d_work, d_ipiv, tr, equilibrate, try_fp16, kappa_max, d_r, d_c, gs, pre, post,
                     [&](const double *pr, const double *po, mpf_ir_stats &worst, bool &stands) {
                         std::fill(cols.begin(), cols.end(), mpf_ir_stats{});
                         int r2 = blk_refine_core(BlkSys{c, tr, d_A, lda, d_work, N, N, pr, po}, rhs, max_iter, tol, cols.data());
                         if (r2) return r2;
                         worst = cols[worst_column(cols.data(), cols.size())];
                         stands = worst.converged != 0;
                         return 0;
                     });
    if (rc) return rc;
    const double ms_attempt = gs.ir_final.ms_total;
    for (auto &s : cols) s.ms_total = ms_attempt;
    // 7. the bounds of the ORIGINAL system on the factors that produced the answer
    std::vector<mpf_gerfs_stats> rst((size_t)nrhs);
    if (ferr) {
        const auto t1 = std::chrono::steady_clock::now();
        rc = blk_bounds_core(BlkSys{c, tr, d_A, lda, d_work, N, N, pre, post}, rhs, itmax, ferr, berr, rst.data());
        if (rc) return rc;
        MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));
        const double ms = ms_since(t1);
        for (auto &s : rst) s.ms_total = ms;
        gs.ms_ir += ms;
    }
    MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));
    gs.ms_total = ms_since(t_all);
    if (stats) *stats = gs;
    if (ir) std::copy(cols.begin(), cols.end(), ir);
    if (rfs && ferr) std::copy(rst.begin(), rst.end(), rfs);
    rc = solve_check_waits(c);
    if (rc) return rc;
    return gs.ir_final.converged ? 0 : 1;
}

int mpf_gerpvgrw(mpf_ctx *c, const double *d_A, int64_t lda, const double *d_LU, int64_t ldlu, int64_t N, const double *d_r,
                 const double *d_c, double *rpvgrw) {
    if (!c) return -1;
    if (N <= 0 || lda < N || ldlu < N) { c->err = "gerpvgrw: bad N / lda / ldlu"; return -1; }
    if (!d_A || !d_LU || !rpvgrw) { c->err = "gerpvgrw: null pointer"; return -1; }
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    Ext e;
    int rc = ext_vectors(c, N, e);
    return rc ? rc : gerpvgrw_core(c, e, d_A, lda, d_LU, ldlu, N, d_r, d_c, *rpvgrw);
}

int mpf_gesvxx_block(mpf_ctx *c, const double *d_A, int64_t lda, int64_t N, int32_t nb, double *d_work, int32_t *d_ipiv, int32_t nrhs,
                     const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t trans, int32_t equilibrate, int32_t try_fp16,
                     double kappa_max, int32_t max_iter, double tol, int32_t ithresh, double *d_r, double *d_c, double *err_norm,
                     double *err_comp, double *berr, double *rpvgrw, mpf_gesvx_stats *stats, mpf_ir_stats *ir, mpf_gerfsx_stats *xr) {
    if (!c) return -1;
    if (N <= 0 || nrhs < 0) { c->err = "gesvxx_block: N must be positive, nrhs >= 0"; return -1; }
    if (lda < N || ldb < N || ldx < N) { c->err = "gesvxx_block: leading dimension < N"; return -1; }
    if (trans < 0 || trans > 1 || equilibrate < 0 || equilibrate > 2 || try_fp16 < 0 || try_fp16 > 2) {
        c->err = "gesvxx_block: trans must be 0 / 1, equilibrate 0 / 1 / 2, try_fp16 0 / 1 / 2";
        return -1;
    }
    if (nrhs == 0) return 0;
    if (!d_A || !d_work || !d_ipiv || !d_B || !d_X || !err_norm || !err_comp) { c->err = "gesvxx_block: null pointer"; return -1; }
    if (max_iter > 31) max_iter = 31;
    if (ithresh <= 0) ithresh = 10;
    if (ithresh > 31) ithresh = 31;
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    const auto t_all = std::chrono::steady_clock::now();
    mpf_gesvx_stats gs{};
    Ext e;
    int rc = ext_vectors(c, N, e);
    if (rc) return rc;
    const bool tr = trans == 1;
    const double *pre = nullptr, *post = nullptr;
    std::vector<mpf_ir_stats> cols((size_t)nrhs);
    std::vector<mpf_gerfsx_stats> xcols((size_t)nrhs);
    const BlkRhs rhs{nrhs, d_B, ldb, d_X, ldx};
    double ms_x = 0;
    // one attempt: (a) the plain refinement of all columns on the factors in d_work, its summary the worst column; (b) the
    // extra-precise loop on that X with a fresh rule state.  It stands iff every column ends (b) converged.
    rc = gesvx_steps(c, e, d_A, lda, N, nb, d_work, d_ipiv, tr, equilibrate, try_fp16, kappa_max, d_r, d_c, gs, pre, post,
                     [&](const double *pr, const double *po, mpf_ir_stats &worst, bool &stands) {
                         const BlkSys sys{c, tr, d_A, lda, d_work, N, N, pr, po};
                         std::fill(cols.begin(), cols.end(), mpf_ir_stats{});
                         std::fill(xcols.begin(), xcols.end(), mpf_gerfsx_stats{});
                         int r2 = blk_refine_core(sys, rhs, max_iter, tol, cols.data());
                         if (r2) return r2;
                         worst = cols[worst_column(cols.data(), cols.size())];
                         MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));   // (stage (b)'s own time)
                         const auto t1 = std::chrono::steady_clock::now();
                         r2 = blk_xrefine_core(sys, rhs, ithresh, err_norm, err_comp, xcols.data(), berr);
                         if (r2) return r2;
                         MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));
                         ms_x = ms_since(t1);
                         stands = true;
                         for (const auto &q : xcols) stands = stands && q.x_state == XrCol::X_CONV;
                         return 0;
                     });
    if (rc) return rc;
    for (auto &s : cols) s.ms_total = gs.ir_final.ms_total;
    bool all = true;
    for (auto &q : xcols) { q.ms_total = ms_x; all = all && q.x_state == XrCol::X_CONV; }
    if (rpvgrw) {   // of the factors in d_work against A with the scales that were applied
        const double *r = tr ? post : pre, *cs = tr ? pre : post;
        rc = gerpvgrw_core(c, e, d_A, lda, d_work, N, N, r, cs, *rpvgrw);
        if (rc) return rc;
    }
    MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));
    gs.ms_total = ms_since(t_all);
    if (stats) *stats = gs;
    if (ir) std::copy(cols.begin(), cols.end(), ir);
    if (xr) std::copy(xcols.begin(), xcols.end(), xr);
    rc = solve_check_waits(c);
    if (rc) return rc;
    return all ? 0 : 1;
}

} // extern "C"
