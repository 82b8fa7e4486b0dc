// What the host files of the solve layer share (mpf_solve.cpp, mpf_expert.cpp, mpf_block.cpp, mpf_dist.cpp):
// the rules (solve_rules.h), the one vector refinement loop, the read-back and timing helpers.
#pragma once
#include "mpf_internal.h"
#include "solve_rules.h"
#include <chrono>
#include <cmath>

inline double ms_since(std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}
// mpf_solve.cpp: k device scalars back on the host (synchronises c->stream); ipiv = 1 .. N as the factorizations expect it on entry
int read_scalars(mpf_ctx *c, const double *d, double *out, int k);
int upload_identity_ipiv(mpf_ctx *c, int32_t *d_ipiv, int64_t N);
// out = ||v||_2 through the device scalar d_scal
inline int vec_norm2(mpf_ctx *c, const double *v, int64_t N, double *d_scal, double &out) {
    int rc = launch_norm2(c, v, N, d_scal);
    if (!rc) rc = read_scalars(c, d_scal, &out, 1);
    out = std::sqrt(out);
    return rc;
}
// mpf_expert.cpp: out = post .* op(pre .* rhs), op = (L U)^-1 P (trans = false) or P^T (L U)^-T (trans = true) on factors prepared by
// solve_setup; pre / post: scale vectors or null.  tmp (N doubles) is used by the transposed solve and wherever pre is set.
int factor_solve(mpf_ctx *c, const double *LU, int64_t ld, int64_t N, bool trans, const double *pre, const double *post, double *tmp,
                 const double *rhs, double *out);
// mpf_expert.cpp: the body of mpf_solve_ir_nrhs (trans = false) and mpf_solve_ir_trans (trans = true) after their argument checks
int solve_ir_columns(mpf_ctx *c, bool trans, const double *d_A, int64_t lda, const double *d_LU, int64_t ldlu, const int32_t *d_ipiv,
                     int64_t N, int32_t nrhs, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t max_iter, double tol,
                     mpf_ir_stats *stats);

// Classical refinement of one vector by ir_step's rules: x0 = solve(b); then r = residual(x), ||r|| / ||b|| (a zero ||b|| reads 1),
// x += solve(r).  norm(v, out): the 2-norm on the host; solve(rhs, out); residual(x, r) = b - op(A) x; r and d: the caller's scratch.
template <class Norm, class Solve, class Residual>
int refine_vector(mpf_ctx *c, int64_t N, const double *b, double *x, int32_t max_iter, double tol, mpf_ir_stats &st, double *r, double *d,
                  Norm norm, Solve solve, Residual residual) {
    double nb2 = 0, nr = 0;
    int rc = norm(b, nb2);
    if (rc) return rc;
    if (nb2 == 0) nb2 = 1;
    rc = solve(b, x);
    for (int it = 0; !rc; ++it) {
        rc = residual(x, r);
        if (!rc) rc = norm(r, nr);
        if (rc || !ir_step(st, it, nr / nb2, max_iter, tol)) break;
        rc = solve(r, d);
        if (!rc) rc = launch_axpy(c, 1.0, d, x, N);
    }
    return rc;
}
