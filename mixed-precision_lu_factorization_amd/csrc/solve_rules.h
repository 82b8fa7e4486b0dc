// The decisions of the solve layer, host arithmetic only (no HIP: a plain C++17 compiler takes this file, tests/solve_rules_driver.cpp
// does): when refinement stops, dlacn2's state machine, the summary column of a blocked attempt, dgerfs's constants, GMRES-IR's
// per-column decisions, dgerfsx's per-column state machine.  Every solve path -- refine_vector (solve_common.h), blk_refine_core,
// gecon_core, blk_bounds_core, mpf_gesvx_block, blk_gmres_core, blk_xrefine_core -- takes them from here.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>
#include "../../include/mpf_c.h"

// One refinement step's book-keeping: `rel` = ||r|| / ||b|| after `it` corrections.  Records it, then decides whether another
// correction follows: not at the tolerance (converged), not at max_iter (<= 31: history has 32 entries) or on a NaN, and not when two
// steps in a row each gained less than a factor 0.7 (stalled: plain refinement is not contracting, kappa(A) is too large for these factors).
inline bool ir_step(mpf_ir_stats &st, int it, double rel, int max_iter, double tol) {
    st.rel_residual = rel;
    st.history[it] = rel;
    st.iterations = it;
    if (rel <= tol) { st.converged = 1; return false; }
    if (it >= max_iter || !(rel == rel)) return false;
    if (it >= 2 && st.history[it] > 0.7 * st.history[it - 1] && st.history[it - 1] > 0.7 * st.history[it - 2]) {
        st.stalled = 1;
        return false;
    }
    return true;
}

// The summary of a blocked attempt: the column with the largest final rel_residual (a NaN counts as largest, the first one wins), so
// its `converged` says whether EVERY column converged.
inline size_t worst_column(const mpf_ir_stats *st, size_t n) {
    size_t w = 0;
    for (size_t j = 1; j < n; ++j) {
        const double a = st[j].rel_residual, b = st[w].rel_residual;
        if (b == b && (a != a || a > b)) w = j;
    }
    return w;
}

// LAPACK's constants of dgerfs and dlacn2: dlamch('E') is the relative machine epsilon 2^-53, not the spacing DBL_EPSILON
constexpr double LAPACK_EPS = 0x1p-53;
constexpr int LACN2_ITMAX = 5;
inline double gerfs_safe1(int64_t N) { return (double)(N + 1) * DBL_MIN; }   // nz * safmin
inline double gerfs_safe2(int64_t N) { return gerfs_safe1(N) / LAPACK_EPS; }

// dlacn2 (Hager / Higham estimate of ||B||_1) for one vector, as the decisions between its products; the caller forms the products
// and the reductions they need.  Sequence: 1/N vector -> B x -> first_product; sign(x) -> B^T x -> first_transposed; then, while
// live: e_j -> B x -> product; sign(x) -> B^T x -> transposed; at last the alternating vector -> B x -> final_stage.
// product / transposed return `live` and leave a column that is no longer live alone.
struct Lacn2Col {
    double est = 0;
    int iter = 1;
    int64_t j = 0;       // row of the next unit vector (the argmax of the last B^T x)
    bool live = true;    // still in the loop
    void first_product(double sum, int64_t N) { est = sum; iter = 1; live = N > 1; }   // N == 1: |B| itself, done
    void first_transposed(int64_t argmax) { j = argmax; iter = 2; }
    bool product(double sum, bool signs_repeat) {
        if (!live) return false;
        const double estold = est;
        est = sum;
        if (signs_repeat || est <= estold) live = false;   // repeated sign vector, or no growth: converged
        return live;
    }
    bool transposed(int64_t argmax, double max_abs, double x_at_jlast) {
        if (!live) return false;
        j = argmax;
        if (x_at_jlast != max_abs && iter < LACN2_ITMAX) ++iter;
        else live = false;
        return live;
    }
    void final_stage(double altsum, int64_t N) {
        const double temp = 2.0 * (altsum / (double)(3 * N));
        if (temp > est) est = temp;
    }
};

// GMRES-IR's clamps (mpf_solve_gmres_ir's): restart < 1 reads 30, at most 100; max_outer 1 .. 31 (history has 32 entries)
inline void gmres_clamp(int32_t &max_outer, int32_t &restart) {
    if (restart < 1) restart = 30;
    if (restart > 100) restart = 100;
    if (max_outer < 1) max_outer = 1;
    if (max_outer > 31) max_outer = 31;
}

// GMRES-IR for one column as the decisions between its products (mpf_solve_gmres_ir's arithmetic, tests/gmres_block_model.py); the
// caller forms the products, the orthogonalisation and the norms.  Sequence per outer step: r = b - op(A) x -> outer_check(||r|| / ||b||);
// z = M^-1 r -> begin_inner(||z||); then, while inner_step returns true: w = M^-1 op(A) v_k orthogonalised against v_0 .. v_k ->
// inner_step(h, hn); at last solve_y() and x += sum_{i < k} y[i] v_i.
struct GmresCol {
    int m = 0;           // restart length
    int k = 0;           // inner steps taken in this outer step (= basis vectors that enter x)
    double beta = 0, inner_tol = 0;
    std::vector<double> H, cs, sn, g, y;   // H[i * m + j]: the Hessenberg matrix, triangular after the rotations
    explicit GmresCol(int restart = 1) : m(restart), H((size_t)(restart + 1) * restart), cs(restart), sn(restart), g(restart + 1), y(restart) {}
    // `rel` = ||r|| / ||b|| before outer step `outer`.  Records it; true: an inner loop follows.  False: the column has stopped for good
    // -- converged at the tolerance, or not (max_outer steps done, or a NaN).
    bool outer_check(mpf_gmres_stats &st, int outer, double rel, int max_outer, double tol) const {
        st.rel_residual = rel;
        st.history[outer] = rel;
        st.outer_iterations = outer;
        if (rel <= tol) { st.converged = 1; return false; }
        return !(outer >= max_outer || !(rel == rel));
    }
    // `b` = ||M^-1 r||.  False (b is 0 or a NaN): the column has stopped for good.  Else v_0 = z / b, g = b e_0, and the inner tolerance
    // reduces the preconditioned residual far enough for this outer step to reach the target.
    bool begin_inner(double b, double rel, double tol) {
        k = 0;
        beta = b;
        if (b == 0 || !(b == b)) return false;
        std::fill(g.begin(), g.end(), 0.0);
        g[0] = b;
        inner_tol = std::max(1e-14, std::min(1e-2, 0.1 * tol / rel));
        return true;
    }
    // Column k of the Hessenberg matrix: h[i * stride] = v_i . w for i = 0 .. k (both Gram-Schmidt passes added), hn = ||w|| after them.
    // Applies the earlier rotations, forms the new one, updates g; true: another inner step follows (v_{k+1} = w / hn is needed).
    bool inner_step(mpf_gmres_stats &st, const double *h, size_t stride, double hn) {
        for (int i = 0; i <= k; ++i) H[(size_t)i * m + k] = h[(size_t)i * stride];
        H[(size_t)(k + 1) * m + k] = hn;
        for (int i = 0; i < k; ++i) {
            const double t = cs[i] * H[(size_t)i * m + k] + sn[i] * H[(size_t)(i + 1) * m + k];
            H[(size_t)(i + 1) * m + k] = -sn[i] * H[(size_t)i * m + k] + cs[i] * H[(size_t)(i + 1) * m + k];
            H[(size_t)i * m + k] = t;
        }
        const double a = H[(size_t)k * m + k], b2 = H[(size_t)(k + 1) * m + k], den = std::hypot(a, b2);
        cs[k] = den > 0 ? a / den : 1.0;
        sn[k] = den > 0 ? b2 / den : 0.0;
        H[(size_t)k * m + k] = den;
        H[(size_t)(k + 1) * m + k] = 0;
        g[k + 1] = -sn[k] * g[k];
        g[k] = cs[k] * g[k];
        st.inner_iterations++;
        ++k;
        if (std::fabs(g[k]) <= inner_tol * beta || hn == 0) return false;
        return k < m;
    }
    // back substitution: y[0 .. k)
    void solve_y() {
        for (int i = k - 1; i >= 0; --i) {
            double s2 = g[i];
            for (int j = i + 1; j < k; ++j) s2 -= H[(size_t)i * m + j] * y[j];
            y[i] = s2 / H[(size_t)i * m + i];
        }
    }
};

// mpf_gerfsx's rule for one column (mpf_c.h states it in full): LAPACK dla_gerfsx_extended's state machine with the residual precision
// fixed at "extra" -- wherever LAPACK would raise the precision, the state becomes NOPROG.  The caller forms r = b - op(A) x,
// d = op(A)^-1 r and the three measures; step() is called once per iteration and says whether x += d follows (false: the column has
// stopped for good; the caller also stops it after ithresh iterations), finish() gives the two bounds.
struct XrCol {
    enum { X_WORKING = 0, X_NOPROG = 1, X_CONV = 2, X_NAN = 3 };
    enum { Z_UNSTABLE = -1, Z_WORKING = 0, Z_NOPROG = 1, Z_CONV = 2 };
    static constexpr double RTHRESH = 0.5, DZ_UB = 0.25, HUGEVAL = DBL_MAX;
    int x_state = X_WORKING, z_state = Z_UNSTABLE;
    int corrections = 0;
    double dxratmax = 0, dzratmax = 0, final_dx_x = HUGEVAL, final_dz_z = HUGEVAL, prev_dx = HUGEVAL, prev_dz = HUGEVAL;
    double last_dx_x = HUGEVAL, last_dz = HUGEVAL;   // of the latest step (what a state still WORKING ends with)
    // normx = max |x_i|, normdx = max |d_i|, dz = max |d_i| / |x_i|
    bool step(double normx, double normdx, double dz) {
        if (normx != normx || normdx != normdx || dz != dz || std::isinf(normx) || std::isinf(normdx)) {
            x_state = X_NAN;
            return false;
        }
        const double dx_x = normx != 0 ? normdx / normx : (normdx == 0 ? 0.0 : HUGEVAL);
        const double dxrat = normdx / prev_dx, dzrat = dz / prev_dz;
        last_dx_x = dx_x;
        last_dz = dz;
        if (x_state == X_NOPROG && dxrat <= RTHRESH) x_state = X_WORKING;
        if (x_state == X_WORKING) {
            if (dx_x <= LAPACK_EPS) x_state = X_CONV;
            else if (dxrat > RTHRESH) x_state = X_NOPROG;
            else if (dxratmax < dxrat) dxratmax = dxrat;
            if (x_state > X_WORKING) final_dx_x = dx_x;
        }
        if (z_state == Z_UNSTABLE && dz <= DZ_UB) z_state = Z_WORKING;
        if (z_state == Z_NOPROG && dzrat <= RTHRESH) z_state = Z_WORKING;
        if (z_state == Z_WORKING) {
            if (dz <= LAPACK_EPS) z_state = Z_CONV;
            else if (dz > DZ_UB) { z_state = Z_UNSTABLE; dzratmax = 0; final_dz_z = HUGEVAL; }
            else if (dzrat > RTHRESH) z_state = Z_NOPROG;
            else if (dzratmax < dzrat) dzratmax = dzrat;
            if (z_state > Z_WORKING) final_dz_z = dz;
        }
        if (x_state != X_WORKING && z_state != Z_WORKING) return false;   // this iteration's correction is NOT applied, as in LAPACK
        prev_dx = normdx;
        prev_dz = dz;
        ++corrections;
        return true;
    }
    void finish(int64_t N, double &err_norm, double &err_comp) {
        if (x_state == X_NAN) { err_norm = err_comp = HUGE_VAL; return; }
        if (x_state == X_WORKING) final_dx_x = last_dx_x;
        if (z_state == Z_WORKING) final_dz_z = last_dz;
        const double err_lbnd = std::max(10.0, std::sqrt((double)N)) * LAPACK_EPS;   // dgerfsx's floor
        err_norm = std::max(final_dx_x / (1 - dxratmax), err_lbnd);
        err_comp = std::max(final_dz_z / (1 - dzratmax), err_lbnd);
    }
};
