// The decisions of the solve layer, host arithmetic only (no HIP: a plain C++17 compiler takes this file, tests/solve_rules_driver.cpp
// does): when refinement stops, dlacn2's state machine, the summary column of a blocked attempt, dgerfs's constants.  Every solve path
// -- refine_vector (solve_common.h), blk_refine_core, gecon_core, blk_bounds_core, mpf_gesvx_block -- takes them from here.
#pragma once
#include <cfloat>
#include <cstddef>
#include <cstdint>
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
