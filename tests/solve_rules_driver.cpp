// Stand-alone driver of csrc/solve_rules.h for tests/test_solve_rules_cpu.py (host only: any C++17 compiler, sanitizers welcome).
//   solve_rules_driver lacn2          stdin: n, then the n x n matrix B row by row.  dlacn2's estimate of ||B||_1 through Lacn2Col with
//                                     host products; prints est (hex float), iter, the unit vectors' rows j and the loop's exit
//   solve_rules_driver ir MAXIT TOL   stdin: relative residuals, one per refinement step, pushed through ir_step until it says stop;
//                                     prints the stats
#include "../mixed-precision_lu_factorization_amd/csrc/solve_rules.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {
bool read_double(double &v) {
    char tok[64];
    if (std::scanf("%63s", tok) != 1) return false;
    v = std::strtod(tok, nullptr);   // (takes "nan")
    return true;
}

int run_lacn2() {
    double dn = 0;
    if (!read_double(dn) || dn < 1 || dn > 4096) { std::fprintf(stderr, "lacn2: bad n\n"); return 2; }
    const int64_t n = (int64_t)dn;
    std::vector<double> B((size_t)(n * n));
    for (auto &v : B) if (!read_double(v)) { std::fprintf(stderr, "lacn2: short matrix\n"); return 2; }
    std::vector<double> x((size_t)n), y((size_t)n), isgn((size_t)n);
    auto product = [&](bool transposed) {   // x <- B x or B^T x
        for (int64_t i = 0; i < n; ++i) {
            double s = 0;
            for (int64_t k = 0; k < n; ++k) s += (transposed ? B[(size_t)(k * n + i)] : B[(size_t)(i * n + k)]) * x[(size_t)k];
            y[(size_t)i] = s;
        }
        x = y;
    };
    auto abs_sum = [&]() { double s = 0; for (double v : x) s += std::fabs(v); return s; };
    auto to_signs = [&]() {   // x <- sign(x); does it repeat isgn?  isgn <- x
        bool repeat = true;
        for (int64_t i = 0; i < n; ++i) {
            x[(size_t)i] = x[(size_t)i] >= 0 ? 1.0 : -1.0;
            repeat = repeat && x[(size_t)i] == isgn[(size_t)i];
        }
        isgn = x;
        return repeat;
    };
    auto argmax = [&]() { int64_t j = 0; for (int64_t i = 1; i < n; ++i) if (std::fabs(x[(size_t)i]) > std::fabs(x[(size_t)j])) j = i; return j; };
    Lacn2Col col;
    std::string js, why = "n1";
    std::fill(x.begin(), x.end(), 1.0 / (double)n);
    product(false);
    col.first_product(abs_sum(), n);
    if (col.live) {
        std::fill(isgn.begin(), isgn.end(), 0.0);
        to_signs();
        product(true);
        col.first_transposed(argmax());
        for (;;) {
            js += (js.empty() ? "" : ",") + std::to_string(col.j);
            std::fill(x.begin(), x.end(), 0.0);
            x[(size_t)col.j] = 1.0;
            product(false);
            const double sum = abs_sum();
            const bool repeat = to_signs();
            if (!col.product(sum, repeat)) { why = repeat ? "signs" : "est"; break; }
            product(true);
            const int64_t jlast = col.j, jm = argmax();
            const double at_jlast = x[(size_t)jlast], mx = std::fabs(x[(size_t)jm]);
            if (!col.transposed(jm, mx, at_jlast)) { why = at_jlast != mx ? "itmax" : "jlast"; break; }
        }
        for (int64_t i = 0; i < n; ++i) x[(size_t)i] = (i % 2 ? -1.0 : 1.0) * (1.0 + (double)i / (double)(n - 1));
        product(false);
        col.final_stage(abs_sum(), n);
    }
    std::printf("est %a\niter %d\nj %s\nexit %s\n", col.est, col.iter, js.c_str(), why.c_str());
    return 0;
}

int run_ir(int max_iter, double tol) {
    if (max_iter > 31) max_iter = 31;   // the entry points' clamp: history has 32 entries
    mpf_ir_stats st{};
    int it = 0;
    for (double rel; read_double(rel); ++it)
        if (!ir_step(st, it, rel, max_iter, tol)) break;
    std::printf("iterations %d\nconverged %d\nstalled %d\nrel_residual %a\nhistory", (int)st.iterations, (int)st.converged, (int)st.stalled,
                st.rel_residual);
    for (int i = 0; i <= st.iterations; ++i) std::printf(" %a", st.history[i]);
    std::printf("\n");
    return 0;
}
} // namespace

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "lacn2")) return run_lacn2();
    if (argc == 4 && !std::strcmp(argv[1], "ir")) return run_ir(std::atoi(argv[2]), std::strtod(argv[3], nullptr));
    std::fprintf(stderr, "usage: %s lacn2 | ir MAXIT TOL   (input on stdin)\n", argv[0]);
    return 2;
}
