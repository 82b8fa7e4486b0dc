// Stand-alone driver of GmresCol (csrc/solve_rules.h), GMRES-IR's per-column decisions, for tests/test_gmres_rules_cpu.py: built with
// AddressSanitizer and UBSan and run directly.  Arguments: restart max_outer tol (clamped here as the library clamps them).  stdin is
// one column's transcript, one record per line, as tests/gmres_block_model.py recorded it:
//     O rel                 the residual check before an outer step          -> "O <outer> <go>"
//     B beta                ||M^-1 r||: the inner loop starts                -> "B <go>"
//     S n h_0 .. h_n-1 hn   inner step n - 1: the Hessenberg column          -> "S <k> <go>"
//     Y                     back substitution                                -> "Y <k> y_0 .. y_k-1" (hex floats)
// and at the end "F converged outer_iterations inner_iterations rel_residual | history".  A record that the state machine's own last
// answer rules out (a step after it said stop) ends the run with status 2.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../mixed-precision_lu_factorization_amd/csrc/solve_rules.h"

int main(int argc, char **argv) {
    if (argc != 4) return 1;
    int32_t restart = std::atoi(argv[1]), max_outer = std::atoi(argv[2]);
    const double tol = std::strtod(argv[3], nullptr);
    gmres_clamp(max_outer, restart);
    GmresCol col(restart);
    mpf_gmres_stats st{};
    int outer = 0;
    bool outer_go = true, inner_go = false;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op, tok;
        if (!(in >> op)) continue;
        auto num = [&]() { in >> tok; return std::strtod(tok.c_str(), nullptr); };
        if (op == "O") {
            if (!outer_go) { std::printf("error: outer check after the column stopped\n"); return 2; }
            outer_go = col.outer_check(st, outer, num(), max_outer, tol);
            std::printf("O %d %d\n", outer, (int)outer_go);
            ++outer;
        } else if (op == "B") {
            if (!outer_go) { std::printf("error: inner loop after the column stopped\n"); return 2; }
            inner_go = outer_go = col.begin_inner(num(), st.rel_residual, tol);
            std::printf("B %d\n", (int)inner_go);
        } else if (op == "S") {
            if (!inner_go) { std::printf("error: inner step after the inner loop ended\n"); return 2; }
            int n = 0;
            in >> n;
            if (n != col.k + 1) { std::printf("error: step %d fed as step %d\n", col.k, n - 1); return 2; }
            std::vector<double> h((size_t)n);
            for (auto &v : h) v = num();
            const double hn = num();
            inner_go = col.inner_step(st, h.data(), 1, hn);
            std::printf("S %d %d\n", col.k, (int)inner_go);
        } else if (op == "Y") {
            col.solve_y();
            inner_go = false;
            std::printf("Y %d", col.k);
            for (int i = 0; i < col.k; ++i) std::printf(" %a", col.y[(size_t)i]);
            std::printf("\n");
        } else return 1;
    }
    std::printf("F %d %d %d %a |", st.converged, st.outer_iterations, st.inner_iterations, st.rel_residual);
    for (int i = 0; i <= st.outer_iterations; ++i) std::printf(" %a", st.history[i]);
    std::printf("\n");
    return 0;
}
