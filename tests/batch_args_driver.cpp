// Stand-alone driver of csrc/batch_args.h for tests/test_batch_args_cpu.py (built there with AddressSanitizer and UBSan, run directly).
// stdin: one question per line; stdout: one answer per line.
//   sizes who limit n batch tail...               "ok" or "error <text>"
//   pivots who n batch strideP                    "ok" or "error <text>"
//   strided who what ld stride rows cols batch    "ok" or "error <text>"
//   overlap a n batch lda strideA b ldb strideB   "1" when the two batches of n x n matrices at addresses a and b overlap, else "0"
//   forwards n min_n                              "1" or "0"
//   chunks batch step                             the chunks as "b0:nb", in order ("-" when there is none)
//   chunks_fail batch step at                     the same when the chunk that starts at `at` returns 7, then " rc <what chunks returned>"
//   residual_step max_units max_launch nrhs       the step
//   ferr_step max_launch n nrhs                   the step
//   lange_mode who letter, gecon_mode who letter  the mode or "error <text>"
//   nrhs_trans who nrhs trans                     "ok" or "error <text>"
//   itmax itmax                                   the clamped limit
#include "../mixed-precision_lu_factorization_amd/csrc/batch_args.h"
#include <iostream>
#include <sstream>

namespace ba = batch_args;

static void answer(int rc, const std::string &err) { std::cout << (rc ? "error " + err : std::string("ok")) << '\n'; }

int main() {
    std::string ln;
    while (std::getline(std::cin, ln)) {
        std::istringstream in(ln);
        std::string cmd, who, what, err;
        long long a, b, c, d, e, f, g, h;
        in >> cmd;
        if (cmd == "sizes") {
            std::string tail;
            in >> who >> a >> b >> c;
            std::getline(in >> std::ws, tail);
            answer(ba::check_sizes(err, who.c_str(), (int32_t)a, (int32_t)b, c, tail), err);
        } else if (cmd == "pivots") {
            in >> who >> a >> b >> c;
            answer(ba::check_pivot_stride(err, who.c_str(), (int32_t)a, b, c), err);
        } else if (cmd == "strided") {
            in >> who >> what >> a >> b >> c >> d >> e;
            answer(ba::check_strided(err, who.c_str(), what.c_str(), a, b, c, d, e), err);
        } else if (cmd == "overlap") {
            in >> a >> b >> c >> d >> e >> f >> g >> h;
            std::cout << ba::ranges_overlap((uintptr_t)a, ba::extent((int32_t)b, c, d, e), (uintptr_t)f, ba::extent((int32_t)b, c, g, h)) << '\n';
        } else if (cmd == "forwards") {
            in >> a >> b;
            std::cout << ba::forwards_to_small((int32_t)a, (int32_t)b) << '\n';
        } else if (cmd == "chunks" || cmd == "chunks_fail") {
            c = -1;
            in >> a >> b;
            if (cmd == "chunks_fail") in >> c;
            std::string out;
            const int rc = ba::chunks(a, b, [&](int64_t b0, int64_t nb) {
                out += (out.empty() ? "" : " ") + std::to_string(b0) + ":" + std::to_string(nb);
                return b0 == c ? 7 : 0;
            });
            std::cout << (out.empty() ? "-" : out);
            if (cmd == "chunks_fail") std::cout << " rc " << rc;
            std::cout << '\n';
        } else if (cmd == "residual_step") {
            in >> a >> b >> c;
            std::cout << ba::residual_step(a, b, (int32_t)c) << '\n';
        } else if (cmd == "ferr_step") {
            in >> a >> b >> c;
            std::cout << ba::ferr_step(a, (int32_t)b, (int32_t)c) << '\n';
        } else if (cmd == "lange_mode" || cmd == "gecon_mode") {
            in >> who >> what;
            const int mode = cmd == "lange_mode" ? ba::lange_mode(err, who.c_str(), what.at(0)) : ba::gecon_mode(err, who.c_str(), what.at(0));
            std::cout << (mode < 0 ? "error " + err : std::to_string(mode)) << '\n';
        } else if (cmd == "nrhs_trans") {
            in >> who >> a >> b;
            answer(ba::check_nrhs_trans(err, who.c_str(), (int32_t)a, (int32_t)b), err);
        } else if (cmd == "itmax") {
            in >> a;
            std::cout << ba::clamp_itmax((int32_t)a) << '\n';
        } else {
            return 2;
        }
        if (!in) return 2;
    }
    return 0;
}
