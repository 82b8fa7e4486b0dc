// Stand-alone driver of csrc/vbatch_plan.h with the larger limit, for tests/test_vbatched_blocked_cpu.py (built there with
// AddressSanitizer and UBSan, run directly).
// stdin: mode, batch, has_ld, has_off, min_n, nb, then n[batch], ld[batch] when has_ld, off[batch] when has_off.
//   mode 0: the old call plan(batch, n, ld, off, p, err); mode 1: plan(..., MAXN_BLOCKED, min_n).
// stdout: "error <text>" or the plan, one "key values..." line each: batch, total_n, extent, ld, off, offv, zeros, class<k>, nmax,
// large (the large list), group<g>, gnmax, limits (maxn, min_n), and for every group that is not empty "steps<g>" with the triples
// (j0, first, rows) of factor_steps at panel width nb.
#include "../mixed-precision_lu_factorization_amd/csrc/vbatch_plan.h"
#include <cstdio>
#include <iostream>

template <class V>
static void line(const std::string &key, const V &v, size_t from, size_t count) {
    std::cout << key;
    for (size_t i = 0; i < count; ++i) std::cout << ' ' << (long long)v[from + i];
    std::cout << '\n';
}

int main() {
    long long mode, batch, has_ld, has_off, min_n, nb;
    if (!(std::cin >> mode >> batch >> has_ld >> has_off >> min_n >> nb)) return 2;
    const size_t len = batch > 0 ? (size_t)batch : 0;
    std::vector<int32_t> n(len);
    std::vector<int64_t> ld(len), off(len);
    for (auto &v : n) { long long t; std::cin >> t; v = (int32_t)t; }
    if (has_ld) for (auto &v : ld) { long long t; std::cin >> t; v = t; }
    if (has_off) for (auto &v : off) { long long t; std::cin >> t; v = t; }
    vbatch::Plan p;
    std::string err;
    const int64_t *pl = has_ld ? ld.data() : nullptr, *po = has_off ? off.data() : nullptr;
    const int rc = mode == 0 ? vbatch::plan(batch, n.data(), pl, po, p, err)
                             : vbatch::plan(batch, n.data(), pl, po, p, err, vbatch::MAXN_BLOCKED, (int)min_n);
    if (rc) {
        std::cout << "error " << err << '\n';
        return 0;
    }
    std::cout << "batch " << p.batch << "\ntotal_n " << p.total_n << "\nextent " << p.extent << '\n';
    line("ld", p.ld, 0, len);
    line("off", p.off, 0, len);
    line("offv", p.offv, 0, len);
    line("zeros", p.list, 0, (size_t)p.zeros);
    for (int k = 0; k < vbatch::NCLASS; ++k) line("class" + std::to_string(k), p.list, (size_t)p.start[k], (size_t)p.count[k]);
    line("nmax", p.nmax, 0, vbatch::NCLASS);
    line("large", p.list, (size_t)p.large_start, (size_t)p.large_count);
    for (int g = 0; g < vbatch::NGROUP; ++g) line("group" + std::to_string(g), p.list, (size_t)p.gstart[g], (size_t)p.gcount[g]);
    line("gnmax", p.gnmax, 0, vbatch::NGROUP);
    std::cout << "limits " << p.maxn << ' ' << p.min_n << '\n';
    for (int g = 0; g < vbatch::NGROUP; ++g) {
        if (p.gcount[g] == 0) continue;
        std::vector<int32_t> ns((size_t)p.gcount[g]);
        for (size_t i = 0; i < ns.size(); ++i) ns[i] = p.n[(size_t)p.list[(size_t)p.gstart[g] + i]];
        std::cout << "steps" << g;
        for (const vbatch::Step &s : vbatch::factor_steps(ns.data(), (int64_t)ns.size(), (int)nb))
            std::cout << ' ' << s.j0 << ' ' << s.first << ' ' << s.rows;
        std::cout << '\n';
    }
    return 0;
}
