// Stand-alone driver of csrc/vbatch_plan.h's launch groups for the vbatched expert layer (refine_chunks and the plan's prefix sums by
// list position), for tests/test_vbatched_refine_cpu.py (built there with AddressSanitizer and UBSan, run directly).
// stdin: mode, count, max_launch, nrhs, limit, then n[count].
//   mode 0: n is a list of orders >= 1 in ascending order; refine_chunks(n, count, max_launch, nrhs, limit).
//   mode 1: n is a batch in any order, zeros included; plan(..., MAXN_BLOCKED, min_n = 129), then refine_chunks on list[zeros .. batch).
// stdout: "chunks" with the triples (first, count, nmax); in mode 1 also "zeros", "list" (the matrices of list[zeros .. batch)), "ln",
// "lrow" and "ltile" (batch + 1 each).
#include "../mixed-precision_lu_factorization_amd/csrc/vbatch_plan.h"
#include <iostream>

template <class V>
static void line(const char *key, const V &v, size_t from, size_t count) {
    std::cout << key;
    for (size_t i = 0; i < count; ++i) std::cout << ' ' << (long long)v[from + i];
    std::cout << '\n';
}

int main() {
    long long mode, count, max_launch, nrhs, limit;
    if (!(std::cin >> mode >> count >> max_launch >> nrhs >> limit)) return 2;
    std::vector<int32_t> n(count > 0 ? (size_t)count : 0);
    for (auto &v : n) { long long t; std::cin >> t; v = (int32_t)t; }
    const int32_t *ns = n.data();
    int64_t len = count;
    vbatch::Plan p;
    if (mode == 1) {
        std::string err;
        if (vbatch::plan(count, n.data(), nullptr, nullptr, p, err, vbatch::MAXN_BLOCKED, 129)) {
            std::cout << "error " << err << '\n';
            return 0;
        }
        line("zeros", p.list, 0, (size_t)p.zeros);
        line("list", p.list, (size_t)p.zeros, (size_t)(p.batch - p.zeros));
        line("ln", p.ln, 0, p.ln.size());
        line("lrow", p.lrow, 0, p.lrow.size());
        line("ltile", p.ltile, 0, p.ltile.size());
        ns = p.ln.data() + p.zeros;
        len = p.batch - p.zeros;
    }
    std::cout << "chunks";
    for (const vbatch::Chunk &k : vbatch::refine_chunks(ns, len, max_launch, nrhs, limit)) std::cout << ' ' << k.first << ' ' << k.count << ' ' << k.nmax;
    std::cout << '\n';
    return 0;
}
