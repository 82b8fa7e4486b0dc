// The host plan of a variable-size batch (mpf_vbatch_create; contract in include/mpf_c.h): validation, prefix sums, the overlap test,
// the size classes and their order.  Plain C++ with no HIP and no context, so that a stand-alone program can exercise it
// (tests/vbatch_plan_driver.cpp, under AddressSanitizer and UBSan); tests/vbatched_model.py restates it in numpy.
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <string>
#include <vector>

namespace vbatch {

constexpr int MAXN = 128;
// Size classes by n alone: the largest order of each.  8, 16, 32: the wave forms W = 8 / 16 / 32; 48, 64: the 256-thread workgroup
// forms (H = 1); 96, 128: the 1024-thread ones (H = 2).  The workgroup forms are split in two by LDS footprint: a launch asks for the
// LDS of the largest order in its list, and (n | 1) n doubles is 18 KB at 48 against 33 KB at 64, 73 KB at 96 against 129 KB at 128 --
// with 160 KB per CU that is 8 against 4 workgroups of the H = 1 form and 2 against 1 of the H = 2 form.
constexpr int NCLASS = 7;
constexpr int CLASS_TOP[NCLASS] = {8, 16, 32, 48, 64, 96, 128};

inline int class_of(int n) {   // 1 <= n <= MAXN
    int k = 0;
    while (CLASS_TOP[k] < n) ++k;
    return k;
}

struct Plan {
    int64_t batch = 0, total_n = 0, extent = 0;
    std::vector<int32_t> n;
    std::vector<int64_t> ld, off, offv;
    // the matrices of order 0 first, then class 0, 1, ..: list[start[k] .. start[k] + count[k]) is class k, ordered by n (stable: equal
    // orders keep the batch's order), so that the matrices sharing a wave or a workgroup's teams mostly have the same n
    std::vector<int32_t> list;
    int64_t zeros = 0;                       // list[0 .. zeros): the matrices of order 0
    int64_t start[NCLASS] = {}, count[NCLASS] = {};
    int nmax[NCLASS] = {};                   // the largest order in each class (0: the class is empty)
};

// 0 and the plan, or -1 and a message
inline int plan(int64_t batch, const int32_t *n, const int64_t *ld, const int64_t *off, Plan &p, std::string &err) {
    const char *who = "vbatch_create: ";
    if (batch < 0) { err = std::string(who) + "batch must not be negative"; return -1; }
    if (batch >= ((int64_t)1 << 31)) { err = std::string(who) + "batch >= 2^31 matrices"; return -1; }
    if (batch > 0 && !n) { err = std::string(who) + "null pointer (n)"; return -1; }
    constexpr int64_t LIM = (int64_t)1 << 62;   // extents stay below it, so no sum below overflows
    p = Plan();
    p.batch = batch;
    p.n.assign(n, n + batch);
    p.ld.resize((size_t)batch);
    p.off.resize((size_t)batch);
    p.offv.resize((size_t)batch);
    int64_t run_m = 0, run_v = 0, extent = 0;
    for (int64_t b = 0; b < batch; ++b) {
        const std::string at = " (matrix " + std::to_string(b) + ")";
        const int64_t nb = n[b];
        if (nb < 0) { err = std::string(who) + "n must not be negative" + at; return -1; }
        if (nb > MAXN) {
            err = std::string(who) + "n > 128 is not a small matrix: factor it with mpf_factor_dev (and solve with mpf_getrs)" + at;
            return -1;
        }
        const int64_t l = ld ? ld[b] : nb;
        if (l < nb) { err = std::string(who) + "leading dimension < n" + at; return -1; }
        if (l >= LIM / (MAXN + 1)) { err = std::string(who) + "leading dimension out of range" + at; return -1; }
        const int64_t o = off ? off[b] : run_m;
        if (o < 0) { err = std::string(who) + "offset must not be negative" + at; return -1; }
        const int64_t span = nb > 0 ? (nb - 1) * l + nb : 0;
        if (o >= LIM || o + span >= LIM || run_m + l * nb >= LIM) { err = std::string(who) + "the operand's extent is out of range" + at; return -1; }
        p.ld[(size_t)b] = l;
        p.off[(size_t)b] = o;
        p.offv[(size_t)b] = run_v;
        run_m += l * nb;
        run_v += nb;
        if (nb > 0 && o + span > extent) extent = o + span;
    }
    p.total_n = run_v;
    p.extent = extent;
    if (off) {   // two footprints [off, off + (n - 1) ld + n) that overlap; footprints that only touch are fine.  Packed offsets cannot overlap
        std::vector<int32_t> order;
        order.reserve((size_t)batch);
        for (int64_t b = 0; b < batch; ++b)
            if (n[b] > 0) order.push_back((int32_t)b);
        std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return p.off[a] != p.off[b] ? p.off[a] < p.off[b] : a < b; });
        int64_t end = 0;      // the largest end so far (ends need not ascend with the starts)
        int32_t owner = -1;
        for (const int32_t b : order) {
            if (owner >= 0 && p.off[b] < end) {
                err = std::string(who) + "matrices " + std::to_string(std::min(owner, b)) + " and " + std::to_string(std::max(owner, b)) + " overlap";
                return -1;
            }
            const int64_t e = p.off[b] + (int64_t)(n[b] - 1) * p.ld[b] + n[b];
            if (e > end) { end = e; owner = b; }
        }
    }
    // the classes: a counting sort by n is the stable order inside every class at once
    int64_t by_n[MAXN + 2] = {};
    for (int64_t b = 0; b < batch; ++b) ++by_n[n[b] + 1];
    for (int v = 0; v <= MAXN; ++v) by_n[v + 1] += by_n[v];   // by_n[v]: where order v starts
    p.zeros = by_n[1];
    for (int k = 0; k < NCLASS; ++k) {
        const int lo = k ? CLASS_TOP[k - 1] + 1 : 1, hi = CLASS_TOP[k];
        p.start[k] = by_n[lo];
        p.count[k] = by_n[hi + 1] - by_n[lo];
        p.nmax[k] = 0;
        for (int v = lo; v <= hi; ++v)
            if (by_n[v + 1] > by_n[v]) p.nmax[k] = v;
    }
    p.list.resize((size_t)batch);
    for (int64_t b = 0; b < batch; ++b) p.list[(size_t)by_n[n[b]]++] = (int32_t)b;
    return 0;
}

} // namespace vbatch
