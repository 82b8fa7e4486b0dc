// The host plan of a variable-size batch (mpf_vbatch_create; contract in include/mpf_c.h): validation, prefix sums, the overlap test,
// the size classes and their order.  Plain C++ with no HIP and no context, so that a stand-alone program can exercise it
// (tests/vbatch_plan_driver.cpp, under AddressSanitizer and UBSan); tests/vbatched_model.py restates it in numpy.
// mpf_vbatch_create_blocked uses the same function with the larger limit and a forwarding threshold: the matrices that the fixed-size
// blocked entries would hand to the small kernels stay in the classes, the others form the large list and its launch groups
// (tests/vbatch_plan_blocked_driver.cpp, tests/vbatched_blocked_model.py).  The expert layer cuts the whole ordered list into launch
// groups of its own (refine_chunks; tests/vbatch_plan_refine_driver.cpp, tests/vbatched_refine_model.py).
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

// The limit of mpf_vbatch_create_blocked, and the launch groups of its large list by order: a launch's block size is sized for the
// largest matrix of its group, so with the tops doubling it is never more than twice what the group's smallest matrix needs (as long as
// the forwarding threshold keeps the orders below 129 out of the first group, which is the default).
constexpr int MAXN_BLOCKED = 1024;
constexpr int NGROUP = 3;
constexpr int GROUP_TOP[NGROUP] = {256, 512, 1024};

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
    // The large list (mpf_vbatch_create_blocked only): the matrices that take the blocked kernels, behind the classes in `list`, ordered
    // by n (stable) like them.  A matrix is small, and in a class, when n <= MAXN and n < min_n -- the rule by which the fixed-size
    // blocked entries forward.  list[gstart[g] .. gstart[g] + gcount[g]) is launch group g.
    int maxn = MAXN, min_n = MAXN + 1;
    int64_t large_start = 0, large_count = 0;
    int64_t gstart[NGROUP] = {}, gcount[NGROUP] = {};
    int gnmax[NGROUP] = {};                  // the largest order in each group (0: the group is empty)
    // For the expert layer (refine_chunks below), by list position: ln[i] = the order of entry i, and the sums over the entries before
    // i of their orders (lrow) and of their tiles of REFINE_CT chains (ltile), batch + 1 entries each.  A chunk [a, a + count) of the
    // list lays its workspace out by lrow[i] - lrow[a] and ltile[i] - ltile[a].
    std::vector<int32_t> ln;
    std::vector<int64_t> lrow, ltile;
};

// The launch groups of the expert layer (mpf_lange_vbatched, mpf_gecon_vbatched, mpf_residual_vbatched, mpf_gerfs_vbatched): they take
// every matrix of order >= 1 of either kind of descriptor, list[zeros .. batch), which is in ascending order of n ACROSS the classes
// and the large list -- plan() fills `list` by one counting sort by n, and the classes and groups are ranges of it.  A launch's block is
// sized for its largest matrix, so the range is cut at the tops 64, 128, 256, 512, 1024: a block is at most twice what the group's
// smallest matrix needs and never below one wave.
constexpr int NRTOP = 5;
constexpr int REFINE_TOP[NRTOP] = {64, 128, 256, 512, 1024};
constexpr int REFINE_CT = 16;                 // chains per workgroup of the reduced chains: a matrix has ceil(n / 16) tiles
struct Chunk { int64_t first, count; int nmax; };
// ns[i] = the order of entry i, ascending, 1 <= ns[i] <= 1024.  A chunk holds at most max_launch entries of one group.  limit > 0 (the
// refinement with its bound): a chunk's workspace -- batch_args::ferr_step's count, nrhs (n + 1 + tiles) doubles per matrix, summed over
// the chunk's own matrices -- also stays within `limit` doubles, with at least one matrix per chunk.  The chunks are consecutive and
// cover the list; a matrix's results do not depend on its chunk.
inline std::vector<Chunk> refine_chunks(const int32_t *ns, int64_t count, int64_t max_launch, int64_t nrhs = 0, int64_t limit = 0) {
    std::vector<Chunk> out;
    if (max_launch < 1) max_launch = 1;
    int64_t i = 0;
    while (i < count) {
        int g = 0;
        while (g < NRTOP - 1 && REFINE_TOP[g] < ns[i]) ++g;
        int64_t j = i, work = 0;
        while (j < count && j - i < max_launch && ns[j] <= REFINE_TOP[g]) {
            const int64_t w = nrhs * ((int64_t)ns[j] + 1 + (ns[j] + REFINE_CT - 1) / REFINE_CT);
            if (limit > 0 && j > i && work + w > limit) break;
            work += w;
            ++j;
        }
        out.push_back(Chunk{i, j - i, (int)ns[j - 1]});
        i = j;
    }
    return out;
}

// One panel step of the blocked factorization of `count` list entries ordered by n: the matrices still active at column j0 (n > j0) are
// a suffix of the entries; a step launches only over entries first .. count-1, sized for `rows` = the largest remaining row count.
struct Step { int j0; int64_t first; int rows; };
// ns[i] = the order of entry i, ascending, every one >= 1; nb = the panel width
inline std::vector<Step> factor_steps(const int32_t *ns, int64_t count, int nb) {
    std::vector<Step> steps;
    if (count < 1 || nb < 1) return steps;
    const int nmax = ns[count - 1];
    int64_t first = 0;
    for (int j0 = 0; j0 < nmax; j0 += nb) {
        while (ns[first] <= j0) ++first;      // (ns[count - 1] = nmax > j0: stops inside)
        steps.push_back(Step{j0, first, nmax - j0});
    }
    return steps;
}

// 0 and the plan, or -1 and a message.  maxn = MAXN: mpf_vbatch_create (every matrix in a class, min_n unused); maxn = MAXN_BLOCKED:
// mpf_vbatch_create_blocked with the forwarding threshold min_n (option batched_blocked_min_n)
inline int plan(int64_t batch, const int32_t *n, const int64_t *ld, const int64_t *off, Plan &p, std::string &err, int maxn = MAXN,
                int min_n = MAXN + 1) {
    const char *who = maxn > MAXN ? "vbatch_create_blocked: " : "vbatch_create: ";
    if (batch < 0) { err = std::string(who) + "batch must not be negative"; return -1; }
    if (batch >= ((int64_t)1 << 31)) { err = std::string(who) + "batch >= 2^31 matrices"; return -1; }
    if (batch > 0 && !n) { err = std::string(who) + "null pointer (n)"; return -1; }
    constexpr int64_t LIM = (int64_t)1 << 62;   // extents stay below it, so no sum below overflows
    p = Plan();
    p.batch = batch;
    p.maxn = maxn;
    p.min_n = maxn > MAXN ? min_n : MAXN + 1;
    p.n.assign(n, n + batch);
    p.ld.resize((size_t)batch);
    p.off.resize((size_t)batch);
    p.offv.resize((size_t)batch);
    int64_t run_m = 0, run_v = 0, extent = 0;
    for (int64_t b = 0; b < batch; ++b) {
        const std::string at = " (matrix " + std::to_string(b) + ")";
        const int64_t nb = n[b];
        if (nb < 0) { err = std::string(who) + "n must not be negative" + at; return -1; }
        if (nb > maxn) {
            if (maxn > MAXN) err = std::string(who) + "n > 1024 is not a batch-sized matrix: factor it with mpf_factor_dev (and solve with mpf_getrs)" + at;
            else err = std::string(who) + "n > 128 is not a small matrix: factor it with mpf_factor_dev (and solve with mpf_getrs)" + at;
            return -1;
        }
        const int64_t l = ld ? ld[b] : nb;
        if (l < nb) { err = std::string(who) + "leading dimension < n" + at; return -1; }
        if (l >= LIM / (maxn + 1)) { err = std::string(who) + "leading dimension out of range" + at; return -1; }
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
    // the classes and the large list: a counting sort by n is the stable order inside every class and group at once, and the small
    // matrices (n < thr) come before the large ones
    std::vector<int64_t> by_n((size_t)maxn + 2, 0);
    for (int64_t b = 0; b < batch; ++b) ++by_n[(size_t)n[b] + 1];
    for (int v = 0; v <= maxn; ++v) by_n[(size_t)v + 1] += by_n[(size_t)v];   // by_n[v]: where order v starts
    p.zeros = by_n[1];
    const int thr = std::max(1, std::min(p.min_n, MAXN + 1));   // orders 1 .. thr-1 are small
    for (int k = 0; k < NCLASS; ++k) {
        const int lo = k ? CLASS_TOP[k - 1] + 1 : 1, hi = std::min(CLASS_TOP[k], thr - 1);
        p.start[k] = by_n[(size_t)std::min(lo, thr)];
        p.count[k] = hi >= lo ? by_n[(size_t)hi + 1] - by_n[(size_t)lo] : 0;
        p.nmax[k] = 0;
        for (int v = lo; v <= hi; ++v)
            if (by_n[(size_t)v + 1] > by_n[(size_t)v]) p.nmax[k] = v;
    }
    p.large_start = thr <= maxn ? by_n[(size_t)thr] : batch;
    p.large_count = batch - p.large_start;
    for (int g = 0; g < NGROUP; ++g) {
        const int lo = std::max(thr, g ? GROUP_TOP[g - 1] + 1 : 1), hi = std::min(GROUP_TOP[g], maxn);
        p.gstart[g] = lo <= maxn ? by_n[(size_t)lo] : batch;
        p.gcount[g] = hi >= lo ? by_n[(size_t)hi + 1] - by_n[(size_t)lo] : 0;
        p.gnmax[g] = 0;
        for (int v = lo; v <= hi; ++v)
            if (by_n[(size_t)v + 1] > by_n[(size_t)v]) p.gnmax[g] = v;
    }
    p.list.resize((size_t)batch);
    for (int64_t b = 0; b < batch; ++b) p.list[(size_t)by_n[(size_t)n[b]]++] = (int32_t)b;
    // (one counting sort by n: `list` as a whole is in ascending order of n, the order-0 matrices first)
    p.ln.resize((size_t)batch);
    p.lrow.assign((size_t)batch + 1, 0);
    p.ltile.assign((size_t)batch + 1, 0);
    for (int64_t i = 0; i < batch; ++i) {
        const int32_t v = n[p.list[(size_t)i]];
        p.ln[(size_t)i] = v;
        p.lrow[(size_t)i + 1] = p.lrow[(size_t)i] + v;
        p.ltile[(size_t)i + 1] = p.ltile[(size_t)i] + (v + REFINE_CT - 1) / REFINE_CT;
    }
    return 0;
}

} // namespace vbatch
