// The '/' of the fp16 pivot panel (hgetf2_kernel.cu:108), counted once.  Contract: the IEEE binary32 quotient of the two binary16
// operands, rounded once to binary16 (= the correctly rounded binary16 quotient).  A CUDA __hdiv built on an approximate
// reciprocal (rcp.approx and a multiply, a couple of binary32 ulps off the IEEE quotient) can round to the other neighbour only
// where the IEEE quotient lies that close to a binary16 rounding boundary (a midpoint of two neighbouring binary16 values, the
// overflow threshold 65520 included).  This program counts, over all 2^32 operand pairs, the quotients within 2 binary32 ulps of
// such a boundary: an upper bound on where the two divisions could differ.  Host only:
//     g++ -O2 -std=c++17 -pthread -o hdiv_boundary_count tools/src/hdiv_boundary_count.cpp && ./hdiv_boundary_count
// Pairs with a NaN, an infinity or a zero among the operands have no finite non-zero quotient and are counted apart; the sign
// plays no part (round to nearest is symmetric), so positive operands are enumerated and the counts multiplied by four.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

static float half_value(unsigned h) {   // finite positive binary16 bit pattern -> float (exact)
    const unsigned e = (h >> 10) & 31u, f = h & 1023u;
    return e ? std::ldexp((float)(1024u | f), (int)e - 25) : std::ldexp((float)f, -24);
}

// distance of q (finite, positive) to the nearest binary16 rounding boundary, in ulps of q; a large value when there is none near
static uint32_t boundary_distance(float q) {
    uint32_t b;
    std::memcpy(&b, &q, 4);
    const int e = (int)(b >> 23) - 127;                       // q = M * 2^(e - 23), 2^23 <= M < 2^24 (never subnormal here)
    const uint32_t M = (b & 0x7FFFFFu) | 0x800000u;
    if (e >= 16) return 1u << 30;                             // beyond 65520: infinity on either side
    // boundaries are the odd multiples of half a binary16 ulp: 2^(e - 11) in the normal range, 2^-25 below 2^-14
    const int s = e >= -14 ? 12 : -2 - e;                     // ... = 2^s ulps of q
    if (s > 24) return 1u << 30;                              // q far below the first boundary, 2^-25
    const uint64_t r = (uint64_t)M & ((2ull << s) - 1), mid = 1ull << s;
    return (uint32_t)(r > mid ? r - mid : mid - r);
}

int main() {
    constexpr unsigned FIRST = 0x0001, LAST = 0x7BFF;         // positive, finite, non-zero
    const unsigned nthreads = std::thread::hardware_concurrency() ? std::thread::hardware_concurrency() : 4;
    std::vector<uint64_t> within(nthreads * 4, 0);            // per thread: distance 0, <= 1, <= 2, pairs seen
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nthreads; ++t)
        pool.emplace_back([&, t] {
            uint64_t c0 = 0, c1 = 0, c2 = 0, seen = 0;
            for (unsigned hb = FIRST + t; hb <= LAST; hb += nthreads) {
                const volatile float fb = half_value(hb);
                for (unsigned ha = FIRST; ha <= LAST; ++ha) {
                    const float q = half_value(ha) / fb;      // IEEE binary32 division
                    const uint32_t d = boundary_distance(q);
                    c0 += d == 0; c1 += d <= 1; c2 += d <= 2; ++seen;
                }
            }
            within[4 * t] = c0; within[4 * t + 1] = c1; within[4 * t + 2] = c2; within[4 * t + 3] = seen;
        });
    for (auto &th : pool) th.join();
    uint64_t c0 = 0, c1 = 0, c2 = 0, seen = 0;
    for (unsigned t = 0; t < nthreads; ++t) { c0 += within[4 * t]; c1 += within[4 * t + 1]; c2 += within[4 * t + 2]; seen += within[4 * t + 3]; }
    const uint64_t all = 1ull << 32, finite = 4 * seen;
    std::printf("{\"operand_pairs\": %llu, \"pairs_with_finite_nonzero_operands\": %llu, \"other_pairs\": %llu,\n"
                " \"quotient_on_a_boundary\": %llu, \"within_1_fp32_ulp\": %llu, \"within_2_fp32_ulps\": %llu,\n"
                " \"share_within_2_ulps_of_all_pairs\": %.6g}\n",
                (unsigned long long)all, (unsigned long long)finite, (unsigned long long)(all - finite),
                (unsigned long long)(4 * c0), (unsigned long long)(4 * c1), (unsigned long long)(4 * c2), (double)(4 * c2) / (double)all);
    return 0;
}
