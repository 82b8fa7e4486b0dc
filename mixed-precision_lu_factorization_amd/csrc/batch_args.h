// The argument rules of the strided batched entry points (mpf_*_batched, mpf_*_batched_blocked; contracts in include/mpf_c.h, the
// entries in mpf_batched.cpp): the size check, the strided-operand check, the norm letters, the nrhs / trans refusal and the itmax clamp
// (these four also the mpf_*_vbatched entries'), getri's out-of-place test, the rule by which a blocked entry takes the small kernels,
// and the chunks of a batch longer than one launch.  Plain C++ with no HIP and no context, the error text
// through a std::string, so that a stand-alone program can exercise it (tests/batch_args_driver.cpp, under AddressSanitizer and UBSan;
// tests/test_batch_args_cpu.py holds the texts as literals) -- as vbatch_plan.h is for the variable-size half.
#pragma once
#include <cstdint>
#include <string>

namespace batch_args {

constexpr int32_t SMALL_MAXN = 128;      // the small entries (batched.hip, batched_refine.hip)
constexpr int32_t BLOCKED_MAXN = 1024;   // the blocked ones

// n and batch against the limit of the entry's family (SMALL_MAXN or BLOCKED_MAXN); tail: where the message sends a larger matrix
inline int check_sizes(std::string &err, const char *who, int32_t limit, int32_t n, int64_t batch, const std::string &tail) {
    if (n < 0 || batch < 0) { err = std::string(who) + ": n and batch must not be negative"; return -1; }
    if (n > limit) {
        err = std::string(who) + ": n > " + std::to_string(limit) + " is not a " + (limit > SMALL_MAXN ? "batch-sized" : "small") + " matrix: " + tail;
        return -1;
    }
    return 0;
}
inline int check_pivot_stride(std::string &err, const char *who, int32_t n, int64_t batch, int64_t strideP) {
    if (batch > 1 && strideP < n) { err = std::string(who) + ": stride of ipiv < n"; return -1; }
    return 0;
}
// what every entry asks of a strided batch of `rows` x `cols` column-major matrices; a batch of one has no stride
inline int check_strided(std::string &err, const char *who, const char *what, int64_t ld, int64_t stride, int64_t rows, int64_t cols,
                         int64_t batch) {
    if (ld < rows) { err = std::string(who) + ": leading dimension of " + what + " < n"; return -1; }
    if (batch > 1 && stride < ld * cols) { err = std::string(who) + ": stride of " + what + " is smaller than one matrix"; return -1; }
    return 0;
}

// The rules every layout shares (strided, blocked and, with the descriptor's checks around them, vbatched entries).
// lange's norm letter in either case: mode 0 ('1' or 'O'), 1 ('I'), 2 ('M'); -1 with the text for any other
inline int lange_mode(std::string &err, const char *who, char norm) {
    if (norm == '1' || norm == 'O' || norm == 'o') return 0;
    if (norm == 'I' || norm == 'i') return 1;
    if (norm == 'M' || norm == 'm') return 2;
    err = std::string(who) + ": norm must be '1', 'O', 'I' or 'M'";
    return -1;
}
// gecon's: 0 ('1' or 'O'), 1 ('I'); -1 with the text for any other
inline int gecon_mode(std::string &err, const char *who, char norm) {
    if (norm == '1' || norm == 'O' || norm == 'o') return 0;
    if (norm == 'I' || norm == 'i') return 1;
    err = std::string(who) + ": norm must be '1', 'O' or 'I'";
    return -1;
}
// what every solve, residual and refinement asks of nrhs and trans, in this order
inline int check_nrhs_trans(std::string &err, const char *who, int32_t nrhs, int32_t trans) {
    if (nrhs < 0) { err = std::string(who) + ": nrhs must not be negative"; return -1; }
    if (trans != 0 && trans != 1) { err = std::string(who) + ": trans must be 0 or 1"; return -1; }
    return 0;
}
// the refinement's iteration limit (mpf_gerfs's rule): the default of 5 for itmax <= 0, at most 31
inline int clamp_itmax(int32_t itmax) { return itmax <= 0 ? 5 : (itmax > 31 ? 31 : itmax); }

// the doubles from the first element of a batch of n x n matrices to its last (n, batch >= 1)
inline int64_t extent(int32_t n, int64_t batch, int64_t ld, int64_t stride) { return (batch - 1) * stride + (int64_t)(n - 1) * ld + n; }
// two ranges of doubles at addresses a and b
inline bool ranges_overlap(uintptr_t a, int64_t na, uintptr_t b, int64_t nb) {
    return a < b + (size_t)nb * sizeof(double) && b < a + (size_t)na * sizeof(double);
}

// a blocked entry takes the small entry's kernels for n below option batched_blocked_min_n (and within the small limit): the same bits
// by contract
inline bool forwards_to_small(int32_t n, int32_t min_n) { return n <= SMALL_MAXN && n < min_n; }

// f(b0, nb) for every chunk of at most `step` matrices of the batch, in order; stops at the first f that does not return 0
template <class F>
int chunks(int64_t batch, int64_t step, F f) {
    for (int64_t b0 = 0; b0 < batch; b0 += step) {
        const int rc = f(b0, batch - b0 < step ? batch - b0 : step);
        if (rc) return rc;
    }
    return 0;
}
// the residual: a launch takes at most max_units (matrix, column) pairs and max_launch matrices (nrhs >= 1)
inline int64_t residual_step(int64_t max_units, int64_t max_launch, int32_t nrhs) {
    const int64_t step = max_units / nrhs;
    return step > max_launch ? max_launch : step;
}
// the elementwise kernels of the equilibration (one thread per element, 32-bit element numbers): as many matrices of `per` >= 1
// elements each as stay below 2^31 elements and within max_launch matrices, at least one (the caller keeps per < 2^31)
inline int64_t elements_step(int64_t max_launch, int64_t per) {
    const int64_t fit = (((int64_t)1 << 31) - 1) / per;
    return fit < 1 ? 1 : (fit < max_launch ? fit : max_launch);
}
// the blocked refinement with the bound: also as many matrices as keep a chunk's workspace (n + 1 doubles per column, one per column
// and tile of 16 chains) within 256 MB, at least one; a matrix's results do not depend on the chunk
inline int64_t ferr_step(int64_t max_launch, int32_t n, int32_t nrhs) {
    const int64_t fit = ((int64_t)1 << 25) / ((int64_t)nrhs * (n + 1 + (n + 15) / 16));
    return fit < 1 ? 1 : (fit < max_launch ? fit : max_launch);
}

} // namespace batch_args
