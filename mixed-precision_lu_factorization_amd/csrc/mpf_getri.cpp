// Inverse and determinant from the factors of mpf_factor_dev (no reference counterpart; LAPACK dgetri and LINPACK dgedi's determinant):
//   mpf_getri    inv(A) = Dc inv(U) inv(L) P Dr, out of place, right-looking in three stages over the result itself; the O(N^3) part is
//                launch_dgemm_minus with K = 256
//   mpf_getdet   det(A) = mant 2^expo in one fixed order
// Kernels in getri.hip; the contracts are in include/mpf_c.h.
#include "solve_common.h"
#include <cstdio>
#include <cstring>

namespace {
constexpr int GB = 256;   // the solves' diagonal block (launch_trsv_prepare's 256 x 256 inverses)

// pivots to the host, range-checked
int fetch_ipiv(mpf_ctx *c, const char *who, const int32_t *d_ipiv, int64_t N, std::vector<int32_t> &ip) {
    ip.resize((size_t)N);
    MPF_HIP_TRY(c, hipMemcpyAsync(ip.data(), d_ipiv, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int64_t i = 0; i < N; ++i)
        if (ip[(size_t)i] < 1 || ip[(size_t)i] > N) { c->err = std::string(who) + ": ipiv entry out of range"; return -1; }
    return 0;
}
} // namespace

extern "C" {

int mpf_getri(mpf_ctx *c, const double *d_LU, int64_t ldlu, const int32_t *d_ipiv, int64_t N, const double *d_r, const double *d_c,
              double *d_inv, int64_t ldinv) {
    if (!c) return -1;
    if (N < 0) { c->err = "getri: N must not be negative"; return -1; }
    if (N == 0) return 0;
    if (ldlu < N || ldinv < N) { c->err = "getri: leading dimension < N"; return -1; }
    if (!d_LU || !d_ipiv || !d_inv) { c->err = "getri: null pointer"; return -1; }
    {   // the result is built in d_inv while the factors are still being read
        const uintptr_t a0 = (uintptr_t)d_LU, a1 = a0 + (size_t)((N - 1) * ldlu + N) * sizeof(double);
        const uintptr_t b0 = (uintptr_t)d_inv, b1 = b0 + (size_t)((N - 1) * ldinv + N) * sizeof(double);
        if (a0 < b1 && b0 < a1) { c->err = "getri: d_inv overlaps d_LU (the inverse is formed out of place)"; return -1; }
    }
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    int rc = mpf_ensure_solve_buf(c, N);
    if (rc) return rc;
    // dgetri's / dtrtri's rule: a zero on U's diagonal is reported before anything is written
    double *scal = c->solve_buf + 4 * c->solve_n, z = 0;
    rc = launch_diag_zero(c, d_LU, ldlu, N, scal);
    if (!rc) rc = read_scalars(c, scal, &z, 1);
    if (rc) return rc;
    if (z != 0) return (int)z;

    // dgetri's column interchanges, j = N - 2 .. 0, composed: column j of the result is column src[j] of inv(U) inv(L)
    std::vector<int32_t> ip, src((size_t)N);
    rc = fetch_ipiv(c, "getri", d_ipiv, N, ip);
    if (rc) return rc;
    for (int64_t j = 0; j < N; ++j) src[(size_t)j] = (int32_t)j;
    for (int64_t j = N - 2; j >= 0; --j) {
        const int64_t p = (int64_t)ip[(size_t)j] - 1;
        if (p != j) std::swap(src[(size_t)j], src[(size_t)p]);
    }
    MPF_HIP_TRY(c, hipMemcpyAsync(c->perm_buf, src.data(), (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));   // `src` is a host temporary

    const int64_t nblk = (N + GB - 1) / GB;
    MPF_HIP_TRY(c, c->getri_buf.grow(nblk * GB * GB));
    const double *invL = c->trsv_inv256, *invU = c->trsv_inv256 + nblk * GB * GB;
    double *W = d_inv, *scratch = c->getri_buf;

    const bool tl = c->tune.timeline != 0;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    auto mark = [&](int i) {
        if (!tl) return;
        if (hipEventCreate(&ev[i]) == hipSuccess) hipEventRecord(ev[i], c->stream);
    };
    auto stages = [&]() -> int {
        int r2 = launch_trsv_prepare(c, d_LU, ldlu, N);
        if (!r2) r2 = launch_getri_transpose(c, invL, scratch, nblk);
        if (!r2) r2 = launch_getri_init(c, W, ldinv, N);
        if (r2) return r2;
        mark(0);
        // stage 1: inv(U) into the upper triangle.  Block row k from the last one up: X(k, k:) = inv(U_kk) R(k, k:), then
        // R(0:k, k:) -= U(0:k, k) X(k, k:)
        for (int64_t k = nblk - 1; k >= 0; --k) {
            const int64_t kb = k * GB;
            const int w = (int)((N - kb) < GB ? (N - kb) : GB);
            r2 = launch_getri_tri(c, false, invU + k * GB * GB, W, ldinv, kb, kb, w, N - kb);
            if (!r2) r2 = launch_dgemm_minus(c, kb, N - kb, w, d_LU + kb * ldlu, ldlu, W + kb + kb * ldinv, ldinv, W + kb * ldinv, ldinv);
            if (r2) return r2;
        }
        mark(1);
        // stage 2: X L = inv(U).  Block column j from the last one down: X(:, j) = R(:, j) inv(L_jj), then
        // R(:, 0:j) -= X(:, j) L(j, 0:j)
        for (int64_t j = nblk - 1; j >= 0; --j) {
            const int64_t jb = j * GB;
            const int w = (int)((N - jb) < GB ? (N - jb) : GB);
            r2 = launch_getri_tri(c, true, scratch + j * GB * GB, W, ldinv, 0, jb, w, N);
            if (!r2) r2 = launch_dgemm_minus(c, N, jb, w, W + jb * ldinv, ldinv, d_LU + jb, ldlu, W, ldinv);
            if (r2) return r2;
        }
        mark(2);
        // stage 3: the interchanges and the scales, one pass (the transposed inverses are no longer needed: the scratch is the panel)
        r2 = launch_getri_permute(c, W, ldinv, N, c->perm_buf, d_r, d_c, scratch);
        mark(3);
        return r2;
    };
    rc = stages();
    const hipError_t se = hipStreamSynchronize(c->stream);
    if (tl && !rc && se == hipSuccess && ev[0] && ev[1] && ev[2] && ev[3]) {   // device time of the three stages
        float ms[3] = {0, 0, 0};
        for (int i = 0; i < 3; ++i) hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]);
        fprintf(stderr, "GETRI_TL %.4f %.4f %.4f\n", ms[0], ms[1], ms[2]);
    }
    for (auto e : ev) if (e) hipEventDestroy(e);
    if (rc) return rc;
    MPF_HIP_TRY(c, se);
    return 0;
}

int mpf_getdet(mpf_ctx *c, const double *d_LU, int64_t ldlu, const int32_t *d_ipiv, int64_t N, const double *d_r, const double *d_c,
               double *mant, int64_t *expo) {
    if (!c) return -1;
    if (!mant || !expo) { c->err = "getdet: null pointer"; return -1; }
    if (N < 0) { c->err = "getdet: N must not be negative"; return -1; }
    if (N == 0) { *mant = 0.5; *expo = 1; return 0; }
    if (ldlu < N) { c->err = "getdet: leading dimension < N"; return -1; }
    if (!d_LU || !d_ipiv) { c->err = "getdet: null pointer"; return -1; }
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    const int64_t nch = (N + GB - 1) / GB;
    MPF_HIP_TRY(c, c->getri_buf.grow(2 * nch + 2));
    double *out = c->getri_buf + 2 * nch;
    int rc = launch_getdet(c, d_LU, ldlu, d_ipiv, N, d_r, d_c, c->getri_buf, out);
    if (rc) return rc;
    double res[2];
    rc = read_scalars(c, out, res, 2);
    if (rc) return rc;
    *mant = res[0];
    std::memcpy(expo, &res[1], sizeof(int64_t));
    return 0;
}

} // extern "C"
