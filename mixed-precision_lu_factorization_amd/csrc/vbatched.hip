// LU, solve, inverse and determinant of many small matrices of DIFFERENT orders (mpf_getrf_vbatched, mpf_getrs_vbatched,
// mpf_getri_vbatched, mpf_getdet_vbatched; contracts in include/mpf_c.h, descriptor and host side in mpf_batched.cpp, the host plan in
// vbatch_plan.h).
//
// The arithmetic is vbatched_body.h's: the bodies of batched.hip's fixed-size kernels, statement for statement, so a matrix's bits are
// those of the fixed-size entry on that matrix alone.  What is new here is where a matrix comes from: a kernel takes entry i of a class
// list, reads the matrix's index b = idx[i], then n[b], off[b], ld[b] and offv[b], and calls the body.  The host has put every matrix
// into the class of the form that the fixed-size entry would take for its n and ordered each class by n.
//   wave forms (class top 8, 16, 32)      the G = 64 / W matrices of a wave have their own n <= W.  The column steps run to the largest n
//                                         of the wave (wave max by __shfl_xor, then readfirstlane: the step tests stay scalar); the bodies
//                                         are compiled with RG = true, which keeps every lane in every cross-lane operation and guards the
//                                         few places where a step past a matrix's own n would otherwise change its rows.  The last wave of
//                                         a list may hold fewer than G matrices: the missing ones have n = 0.
//   workgroup forms (48, 64; 96, 128)     n is uniform per workgroup (per team in the solve's TS < 64 forms); the LDS leading dimension is
//                                         n[b] | 1; the launch's dynamic LDS is sized for the largest n in the list.
// Every launch is an ordinary launch; nothing waits for another workgroup.
#include "vbatched_body.h"

namespace {

struct bt_entry { int b, n; long long off, ld, offv; };
// entry i of the list (i < count), or n = 0
__device__ __forceinline__ bt_entry bt_fetch(const BtRagged &v, const int *idx, long long i, long long count) {
    bt_entry e = {0, 0, 0, 0, 0};
    if (i < count) {
        e.b = idx[i];
        e.n = v.n[e.b];
        e.off = v.off[e.b];
        e.ld = v.ld[e.b];
        e.offv = v.offv[e.b];
    }
    return e;
}
// the largest n among the wave's matrices, in a scalar register (every lane of the wave executes this)
template <int W>
__device__ __forceinline__ int bt_wave_nmax(int n) {
#pragma unroll
    for (int o = 32; o >= W; o >>= 1) { const int n1 = __shfl_xor(n, o); n = n1 > n ? n1 : n; }
    return __builtin_amdgcn_readfirstlane(n);
}

template <int W, bool FUSED>
__global__ __launch_bounds__(BT_T) void bt_vgetrf_wave_kernel(double *A, BtRagged v, const int *idx, long long count, int *ipiv, int *info) {
    constexpr int G = 64 / W;
    const int lane = threadIdx.x & 63, r = lane & (W - 1), g = lane / W;
    const long long i0 = ((long long)blockIdx.x * (BT_T / 64) + (threadIdx.x >> 6)) * G;
    if (i0 >= count) return;                                    // (the whole wave)
    const bt_entry e = bt_fetch(v, idx, i0 + g, count);
    const int nw = bt_wave_nmax<W>(e.n);
    bt_getrf_wave_body<W, FUSED, true>(A + e.off, e.ld, e.n, nw, r < e.n, ipiv + e.offv, info ? info + e.b : nullptr);
}

template <bool FUSED, int H>
__global__ __launch_bounds__(H == 1 ? 256 : 1024) void bt_vgetrf_wg_kernel(double *A, BtRagged v, const int *idx, int *ipiv, int *info) {
    const bt_entry e = bt_fetch(v, idx, blockIdx.x, (long long)gridDim.x);
    bt_getrf_wg_body<FUSED, H>(A + e.off, e.ld, e.n, ipiv + e.offv, info ? info + e.b : nullptr);
}

// region: the bytes of LDS between two teams (bt_getrs_lds of the list's largest n)
template <int H, int TS>
__global__ __launch_bounds__(BT_T) void bt_vgetrs_kernel(int trans, const double *LU, BtRagged v, const int *idx, long long count, const int *ipiv,
                                                        int nrhs, double *B, long long ldb, unsigned region) {
    const int tid = threadIdx.x, team = tid / TS, tt = tid - team * TS;
    const long long i = (long long)blockIdx.x * (BT_T / TS) + team;
    const bt_entry e = bt_fetch(v, idx, i, count);
    int nw = e.n;
    if (TS < 64) nw = bt_wave_nmax<TS < 64 ? TS : 64>(e.n);     // (every wave of the workgroup has a team of the list or none: uniform per wave)
    double *T = (double *)(bt_smem + (size_t)team * region);
    bt_getrs_body<H, TS, (TS < 64)>(trans, LU + e.off, e.ld, e.n, nw, i < count, ipiv + e.offv, nrhs, B + e.offv, ldb, T, tt);
}

template <int W>
__global__ __launch_bounds__(BT_T) void bt_vgetri_wave_kernel(const double *LU, BtRagged v, const int *idx, long long count, const int *ipiv,
                                                             double *inv, int *info) {
    constexpr int G = 64 / W;
    const int lane = threadIdx.x & 63, r = lane & (W - 1), g = lane / W;
    const long long i0 = ((long long)blockIdx.x * (BT_T / 64) + (threadIdx.x >> 6)) * G;
    if (i0 >= count) return;                                    // (the whole wave)
    const bt_entry e = bt_fetch(v, idx, i0 + g, count);
    const int nw = bt_wave_nmax<W>(e.n);
    bt_getri_wave_body<W, true>(LU + e.off, e.ld, e.n, nw, r < e.n, ipiv + e.offv, inv + e.off, e.ld, info ? info + e.b : nullptr);
}

template <int H>
__global__ __launch_bounds__(H == 1 ? 256 : 1024) void bt_vgetri_wg_kernel(const double *LU, BtRagged v, const int *idx, const int *ipiv, double *inv,
                                                                          int *info) {
    const bt_entry e = bt_fetch(v, idx, blockIdx.x, (long long)gridDim.x);
    bt_getri_wg_body<H>(LU + e.off, e.ld, e.n, ipiv + e.offv, inv + e.off, e.ld, info ? info + e.b : nullptr);
}

template <int TS>
__global__ __launch_bounds__(BT_T) void bt_vgetdet_kernel(const double *LU, BtRagged v, const int *idx, long long count, const int *ipiv, double *mant,
                                                         int *expo) {
    const long long i = TS == 1 ? (long long)blockIdx.x * BT_T + threadIdx.x : (long long)blockIdx.x * (BT_T / 64) + (threadIdx.x >> 6);
    if (i >= count) return;                                      // (TS = 64: the whole wave)
    const bt_entry e = bt_fetch(v, idx, i, count);
    bt_getdet_body<TS>(LU + e.off, e.ld, e.n, ipiv + e.offv, mant + e.b, expo + e.b);
}

__global__ __launch_bounds__(BT_T) void bt_vempty_kernel(const int *idx, long long count, int *info, double *mant, int *expo) {
    const long long i = (long long)blockIdx.x * BT_T + threadIdx.x;
    if (i >= count) return;
    const int b = idx[i];
    if (info) info[b] = 0;
    if (mant) { mant[b] = 0.5; expo[b] = 1; }                    // the empty product, mpf_getdet's N = 0 case
}

int bt_vattrs(mpf_ctx *c) {
    if (c->attr_done & ATTR_VBATCHED) return 0;
    const void *ks[] = {(const void *)bt_vgetrf_wg_kernel<false, 1>, (const void *)bt_vgetrf_wg_kernel<true, 1>,
                        (const void *)bt_vgetrf_wg_kernel<false, 2>, (const void *)bt_vgetrf_wg_kernel<true, 2>,
                        (const void *)bt_vgetri_wg_kernel<1>, (const void *)bt_vgetri_wg_kernel<2>,
                        (const void *)bt_vgetrs_kernel<1, 8>, (const void *)bt_vgetrs_kernel<1, 16>, (const void *)bt_vgetrs_kernel<1, 32>,
                        (const void *)bt_vgetrs_kernel<1, 256>, (const void *)bt_vgetrs_kernel<2, 256>};
    for (const void *k : ks) MPF_HIP_TRY(c, hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    c->attr_done |= ATTR_VBATCHED;
    return 0;
}

bool bt_vrange(mpf_ctx *c, const char *who, int64_t count, int top, int nmax) {
    const bool ok = count <= BT_MAX_LAUNCH && nmax >= 1 && nmax <= top && top <= BT_MAXN;
    if (!ok) c->err = std::string(who) + ": size out of range";
    return ok;
}

} // namespace

// ---- launchers: one launch each on count <= BT_MAX_LAUNCH entries of one class list (the host splits longer lists) -----------------------
int launch_getrf_vbatched(mpf_ctx *c, const BtRagged &v, const int32_t *idx, int64_t count, int top, int nmax, double *A, int *ipiv, int *info,
                          int fused) {
    if (count < 1) return 0;
    if (!bt_vrange(c, "launch_getrf_vbatched", count, top, nmax)) return -1;
    if (top <= 32) {
#define BT_WAVE(W_)                                                                                                                  \
        do {                                                                                                                         \
            const long long per = (BT_T / W_);                                                                                       \
            const unsigned g = (unsigned)((count + per - 1) / per);                                                                  \
            if (fused) bt_vgetrf_wave_kernel<W_, true><<<g, BT_T, 0, c->stream>>>(A, v, idx, count, ipiv, info);                      \
            else bt_vgetrf_wave_kernel<W_, false><<<g, BT_T, 0, c->stream>>>(A, v, idx, count, ipiv, info);                           \
        } while (0)
        if (top <= 8) BT_WAVE(8);
        else if (top <= 16) BT_WAVE(16);
        else BT_WAVE(32);
#undef BT_WAVE
    } else {
        { const int e = bt_vattrs(c); if (e) return e; }
        const size_t lds = bt_getrf_wg_lds(nmax);
        if (top <= 64) {
            if (fused) bt_vgetrf_wg_kernel<true, 1><<<(unsigned)count, 256, lds, c->stream>>>(A, v, idx, ipiv, info);
            else bt_vgetrf_wg_kernel<false, 1><<<(unsigned)count, 256, lds, c->stream>>>(A, v, idx, ipiv, info);
        } else {
            if (fused) bt_vgetrf_wg_kernel<true, 2><<<(unsigned)count, 1024, lds, c->stream>>>(A, v, idx, ipiv, info);
            else bt_vgetrf_wg_kernel<false, 2><<<(unsigned)count, 1024, lds, c->stream>>>(A, v, idx, ipiv, info);
        }
    }
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

int launch_getrs_vbatched(mpf_ctx *c, const BtRagged &v, const int32_t *idx, int64_t count, int top, int nmax, int trans, const double *LU,
                          const int *ipiv, int nrhs, double *B, int64_t ldb) {
    if (count < 1 || nrhs < 1) return 0;
    if (!bt_vrange(c, "launch_getrs_vbatched", count, top, nmax)) return -1;
    { const int e = bt_vattrs(c); if (e) return e; }
    const size_t region = bt_getrs_lds(nmax);
#define BT_SOLVE(H_, TS_)                                                                                                                \
    do {                                                                                                                                 \
        const int per_wg = BT_T / TS_;                                                                                                   \
        const unsigned g = (unsigned)((count + per_wg - 1) / per_wg);                                                                    \
        bt_vgetrs_kernel<H_, TS_><<<g, BT_T, region * per_wg, c->stream>>>(trans, LU, v, idx, count, ipiv, nrhs, B, ldb, (unsigned)region); \
    } while (0)
    if (top <= 8) BT_SOLVE(1, 8);
    else if (top <= 16) BT_SOLVE(1, 16);
    else if (top <= 32) BT_SOLVE(1, 32);
    else if (top <= 64) BT_SOLVE(1, 256);
    else BT_SOLVE(2, 256);
#undef BT_SOLVE
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

int launch_getri_vbatched(mpf_ctx *c, const BtRagged &v, const int32_t *idx, int64_t count, int top, int nmax, const double *LU,
                          const int *ipiv, double *inv, int *info) {
    if (count < 1) return 0;
    if (!bt_vrange(c, "launch_getri_vbatched", count, top, nmax)) return -1;
    if (top <= 32) {
#define BT_INV(W_)                                                                                                                   \
        do {                                                                                                                         \
            const long long per = (BT_T / W_);                                                                                       \
            const unsigned g = (unsigned)((count + per - 1) / per);                                                                  \
            bt_vgetri_wave_kernel<W_><<<g, BT_T, 0, c->stream>>>(LU, v, idx, count, ipiv, inv, info);                                 \
        } while (0)
        if (top <= 8) BT_INV(8);
        else if (top <= 16) BT_INV(16);
        else BT_INV(32);
#undef BT_INV
    } else {
        { const int e = bt_vattrs(c); if (e) return e; }
        const size_t lds = bt_getri_wg_lds(nmax);
        if (top <= 64) bt_vgetri_wg_kernel<1><<<(unsigned)count, 256, lds, c->stream>>>(LU, v, idx, ipiv, inv, info);
        else bt_vgetri_wg_kernel<2><<<(unsigned)count, 1024, lds, c->stream>>>(LU, v, idx, ipiv, inv, info);
    }
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

int launch_getdet_vbatched(mpf_ctx *c, const BtRagged &v, const int32_t *idx, int64_t count, int top, const double *LU, const int *ipiv,
                           double *mant, int *expo) {
    if (count < 1) return 0;
    if (!bt_vrange(c, "launch_getdet_vbatched", count, top, 1)) return -1;
    if (top <= 32) {
        const unsigned g = (unsigned)((count + BT_T - 1) / BT_T);
        bt_vgetdet_kernel<1><<<g, BT_T, 0, c->stream>>>(LU, v, idx, count, ipiv, mant, expo);
    } else {
        const unsigned g = (unsigned)((count + BT_T / 64 - 1) / (BT_T / 64));
        bt_vgetdet_kernel<64><<<g, BT_T, 0, c->stream>>>(LU, v, idx, count, ipiv, mant, expo);
    }
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

int launch_vbatched_empty(mpf_ctx *c, const int32_t *idx, int64_t count, int *info, double *mant, int *expo) {
    if (count < 1 || (!info && !mant)) return 0;
    if (count > BT_MAX_LAUNCH) { c->err = "launch_vbatched_empty: size out of range"; return -1; }
    bt_vempty_kernel<<<(unsigned)((count + BT_T - 1) / BT_T), BT_T, 0, c->stream>>>(idx, count, info, mant, expo);
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}
