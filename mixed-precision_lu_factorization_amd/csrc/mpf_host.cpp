// C++ host side of libmpf_amd.so, the part every other host file stands on: the option table (the library's only reads of the
// environment), the context, the device report and the C entry points of the step operators (include/mpf_c.h).  The factor schedules:
// mpf_factor.cpp, factor_rm.cpp; the host-buffer path and MPF(): mpf_factor_host.cpp; the solves: mpf_solve.cpp and its neighbours.
#include "mpf_internal.h"
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>

std::string &noctx_error() { static thread_local std::string s; return s; }

// ---- per-context options ---------------------------------------------------------------------------------------------
// One table: option name (mpf_set_option / mpf_get_option), the environment variable that gives its DEFAULT when a context
// is created, and where it lives in the context.  Nothing else in the library reads the environment.
namespace {
struct OptDesc { const char *name, *env; size_t off; bool wide; long long lo, hi; };
#define OPT_I(field, env, lo, hi) {#field, env, offsetof(MpfTuning, field), false, lo, hi}
#define OPT_L(field, env, lo, hi) {#field, env, offsetof(MpfTuning, field), true, lo, hi}
const OptDesc kOpts[] = {
    OPT_I(safe_pivots, "MPF_SAFE_PIVOTS", 0, 1),
    OPT_I(pivot_fp64, "MPF_PIVOT_FP64", 0, 2),
    OPT_I(chain_pipeline, "MPF_CHAIN_PIPELINE", 0, 1),
    OPT_L(chain_pipeline_below, "MPF_CHAIN_PIPELINE_BELOW", 0, 1ll << 40),
    OPT_I(fp16_work32, "MPF_FP16_WORK32", 0, 1),
    OPT_I(superpanel_fp16, "MPF_SUPERPANEL", 0, 8),
    OPT_I(superpanel_fp64, "MPF_SUPERPANEL_FP64", 1, 8),
    OPT_I(no_lookahead, "MPF_NO_LOOKAHEAD", 0, 1),
    OPT_I(verbose, "MPF_VERBOSE", 0, 1),
    OPT_I(timeline, "MPF_TIMELINE", 0, 1),
    OPT_L(hp_spin_limit, "MPF_HP_SPIN_LIMIT", 1, 1ll << 31),
    OPT_L(hp_gate_ticks, "MPF_HP_GATE_TICKS", 0, 1ll << 40),
    OPT_I(hp_acq_fence, "MPF_HP_ACQ_FENCE", 0, 1),
    OPT_I(hp_window, "MPF_HP_WINDOW", -1, 1 << 30),
    OPT_I(hgemm_pad, "MPF_HGEMM_PAD", 0, 65536),
    OPT_I(hgemm_split_pad, "MPF_HGEMM_SPLIT_PAD", 0, 65536),
    OPT_I(hgemm_big, "MPF_HGEMM_BIG", 0, 1),
    OPT_I(hgemm_big_tile, "MPF_HGEMM_BIG_TILE", 0, 5),
    OPT_I(hgemm_mfma16, "MPF_HGEMM_MFMA16", 0, 1),
    OPT_I(dgemm_dma, "MPF_DGEMM_DMA", 0, 1),
    OPT_I(lazy_gather, "MPF_LAZY_GATHER", 0, 2),
    OPT_I(lazy_onepass_max_rows, "MPF_LAZY_ONEPASS_MAX_ROWS", 0, 32768),
    OPT_I(dpanel_fused_form, "MPF_DPANEL_FUSED", 0, 1),
    OPT_I(dist_instalments, "MPF_DIST_INSTALMENTS", 0, 1),
    OPT_L(dist_instalment_min_bytes, "MPF_DIST_INSTALMENT_MIN_BYTES", 0, 1ll << 40),
    OPT_I(generic_fused, "MPF_GENERIC_FUSED", 0, 1),
    OPT_I(fp16_fused, "MPF_FP16_FUSED", 0, 1),
    OPT_I(fp64_rowmajor, "MPF_FP64_ROWMAJOR", 0, 1),
    OPT_L(fp64_rowmajor_min_n, "MPF_FP64_ROWMAJOR_MIN_N", 0, 1ll << 40),
    OPT_I(trsm_laswp_fused, "MPF_TRSM_LASWP_FUSED", 0, 1),
    OPT_I(fp64_two_lanes, "MPF_FP64_TWO_LANES", 0, 1 << 30),
    OPT_I(fp64_lane_a_pct, "MPF_FP64_LANE_A_PCT", 20, 90),
    OPT_I(fp64_pair, "MPF_FP64_PAIR", 0, 1),
    OPT_L(fp64_pair_min_n, "MPF_FP64_PAIR_MIN_N", 0, 1ll << 40),
    OPT_I(event_timers, "MPF_EVENT_TIMERS", 0, 2),
    OPT_I(dist_world1_loop, "MPF_DIST_WORLD1_LOOP", 0, 1),
    OPT_I(gesv_fp64_tflops, "MPF_GESV_FP64_TFLOPS", 0, 1000),
    OPT_I(gate_wait_value, "MPF_GATE_WAIT_VALUE", 0, 1),
    OPT_I(host_sink, "MPF_HOST_SINK", 0, 1),
    OPT_I(sink_trace, "MPF_SINK_TRACE", 0, 1),
    OPT_I(hp_half_slabs, "MPF_HP_HALF_SLABS", 0, 1),
    OPT_I(hp_half_slabs_rows, "MPF_HP_HALF_SLABS_ROWS", 256, 32768),
    OPT_I(hp_local_xcd, "MPF_HP_LOCAL_XCD", 0, 2),
    OPT_I(host_late_parts, "MPF_HOST_LATE_PARTS", 0, 4),
    OPT_L(host_late_min_n, "MPF_HOST_LATE_MIN_N", 0, 1ll << 40),
    OPT_I(host_first_pct, "MPF_HOST_FIRST_PCT", 5, 100),
    OPT_I(host_late_q_pct, "MPF_HOST_LATE_Q_PCT", 1, 1000),
    OPT_L(host_sink_min_n, "MPF_HOST_SINK_MIN_N", 0, 1ll << 40),
    OPT_I(dist_solve_p2p, "MPF_DIST_SOLVE_P2P", 0, 1),
    OPT_I(gmres_group_tiles, "MPF_GMRES_GROUP_TILES", 0, 16),
    OPT_I(batched_blocked_min_n, "MPF_BATCHED_BLOCKED_MIN_N", 0, 1025),
    OPT_I(batched_blocked_nb, "MPF_BATCHED_BLOCKED_NB", 0, 32),
    OPT_I(batched_blocked_inv_ct, "MPF_BATCHED_BLOCKED_INV_CT", 0, 16),
#ifdef MPF_PROBE
    OPT_I(batched_blocked_valu, "MPF_BATCHED_BLOCKED_VALU", 0, 1),
    OPT_I(batched_blocked_stages, "MPF_BATCHED_BLOCKED_STAGES", 0, 7),
    OPT_I(hp_stamp, "MPF_HP_STAMP", 0, 1),
    OPT_I(hp_r256_upto, "MPF_HP_R256_UPTO", 0, 1 << 30),
    OPT_I(dgemm_w8, "MPF_DGEMM_W8", 0, 1),
    OPT_I(gemm_lds_pad, "MPF_GEMM_LDS_PAD", 0, 65536),
    OPT_I(hgemm_big_reg, "MPF_HGEMM_BIG_REG", 0, 1),
    OPT_I(hgemm_dbg, "MPF_HGEMM_DBG", 0, 8191),
#endif
};
#undef OPT_I
#undef OPT_L
void opt_store(MpfTuning &t, const OptDesc &d, long long v) {
    if (v < d.lo) v = d.lo;
    if (v > d.hi) v = d.hi;
    char *p = (char *)&t + d.off;
    if (d.wide) *(long long *)p = v; else *(int *)p = (int)v;
}
long long opt_load(const MpfTuning &t, const OptDesc &d) {
    const char *p = (const char *)&t + d.off;
    return d.wide ? *(const long long *)p : (long long)*(const int *)p;
}
void tuning_from_env(MpfTuning &t) {   // called by mpf_create only
    for (const OptDesc &d : kOpts)
        if (const char *e = getenv(d.env)) if (*e) opt_store(t, d, atoll(e));
}
} // namespace

extern "C" {

int mpf_create(mpf_ctx **out, int device) {
    if (!out) return -1;
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) return fail(nullptr, -3, "No HIP devices available.");
    if (device < 0 || device >= ndev) return fail(nullptr, -1, "mpf_create: bad device index");
    mpf_ctx *c = new mpf_ctx();
    tuning_from_env(c->tune);
    c->device = device;
    if (hipSetDevice(device) != hipSuccess) { delete c; return fail(nullptr, -2, "hipSetDevice failed"); }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->num_cus = prop.multiProcessorCount;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return fail(nullptr, -2, "hipStreamCreate failed"); }
    c->own_stream = true;
    {
        int lo = 0, hi = 0;
        hipDeviceGetStreamPriorityRange(&lo, &hi); // hi = numerically lowest = highest priority
        if (hipStreamCreateWithPriority(&c->pstream, hipStreamNonBlocking, hi) != hipSuccess) c->pstream = nullptr;
        if (hipStreamCreateWithPriority(&c->tstream, hipStreamNonBlocking, hi) != hipSuccess) c->tstream = nullptr;
    }
    if (hipMalloc((void **)&c->ws, sizeof(MpfWorkspace)) != hipSuccess) { hipStreamDestroy(c->stream); delete c; return fail(nullptr, -2, "hipMalloc(workspace) failed"); }
    hipMemset(c->ws, 0, sizeof(MpfWorkspace));
    // 8 bytes of signal memory for option gate_wait_value (a stream waits on the pivot kernel's progress word); optional
    if (hipExtMallocWithFlags((void **)&c->hp_signal, 8, hipMallocSignalMemory) != hipSuccess) { c->hp_signal = nullptr; (void)hipGetLastError(); }
    else hipMemset(c->hp_signal, 0, 8);
    hipEventCreate(&c->ev0);
    hipEventCreate(&c->ev1);
    *out = c;
    return 0;
}

int mpf_destroy(mpf_ctx *c) {
    if (!c) return 0;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    if (c->ws) hipFree(c->ws);
    if (c->hp_signal) hipFree(c->hp_signal);
    mpf_rccl_destroy(c);
    sink_destroy(c);
    feed_destroy(c);
    if (c->ev0) hipEventDestroy(c->ev0);
    if (c->ev1) hipEventDestroy(c->ev1);
    if (c->pstream) { hipStreamSynchronize(c->pstream); hipStreamDestroy(c->pstream); }
    if (c->tstream) { hipStreamSynchronize(c->tstream); hipStreamDestroy(c->tstream); }
    if (c->xstream) { hipStreamSynchronize(c->xstream); hipStreamDestroy(c->xstream); }
    for (hipEvent_t e : c->ev_pool) hipEventDestroy(e);
    if (c->own_stream && c->stream) hipStreamDestroy(c->stream);
    delete c;   // (the scratch buffers go with it, every stream synchronised)
    return 0;
}

int mpf_set_stream(mpf_ctx *c, void *hip_stream) {
    if (!c) return -1;
    if (c->own_stream && c->stream) { hipStreamSynchronize(c->stream); hipStreamDestroy(c->stream); }
    c->stream = (hipStream_t)hip_stream;
    c->own_stream = false;
    return 0;
}

int mpf_synchronize(mpf_ctx *c) {
    if (!c) return -1;
    MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return 0;
}

const char *mpf_last_error(mpf_ctx *c) { return c ? c->err.c_str() : noctx_error().c_str(); }

int mpf_get_stats(mpf_ctx *c, mpf_stats *out) {
    if (!c || !out) return -1;
    *out = c->stats;
    return 0;
}

int mpf_set_option(mpf_ctx *c, const char *name, int64_t value) {
    if (!c || !name) return -1;
    for (const OptDesc &d : kOpts)
        if (!strcmp(d.name, name)) {
            opt_store(c->tune, d, (long long)value);
            // kernel attributes (dynamic-LDS sizes, occupancy answers) depend on options: every family sets its own again
            c->attr_done = 0; c->attr_big = 0;
            return 0;
        }
    return fail(c, -1, std::string("mpf_set_option: unknown option '") + name + "'");
}
int mpf_get_option(mpf_ctx *c, const char *name, int64_t *value) {
    if (!c || !name || !value) return -1;
    for (const OptDesc &d : kOpts)
        if (!strcmp(d.name, name)) { *value = (int64_t)opt_load(c->tune, d); return 0; }
    return fail(c, -1, std::string("mpf_get_option: unknown option '") + name + "'");
}
int mpf_option_name(int32_t index, char *buf, int64_t buflen) { // enumerate: returns the number of options
    const int n = (int)(sizeof kOpts / sizeof kOpts[0]);
    if (index >= 0 && index < n && buf && buflen > 0) { strncpy(buf, kOpts[index].name, (size_t)buflen - 1); buf[buflen - 1] = 0; }
    return n;
}

int mpf_device_report(char *buf, int64_t buflen) {
    // HIP analogue of reference check_cooperative_groups.cu:4-48 (device properties + cooperative-launch support), plus what
    // this library's design depends on: LDS per CU (the pivot kernel's slab), CU count (its residency bound), L2 / Infinity
    // Cache, the RCCL version and the xGMI link matrix of the node
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) ndev = 0;
    std::string s = "HIP devices: " + std::to_string(ndev) + "\n";
    int rt = 0, drv = 0;
    if (ndev > 0 && hipRuntimeGetVersion(&rt) == hipSuccess && hipDriverGetVersion(&drv) == hipSuccess)
        s += "HIP runtime " + std::to_string(rt) + " driver " + std::to_string(drv) + "\n";
    const int rv = ndev > 0 ? mpf_rccl_version() : -1;
    s += rv > 0 ? "RCCL version " + std::to_string(rv / 10000) + "." + std::to_string(rv / 100 % 100) + "." + std::to_string(rv % 100) + " (NCCL API, dlopen)\n"
                : std::string("RCCL: not loaded\n");
    for (int d = 0; d < ndev; ++d) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, d) != hipSuccess) continue;
        int coop = 0, lds_cu = 0, l2 = 0, clk = 0, memclk = 0, buswidth = 0;
        hipDeviceGetAttribute(&coop, hipDeviceAttributeCooperativeLaunch, d);
        hipDeviceGetAttribute(&lds_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, d);
        hipDeviceGetAttribute(&l2, hipDeviceAttributeL2CacheSize, d);
        hipDeviceGetAttribute(&clk, hipDeviceAttributeClockRate, d);
        hipDeviceGetAttribute(&memclk, hipDeviceAttributeMemoryClockRate, d);
        hipDeviceGetAttribute(&buswidth, hipDeviceAttributeMemoryBusWidth, d);
        char line[768];
        snprintf(line, sizeof line,
                 "device %d: %s arch %s CUs %d maxThreadsPerBlock %d LDS/block %zu B LDS/CU %d B warpSize %d regs/block %d "
                 "L2 %d KiB clock %d MHz memclock %d MHz bus %d bit HBM %.1f GiB cooperativeLaunch %d pivot-kernel rows/launch %d\n",
                 d, p.name, p.gcnArchName, p.multiProcessorCount, p.maxThreadsPerBlock, p.sharedMemPerBlock, lds_cu, p.warpSize,
                 p.regsPerBlock, l2 / 1024, clk / 1000, memclk / 1000, buswidth, (double)p.totalGlobalMem / (1024.0 * 1024.0 * 1024.0), coop,
                 HP_R * (p.multiProcessorCount < HP_MAXG ? p.multiProcessorCount : HP_MAXG));
        s += line;
    }
    if (ndev > 1) { // xGMI topology: link type and hop count of every device pair, peer access
        s += "link matrix (type:hops, type 4 = xGMI; P = peer access):\n";
        for (int a = 0; a < ndev; ++a) {
            std::string row = "  dev " + std::to_string(a) + ":";
            for (int b = 0; b < ndev; ++b) {
                if (a == b) { row += "   -  "; continue; }
                uint32_t lt = 0, hops = 0;
                int peer = 0;
                hipDeviceCanAccessPeer(&peer, a, b);
                if (hipExtGetLinkTypeAndHopCount(a, b, &lt, &hops) != hipSuccess) { lt = 0; hops = 0; }
                char cell[32];
                snprintf(cell, sizeof cell, " %u:%u%s", lt, hops, peer ? "P" : " ");
                row += cell;
            }
            s += row + "\n";
        }
    }
    if (buf && buflen > 0) { strncpy(buf, s.c_str(), (size_t)buflen - 1); buf[buflen - 1] = 0; }
    return ndev;
}

// ---- step operators ----------------------------------------------------------------------------
int mpf_double_to_fp16(mpf_ctx *c, const double *d_in, uint16_t *d_out, int64_t n) {
    if (!c) return -1;
    return launch_double_to_fp16(c, d_in, d_out, n);
}
int mpf_hdiv(mpf_ctx *c, const uint16_t *a, const uint16_t *b, uint16_t *q, int64_t n) {
    if (!c) return -1;
    return launch_hdiv(c, a, b, q, n);
}
int mpf_hgetf2_pivots(mpf_ctx *c, const double *d_A, int64_t lda, int32_t rows, int32_t cols, int32_t ipiv_offset,
                      int32_t *d_ipiv, uint16_t *d_panel16_out) {
    if (!c || !d_A || !d_ipiv) return -1;
    if (lda < rows) return fail(c, -1, "hgetf2_pivots: lda < rows");
    if (cols > 65535) return fail(c, -1, "hgetf2_pivots: panel width > 65535");
    if (!safe_pivots(c) && hgetf2_lds_eligible(c, rows, cols))
        return launch_hgetf2(c, d_A, lda, nullptr, 0, rows, cols, ipiv_offset, d_ipiv, d_panel16_out, rows, nullptr);
    return launch_hgetf2_generic(c, d_A, lda, nullptr, 0, rows, cols, ipiv_offset, d_ipiv, d_panel16_out, rows);
}
int mpf_hgetf2(mpf_ctx *c, uint16_t *d_panel16, int64_t ld, int32_t rows, int32_t cols, int32_t *d_ipiv_panel) {
    if (!c || !d_panel16 || !d_ipiv_panel) return -1;
    if (ld < rows) return fail(c, -1, "hgetf2: ld < rows");
    if (!safe_pivots(c) && hgetf2_lds_eligible(c, rows, cols))
        return launch_hgetf2(c, nullptr, 0, d_panel16, ld, rows, cols, 0, d_ipiv_panel, nullptr, 0, nullptr);
    return launch_hgetf2_generic(c, nullptr, 0, d_panel16, ld, rows, cols, 0, d_ipiv_panel, nullptr, 0);
}
int mpf_laswp(mpf_ctx *c, double *d_A, int64_t lda, int64_t ncols, int32_t k, int32_t cols, const int32_t *d_ipiv) {
    if (!c || !d_A || !d_ipiv) return -1;
    if (cols > HP_MAXCOLS) return launch_laswp_seq(c, d_A, lda, ncols, k, cols, d_ipiv, lda); // any number of swaps, MPF.cu:42-59 as it stands
    return launch_laswp(c, d_A, lda, ncols, k, cols, d_ipiv);
}
int mpf_dgetf2_npv(mpf_ctx *c, double *d_P, int64_t ld, int32_t rows, int32_t cols, int32_t fused) {
    if (!c || !d_P) return -1;
    if (ld < rows) return fail(c, -1, "dgetf2_npv: ld < rows");
    return launch_dgetf2_npv(c, d_P, ld, rows, cols, fused, 0);
}
int mpf_dgetf2_piv(mpf_ctx *c, double *d_P, int64_t ld, int32_t rows, int32_t cols, int32_t fused, int32_t ipiv_offset,
                   int32_t *d_ipiv, int32_t *info) {
    if (!c || !d_P || !d_ipiv) return -1;
    if (rows < 1 || cols < 1 || cols > 65535) return fail(c, -1, "dgetf2_piv: need rows >= 1 and 1 <= cols <= 65535");
    if (ld < rows) return fail(c, -1, "dgetf2_piv: ld < rows");
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    const int imax = INT_MAX;
    MPF_HIP_TRY(c, hipMemcpyAsync(&c->ws->info, &imax, sizeof(int), hipMemcpyHostToDevice, c->stream));
    const int rc = launch_dgetf2_piv(c, d_P, ld, rows, cols, fused, 0, ipiv_offset, d_ipiv);
    if (rc || !info) return rc;
    int v = 0;
    MPF_HIP_TRY(c, hipMemcpyAsync(&v, &c->ws->info, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));
    *info = v == INT_MAX ? 0 : v;
    return 0;
}
int mpf_dgetf2_tp(mpf_ctx *c, double *d_P, int64_t ld, int32_t rows, int32_t cols, int32_t fused, int32_t ipiv_offset,
                  int32_t *d_ipiv, int32_t *info) {
    if (!c || !d_P || !d_ipiv) return -1;
    if (rows < 1 || cols < 1 || cols > 65535) return fail(c, -1, "dgetf2_tp: need rows >= 1 and 1 <= cols <= 65535");
    if (ld < rows) return fail(c, -1, "dgetf2_tp: ld < rows");
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    const int imax = INT_MAX;
    MPF_HIP_TRY(c, hipMemcpyAsync(&c->ws->info, &imax, sizeof(int), hipMemcpyHostToDevice, c->stream));
    const int rc = launch_dgetf2_tp(c, d_P, ld, rows, cols, fused, 0, ipiv_offset, d_ipiv);
    if (rc || !info) return rc;
    int v = 0;
    MPF_HIP_TRY(c, hipMemcpyAsync(&v, &c->ws->info, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));
    *info = v == INT_MAX ? 0 : v;
    return 0;
}
int mpf_dtrsm_llnu(mpf_ctx *c, int32_t m, int64_t n, const double *d_L, int64_t ldl, double *d_B, int64_t ldb) {
    if (!c) return -1;
    if (m > 0 && n > 0 && (ldl < m || ldb < m)) return fail(c, -1, "dtrsm: leading dimension < m");
    return launch_dtrsm_llnu(c, m, n, d_L, ldl, d_B, ldb);
}
int mpf_dgemm_minus(mpf_ctx *c, int64_t m, int64_t n, int32_t k, const double *d_A, int64_t lda, const double *d_B,
                    int64_t ldb, double *d_C, int64_t ldc) {
    if (!c) return -1;
    if (m > 0 && n > 0 && k > 0 && (lda < m || ldb < k || ldc < m)) return fail(c, -1, "dgemm: bad leading dimension");
    return launch_dgemm_minus(c, m, n, k, d_A, lda, d_B, ldb, d_C, ldc);
}

int mpf_ensure_h_images(mpf_ctx *c, int64_t rows, int kmax, bool big) {
    kmax = (kmax + 63) & ~63;
    if (c->h_L && c->h_rows >= rows && c->h_kmax >= kmax && (!big || c->h_Lb[0])) return 0;
    if (rows < c->h_rows) rows = c->h_rows;
    if (kmax < c->h_kmax) kmax = c->h_kmax;
    big = big || c->h_Lb[0];
    c->h_L.release(); c->h_U.release();
    for (auto &b : c->h_Lb) b.release();
    c->h_rows = 0; c->h_kmax = 0;
    const int64_t elems = 2 * rows * kmax; // hi image, then lo image (split mode)
    MPF_HIP_TRY(c, c->h_L.grow(elems));
    MPF_HIP_TRY(c, c->h_U.grow(elems));
    if (big) for (auto &b : c->h_Lb) MPF_HIP_TRY(c, b.grow(elems));
    c->h_rows = rows; c->h_kmax = kmax;
    return 0;
}

int mpf_hgemm_minus(mpf_ctx *c, int64_t m, int64_t n, int32_t k, const double *d_A, int64_t lda, const double *d_B,
                    int64_t ldb, double *d_C, int64_t ldc, int32_t split) {
    if (!c) return -1;
    if (m <= 0 || n <= 0 || k <= 0) return 0;
    if (k > 8 * HP_MAXCOLS) return fail(c, -1, "hgemm: k > 2048");
    if (lda < m || ldb < k || ldc < m) return fail(c, -1, "hgemm: bad leading dimension");
    int rc = mpf_ensure_h_images(c, m > n ? m : n, k, false);
    if (!rc) rc = launch_cvt_l21(c, d_A, lda, m, k, split);
    if (!rc) rc = launch_hgemm_minus(c, m, n, k, d_B, ldb, d_C, ldc, split);
    return rc;
}

int mpf_hgemm_minus_f32(mpf_ctx *c, int64_t m, int64_t n, int32_t k, const double *d_A, int64_t lda, const double *d_B,
                        int64_t ldb, float *d_C, int64_t ldc, int32_t split) {
    if (!c || !d_A || !d_B || !d_C) return -1;
    if (m <= 0 || n <= 0 || k <= 0) return 0;
    if (k > 8 * HP_MAXCOLS) return fail(c, -1, "hgemm: k > 2048");
    if (lda < m || ldb < k || ldc < m) return fail(c, -1, "hgemm: bad leading dimension");
    int rc = mpf_ensure_h_images(c, m > n ? m : n, k, false);
    if (!rc) rc = launch_cvt_l21(c, d_A, lda, m, k, split);
    c->hgemm_standalone = true;   // (a call of its own: nothing of a panel chain waits for CUs beside it -- see launch_hgemm_ptrs)
    if (!rc) rc = launch_hgemm_minus_w32(c, m, n, k, d_B, ldb, d_C, ldc, split);
    c->hgemm_standalone = false;
    return rc;
}

int mpf_w32_from_f64(mpf_ctx *c, const double *d_A, int64_t lda, float *d_W, int64_t ldw, int64_t rows, int64_t cols) {
    if (!c || !d_A || !d_W) return -1;
    if (lda < rows || ldw < cols) return fail(c, -1, "w32_from_f64: bad leading dimension");
    return launch_cvt_f64_f32(c, d_A, lda, d_W, ldw, rows, cols);
}
int mpf_w32_to_f64(mpf_ctx *c, const float *d_W, int64_t ldw, double *d_A, int64_t lda, int64_t rows, int64_t cols) {
    if (!c || !d_A || !d_W) return -1;
    if (lda < rows || ldw < cols) return fail(c, -1, "w32_to_f64: bad leading dimension");
    return launch_cvt_f32_f64(c, d_W, ldw, d_A, lda, rows, cols);
}
int mpf_w32_laswp(mpf_ctx *c, float *d_W, int64_t ldw, int64_t ncols, int32_t k, int32_t cols, const int32_t *d_ipiv) {
    if (!c || !d_W || !d_ipiv) return -1;
    if (cols < 1 || cols > HP_MAXCOLS) return fail(c, -1, "w32_laswp: 1 <= cols <= 256");
    if (ldw < ncols) return fail(c, -1, "w32_laswp: ldw < ncols");
    const int64_t need = (int64_t)LASWP_MAXMOVED * ncols / 2 + 1;    // doubles: 2 * HP_MAXCOLS moved rows x ncols floats
    if (need > c->perm_tmp.cap()) {
        MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));
        MPF_HIP_TRY(c, c->perm_tmp.grow(need));
    }
    int rc = launch_laswp_plan(c, d_ipiv, k, cols, &c->ws->list0);
    if (!rc) rc = launch_laswp_from_list_f32(c, d_W, ldw, ncols, &c->ws->list0);
    return rc;
}

// rows of the tallest panel the LDS pivot kernel takes (in either form) beside `waiters` workgroups that wait for it (0: alone);
// waiters < 0: beside the pipelined chain's gated interchange kernel on a panel of -waiters columns
int64_t mpf_hgetf2_capacity_rows(mpf_ctx *c, int32_t waiters, int32_t form) {
    if (!c || form < 0 || form > 2) return -1;
    if (hipSetDevice(c->device) != hipSuccess) return -2;
    return (int64_t)hgetf2_capacity_rows(c, waiters < 0 ? laswp_gated_grid(-waiters) : waiters, form);
}

} // extern "C"
