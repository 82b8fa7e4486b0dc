// The host-buffer path: mpf_factor_host (upload with its late-segment plan, mpf_factor_dev, block rows home through the row sink),
// mpf_trim, and the drop-in C++ symbol MPF() (include/MPF.h) on a context of its own.
#include "solve_common.h"
#include "../../include/MPF.h"
#include <cstring>
#include <iostream>
#include <mutex>

// Device copies of the host entry point's buffers live in the context and only ever grow (round 4): the reference allocates and
// frees them inside every MPF() call (MPF.cu:80-94,250-255), which at N = 32768 cost 275 ms of a 1037-ms call here;
// benchmark.cpp:181-266 calls MPF() once per matrix of a file.  mpf_trim() gives the memory back.
static int ensure_host_copies(mpf_ctx *c, int64_t N) {
    MPF_HIP_TRY(c, c->host_A.grow(N * N));   // 64-bit: the reference overflows int here (MPF.cu:81)
    MPF_HIP_TRY(c, c->host_P.grow(N));
    return 0;
}

int mpf_trim(mpf_ctx *c) {
    if (!c) return -1;
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->host_A.release(); c->host_P.release(); c->host_A0.release();
    sink_trim(c);
    feed_trim(c);
    c->r64.release(); c->rm_tmp.release(); c->rm_lt.release(); c->rm_pair.release();
    c->w32.release();
    return 0;
}

int mpf_factor_host(mpf_ctx *c, double *A_host, int64_t N, int32_t nb, int32_t *ipiv_host, const mpf_opts *opts) {
    if (!c || !A_host || !ipiv_host) return -1;
    if (N <= 0 || nb <= 0) return fail(c, -1, "mpf_factor: N and panel width must be positive");
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    { const int e = ensure_host_copies(c, N); if (e) return e; }
    double *dA = c->host_A;
    int32_t *dP = c->host_P;
    const size_t bytes = (size_t)N * (size_t)N * sizeof(double), pbytes = (size_t)N * sizeof(int32_t);
    // Block rows leave while the factorization runs (rowsink.hip) when the schedule is one that reports them -- the look-ahead
    // schedules of the fp64 mode, which is what MPF() runs.  The caller's buffer is then partly results before the call knows that it
    // succeeded, so the matrix as uploaded is kept on the device (a device-to-device copy, ~4 ms at N = 32768) for the one failure
    // the call recovers from by itself: a pivot kernel whose workgroups were not all resident (-4) -> once more on the generic path.
    const bool want_sink = c->tune.host_sink && N >= c->tune.host_sink_min_n && c->pstream != nullptr && !(opts && (opts->sync_timing || opts->no_lookahead)) &&
                           !(opts && opts->trailing != MPF_TRAIL_FP64) && !(opts && opts->pivot_path == 1) &&
                           !(opts && opts->pivot_search != 0) && !c->tune.pivot_fp64;   // (the generic schedule reports no block rows)
    bool armed = false;
    if (want_sink) {
        if (c->host_A0.grow((int64_t)((bytes + pbytes + sizeof(double) - 1) / sizeof(double))) != hipSuccess)   // A, then P
            (void)hipGetLastError();   // (no room for the snapshot: the plain way)
        if (c->host_A0) {
            const int e = sink_attach(c, A_host, N, nb);
            if (e < 0) return e;
            armed = e == 0;
        }
    }
    // The way up (round 5): only the first part of the matrix goes up before the factorization starts; the rest follows in column
    // segments while the first panels are factored on what is there (LatePlan, factor_lookahead_rm; rowsink.hip for the transport).
    // Planned only where that schedule is the one that will run (fp64 mode, N >= fp64_rowmajor_min_n, panels the LDS pivot kernel takes).
    LatePlan plan;
    const int64_t npan = (N + nb - 1) / nb;
    int parts = c->tune.host_late_parts;
    if (!want_sink || !c->tune.fp64_rowmajor || N < c->tune.fp64_rowmajor_min_n || N < c->tune.host_late_min_n || npan < 32 || c->tune.no_lookahead || safe_pivots(c) ||
        !hgetf2_lds_eligible(c, (int)N, (int)nb) || c->tune.superpanel_fp64 > 1 || (opts && opts->superpanel > 1)) parts = 0;
    if (parts > 0 && !c->late_flags) {
        if (c->late_flags.grow(16) != hipSuccess) { (void)hipGetLastError(); parts = 0; }
        else memset(c->late_flags, 0, 16 * sizeof(unsigned));
    }
    if (parts > 0 && mpf_ensure_rowmajor_copy(c, N, N, nb) != 0) parts = 0;
    if (parts > 0) {
        // first part: host_first_pct of the columns; the late segments share the rest equally; when a segment is due is decided below,
        // once the first part's upload has been timed
        const int64_t first = ((N * c->tune.host_first_pct / 100 + nb - 1) / nb) * nb;
        plan.nseg = parts;
        for (int i = 0; i < parts; ++i) {
            int64_t c0 = first + ((N - first) * i / parts / nb) * nb;
            if (c0 < 4 * (int64_t)nb) c0 = 4 * (int64_t)nb;
            plan.c0[i] = c0;
            plan.q[i] = 1;
            if (i && plan.c0[i] <= plan.c0[i - 1]) { plan.nseg = 0; break; }
        }
        if (plan.nseg && plan.c0[0] >= N) plan.nseg = 0;
        plan.flags = c->late_flags;
        plan.seq = ++c->late_seq;
        plan.snapshot = armed ? c->host_A0 : nullptr;
    }
    const int64_t up_cols = plan.nseg ? plan.c0[0] : N;
    const size_t up_bytes = (size_t)up_cols * (size_t)N * sizeof(double);
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    hipMemsetAsync(&c->ws->flags[1], 0, sizeof(int), c->stream);
    hipEventRecord(e0, c->stream);
    const auto t_up0 = std::chrono::steady_clock::now();
    hipMemcpyAsync(dA, A_host, up_bytes, hipMemcpyHostToDevice, c->stream);   // (from pageable memory: returns when the copy is done)
    const double up_ms = ms_since(t_up0);
    hipMemcpyAsync(dP, ipiv_host, pbytes, hipMemcpyHostToDevice, c->stream);
    hipEventRecord(e1, c->stream);
    if (plan.nseg) {
        // When is a segment due?  As soon as it is there -- earlier, the main stream waits for the link; later, more panels are replayed on
        // it one by one with their small launches in the open.  Arrival: the link's rate as just measured on the first part (the late
        // segments go through host threads and pinned buffers: not faster than that, 45 GB/s assumed at most).  The device's progress: the
        // updates' flops on the columns that are there at 58 TFLOP/s, a panel never faster than its pivot chain (2.4 us per column);
        // host_late_q_pct scales the estimate (100 = as computed; the default leans late: waiting costs more than replaying).
        double gbps = up_ms > 0 ? (double)up_bytes / up_ms / 1e6 : 45.0;
        if (gbps > 45.0) gbps = 45.0;
        if (gbps < 5.0) gbps = 5.0;
        const double fl_per_ms = 58e9, chain_ms = nb * 2.4e-3;
        double t = 0, arrive = 0;
        int64_t k = 0, ce = plan.c0[0];
        for (int i = 0; i < plan.nseg; ++i) {
            const int64_t hi = i + 1 < plan.nseg ? plan.c0[i + 1] : N, w = hi - plan.c0[i];
            arrive += (double)w * N * 8 / gbps / 1e6 * (c->tune.host_late_q_pct / 100.0);
            while (t < arrive && (k / nb + 3) * (int64_t)nb <= ce) {   // panel k on the columns [.., ce)
                const double rows = (double)(N - k - nb), cols = (double)(ce - k - nb);
                const double upd = 2.0 * rows * cols * nb / fl_per_ms;
                t += upd > chain_ms ? upd : chain_ms;
                k += nb;
            }
            plan.q[i] = (int)(k / nb) > 0 ? (int)(k / nb) : 1;
            for (int64_t kj = 0; kj < k; kj += nb) t += 2.0 * (double)(N - kj - nb) * (double)w * nb / fl_per_ms;   // the replay
            if (t < arrive) t = arrive;
            ce = hi;
        }
        if (c->tune.sink_trace) {
            fprintf(stderr, "late plan: first part %lld columns up in %.1f ms (%.1f GB/s)", (long long)plan.c0[0], up_ms, up_ms > 0 ? (double)up_bytes / up_ms / 1e6 : 0.0);
            for (int i = 0; i < plan.nseg; ++i) fprintf(stderr, "; segment from column %lld due at panel %d", (long long)plan.c0[i], plan.q[i]);
            fprintf(stderr, "\n");
        }
    }
    if (armed) {
        hipMemcpyAsync(c->host_A0, dA, up_bytes, hipMemcpyDeviceToDevice, c->stream);
        hipMemcpyAsync((char *)c->host_A0.get() + bytes, dP, pbytes, hipMemcpyDeviceToDevice, c->stream);
    }
    if (plan.nseg) {
        const int e = feed_start(c, A_host, dA, N, &plan);
        if (e) {   // (no upload threads to be had: the rest of the matrix goes up here and now, as without a plan)
            hipMemcpyAsync(dA + up_cols * N, A_host + up_cols * N, bytes - up_bytes, hipMemcpyHostToDevice, c->stream);
            if (armed) hipMemcpyAsync(c->host_A0 + up_cols * N, dA + up_cols * N, bytes - up_bytes, hipMemcpyDeviceToDevice, c->stream);
            plan.nseg = 0;
        } else c->late = &plan;
    }
    int rc = mpf_factor_dev(c, dA, N, N, nb, dP, opts);
    c->late = nullptr;
    {   // the upload thread has long finished when the factorization has; a plan the schedule did not take was waited for inside mpf_factor_dev
        const int e = feed_finish(c);
        if (e && rc >= 0) rc = e;
        int gave = 0;
        if (plan.nseg && hipMemcpy(&gave, &c->ws->flags[1], sizeof(int), hipMemcpyDeviceToHost) == hipSuccess && gave && rc >= 0)
            rc = fail(c, -2, "mpf_factor_host: the factorization gave up waiting for a late column segment");
        if (armed && plan.nseg)      // segments the schedule did not reach (it failed before): their snapshot is taken now, from the untouched columns
            for (int i = 0; i < plan.nseg; ++i)
                if (!plan.snapped[i]) {
                    const int64_t lo = plan.c0[i], hi = i + 1 < plan.nseg ? plan.c0[i + 1] : N;
                    hipMemcpyAsync(c->host_A0 + lo * N, dA + lo * N, (size_t)(hi - lo) * N * sizeof(double), hipMemcpyDeviceToDevice, c->stream);
                }
    }
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    const double ms_h2d = ms;
    const auto t_done = std::chrono::steady_clock::now();
    int sent = 0;
    const int npanels = (int)((N + nb - 1) / nb);
    int sk = armed ? sink_finish(c, &sent) : 1;   // 0: a schedule took the sink (sent block rows are in A_host), 1: nobody did, < 0: HIP error
    if (sk < 0) rc = sk;
    if (rc == -4 && sk == 0 && sent > 0) {
        // (the reference has no such failure mode: MPF.cu:126-140 is a cooperative launch)
        const std::string why = c->err;
        std::cerr << "mpf_factor_host: " << why << " -- " << sent << " block rows had left already; repeating on the generic pivot path from the uploaded matrix" << std::endl;
        hipMemcpyAsync(dA, c->host_A0, bytes, hipMemcpyDeviceToDevice, c->stream);
        hipMemcpyAsync(dP, (char *)c->host_A0.get() + bytes, pbytes, hipMemcpyDeviceToDevice, c->stream);
        mpf_opts o2{};
        if (opts) o2 = *opts;
        o2.pivot_path = 1;
        rc = mpf_factor_dev(c, dA, N, N, nb, dP, &o2);
        if (rc == -4) c->err = why;
        sent = 0;
        sk = 1;        // (this factorization did not go through the sink: its matrix goes home in one piece)
    }
    c->stats.ms_h2d = ms_h2d;
    c->stats.host_late_segments = (rc >= 0 && plan.taken) ? plan.nseg : 0;
    if (rc >= 0) {
        hipError_t se = hipSuccess;
        if (sk == 0 && sent == npanels) {   // every block row is home
            hipMemcpyAsync(ipiv_host, dP, pbytes, hipMemcpyDeviceToHost, c->stream);
            se = hipStreamSynchronize(c->stream);
            c->stats.host_rows_streamed = npanels;
        } else {
            // (a schedule that gave its rows to the sink has skipped its deferred left-hand interchanges: if the sink stopped early without
            //  an error of the factorization -- it cannot, short of a HIP error, but the matrix must never go home half-permuted -- they are due now)
            if (sk == 0 && sent < npanels) (void)launch_lazy_left_swaps(c, dA, N, N, nb, npanels, c->lists);
            hipMemcpyAsync(A_host, dA, bytes, hipMemcpyDeviceToHost, c->stream);
            hipMemcpyAsync(ipiv_host, dP, pbytes, hipMemcpyDeviceToHost, c->stream);
            se = hipStreamSynchronize(c->stream);
        }
        // what the call still spent on the way home after the factorization's last kernel (wall clock)
        c->stats.ms_d2h = ms_since(t_done);
        if (se != hipSuccess) rc = fail(c, -2, std::string("D2H failed: ") + hipGetErrorString(se));
    }
    hipEventDestroy(e0); hipEventDestroy(e1);
    // rc < 0: with the sink (default for N >= host_sink_min_n in the fp64 mode) the caller's matrix may hold finished block rows
    // beside untouched ones; without it nothing has been copied back
    return rc;
}

// ---- the reference's own symbol (MPF.h:3, C++ linkage) -------------------------------------------
// The reference builds and tears down everything inside every call (MPF.cu:69-97,250-255).  Here the context -- streams,
// workspace, the device copy of the matrix, the row-major working copy -- is created by the first call and lives until the
// process exits: benchmark.cpp:181-266 calls MPF() once per matrix in a loop, and the second call pays H2D + factor + D2H only.
// Calls are serialised (the reference is not re-entrant either: file-scope scratch, hgetf2_kernel.cu:6-7).
namespace {
std::mutex g_mpf_mu;
mpf_ctx *g_mpf_ctx = nullptr;
struct MpfAtExit { ~MpfAtExit() { if (g_mpf_ctx) { mpf_destroy(g_mpf_ctx); g_mpf_ctx = nullptr; } } } g_mpf_at_exit;
}  // namespace

void MPF(double *A, int N, int r, int *IPIV) {
    std::lock_guard<std::mutex> lk(g_mpf_mu);
    if (!g_mpf_ctx && mpf_create(&g_mpf_ctx, 0) != 0) { // reference MPF.cu:69-75: message on stderr, buffers untouched
        g_mpf_ctx = nullptr;
        const char *why = mpf_last_error(nullptr);
        std::cerr << (*why ? why : "No HIP devices available.") << std::endl;
        return;
    }
    mpf_ctx *c = g_mpf_ctx;
    mpf_opts o{};
    o.verbose = c->tune.verbose; // the reference prints one line per panel (MPF.cu:137); off by default here (MPF_VERBOSE=1)
    int rc = mpf_factor_host(c, A, N, r, IPIV, &o);
    if (rc == -4) {
        // The LDS pivot kernel's workgroups were not all resident (something else holds CUs): the reference has no such failure
        // mode (MPF.cu:126-140 is a cooperative launch).  Nothing has been copied back, so the caller's buffers are intact: run
        // the call again on the generic pivot path, which never waits for another workgroup.
        std::cerr << "MPF: " << mpf_last_error(c) << " -- retrying on the generic pivot path" << std::endl;
        o.pivot_path = 1;
        rc = mpf_factor_host(c, A, N, r, IPIV, &o);
    }
    if (rc < 0) std::cout << "MPF error: " << mpf_last_error(c) << std::endl; // reference prints and continues (:134-138)
}
