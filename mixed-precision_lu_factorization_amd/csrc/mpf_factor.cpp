// The factor schedules of the single-GPU driver: the MPF panel loop (reference MPF.cu:66-256) re-architected as asynchronous HIP
// streams of kernels with no per-panel host synchronisation.  mpf_factor_dev picks the schedule; the fp64 row-major one: factor_rm.cpp.
#include "factor_common.h"
#include <climits>
#include <cstdio>

// ---- pieces all schedules share, mpf_factor_dist's among them (factor_common.h) --------------------------------------------------
int factor_check_args(mpf_ctx *c, const char *who, const char *ldname, int64_t N, int32_t nb, int64_t ld, const mpf_opts &o) {
    const std::string w = std::string(who) + ": ";
    if (N <= 0 || nb <= 0) return fail(c, -1, w + "N and panel width must be positive");
    if (ld < N) return fail(c, -1, w + ldname + " < N");
    if (N > INT_MAX / 2) return fail(c, -1, w + "N too large");
    if (nb > 65535) return fail(c, -1, w + "panel width > 65535");
    if (o.trailing < MPF_TRAIL_FP64 || o.trailing > MPF_TRAIL_FP16X3) return fail(c, -1, w + "unknown trailing mode");
    return 0;
}

int factor_report(mpf_ctx *c, mpf_stats &st, int rc, const std::function<hipError_t()> &wait, const char *what, const char *timeout_text) {
    hipEventRecord(c->ev1, c->stream);
    const hipError_t se = wait();
    if (rc) return rc;
    if (se != hipSuccess) return fail(c, -2, std::string(what) + " failed: " + hipGetErrorString(se));
    float ms = 0;
    hipEventElapsedTime(&ms, c->ev0, c->ev1);
    st.ms_total = ms;
    int info = 0, flags0 = 0;
    MPF_HIP_TRY(c, hipMemcpy(&info, &c->ws->info, sizeof(int), hipMemcpyDeviceToHost));
    MPF_HIP_TRY(c, hipMemcpy(&flags0, &c->ws->hp_timeouts, sizeof(int), hipMemcpyDeviceToHost));
    st.info = info == INT_MAX ? 0 : info;
    st.hpanel_timeouts = flags0;
    c->stats = st;
    return flags0 ? fail(c, -4, timeout_text) : st.info;
}

int panel_pivots(const FactorArgs &f, const PanelView &v, hipStream_t s, int waiters, bool generic) {
    mpf_ctx *c = f.c;
    return f.ev.timed(f.st.ms_hpanel, s, [&] {
        if (!generic) return launch_hgetf2(c, v.A + v.k, v.lda, nullptr, 0, v.pr, v.pc, (int)v.k, v.ipiv, nullptr, 0, v.ml, waiters, pref_window_rows(f.o));
        f.st.pivot_path = 1;
        int e = launch_hgetf2_generic(c, v.A + v.k, v.lda, nullptr, 0, v.pr, v.pc, (int)v.k, v.ipiv, nullptr, 0);
        if (!e) e = launch_laswp_plan(c, v.ipiv, (int)v.k, v.pc, v.ml);
        return e; });
}

int panel_tail(const FactorArgs &f, const PanelView &v, hipStream_t s) {
    return f.ev.timed(f.st.ms_dpanel, s, [&] {
        int e = launch_laswp_from_list(f.c, v.A, v.lda, v.pc, v.ml);
        if (!e) e = launch_dgetf2_npv(f.c, v.A + v.k, v.lda, v.pr, v.pc, f.o.fused_panel, (int)v.k);
        return e; });
}

int panel_pieces(const FactorArgs &f, const PanelView &v, int np, const std::function<int(int)> &after_piece) {
    int e = 0;
    for (int q = 0; q < np && !e; ++q) {
        e = launch_laswp_block_gated(f.c, v.A, v.lda, v.pc, (int)v.k + 32 * q, 32, v.ipiv + 32 * q, f.N, 32 * (q + 1));
        if (!e) e = launch_dgetf2_npv_piece(f.c, v.A + v.k, v.lda, v.pr, v.pc, f.o.fused_panel, (int)v.k, q);
        if (!e && after_piece) e = after_piece(q);
    }
    return e;
}

int launch_generic_update(mpf_ctx *c, const mpf_opts &o, int64_t m, int64_t n, int pc, const double *L21, int64_t ldl, double *U12, int64_t ldu) {
    if (o.trailing == MPF_TRAIL_FP64) return launch_dgemm_minus(c, m, n, pc, L21, ldl, U12, ldu, U12 + pc, ldu);
    int e = 0;
    const int kcmax = c->h_kmax;                 // K capacity of the fp16 operand images
    for (int k0 = 0; k0 < pc && !e; k0 += kcmax) {
        const int kc = (pc - k0) < kcmax ? (pc - k0) : kcmax;
        e = launch_cvt_l21(c, L21 + (int64_t)k0 * ldl, ldl, m, kc, o.trailing == MPF_TRAIL_FP16X3);
        if (!e) e = launch_hgemm_minus(c, m, n, kc, U12 + k0, ldu, U12 + pc, ldu, o.trailing == MPF_TRAIL_FP16X3);
    }
    return e;
}

int far_zero_padding(const FactorArgs &f, int64_t ncols, const ImageGeom &g) {
    mpf_ctx *c = f.c;
    if (f.o.trailing == MPF_TRAIL_FP64 || f.nb % 64 == 0 || ncols <= 0) return 0;
    const size_t bytes = (size_t)ncols * g.kst * sizeof(unsigned short);
    MPF_HIP_TRY(c, hipMemsetAsync(c->h_U, 0, bytes, c->stream));
    if (f.o.trailing == MPF_TRAIL_FP16X3) MPF_HIP_TRY(c, hipMemsetAsync(c->h_U + c->h_rows * c->h_kmax, 0, bytes, c->stream));
    return 0;
}

// Full width: one launch of each kind per block instead of one per column piece (a 256-row TRSM costs the same ~90 us for 7000 columns
// as for 28000).  The rows of block p lose what the one-level schedule would have given them panel by panel: identical bits.
int far_block_row(const FactorArgs &f, const FarView &v, const ImageGeom &g, int64_t s0, int p) {
    mpf_ctx *c = f.c; EvPool &ev = f.ev; mpf_stats &st = f.st;
    hipStream_t S = c->stream;
    const bool f64 = f.o.trailing == MPF_TRAIL_FP64, split = f.o.trailing == MPF_TRAIL_FP16X3;
    const int nb = f.nb, K = p * nb;
    const int64_t kq = s0 + K, n = v.ncols;
    MovedList *ml = c->lists + (kq / nb);
    double *Ar = v.A + kq;                                  // the block's rows of the far columns
    float *Wr = v.W ? v.W + kq * v.ldw : nullptr;
    int e = ev.timed(st.ms_laswp, S, [&] { return v.W ? launch_laswp_from_list_f32(c, v.W, v.ldw, n, ml) : launch_laswp_from_list(c, v.A, v.lda, n, ml); });
    if (!e && p > 0) {
        if (f64) e = ev.timed(st.ms_trsm, S, [&] { return launch_dgemm_minus(c, nb, n, K, v.Lsp + kq, v.ldl, v.A + s0, v.lda, Ar, v.lda); }, &st.ms_blockrow);
        else {
            e = ev.timed(st.ms_cvt, S, [&] { return launch_cvt_l21(c, v.Lsp + kq, v.ldl, nb, K, split, 0, g.brow_l_off); });
            if (!e) e = ev.timed(st.ms_trsm, S, [&] {
                return v.W ? launch_hgemm_images_rowmajor(c, nb, n, K, Wr, v.ldw, split, 0, g.brow_l_off, 0, 0, g.kst)
                           : launch_hgemm_images(c, nb, n, K, Ar, v.lda, false, split, 0, g.brow_l_off, 0, 0, g.kst); }, &st.ms_blockrow);
        }
    }
    if (!e && v.W) e = ev.timed(st.ms_cvt, S, [&] { return launch_cvt_f32_f64(c, Wr, v.ldw, Ar, v.lda, nb, n); });
    if (!e) e = ev.timed(st.ms_trsm, S, [&] { return launch_dtrsm_llnu(c, nb, n, v.L11, v.ld11, Ar, v.lda); }, &st.ms_blockrow);
    if (!e && !f64) e = ev.timed(st.ms_cvt, S, [&] { return launch_cvt_u12(c, Ar, v.lda, nb, n, split, (int64_t)K, g.kst); });
    return e;
}

int far_big_update(const FactorArgs &f, const FarView &v, const ImageGeom &g, int64_t s0, int64_t s1, int64_t col, int64_t ncols, int img) {
    mpf_ctx *c = f.c; mpf_stats &st = f.st;
    const bool f64 = f.o.trailing == MPF_TRAIL_FP64, split = f.o.trailing == MPF_TRAIL_FP16X3;
    const int64_t mrows = f.N - s1;
    const int K = (int)(s1 - s0);
    if (ncols <= 0 || mrows <= 0) return 0;
    double *C = v.A + col * v.lda + s1;
    const int e = f.ev.timed(st.ms_gemm, c->stream, [&] {
        if (f64) return launch_dgemm_minus(c, mrows, ncols, K, v.Lsp + s1, v.ldl, v.A + col * v.lda + s0, v.lda, C, v.lda);
        return v.W ? launch_hgemm_images_rowmajor(c, mrows, ncols, K, v.W + s1 * v.ldw + col, v.ldw, split, img, 0, col * g.kst, 0, g.kst)
                   : launch_hgemm_images(c, mrows, ncols, K, C, v.lda, false, split, img, 0, col * g.kst, 0, g.kst); }, &st.ms_gemm_big);
    const double cb = v.W ? 8.0 : 16.0, opb = f64 ? 8.0 : (split ? 4.0 : 2.0);
    count_gemm(st, f.o, mrows, ncols, K, cb);
    st.gemm_big_flops += 2.0 * (double)mrows * (double)ncols * K;
    st.gemm_big_bytes += cb * (double)mrows * (double)ncols + opb * K * (double)(mrows + ncols);
    st.gemm_big_launches++;
    return e;
}

// ---- the panel loop (MPF.cu:100-242) -------------------------------------------------------------

// trailing GEMM of one panel in the selected mode (fp16 mode: the L21 image must already be in c->h_L)
static int trail_gemm(mpf_ctx *c, const mpf_opts &o, int64_t m, int64_t n, int pc, const double *L21, const double *U12,
                      double *C, int64_t lda) {
    if (o.trailing != MPF_TRAIL_FP64) return launch_hgemm_minus(c, m, n, pc, U12, lda, C, lda, o.trailing == MPF_TRAIL_FP16X3);
    return launch_dgemm_minus(c, m, n, pc, L21, lda, U12, lda, C, lda);
}

// Single-stream schedule with a host synchronisation after every phase (per-phase timers).
static int factor_sync_timed(mpf_ctx *c, double *d_A, int64_t lda, int64_t N, int32_t nb, int32_t *d_ipiv,
                             const mpf_opts &o, mpf_stats &st) {
    hipEvent_t pe0, pe1;
    hipEventCreate(&pe0); hipEventCreate(&pe1);
    auto phase = [&](double &acc, auto &&fn) -> int {
        hipEventRecord(pe0, c->stream);
        int rc = fn();
        hipEventRecord(pe1, c->stream);
        hipEventSynchronize(pe1);
        float ms = 0; hipEventElapsedTime(&ms, pe0, pe1);
        acc += ms;
        return rc;
    };
    int rc = 0;
    for (int64_t k = 0; k < N && rc == 0; k += nb) {
        const int pc = (int)((N - k) < nb ? (N - k) : nb);   // MPF.cu:101
        const int pr = (int)(N - k);                         // MPF.cu:102
        if (pr <= 1) break;                                  // MPF.cu:104 (1x1 tail: nothing to do)
        double *Ap = d_A + k * lda + k;
        MovedList *ml = c->lists + (k / nb);
        rc = phase(st.ms_hpanel, [&] { return launch_hgetf2(c, Ap, lda, nullptr, 0, pr, pc, (int)k, d_ipiv + k, nullptr, 0, ml, 0, pref_window_rows(o)); });
        if (rc) break;
        // MPF.cu:162 on the panel and everything right of it; the columns left of it are deferred (laswp.hip)
        rc = phase(st.ms_laswp, [&] { return launch_laswp_from_list(c, d_A + k * lda, lda, N - k, ml); });
        if (rc) break;
        rc = phase(st.ms_dpanel, [&] { return launch_dgetf2_npv(c, Ap, lda, pr, pc, o.fused_panel, (int)k); });
        if (rc) break;
        if (k + pc < N) {                                    // MPF.cu:203
            const int64_t n = N - k - pc;
            double *A12 = d_A + (k + pc) * lda + k;
            rc = phase(st.ms_trsm, [&] { return launch_dtrsm_llnu(c, pc, n, Ap, lda, A12, lda); });           // :215
            if (rc) break;
            rc = phase(st.ms_gemm, [&] {
                int e = o.trailing != MPF_TRAIL_FP64 ? launch_cvt_l21(c, Ap + pc, lda, n, pc, o.trailing == MPF_TRAIL_FP16X3) : 0;
                if (!e) e = trail_gemm(c, o, n, n, pc, Ap + pc, A12, A12 + pc, lda);
                return e; }); // :230
            if (rc) break;
            count_gemm(st, o, n, n, pc);
        }
        st.panels++;
        if (o.verbose) printf("panel k=%lld rows=%d cols=%d\n", (long long)k, pr, pc);
    }
    if (!rc) rc = phase(st.ms_laswp, [&] { return launch_lazy_left_swaps(c, d_A, lda, N, nb, (int)((N + nb - 1) / nb), c->lists); });
    hipEventDestroy(pe0); hipEventDestroy(pe1);
    return rc;
}

// Generic schedule: the reference's own loop (MPF.cu:100-242) step by step on one stream, for everything the tuned
// schedules do not cover -- panels wider than 256 columns, matrices taller than the LDS pivot kernel's 256 rows x #CUs,
// devices / callers that must not run a kernel whose workgroups wait for each other (o.pivot_path = 1).  Interchanges
// are the reference's sequential per-column swaps over ALL N columns (no deferred left-hand side), the TRSM is blocked
// by 256 rows, K is cut to what the update kernels address.  Same per-element operations in the same order as the
// tuned schedules: results are bit-identical (tests/test_gpu_generic.py).
// piv64 (mpf_opts.pivot_search = 1: partial pivoting, 2: tournament pivoting -- the other panel launcher): the pivot kernel, the interchange and the no-pivot panel give way to ONE pivoting fp64 panel
// (dpivot.hip, booked under ms_dpanel), which exchanges the panel's own columns itself; the interchange then covers the columns
// left and right of the panel.  TRSM and update are the same.
static int factor_generic(mpf_ctx *c, double *d_A, int64_t lda, int64_t N, int32_t nb, int32_t *d_ipiv, const mpf_opts &o,
                          mpf_stats &st, bool force_generic_pivots, int piv64) {
    EvPool ev(c);
    ev.keep = &st.ms_gemm;
    hipStream_t S = c->stream;
    int rc = 0;
    for (int64_t k = 0; k < N && rc == 0; k += nb) {
        const int pc = (int)((N - k) < nb ? (N - k) : nb);   // MPF.cu:101
        const int pr = (int)(N - k);                         // MPF.cu:102
        if (pr <= 1) break;                                  // MPF.cu:104
        double *Ap = d_A + k * lda + k;
        if (piv64) {
            rc = ev.timed(st.ms_dpanel, S, [&] {
                return piv64 == 2 ? launch_dgetf2_tp(c, Ap, lda, pr, pc, o.fused_panel, (int)k, (int)k, d_ipiv + k)
                                  : launch_dgetf2_piv(c, Ap, lda, pr, pc, o.fused_panel, (int)k, (int)k, d_ipiv + k); });
            if (rc) break;
            rc = ev.timed(st.ms_laswp, S, [&] {
                int e = launch_laswp_seq(c, d_A, lda, k, (int)k, pc, d_ipiv + k, N);
                if (!e) e = launch_laswp_seq(c, d_A + (k + pc) * lda, lda, N - k - pc, (int)k, pc, d_ipiv + k, N);
                return e; });
            if (rc) break;
        } else {
            rc = ev.timed(st.ms_hpanel, S, [&] {
                if (!force_generic_pivots && hgetf2_lds_eligible(c, pr, pc))
                    return launch_hgetf2(c, Ap, lda, nullptr, 0, pr, pc, (int)k, d_ipiv + k, nullptr, 0, nullptr, 0, pref_window_rows(o));
                st.pivot_path = 1;
                return launch_hgetf2_generic(c, Ap, lda, nullptr, 0, pr, pc, (int)k, d_ipiv + k, nullptr, 0); });
            if (rc) break;
            rc = ev.timed(st.ms_laswp, S, [&] { return launch_laswp_seq(c, d_A, lda, N, (int)k, pc, d_ipiv + k, N); });   // :162
            if (rc) break;
            rc = ev.timed(st.ms_dpanel, S, [&] { return launch_dgetf2_npv(c, Ap, lda, pr, pc, o.fused_panel, (int)k); });  // :183
            if (rc) break;
        }
        if (k + pc < N) {                                    // MPF.cu:203
            const int64_t n = N - k - pc;
            double *A12 = d_A + (k + pc) * lda + k;
            rc = ev.timed(st.ms_trsm, S, [&] { return launch_dtrsm_llnu(c, pc, n, Ap, lda, A12, lda); });             // :215
            if (rc) break;
            rc = ev.timed(st.ms_gemm, S, [&] { return launch_generic_update(c, o, n, n, pc, Ap + pc, lda, A12, lda); });      // :230
            if (rc) break;
            count_gemm(st, o, n, n, pc);
        }
        st.panels++;
        if (o.verbose) printf("panel k=%lld rows=%d cols=%d (generic schedule%s)\n", (long long)k, pr, pc, piv64 == 2 ? ", fp64 tournament pivoting" : piv64 ? ", fp64 pivot search" : "");
    }
    hipError_t se = hipStreamSynchronize(S);
    if (!rc && se != hipSuccess) return fail(c, -2, std::string("factorization failed: ") + hipGetErrorString(se));
    ev.collect();
    return rc;
}

// The plain chain of the panel at k on stream s: pivot kernel, then the interchange of the panel's own columns and the fp64 panel.
static PanelView panel_at(const FactorArgs &f, int64_t k) {
    const int64_t pr = f.N - k;
    return {f.d_A + k * f.lda, f.lda, k, (int)pr, (int)(pr < f.nb ? pr : f.nb), f.c->lists + (k / f.nb), f.d_ipiv + k};
}
int panel_chain(const FactorArgs &f, int64_t k, hipStream_t s) {
    if (f.N - k <= 1) return 0;
    StreamSwap sw(f.c, s);
    const PanelView v = panel_at(f, k);
    int e = panel_pivots(f, v, s, 0);
    if (!e) e = panel_tail(f, v, s);
    f.st.panels++;
    return e;
}

// The chain of the NEXT panel (at nx) on the side streams, behind e1: the panel's columns are up to date (recorded by the caller).
// What the caller gets back: the launches' error code and the events that mark the chain's end -- `a` alone for the plain chain
// (on P), `a` and `b` for the pipelined one (`a` follows the pivot kernel on P: its moved-row list is complete; `b` the last
// fp64-panel piece on T).
//
// Pipelined: the fp64 panel FOLLOWS the pivot kernel instead of waiting for it.  The pivot kernel (stream P) publishes its progress
// every 32 columns; stream T runs, per 32-column sub-panel s: a gate (waits for the pivots of columns < 32 (s + 1)), the reference's
// sequential interchange of exactly those 32 pivots on the panel's columns (LASWP applied in instalments is LASWP: MPF.cu:47-57),
// and piece s of the fp64 panel -- whose rows below the sub-panel are row-independent, so the swaps still to come only move finished
// rows around (what LAPACK's blocked dgetf2 does).  Same operations per element as the plain chain: bit-identical.  The plain
// chain runs when the shape has no pieces or there is no third stream, and in the two cases below.
ChainEnd chain_behind(const FactorArgs &f, int64_t nx, hipEvent_t e1) {
    mpf_ctx *c = f.c; EvPool &ev = f.ev;
    const PanelView v = panel_at(f, nx);
    hipStream_t P = c->pstream, T = c->tstream;
    const int np = dgetf2_npv_pieces(c, v.pc);
    const int waiters = (c->tune.gate_wait_value && c->hp_signal) ? 0 : laswp_gated_grid(v.pc);   // (a stream that waits holds no CU)
    const bool piped = c->tune.chain_pipeline && np != 0 && T && P &&
        // fp64 mode: while the update is the longer side (large trailing matrix) the chain hides under it anyway, and the extra
        // launches beside it only cost the update time (measured + 4 ms per factorization): pipeline the chain-bound panels only
        !(f.o.trailing == MPF_TRAIL_FP64 && v.pr > c->tune.chain_pipeline_below) &&
        // the gated interchange kernel's workgroups wait for the pivot kernel while sitting on CUs: the panel must fit beside them
        // (else the chain runs unpipelined: nobody waits for a kernel whose workgroups cannot all become resident)
        hgetf2_fits_beside(c, v.pr, v.pc, waiters);
    ChainEnd r;
    hipStreamWaitEvent(P, e1, 0);
    if (!piped) {
        r.rc = panel_chain(f, nx, P);
        r.a = ev.get();
        hipEventRecord(r.a, P);
        return r;
    }
    hipStreamWaitEvent(T, e1, 0);
    {
        StreamSwap sw(c, P);
        r.rc = panel_pivots(f, v, P, waiters);
        r.a = ev.get();
        hipEventRecord(r.a, P);
    }
    if (!r.rc) {
        StreamSwap sw(c, T);
        r.rc = ev.timed(f.st.ms_dpanel, T, [&] { return panel_pieces(f, v, np); });
        r.b = ev.get();
        hipEventRecord(r.b, T);
    }
    f.st.panels++;
    return r;
}

// The end of a look-ahead schedule, once the caller has joined into the main stream whatever its last step there depends on: that
// step (with a row sink the last block rows leave -- the sink applies the left-hand interchanges on the way out, the device matrix
// keeps them owed; otherwise the deferred left-hand interchanges run), then the host waits for every stream of the schedule and
// reports.  rc of a failed launch wins over a stream's error.
int factor_epilogue(const FactorArgs &f, int rc, bool sink, int sb, bool side_streams) {
    mpf_ctx *c = f.c;
    hipStream_t S = c->stream;
    const int npanels = (int)((f.N + f.nb - 1) / f.nb);
    if (sink) sink_notify(c, npanels, S);
    else if (!rc) {
        rc = f.ev.timed(f.st.ms_laswp, S, [&] { return launch_lazy_left_swaps(c, f.d_A, f.lda, f.N, f.nb, npanels, c->lists, sb); });
        f.st.lazy_onepass_blocks = c->lazy_onepass_blocks;
    }
    hipError_t se = sink_stream_wait(c, S);   // (hipStreamSynchronize unless a sink's thread is copying)
    hipError_t sp = side_streams ? sink_stream_wait(c, c->pstream) : hipSuccess;
    if (side_streams && c->tstream) { const hipError_t stt = sink_stream_wait(c, c->tstream); if (sp == hipSuccess) sp = stt; }
    if (!rc && (se != hipSuccess || sp != hipSuccess))
        return fail(c, -2, std::string("factorization failed: ") + hipGetErrorString(se != hipSuccess ? se : sp));
    f.ev.collect();
    f.st.lookahead = side_streams ? 1 : 0;
    return rc;
}

// Look-ahead schedule.  Main stream S: trailing updates and the row interchanges of everything outside the
// next panel.  Side stream P (high priority): the latency-bound chain of the NEXT panel -- fp16 pivots, the
// interchange of the panel's own columns, the fp64 panel -- which starts as soon as the update of panel k has
// reached the next panel's columns (the "strip") and runs under the rest of that update.
//   S: [swap_k others] [trsm_k strip][gemm_k strip] E1 [trsm_k rest][gemm_k rest] wait(E2) [swap_k+1 others] ...
//   P:                                   wait(E1) [pivots_k+1][swap_k+1 strip][dpanel_k+1] E2
// Per element the operations and their order are those of the single-stream schedule: results are identical.
// (Tried and dropped: confining S to 192 CUs and giving P the other 64 through hipExtStreamCreateWithCUMask for the
//  chain-bound panels.  In isolation the pivot kernel under a running hgemm went from 1766 us to 802 us, but in the
//  schedule the fp64 panel and the strip updates lost more on the smaller partitions than the pivot kernel gained:
//  fp64 537 vs 517 ms, fp16 322 vs 301 ms at N = 32768.)
static int factor_lookahead(mpf_ctx *c, double *d_A, int64_t lda, int64_t N, int32_t nb, int32_t *d_ipiv,
                            const mpf_opts &o, mpf_stats &st) {
    hipStream_t S = c->stream, P = c->pstream;
    EvPool ev(c);
    ev.keep = &st.ms_gemm;
    const FactorArgs f{c, ev, st, o, d_A, lda, N, nb, d_ipiv};
    int rc = 0;
    const bool sink = sink_take(c, d_A, lda, N, nb);   // (mpf_factor_host: block rows leave as they become final, rowsink.hip)
    stream_join(ev, S, P);   // P must see everything already queued on S (the input matrix may still be in flight there)
    // panel 0 has nothing to hide under
    {
        const int pc = (int)(N < nb ? N : nb), pr = (int)N;
        if (pr > 1) {
            rc = ev.timed(st.ms_hpanel, S, [&] {
                int e = launch_hgetf2(c, d_A, lda, nullptr, 0, pr, pc, 0, d_ipiv, nullptr, 0, c->lists, 0, pref_window_rows(o));
                const int64_t first = (int64_t)pc + nb < N ? (int64_t)pc + nb : N; // panel 0 and the strip right of it
                if (!e) e = launch_laswp_from_list(c, d_A, lda, first, c->lists);
                if (!e) e = launch_dgetf2_npv(c, d_A, lda, pr, pc, o.fused_panel, 0);
                return e;
            });
            st.panels++;
        }
    }
    for (int64_t k = 0; k < N && rc == 0; k += nb) {
        const int pc = (int)((N - k) < nb ? (N - k) : nb);
        if (N - k <= 1 || k + pc >= N) break;
        const int64_t n = N - k - pc;          // trailing size
        const int64_t nx = k + pc;             // first row/column of the next panel
        const int pc2 = (int)((N - nx) < nb ? (N - nx) : nb);
        const bool has_next = (N - nx) > 1;
        double *Ap = d_A + k * lda + k;
        double *A12 = d_A + nx * lda + k;      // U12 block row, starts at the strip
        const int64_t ns = has_next ? pc2 : n; // columns updated before the side stream may start
        // ---- strip (or everything, when no panel follows) ---------------------------------------------
        rc = ev.timed(st.ms_trsm, S, [&] { return launch_dtrsm_llnu(c, pc, ns, Ap, lda, A12, lda); });
        if (rc) break;
        rc = ev.timed(st.ms_gemm, S, [&] {
            int e = o.trailing != MPF_TRAIL_FP64 ? launch_cvt_l21(c, Ap + pc, lda, n, pc, o.trailing == MPF_TRAIL_FP16X3) : 0; // once per panel
            if (!e) e = trail_gemm(c, o, n, ns, pc, Ap + pc, A12, A12 + pc, lda);
            return e; });
        if (rc) break;
        count_gemm(st, o, n, ns, pc);
        if (!has_next) break;
        hipEvent_t e1 = ev.get();
        hipEventRecord(e1, S);
        // ---- side streams: the whole chain of panel k+1 ---------------------------------------------------
        const ChainEnd next = chain_behind(f, nx, e1);
        rc = next.rc;
        if (rc) break;
        // ---- main stream: interchanges of panel k on the columns right of the strip (the strip and the panel had
        //      theirs before the strip update), the rest of update k, then panel k+1's interchanges on the next strip
        if (n > pc2) {
            rc = ev.timed(st.ms_laswp, S, [&] {
                return launch_laswp_from_list(c, d_A + (nx + pc2) * lda, lda, N - nx - pc2, c->lists + (k / nb)); });
            if (rc) break;
            double *A12r = A12 + (int64_t)pc2 * lda;
            rc = ev.timed(st.ms_trsm, S, [&] { return launch_dtrsm_llnu(c, pc, n - pc2, Ap, lda, A12r, lda); });
            if (rc) break;
            if (sink) sink_notify(c, (int)(k / nb) + 1, S);   // block row k: pivoted, U solved
            rc = ev.timed(st.ms_gemm, S, [&] { return trail_gemm(c, o, n, n - pc2, pc, Ap + pc, A12r, A12r + pc, lda); });
            if (rc) break;
            count_gemm(st, o, n, n - pc2, pc);
        }
        hipStreamWaitEvent(S, next.a, 0);
        if (next.b) hipStreamWaitEvent(S, next.b, 0);
        rc = ev.timed(st.ms_laswp, S, [&] { // only the next strip now: it is all the next strip update needs
            const int64_t s0 = nx + pc2;
            const int64_t sw = (N - s0) < nb ? (N - s0) : nb;
            return sw > 0 ? launch_laswp_from_list(c, d_A + s0 * lda, lda, sw, c->lists + (nx / nb)) : 0;
        });
        if (o.verbose) printf("panel k=%lld rows=%lld cols=%d (look-ahead)\n", (long long)nx, (long long)(N - nx), pc2);
    }
    if (sink) stream_join(ev, P, S);   // the last block rows leave behind the last chain
    return factor_epilogue(f, rc, sink, 1, true);
}

// Two-level schedule (default of the fp16 trailing modes).  The fp16 update streams the trailing matrix through the chip
// once per launch: with K = nb = 256 it is HBM-bound at ~5 % of the fp16 MFMA peak.  Here `sb` panels form a super-panel
// [c0, c1): inside it a panel only updates an INNER REGION of at most (sb + 1) * nb columns (right-looking, K = nb, on the
// fp64 matrix), and everything right of the inner region gets ONE update with K = sb * nb per super-panel -- after the
// interchanges of the sb panels and the U block-row
//   U[c0:c1, cols] = L_SS^-1 A[c0:c1, cols]      (one blocked fp64 TRSM over the super-panel's unit-lower block)
// so the trailing matrix is read and written N / (sb * nb) times instead of N / nb times.
//
// Inner region = the super-panel's own columns PLUS the next super-panel's first panel [c1, c1 + nb) (round 3).  That
// look-ahead panel is brought up to date panel by panel like the super-panel's own columns, so when the last panel of the
// super-panel is done the next pivot kernel starts at once: the heavy end-of-super-panel work (operand images, block-row,
// K = sb * nb update of the next inner region's columns, conversions) runs UNDER that chain instead of in front of it, and
// every panel of the factorization has the same short critical path (chain + one strip step).
//
// What is right of the inner region is owed the super-panel's update: the columns that join the next inner region
// [c1 + nb, c2 + nb) get it at the end of the super-panel, the rest as a pending job that the main stream works off in
// pieces, left to right, one under each panel chain of the next super-panel.  Two L images stay alive for that.
// fp16 modes: the matrix right of the inner region lives in an fp32 WORKING COPY W (same coordinates as A, but ROW-major:
// element (i, j) at W[i * N + j]): the K-updates then move 8 instead of 16 bytes of HBM per element and an interchange moves
// contiguous row segments instead of one element per 64-byte sector (laswp.hip).  A column range returns to fp64
// when it joins the inner region (panels, TRSMs and the finished factors are fp64); the block-row of a super-panel is
// converted just before its TRSM.  The products are fp16 x fp16 anyway (contract C6): an fp32 accumulator of the trailing
// matrix adds 2^-24 per update to an error of 2^-11 per product.  Option fp16_work32 = 0 updates the fp64 matrix in place.
// fp64 mode (option superpanel_fp64 > 1): same loop, updates straight from the matrix; per element the fma chain is the
// one-level schedule's (k ascending across the panels): identical bits.  overlap = false: same operations on one stream.
static int factor_superpanel(mpf_ctx *c, double *d_A, int64_t lda, int64_t N, int32_t nb, int32_t *d_ipiv, const mpf_opts &o,
                             mpf_stats &st, int sb, bool overlap) {
    // Three lanes (overlap = true; otherwise everything runs on the one stream, same operations):
    //   chain    P (+ T): pivots and fp64 panel of the next panel;
    //   inner    Ci (high priority): the short critical work between two chains -- interchanges of the super-panel's earlier
    //            columns, the strip step that releases the next chain (E1), the rest of the inner region;
    //   far      S: everything right of the inner region (block-row tasks, operand images, K = sb * nb updates, conversions).
    // The lanes meet only at events: a far launch never sits in front of a strip step in a queue, and far work that takes
    // longer than one chain spills under the next one instead of delaying it.
    hipStream_t S = c->stream, P = overlap ? c->pstream : c->stream;
    // (the inner lane shares the chain's second stream T: its work sits between two chains, when T is idle -- a fourth stream
    //  of its own would exceed the four hardware queues a process gets by default, and streams that share a queue serialise)
    hipStream_t Ci = (overlap && c->tstream) ? c->tstream : c->stream;
    const bool lanes = Ci != S;
    EvPool ev(c);
    ev.keep = &st.ms_gemm;
    const FactorArgs f{c, ev, st, o, d_A, lda, N, nb, d_ipiv};
    int rc = 0;
    const bool split = o.trailing == MPF_TRAIL_FP16X3;
    const bool f64 = o.trailing == MPF_TRAIL_FP64;
    const bool use32 = !f64 && c->tune.fp16_work32 != 0 && N > (int64_t)(sb + 1) * nb;
    float *W = nullptr;
    const int64_t ldw = N;
    if (use32) {
        MPF_HIP_TRY(c, c->w32.grow(N * N));
        W = c->w32;
    }
    if (overlap) stream_join(ev, S, P);
    const int64_t sbw = (int64_t)sb * nb;
    const ImageGeom g = image_geom(N, N - (int64_t)(sb + 1) * nb, sb, nb, c->h_kmax, f64);
    auto width = [&](int64_t k) { return (int)((N - k) < nb ? (N - k) : nb); };
    auto side_chain = [&](int64_t kx, hipEvent_t e1, hipEvent_t &e2) -> int { // chain of the panel at kx (N - kx > 1) behind E1, E2 behind all of it
        if (!overlap) return panel_chain(f, kx, S);
        const ChainEnd next = chain_behind(f, kx, e1);
        e2 = next.a;
        if (!next.rc && next.b) {   // pipelined: one event behind both of its streams
            e2 = ev.get();
            hipStreamWaitEvent(c->tstream, next.a, 0);
            hipEventRecord(e2, c->tstream);
        }
        return next.rc;
    };
    // one right-looking step of panel k (width pc) on the inner-region columns [col0, col0 + ncols), all in the fp64 matrix, on
    // the inner lane: interchange, TRSM with the panel's L11, K = pc update of the rows below.  need_img: convert the panel's L21
    // image first.
    // the panel's L21 image (fp16 modes): on the pivot stream, which is idle between two pivot kernels, beside the strip's TRSM
    hipEvent_t img_ready = nullptr;
    auto l21_image = [&](int64_t k, int pc) -> int {
        if (f64) return 0;
        const int64_t mrows = N - k - pc;
        if (mrows <= 0) return 0;
        hipStream_t Is = (lanes && P != S) ? P : Ci;
        if (Is != Ci) stream_join(ev, Ci, Is);   // the chain of panel k is done (Ci waited for it)
        StreamSwap sw(c, Is);
        int e = ev.timed(st.ms_cvt, Is, [&] { return launch_cvt_l21(c, d_A + k * lda + k + pc, lda, mrows, pc, split); });
        if (Is != Ci) { img_ready = ev.get(); hipEventRecord(img_ready, Is); } else img_ready = nullptr;
        return e;
    };
    auto inner_step = [&](int64_t k, int pc, int64_t col0, int64_t ncols, bool first) -> int {
        if (ncols <= 0) return 0;
        StreamSwap sw(c, Ci);
        double *Ap = d_A + k * lda + k, *A12 = d_A + col0 * lda + k;
        const int64_t mrows = N - k - pc;
        int e = ev.timed(st.ms_trsm, Ci, [&] { return launch_dtrsm_llnu(c, pc, ncols, Ap, lda, A12, lda); });
        if (e || mrows <= 0) return e;
        if (!f64) {
            e = ev.timed(st.ms_cvt, Ci, [&] { return launch_inner_u_image(c, o, A12, lda, pc, ncols, g.inner_u_off); });
            if (first && img_ready) hipStreamWaitEvent(Ci, img_ready, 0);
        }
        if (!e) e = ev.timed(st.ms_gemm, Ci, [&] { return launch_inner_gemm(c, o, mrows, ncols, pc, Ap + pc, lda, A12, lda, g.inner_u_off); });
        count_gemm(st, o, mrows, ncols, pc);
        return e;
    };
    // ---- far lane: everything right of the inner region ("far" columns [f0, N) of the super-panel [s0, s1)) -----------------------
    // U block-row, one block per finished panel p of the super-panel (task T_p: far_block_row, factor_common.h).
    // Then the update itself: operand image of L[s1.., s0..s1) once, the kernel on the columns that join the next inner region
    // first (they return to fp64: event NI releases the inner lane), then on all the rest in one launch.  U image:
    // Uh[n_far][kst] at the start of the context's U buffer; the inner region's steps keep their small image behind it.
    struct Far { bool on = false; int64_t s0 = 0, s1 = 0, f0 = 0; int done = 0, img = 1; } far;
    std::vector<hipEvent_t> panel_done;   // per panel of the current super-panel: recorded on the inner lane after its eager interchanges
    // the far job's columns: in the matrix (fp64 mode, fp16 modes in place) or in the fp32 copy; L and the L11 of panel p in the matrix
    auto far_view = [&](const Far &fj, int p) -> FarView {
        const int64_t kq = fj.s0 + (int64_t)p * nb;
        return {d_A + fj.f0 * lda, lda, use32 ? W + fj.f0 : nullptr, ldw, N - fj.f0, d_A + fj.s0 * lda, lda, d_A + kq * lda + kq, lda};
    };
    auto far_task = [&](int p) -> int {   // T_p of the current far job
        if (N - far.f0 <= 0) return 0;
        if (lanes) hipStreamWaitEvent(S, panel_done[(size_t)p], 0);
        return far_block_row(f, far_view(far, p), g, far.s0, p);
    };
    auto far_tasks_upto = [&](int ready) -> int { // run the block-row tasks of the panels 0 .. ready - 1 that have not run yet
        int e = 0;
        while (far.on && !e && far.done < ready) { e = far_task(far.done); far.done++; }
        return e;
    };
    // the K = s1 - s0 update of the far job on the columns [col0, col0 + ncols) (block-row and U image complete)
    auto big_update = [&](const Far &fj, int64_t col0, int64_t ncols) { return far_big_update(f, far_view(fj, 0), g, fj.s0, fj.s1, col0 - fj.f0, ncols, fj.img); };
    // a column range that joins the next inner region returns to fp64: rows >= r0 (above them: finished U rows in A)
    auto back_to_f64 = [&](int64_t r0, int64_t col0, int64_t ncols) -> int {
        if (!use32 || ncols <= 0) return 0;
        return ev.timed(st.ms_cvt, S, [&] { return launch_cvt_f32_f64(c, W + r0 * ldw + col0, ldw, d_A + col0 * lda + r0, lda, N - r0, ncols); });
    };
    // Without lanes (single stream) the far work is issued in the same program order, so a pending job is just a deferred
    // launch: the rest of a super-panel's update is issued right after the part the next inner region needs.
    auto inner_end = [&](int64_t c1) { return (c1 + nb) < N ? (c1 + nb) : N; };   // inner region of the super-panel ending at c1
    {
        const int64_t e1 = inner_end(sbw < N ? sbw : N);
        if (use32 && e1 < N) rc = ev.timed(st.ms_cvt, S, [&] { return launch_cvt_f64_f32(c, d_A + e1 * lda, lda, W + e1, ldw, N, N - e1); });
    }
    if (!rc) rc = panel_chain(f, 0, S);
    hipEvent_t chain_done = nullptr;       // the chain of the panel the next iteration starts with
    if (lanes) { chain_done = ev.get(); hipEventRecord(chain_done, S); }
    hipEvent_t ni_ready = nullptr;         // the columns that joined the current inner region are back in fp64 and up to date (far lane)
    int next_img = 1;
    for (int64_t c0 = 0; c0 < N && rc == 0; c0 += sbw) {
        const int64_t c1 = (c0 + sbw) < N ? (c0 + sbw) : N;
        const int64_t e1c = inner_end(c1);
        const int npan = (int)((c1 - c0 + nb - 1) / nb);
        far = Far();
        if (e1c < N) {
            far.on = true; far.s0 = c0; far.s1 = c1; far.f0 = e1c; far.img = next_img; next_img = 3 - next_img;
            rc = far_zero_padding(f, N - e1c, g);
        }
        panel_done.assign((size_t)npan, nullptr);
        bool stop = false;
        int it = 0;
        for (int64_t k = c0; k < c1 && rc == 0; k += nb, ++it) {
            const int pc = width(k);
            const int64_t nx = k + pc;
            if (lanes) {
                hipStreamWaitEvent(Ci, chain_done, 0);
                if (it == 0 && ni_ready) hipStreamWaitEvent(Ci, ni_ready, 0);   // this super-panel's new inner columns
            }
            // ONE interchange launch for the whole inner region: the super-panel's earlier columns [c0, k) (now, not with the deferred
            // ones at the end: the K = c1 - c0 update reads them in final row order) and the columns [nx, e1) right of the panel
            {
                StreamSwap sw(c, Ci);
                const int64_t right = (N - k <= 1 || nx >= N) ? 0 : e1c - nx;
                if ((k - c0) + right > 0)
                    rc = ev.timed(st.ms_laswp, Ci, [&] { return launch_laswp_from_list_hole(c, d_A + c0 * lda, lda, (k - c0) + right, c->lists + (k / nb), k - c0, pc); });
            }
            if (rc) break;
            if (lanes) { panel_done[(size_t)it] = ev.get(); hipEventRecord(panel_done[(size_t)it], Ci); }
            if (N - k <= 1 || nx >= N) { stop = true; break; }
            hipEvent_t e2 = nullptr;
            const int64_t sw_ = (e1c - nx) < nb ? (e1c - nx) : nb;     // the strip = the next panel's columns: always inside the inner region
            rc = l21_image(k, pc);
            if (!rc) rc = inner_step(k, pc, nx, sw_, true);
            hipEvent_t e1 = nullptr;
            if (!rc && overlap) { e1 = ev.get(); hipEventRecord(e1, Ci); }   // E1: the next panel's columns are up to date
            // the rest of the inner region is issued BEFORE the chain's launches: on the shared stream it runs beside the first
            // 32 columns of the pivot kernel (stream P), and the fp64 panel's pieces (this stream) follow 32 columns behind anyway
            if (!rc) rc = inner_step(k, pc, nx + sw_, e1c - nx - sw_, false);
            if (!rc && N - nx > 1) rc = side_chain(nx, e1, e2);
            // ---- far lane: panels c0 .. k of this super-panel are complete ----------------------------------------------------
            if (!rc) rc = far_tasks_upto(it + 1);
            if (rc) break;
            if (nx >= c1 && far.on) {
                // the super-panel is complete: its update on the columns that join the next inner region first, then the rest
                const int64_t c2 = (c1 + sbw) < N ? (c1 + sbw) : N;
                const int64_t e2c = inner_end(c2);
                if (!rc && !f64) rc = ev.timed(st.ms_cvt, S, [&] { return launch_cvt_l21(c, d_A + c0 * lda + c1, lda, N - c1, (int)(c1 - c0), split, far.img); });
                if (!rc) rc = big_update(far, e1c, e2c - e1c);
                if (!rc) rc = back_to_f64(c1, e1c, e2c - e1c);
                if (lanes) { ni_ready = ev.get(); hipEventRecord(ni_ready, S); }
                if (!rc) rc = big_update(far, e2c, N - e2c);
                if (rc) break;
            }
            if (overlap) { if (e2) { if (lanes) chain_done = e2; else hipStreamWaitEvent(S, e2, 0); } }
            if (o.verbose) printf("panel k=%lld rows=%lld (super-panel [%lld, %lld))\n", (long long)nx, (long long)(N - nx), (long long)c0, (long long)c1);
        }
        if (stop) break;
    }
    if (lanes) {
        stream_join(ev, Ci, S);
        if (chain_done) hipStreamWaitEvent(S, chain_done, 0);
    }
    return factor_epilogue(f, rc, false, sb, overlap);   // (the inner lane's stream Ci is S or T: among the streams it waits for)
}

int mpf_factor_setup(mpf_ctx *c, int64_t N, int32_t nb, int32_t npanels, bool lists) {
    if (lists) {
        MPF_HIP_TRY(c, c->lists.grow(npanels));
        // N x nb doubles for the deferred left-hand interchanges; at least N x 256 so that the scratch also holds the
        // 2 * HP_MAXCOLS moved rows x N (or a rank's local) columns (fp32) of an interchange on the row-major working copy
        MPF_HIP_TRY(c, c->perm_tmp.grow(N * (int64_t)(nb > HP_MAXCOLS ? nb : HP_MAXCOLS)));
        MPF_HIP_TRY(c, c->Fmap.grow(2 * N));   // the map and its inverse
        if (c->tune.lazy_gather == 2) MPF_HIP_TRY(c, c->lazy_snap.grow(lazy_snap_elems(N, nb, npanels, 1)));   // (super-panels keep fewer snapshots)
        MPF_HIP_TRY(c, hipMemsetAsync(c->lists, 0, (size_t)npanels * sizeof(MovedList), c->stream));
    }
    const int imax = INT_MAX;
    MPF_HIP_TRY(c, hipMemcpyAsync(&c->ws->info, &imax, sizeof(int), hipMemcpyHostToDevice, c->stream));
    MPF_HIP_TRY(c, hipMemsetAsync(&c->ws->hp_timeouts, 0, sizeof(int), c->stream));
    return 0;
}

int mpf_factor_dev(mpf_ctx *c, double *d_A, int64_t lda, int64_t N, int32_t nb, int32_t *d_ipiv, const mpf_opts *opts) {
    if (!c || !d_A || !d_ipiv) return -1;
    mpf_opts o{};
    if (opts) o = *opts;
    if (factor_check_args(c, "mpf_factor", "lda", N, nb, lda, o)) return -1;
    if (o.pivot_search < 0 || o.pivot_search > 2)
        return fail(c, -1, "mpf_factor: unknown pivot_search (0: fp16 image, 1: fp64 partial pivoting, 2: fp64 tournament pivoting)");
    // fp64 pivot rules (1 partial, 2 tournament pivoting): the generic schedule's loop in every mode; an explicit rule wins over the option
    const int piv64 = o.pivot_search != 0 ? o.pivot_search : c->tune.pivot_fp64;
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    // tuned schedules need every panel to fit the LDS pivot kernel (<= 256 columns, all its workgroups resident at once);
    // anything else, and callers that ask for it, get the generic schedule
    const bool force_generic = o.pivot_path == 1 || safe_pivots(c);
    const bool generic = piv64 || force_generic || !hgetf2_lds_eligible(c, (int)N, (int)(nb < N ? nb : N));
    // super-panels need equal-width column blocks left of every panel (deferred interchanges), i.e. N > sb * nb columns of nb
    const int want_sb = wanted_superpanel(c, o, N);
    const int sb = (!generic && !o.sync_timing && (int64_t)want_sb * nb < N) ? want_sb : 1;
    if (o.trailing != MPF_TRAIL_FP64) {
        const int64_t kimg = (int64_t)sb * nb < 8 * HP_MAXCOLS ? (int64_t)sb * nb : 8 * HP_MAXCOLS; // the generic schedule cuts K to the images
        int e = mpf_ensure_h_images(c, N + HP_MAXCOLS + 64, (int)kimg, sb > 1); if (e) return e;   // + room for the block-row L images
    }
    { const int e = mpf_factor_setup(c, N, nb, (int)((N + nb - 1) / nb), !generic); if (e) return e; }
    if (piv64) { const int e = piv64 == 2 ? dgetf2_tp_reserve(c, (int)N) : dgetf2_piv_reserve(c, (int)N); if (e) return e; }
    mpf_stats st{};
    st.n = N; st.nb = nb; st.superpanel = sb;
    st.pivot_search = piv64;
    st.fp16_fused = piv64 ? 0 : (c->tune.fp16_fused != 0);   // what ran: the fp64 pivot rules run no fp16 panel
    const bool lookahead = !o.sync_timing && !o.no_lookahead && !c->tune.no_lookahead && c->pstream != nullptr;
    // the row-major working copy of the fp64 mode is allocated BEFORE the clock starts (a context's first call pays hipMalloc
    // of N x N doubles once; ms_total is the factorization)
    const bool use_rm = !generic && sb <= 1 && lookahead && o.trailing == MPF_TRAIL_FP64 && c->tune.fp64_rowmajor &&
                        N >= c->tune.fp64_rowmajor_min_n && N > nb && mpf_ensure_rowmajor_copy(c, N, N, nb) == 0;
    // the paired bulk phase keeps two row-major images of a pair's L21, [rows][2 nb]; without room for them the one-level loop runs
    bool use_pairs = use_rm && c->tune.fp64_pair && c->tune.fp64_two_lanes > 0 && c->tstream && nb % 16 == 0 && N > c->tune.fp64_pair_min_n;
    // (and none while the first pivot kernels need nearly every CU: factor_rm_pairs starts at panel 0 or not at all -- N = 65536 stays one-level)
    if (use_pairs && !pivots_fit_beside_update(c, N - nb)) use_pairs = false;
    if (use_pairs && c->rm_pair.grow(4 * N * (int64_t)nb) != hipSuccess) { (void)hipGetLastError(); use_pairs = false; }
    if (c->late && !use_rm) {   // (mpf_factor_host planned on the row-major schedule and it is not the one that runs: everything has to be here first)
        const int e = feed_finish(c);
        c->late = nullptr;
        if (e) return e;
    }
    MPF_HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
    int rc;
    if (generic) rc = factor_generic(c, d_A, lda, N, nb, d_ipiv, o, st, force_generic, piv64);
    else if (sb > 1) rc = factor_superpanel(c, d_A, lda, N, nb, d_ipiv, o, st, sb, lookahead);
    else if (use_rm) rc = factor_lookahead_rm(c, d_A, lda, N, nb, d_ipiv, o, st, use_pairs);
    else if (lookahead) rc = factor_lookahead(c, d_A, lda, N, nb, d_ipiv, o, st);
    else rc = factor_sync_timed(c, d_A, lda, N, nb, d_ipiv, o, st);
    const double h2d = c->stats.ms_h2d, d2h = c->stats.ms_d2h;   // (mpf_factor_host's transfers: they outlive the statistics of this call)
    rc = factor_report(c, st, rc, [&] { return sink_stream_wait(c, c->stream); }, "factorization",
                       "fp16 pivot kernel: inter-workgroup hand-off timed out (its workgroups were not all resident: GPU "
                       "shared with another process?).  d_A and ipiv are invalid.  Use mpf_opts.pivot_path = 1 or MPF_SAFE_PIVOTS=1");
    c->stats.ms_h2d = h2d; c->stats.ms_d2h = d2h;
    if (o.trailing == MPF_TRAIL_FP64 && N >= 8192 && st.ms_total > 0)   // what mpf_gesv prices an fp64 refactorization with
        c->fp64_rate_tflops = 2.0 / 3.0 * (double)N * (double)N * (double)N / (st.ms_total * 1e-3) / 1e12;
    return rc;
}
