// The fp64 mode's look-ahead schedule on a ROW-MAJOR working copy of the trailing matrix: the five steps on that copy (RmView,
// factor_common.h -- the multi-rank loop of mpf_dist.cpp runs them on a rank's local columns), the paired bulk phase, the one-level
// loop with its two-lane and one-lane turns, the replay of the panels on late column segments (mpf_factor_host's LatePlan).
#include "factor_common.h"
#include <cstdio>

// ---- the steps: each issues its launches on c->stream (the caller's StreamSwap scope) under one timer on stream s ------------------------
int rm_swap(const FactorArgs &f, const RmView &v, hipStream_t s, int64_t c, int64_t w, std::initializer_list<const MovedList *> lists, int64_t scratch_off) {
    return f.ev.timed(f.st.ms_laswp, s, [&] {
        int e = 0;
        for (const MovedList *ml : lists) if (!e) e = launch_laswp_from_list_rm64(f.c, v.r(0, c), v.ldr, w, ml, scratch_off);
        return e; });
}
int rm_solve_u(const FactorArgs &f, const RmView &v, hipStream_t s, const double *L11, int64_t ld11, int64_t k, int pc, int64_t c, int64_t w) {
    return f.ev.timed(f.st.ms_trsm, s, [&] { return launch_dtrsm_llnu_strided(f.c, pc, w, L11, ld11, v.r(k, c), v.ldr, 1); });
}
int rm_update(const FactorArgs &f, const RmView &v, hipStream_t s, int64_t ku, int K, int64_t r0, int64_t rows, int64_t c, int64_t w, const double *Limg, int64_t ldimg) {
    const int e = f.ev.timed(f.st.ms_gemm, s, [&] { return launch_dgemm_minus(f.c, w, rows, K, v.r(ku, c), v.ldr, Limg, ldimg, v.r(r0, c), v.ldr); });
    count_gemm(f.st, f.o, rows, w, K);
    return e;
}
int rm_home(const FactorArgs &f, const RmView &v, hipStream_t s, int64_t row, int64_t rows, int64_t c, int64_t w, int64_t split) {
    return f.ev.timed(f.st.ms_cvt, s, [&] {
        if (split <= 0) return launch_transpose64(f.c, v.a(row, c), v.lda, v.r(row, c), v.ldr, rows, w, false);
        int e = launch_transpose64(f.c, v.a(row, c), v.lda, v.r(row, c), v.ldr, split, w, false);
        if (!e) e = launch_transpose64(f.c, v.a(row + split, c), v.lda, v.r(row + split, c), v.ldr, rows - split, w, false);
        return e; });
}
int rm_l_image(const FactorArgs &f, hipStream_t s, const double *src, int64_t lds, int64_t rows, int64_t cols, double *img, int64_t ldimg) {
    return f.ev.timed(f.st.ms_cvt, s, [&] { return launch_transpose64(f.c, const_cast<double *>(src), lds, img, ldimg, rows, cols, true); });
}

// Does the pivot kernel of a panel of `rows` rows fit BESIDE a running update?  It takes one workgroup -- one CU's whole LDS -- per
// HP_R rows, all resident at once: with (nearly) every CU needed, a small launch or an update workgroup on a few of them would hold
// all the others spinning until the update has drained (N = 65536 measured 3583 ms with the two lanes from the first panel on
// against 3336 without).
bool pivots_fit_beside_update(const mpf_ctx *c, int64_t rows) {
    return c->num_cus <= 0 || (rows + HP_R - 1) / HP_R <= (int64_t)c->num_cus * 4 / 5;
}

// The two column lanes' split of the columns [lo, hi): lane A = [lo, cm) gets option fp64_lane_a_pct of them, in whole 128-column
// tiles, lane B at least one tile.  A split (cm >= 0) stays until lane A's share has dropped by 10 points.  True at a (re-)split.
static bool lane_split(const mpf_ctx *c, int64_t lo, int64_t hi, int64_t &cm) {
    const int64_t cw = hi - lo;
    if (cm >= 0 && (cm - lo) * 100 >= cw * (c->tune.fp64_lane_a_pct - 10)) return false;
    cm = lo + ((cw * c->tune.fp64_lane_a_pct / 100 + 127) / 128) * 128;
    if (cm > hi - 128) cm = hi - 128;
    return true;
}

// buffers of factor_lookahead_rm: the N x N fp64 row-major copy, the interchange scratch (2 * HP_MAXCOLS rows x N) and the
// panel's row-major L21 (N x nb).  Returns non-zero (and leaves the context usable) when the device has no room: the caller
// then runs the in-place schedule.
int mpf_ensure_rowmajor_copy(mpf_ctx *c, int64_t N, int64_t cols, int32_t nb) {   // N rows x cols columns (mpf_factor_dist: the local columns)
    const bool bad = c->r64.grow(N * cols) || c->rm_tmp.grow((int64_t)LASWP_MAXMOVED * cols) ||
                     c->rm_lt.grow(3 * N * (int64_t)nb);   // two L21 images: panel k + 1's is written while update k still reads; the third: the replay on late column segments (LatePlan)
    if (bad) {   // no room: the in-place schedule runs, and nothing of this one stays resident
        (void)hipGetLastError();
        c->r64.release(); c->rm_tmp.release(); c->rm_lt.release();
        return 1;
    }
    return 0;
}

// Running state of factor_lookahead_rm's loop from one turn to the next.  The paired bulk phase leaves it as a two-lane turn would:
// the first panel the loop runs (k0; its chain is queued: chain_a), the last pair's lane updates on the main stream (doneL, doneR)
// and the lanes' split column -- the state of R at a pair boundary is the state the loop expects after a panel's update.
struct RmLoop {
    int64_t k0 = 0;                                      // first panel of the one-level loop
    hipEvent_t chain_a = nullptr, chain_b = nullptr;     // the chain of the CURRENT panel is complete (what the main stream waited for at the end of a one-lane turn)
    hipEvent_t doneL = nullptr, doneR = nullptr, prevR = nullptr;   // L(k - 1), R(k - 1), R(k - 2) on the main stream
    hipEvent_t init_done = nullptr;                      // the copy R is complete
    int64_t cm = -1;                                     // first column of lane B; -1: one lane
    bool was_two = false, sink = false;                  // the turn before ran two lanes (or was a pair); block rows leave as they become final (rowsink.hip)
    LatePlan *lp = nullptr; int lseg = 0;                // mpf_factor_host: columns from lp->c0[0] on are still on their way up; the next late segment
    int64_t ce = 0;                                      // first column that is not here yet
};
// One turn of the loop: the panel at k of pc columns, the next at nx of pc2, the trailing size n; ns: the columns updated before the
// side stream may start -- the strip, or everything when no panel follows; the panel's row-major L21 image and its moved-row list.
struct RmTurn {
    int64_t k, nx, n, ns; int pc, pc2; bool has_next; double *LT; const MovedList *lk;
    RmTurn(const FactorArgs &f, int64_t k_) : k(k_) {
        pc = (int)((f.N - k) < f.nb ? (f.N - k) : f.nb); nx = k + pc; n = f.N - nx;
        pc2 = (int)((f.N - nx) < f.nb ? (f.N - nx) : f.nb); has_next = (f.N - nx) > 1; ns = has_next ? pc2 : n;
        LT = f.c->rm_lt + ((k / f.nb) & 1) * f.N * (int64_t)f.nb; lk = f.c->lists + (k / f.nb);
    }
};

// Paired bulk phase of the row-major schedule (fp64 mode, while the update is the longer side): the panels run in pairs (k, k1 = k + nb),
// and everything right of the pair's INNER REGION [k1, k3 = k + 3 nb) is passed over ONCE per pair, by an update with K = 2 nb over
// [L(k) | L(k1)] and the 512 U rows, instead of once per panel -- per element the same chain c = fma(-a_kk, b_kk, c), kk ascending across
// the two panels (contract C5): identical bits.  The update kernel pays a fixed time per C tile per pass (load, store, hand-over:
// 65-67 TFLOP/s at K = 256 against 71 at K = 512 on these operands, profiles/pair_dgemm_probe.log), and a pair halves the passes.
//   inner region, panel by panel at full height with K = nb as in the one-level loop (helper stream T):
//     i1(k):  interchange k, TRSM, update on [k1, k2) -> chain k1 may start;  the same on [k2, k3);
//     i2(k1): interchange k1, TRSM, update on [k2, k3) -> chain k2 may start;
//   far columns, per column range (X = [k3, k5) that joins the next pair's inner region, lane A = [k5, cm), lane B = [cm, N)), after
//   chain k1 (helper stream T, under the other lane's update):
//     interchanges k AND k1 (both before any arithmetic on block row k1: a row of [k1, k2) that has received panel k's update must
//     not change places with one that has not);  U[k:k1] = L11(k)^-1 R[k:k1];  R[k1:k2] -= L(k)[k1:k2] U[k:k1] (K = nb, 256 rows);
//     U[k1:k2] = L11(k1)^-1 R[k1:k2];  both U block rows back to A;
//   main stream: nothing but  X(p) | A(p) | B(p) | X(p + 1) | ...  with K = 2 nb, rows k2 .. N.
// One row-major image per pair holds both panels' L21, rows k1 .. N, leading dimension 2 nb: L(k) goes in right behind chain k and
// serves the inner region as it is; the left-hand interchanges are deferred in this schedule, so after chain k1 its rows receive panel
// k1's interchange (contiguous rows of nb doubles) before the far columns use it, and L(k1) goes in beside it.  Two images alive: the
// next pair's is written while this pair's lane B still reads.
// The pivot kernels keep starting at a seam (the first of a pair at B(p - 1) | X(p), the second at A(p) | B(p)), as in the two-lane loop.
// Hand-over to the one-level loop: RmLoop (h.chain_a comes in as the chain of panel h.k0 = 0).
static int factor_rm_pairs(const FactorArgs &f, const RmView &v, RmLoop &h) {
    mpf_ctx *c = f.c; EvPool &ev = f.ev; hipStream_t S = c->stream, P = c->pstream, T = c->tstream;
    const int64_t N = f.N, nb = f.nb, ldp = 2 * nb;
    int rc = 0;
    hipEvent_t doneX = nullptr, &doneA = h.doneL, &doneB = h.doneR;   // the last X, A and B on the main stream: the loop's L and R
    int64_t &cm = h.cm, k = h.k0;
    // Lane B of a pair is launched one turn late, when the chain that starts at the seam in front of it (the next pair's second panel)
    // has been queued: the main stream waits for an event the pivot stream records right before its pivot kernel (`ps`), so the pivot
    // kernel is dispatched first.  Both wait for the same update to end, and a pivot kernel that comes second finds every CU taken
    // by update workgroups (it needs a CU's whole LDS): measured 2.6 ms instead of 0.7 per kernel of <= 20000 rows.
    struct { bool valid = false; int64_t k = 0, c_lo = 0, w = 0; const double *PI2 = nullptr; hipEvent_t ready = nullptr; } pendB;
    auto far_update = [&](int64_t kk, const double *pi2, int64_t c_lo, int64_t w) -> int {   // rows kk + 2 nb .. N, K = 2 nb
        const int64_t r0 = kk + 2 * nb;
        return rm_update(f, v, S, kk, (int)(2 * nb), r0, N - r0, c_lo, w, pi2, ldp);
    };
    auto flush_B = [&](hipEvent_t ps) -> int {
        if (!pendB.valid) return 0;
        hipStreamWaitEvent(S, pendB.ready, 0);
        if (ps) hipStreamWaitEvent(S, ps, 0);
        const int e = far_update(pendB.k, pendB.PI2, pendB.c_lo, pendB.w);
        doneB = ev.get();
        hipEventRecord(doneB, S);
        pendB.valid = false;
        return e;
    };
    for (; rc == 0; k += 2 * nb) {
        const int64_t k1 = k + nb, k2 = k1 + nb, k3 = k2 + nb, k5 = k3 + 2 * nb;
        // four full panels and two lanes of at least one tile right of them; the update the longer side; the pivot kernels fit
        // beside an update (factor_lookahead_rm's two-lane condition)
        if (k5 + 256 > N || (N - k1) <= c->tune.fp64_pair_min_n) break;
        if (!pivots_fit_beside_update(c, N - k1)) break;
        const bool resplit = lane_split(c, k5, N, cm);
        const double *Lk = v.a(k, k), *Lk1 = v.a(k1, k1);               // the two panels' L11
        // the pair's image as a view: row r of the MATRIX at img.r(r, .) (it holds the rows k1 .. N: its row 0 is virtual)
        const RmView img{nullptr, 0, c->rm_pair + ((k / (2 * nb)) & 1) * N * ldp - k1 * ldp, ldp};
        const double *PI = img.r(k1, 0), *PI2 = img.r(k2, 0);
        const MovedList *lk = c->lists + (k / nb), *lk1 = c->lists + (k1 / nb);
        hipEvent_t lt_ready = ev.get(), e1 = ev.get(), inner_done = ev.get(), chain1 = ev.get(), pi_ready = ev.get(), e2 = ev.get(),
                   chain2 = ev.get(), evX = ev.get(), evA = ev.get(), evB = ev.get(), ps1 = ev.get(), ps2 = ev.get();
        {   // L(k) into the pair's image, on the pivot stream right behind chain k; lane B of the pair before the last read this image
            // (the last lane B launched so far: the one of the pair before is still pending)
            if (doneB) hipStreamWaitEvent(P, doneB, 0);
            StreamSwap sw(c, P);
            rc = rm_l_image(f, P, v.a(k1, k), v.lda, N - k1, nb, img.r(k1, 0), ldp);
            hipEventRecord(lt_ready, P);
        }
        if (rc) break;
        {   // ---- i1(k): panel k on the inner region [k1, k3), the strip [k1, k2) first ------------------------------------------
            hipStreamWaitEvent(T, h.chain_a, 0);
            hipStreamWaitEvent(T, doneX ? doneX : h.init_done, 0);
            StreamSwap sw(c, T);
            rc = rm_swap(f, v, T, k1, k3 - k1, {lk}, (int64_t)LASWP_MAXMOVED * k1);
            if (!rc) rc = rm_solve_u(f, v, T, Lk, v.lda, k, (int)nb, k1, nb);
            hipStreamWaitEvent(T, lt_ready, 0);
            if (!rc) rc = rm_update(f, v, T, k, (int)nb, k1, N - k1, k1, nb, PI, ldp);
            if (!rc) rc = rm_home(f, v, T, k1, N - k1, k1, nb);
            hipEventRecord(e1, T);
            if (!rc) rc = rm_solve_u(f, v, T, Lk, v.lda, k, (int)nb, k2, nb);
            if (!rc) rc = rm_update(f, v, T, k, (int)nb, k1, N - k1, k2, nb, PI, ldp);
            if (!rc) rc = rm_home(f, v, T, k, nb, k1, k3 - k1);
            hipEventRecord(inner_done, T);
        }
        if (rc) break;
        {   // ---- chain k1 on P, from the seam A(p - 1) | B(p - 1); then the image: panel k1's interchange on L(k), L(k1) beside it ----
            hipStreamWaitEvent(P, e1, 0);
            if (doneA) hipStreamWaitEvent(P, doneA, 0);
            hipEventRecord(ps1, P);
            rc = panel_chain(f, k1, P);
            hipEventRecord(chain1, P);
            StreamSwap sw(c, P);
            hipStreamWaitEvent(P, inner_done, 0);   // the inner region has read L(k) in panel k's row order
            // (the list holds matrix rows, all of them >= k1: the base is the image's virtual row 0; the scratch of the columns [0, nb) is
            //  free -- every interchange on R in this phase uses the scratch of its own columns, all right of k1)
            if (!rc) rc = rm_swap(f, img, P, 0, nb, {lk1}, 0);
            if (!rc) rc = rm_l_image(f, P, v.a(k2, k1), v.lda, N - k2, nb, img.r(k2, nb), ldp);
            hipEventRecord(pi_ready, P);
        }
        if (!rc) rc = flush_B(ps1);   // B(p - 1), behind chain k1's pivot kernel
        if (rc) break;
        {   // ---- i2(k1): panel k1 on [k2, k3) -------------------------------------------------------------------------------------
            hipStreamWaitEvent(T, chain1, 0);
            StreamSwap sw(c, T);
            rc = rm_swap(f, v, T, k2, nb, {lk1}, (int64_t)LASWP_MAXMOVED * k2);
            if (!rc) rc = rm_solve_u(f, v, T, Lk1, v.lda, k1, (int)nb, k2, nb);
            hipStreamWaitEvent(T, pi_ready, 0);
            if (!rc) rc = rm_update(f, v, T, k1, (int)nb, k2, N - k2, k2, nb, img.r(k2, nb), ldp);
            if (!rc) rc = rm_home(f, v, T, k2, N - k2, k2, nb);
            hipEventRecord(e2, T);
            if (!rc) rc = rm_home(f, v, T, k1, nb, k2, nb);
        }
        if (rc) break;
        {   // ---- chain k2 on P, from the seam B(p - 1) | X(p) --------------------------------------------------------------------------
            hipStreamWaitEvent(P, e2, 0);
            if (doneB) hipStreamWaitEvent(P, doneB, 0);
            hipEventRecord(ps2, P);
            rc = panel_chain(f, k2, P);
            hipEventRecord(chain2, P);
        }
        if (rc) break;
        // the small launches of the far columns [c_lo, c_lo + w) on T (behind chain k1 and the image: i2 has waited for both)
        auto far_prep = [&](int64_t c_lo, int64_t w) -> int {
            int e = rm_swap(f, v, T, c_lo, w, {lk, lk1}, (int64_t)LASWP_MAXMOVED * c_lo);
            if (!e) e = rm_solve_u(f, v, T, Lk, v.lda, k, (int)nb, c_lo, w);
            if (!e) e = rm_update(f, v, T, k, (int)nb, k1, nb, c_lo, w, PI, ldp);
            if (!e) e = rm_solve_u(f, v, T, Lk1, v.lda, k1, (int)nb, c_lo, w);
            if (!e) e = rm_home(f, v, T, k, 2 * nb, c_lo, w);
            return e;
        };
        {   // ---- X and lane A: their columns were in lane A of the pair before (at a re-split: in either lane) -----------------------
            if (doneA) hipStreamWaitEvent(T, doneA, 0); else hipStreamWaitEvent(T, h.init_done, 0);
            if (resplit && doneB) hipStreamWaitEvent(T, doneB, 0);
            StreamSwap sw(c, T);
            rc = far_prep(k3, k5 - k3);
            hipEventRecord(evX, T);
            if (!rc) rc = far_prep(k5, cm - k5);
            hipEventRecord(evA, T);
        }
        if (rc) break;
        hipStreamWaitEvent(S, evX, 0);
        hipStreamWaitEvent(S, ps2, 0);   // X(p) behind chain k2's pivot kernel
        rc = far_update(k, PI2, k3, k5 - k3);
        if (rc) break;
        doneX = ev.get();
        hipEventRecord(doneX, S);
        hipStreamWaitEvent(S, evA, 0);
        rc = far_update(k, PI2, k5, cm - k5);
        if (rc) break;
        doneA = ev.get();
        hipEventRecord(doneA, S);
        {   // ---- lane B (behind B(p - 1)), under A(p) -----------------------------------------------------------------------------
            if (doneB) hipStreamWaitEvent(T, doneB, 0);
            StreamSwap sw(c, T);
            rc = far_prep(cm, N - cm);
            hipEventRecord(evB, T);
        }
        if (rc) break;
        pendB.valid = true; pendB.k = k; pendB.PI2 = PI2; pendB.c_lo = cm; pendB.w = N - cm; pendB.ready = evB;
        h.chain_a = chain2;
        if (f.o.verbose) printf("panels k=%lld, %lld rows=%lld (row-major copy, paired: far update K = %d, lanes split at %lld)\n", (long long)k1, (long long)k2, (long long)(N - k1), (int)(2 * nb), (long long)cm);
    }
    if (!rc) rc = flush_B(nullptr);
    h.k0 = k; h.was_two = k > 0;   // (a pair ran: the lanes' last launches are in flight, as after a two-lane turn of the loop)
    return rc;
}

// A late column segment is due: it receives the panels [0, k / nb) one after the other on the main stream (behind the updates queued
// there), then the loop goes on with the wider matrix.
static int rm_replay_late(const FactorArgs &f, const RmView &v, RmLoop &L, const RmTurn &t) {
    mpf_ctx *c = f.c; EvPool &ev = f.ev; hipStream_t S = c->stream;
    const int64_t N = f.N, nb = f.nb;
    LatePlan *lp = L.lp;
    int rc = 0;
    while (lp && L.lseg < lp->nseg && (t.k / nb >= lp->q[L.lseg] || t.nx + t.pc2 > L.ce || !t.has_next)) {
        const int lseg = L.lseg;
        const int64_t c_lo = lp->c0[lseg], c_hi = lseg + 1 < lp->nseg ? lp->c0[lseg + 1] : N, w = c_hi - c_lo;
        double *LT3 = c->rm_lt + 2 * N * nb;
        rc = launch_late_wait(c, lp->flags + lseg, lp->seq);
        if (!rc && lp->snapshot) {
            MPF_HIP_TRY(c, hipMemcpyAsync(lp->snapshot + c_lo * N, v.a(0, c_lo), (size_t)w * N * sizeof(double), hipMemcpyDeviceToDevice, S));
            lp->snapped[lseg] = true;
        }
        if (!rc) rc = rm_l_image(f, S, v.a(0, c_lo), v.lda, N, w, v.r(0, c_lo), v.ldr);
        // The replay, panel by panel, on the main stream.  (With the segment in two halves -- the main stream carrying only the updates, each
        // half's small launches on the helper stream under the other half's update, as in the two-lane loop below -- the call took the
        // same time within the boxes' spread: what the replay phases cost is not their small launches but the chain-bound panels in
        // front of them)
        for (int64_t kj = 0; kj < t.k && rc == 0; kj += nb) {
            const int64_t nxj = kj + nb, nj = N - nxj;
            rc = rm_l_image(f, S, v.a(nxj, kj), v.lda, nj, nb, LT3, nb);
            if (!rc) rc = rm_swap(f, v, S, c_lo, w, {c->lists + (kj / nb)}, (int64_t)LASWP_MAXMOVED * c_lo);
            if (!rc) rc = rm_solve_u(f, v, S, v.a(kj, kj), v.lda, kj, (int)nb, c_lo, w);
            if (!rc) rc = rm_home(f, v, S, kj, nb, c_lo, w);
            if (!rc) rc = rm_update(f, v, S, kj, (int)nb, nxj, nj, c_lo, w, LT3, nb);
            if (L.sink && !rc && c_hi == N) sink_notify(c, (int)(kj / nb) + 1, S);   // block row kj is complete now
        }
        ++L.lseg;
        L.ce = L.lseg < lp->nseg ? lp->c0[L.lseg] : N;
        L.cm = -1;                         // the lanes are cut anew, and lane A's small launches wait for everything queued here
        L.doneR = ev.get();
        hipEventRecord(L.doneR, S);
        L.doneL = nullptr;
    }
    return rc;
}

// Two column lanes while the update is the longer side (trailing size > chain_pipeline_below: the chain is not pipelined there and
// the helper stream T is free).  The columns right of the strip are split at `cm`: lane A = [nx, cm), lane B = [cm, N).  The main
// stream then carries NOTHING BUT the two big updates, L(k), R(k), L(k + 1), ... back to back; every small launch -- a lane's
// interchange, its TRSM, its U write-back, lane A's strip step that releases the next chain -- runs on the high-priority helper
// stream T UNDER the other lane's update instead of between two updates:
//     T:  a(k) | b(k) | a(k + 1) | ...     a(k) = lane A's small launches of panel k (needs L(k - 1) and chain k), b(k) = lane B's (needs R(k - 1))
//     S:  ... R(k - 1) | wait a(k): L(k) | wait b(k): R(k) | ...
// so a(k) runs under R(k - 1) and b(k) under L(k).  Per element nothing changes (each column still gets interchange, TRSM,
// update, in this order): identical bits.  The split point only moves at a re-split (lane A's small launches then wait for
// R(k - 1) too), because a column that changes lanes must have finished its update on the old one.
static int rm_turn_two_lanes(const FactorArgs &f, const RmView &v, RmLoop &L, const RmTurn &t, bool resplit) {
    mpf_ctx *c = f.c; EvPool &ev = f.ev; hipStream_t S = c->stream, P = c->pstream, T = c->tstream;
    const int64_t N = f.N, k = t.k, nx = t.nx, n = t.n, cm = L.cm, ce = L.ce; const int pc = t.pc, pc2 = t.pc2;
    const double *L11 = v.a(k, k);
    const int64_t aw = cm - (nx + pc2);
    int rc = 0;
    if (!L.was_two && k > 0) {   // coming from one lane (the first pivot kernels needed every CU): everything the main stream holds
        L.doneL = ev.get();      // -- the whole update of the panel before -- is what lane A's small launches wait for
        hipEventRecord(L.doneL, S);
    }
    hipEvent_t lt_ready = ev.get();
    {   // L21 row-major, on the pivot stream right behind chain k (P ran it); this image was last read by L / R(k - 2)
        if (L.prevR) hipStreamWaitEvent(P, L.prevR, 0);
        StreamSwap sw(c, P);
        rc = rm_l_image(f, P, v.a(nx, k), v.lda, n, pc, t.LT, pc);
        hipEventRecord(lt_ready, P);
    }
    if (rc) return rc;
    hipEvent_t e1 = ev.get(), e2 = ev.get(), evA = ev.get(), evB = ev.get();
    {   // ---- a(k): lane A's interchange, the strip step, E1, lane A's TRSM and U write-back ---------------------------------
        if (L.chain_a) hipStreamWaitEvent(T, L.chain_a, 0);
        if (L.chain_b) hipStreamWaitEvent(T, L.chain_b, 0);
        if (L.doneL) hipStreamWaitEvent(T, L.doneL, 0); else hipStreamWaitEvent(T, L.init_done, 0);
        if (resplit && L.doneR) hipStreamWaitEvent(T, L.doneR, 0);
        StreamSwap sw(c, T);
        rc = rm_swap(f, v, T, nx, cm - nx, {t.lk}, 0);
        if (!rc) rc = rm_solve_u(f, v, T, L11, v.lda, k, pc, nx, t.ns);
        hipStreamWaitEvent(T, lt_ready, 0);
        if (!rc) rc = rm_update(f, v, T, k, pc, nx, n, nx, t.ns, t.LT, pc);
        // the next panel's columns return to the column-major matrix: rows nx.. (its U rows k..nx follow with lane A's below)
        if (!rc) rc = rm_home(f, v, T, nx, N - nx, nx, pc2);
        hipEventRecord(e1, T);
    }
    if (rc) return rc;
    {   // ---- chain of panel k + 1 on P --------------------------------------------------------------------------------------
        // E1 comes in the middle of R(k - 1).  A pivot kernel launched THERE would trickle onto the chip -- a workgroup needs a
        // whole CU's LDS, a CU only empties when the update's queue does -- and the workgroups that got in early would hold
        // their CUs spinning for milliseconds (measured: 3.5 instead of 1.1 ms per kernel, the update 17 % slower).  It starts
        // at the seam between R(k - 1) and L(k) instead: the chip is empty, the high-priority kernel takes its CUs first.
        hipStreamWaitEvent(P, e1, 0);
        if (L.doneR) hipStreamWaitEvent(P, L.doneR, 0);
        rc = panel_chain(f, nx, P);
        hipEventRecord(e2, P);
    }
    if (rc) return rc;
    {
        StreamSwap sw(c, T);
        rc = rm_solve_u(f, v, T, L11, v.lda, k, pc, nx + pc2, aw);
        if (!rc) rc = rm_home(f, v, T, k, pc, nx, cm - nx);
        hipEventRecord(evA, T);
        // ---- b(k): lane B's interchange, TRSM, U write-back (behind R(k - 1)) ----------------------------------------------
        if (L.doneR) hipStreamWaitEvent(T, L.doneR, 0);
        if (!rc) rc = rm_swap(f, v, T, cm, ce - cm, {t.lk}, (int64_t)LASWP_MAXMOVED * (cm - nx));
        if (!rc) rc = rm_solve_u(f, v, T, L11, v.lda, k, pc, cm, ce - cm);
        if (!rc) rc = rm_home(f, v, T, k, pc, cm, ce - cm);
        hipEventRecord(evB, T);
        if (L.sink && !rc && ce == N) sink_notify(c, (int)(k / f.nb) + 1, T);   // block row k is complete in the column-major matrix
    }
    if (rc) return rc;
    // ---- main stream: the two updates ----------------------------------------------------------------------------------------
    hipStreamWaitEvent(S, evA, 0);
    rc = rm_update(f, v, S, k, pc, nx, n, nx + pc2, aw, t.LT, pc);
    if (rc) return rc;
    L.doneL = ev.get();
    hipEventRecord(L.doneL, S);
    hipStreamWaitEvent(S, evB, 0);
    rc = rm_update(f, v, S, k, pc, nx, n, cm, ce - cm, t.LT, pc);
    if (rc) return rc;
    L.prevR = L.doneR;
    L.doneR = ev.get();
    hipEventRecord(L.doneR, S);
    L.chain_a = e2; L.chain_b = nullptr;
    L.was_two = true;
    if (f.o.verbose) printf("panel k=%lld rows=%lld cols=%d (look-ahead, row-major copy, two lanes split at %lld)\n", (long long)nx, (long long)(N - nx), pc2, (long long)cm);
    return 0;
}

// One lane: the main stream carries the whole step of panel k; the chain of panel k + 1 runs beside the rest of the update.
static int rm_turn_one_lane(const FactorArgs &f, const RmView &v, RmLoop &L, const RmTurn &t) {
    mpf_ctx *c = f.c; EvPool &ev = f.ev; hipStream_t S = c->stream, P = c->pstream, T = c->tstream;
    const int64_t N = f.N, k = t.k, nx = t.nx, n = t.n, ce = L.ce; const int pc = t.pc, pc2 = t.pc2;
    const double *L11 = v.a(k, k);
    const int64_t cw = ce - nx - pc2;      // columns right of the strip (that are here)
    int rc = 0;
    if (L.was_two) {   // the lanes' last small launches and the chain of this panel (the main stream did not wait for either)
        stream_join(ev, T, S);
        if (L.chain_a) hipStreamWaitEvent(S, L.chain_a, 0);
        if (L.chain_b) hipStreamWaitEvent(S, L.chain_b, 0);
        L.was_two = false;
    }
    // ---- L21 row-major; interchanges of panel k on everything right of it (contiguous rows) ---------------------------------
    // (the transposition runs on the pivot stream, idle between two pivot kernels, beside the interchange and the strip's TRSM)
    hipEvent_t lt_ready = ev.get();
    {
        stream_join(ev, S, P);                 // chain k is complete (S has waited for it); the update before the last has read this LT image
        StreamSwap sw(c, P);
        rc = rm_l_image(f, P, v.a(nx, k), v.lda, n, pc, t.LT, pc);
        hipEventRecord(lt_ready, P);
    }
    if (!rc) rc = rm_swap(f, v, S, nx, ce - nx, {t.lk}, 0);
    // ---- strip (or everything, when no panel follows) --------------------------------------------------------------------
    if (!rc) rc = rm_solve_u(f, v, S, L11, v.lda, k, pc, nx, t.ns);
    hipStreamWaitEvent(S, lt_ready, 0);
    if (!rc) rc = rm_update(f, v, S, k, pc, nx, n, nx, t.ns, t.LT, pc);
    if (rc) return rc;
    if (!t.has_next)   // the last rows of U and the last block go home (two launches in one region)
        return rm_home(f, v, S, k, N - k, nx, N - nx, pc);
    // the next panel's columns return to the column-major matrix: rows nx.. (its U rows k..nx follow with the others below)
    rc = rm_home(f, v, S, nx, N - nx, nx, pc2);
    if (rc) return rc;
    hipEvent_t e1 = ev.get();
    hipEventRecord(e1, S);
    // ---- side streams: the whole chain of panel k+1 ---------------------------------------------------------------------
    const ChainEnd next = chain_behind(f, nx, e1);
    rc = next.rc;
    if (rc) return rc;
    // ---- main stream: the rest of update k; the finished U rows of panel k go back to A -------------------------------------
    if (cw > 0) rc = rm_solve_u(f, v, S, L11, v.lda, k, pc, nx + pc2, cw);
    if (rc) return rc;
    // (the write-back of the finished U rows runs on the chain's second stream, behind the chain's own launches: nothing
    //  waits for it before the end of the factorization, and the main stream goes straight on to the update)
    hipStream_t H = T ? T : S;
    {
        if (T) stream_join(ev, S, T);
        StreamSwap sw(c, H);
        rc = rm_home(f, v, H, k, pc, nx, ce - nx);
        if (L.sink && !rc && ce == N) sink_notify(c, (int)(k / f.nb) + 1, H);
    }
    if (!rc && cw > 0) rc = rm_update(f, v, S, k, pc, nx, n, nx + pc2, cw, t.LT, pc);
    if (rc) return rc;
    L.chain_a = next.a; L.chain_b = next.b;
    hipStreamWaitEvent(S, L.chain_a, 0);
    if (L.chain_b) hipStreamWaitEvent(S, L.chain_b, 0);
    if (f.o.verbose) printf("panel k=%lld rows=%lld cols=%d (look-ahead, row-major copy)\n", (long long)nx, (long long)(N - nx), pc2);
    return 0;
}

// Look-ahead schedule of the fp64 mode on a ROW-MAJOR working copy of the trailing matrix (round 3; default for N >= 8192).
// In the column-major matrix an interchange costs a 64-byte HBM sector each way for every moved row of every column right of
// the panel (~36 KB per column per panel, 39 ms of a factorization at N = 32768); the element (i, j) of the copy R lives at
// R[i * N + j], so an interchange moves contiguous row segments (two passes through a scratch image, laswp.hip).  Everything
// right of the current panel lives in R; the panels themselves (pivot kernel, fp64 panel) stay in the caller's column-major
// matrix A, which is also where the results end up:
//   per panel k:  L21 -> row-major scratch LT;  interchange on R (all columns right of the panel);
//                 U12 = L11^-1 R[k.., :]  (same TRSM kernel, addresses through strides);  U rows back to A;
//                 R[nx.., :] -= U12^T-form update: the SAME MFMA GEMM kernel run on the transposed problem
//                     C'(j, i) = R[(nx + i) N + nx + j],  A'(j, kk) = U(kk, j) = R[(k + kk) N + nx + j],  B'(kk, i) = L(i, kk) = LT[i * nb + kk]
//                 (per element the chain c = fma(-u, l, c), kk ascending: the product of the same two numbers as fma(-l, u, c));
//                 the next panel's columns go back to A (transpose) before its chain starts.
// Per element the operations and their order are those of factor_lookahead: bit-identical results (tests).
// pairs: the panels run through factor_rm_pairs while its conditions hold, this loop takes over at a pair boundary.
int factor_lookahead_rm(mpf_ctx *c, double *d_A, int64_t lda, int64_t N, int32_t nb, int32_t *d_ipiv, const mpf_opts &o, mpf_stats &st, bool pairs) {
    hipStream_t S = c->stream, P = c->pstream, T = c->tstream;
    EvPool ev(c);
    ev.keep = &st.ms_gemm;
    const FactorArgs f{c, ev, st, o, d_A, lda, N, nb, d_ipiv};
    const RmView v{d_A, lda, c->r64, N};
    int rc = 0;
    RmLoop L;
    L.sink = sink_take(c, d_A, lda, N, nb);   // (mpf_factor_host: block rows leave as they become final, rowsink.hip)
    // mpf_factor_host with a LatePlan: columns from lp->c0[0] on are still on their way up.  `ce` = first column that is not here yet.
    L.lp = (c->late && !c->late->taken && c->late->nseg > 0 && lda == N) ? c->late : nullptr;
    if (L.lp) L.lp->taken = true;
    L.ce = L.lp ? L.lp->c0[0] : N;
    { hipEvent_t e = ev.get(); hipEventRecord(e, S); hipStreamWaitEvent(P, e, 0); if (T) hipStreamWaitEvent(T, e, 0); }
    const int pc0 = (int)(N < nb ? N : nb);
    if (N > 1) {
        // panel 0 (on the side stream) beside the transposition of everything right of it
        hipEvent_t e0 = ev.get();
        {
            StreamSwap sw(c, P);
            rc = ev.timed(st.ms_hpanel, P, [&] {
                int e = launch_hgetf2(c, d_A, lda, nullptr, 0, (int)N, pc0, 0, d_ipiv, nullptr, 0, c->lists, 0, pref_window_rows(o));
                if (!e) e = launch_laswp_from_list(c, d_A, lda, pc0, c->lists);
                if (!e) e = launch_dgetf2_npv(c, d_A, lda, (int)N, pc0, o.fused_panel, 0);
                return e; });
            hipEventRecord(e0, P);
        }
        st.panels++;
        if (!rc && pc0 < L.ce) rc = rm_l_image(f, S, v.a(0, pc0), lda, N, L.ce - pc0, v.r(0, pc0), v.ldr);
        hipStreamWaitEvent(S, e0, 0);
        L.chain_a = e0;
    }
    L.init_done = ev.get();
    hipEventRecord(L.init_done, S);    // the copy R is complete
    if (pairs && !rc && !L.sink && !L.lp && T && N > 1) rc = factor_rm_pairs(f, v, L);
    for (int64_t k = L.k0; k < N && rc == 0; k += nb) {
        const RmTurn t(f, k);
        if (N - k <= 1 || t.nx >= N) break;
        rc = rm_replay_late(f, v, L, t);
        if (rc) break;
        const int64_t cw = L.ce - t.nx - t.pc2;      // columns right of the strip (that are here)
        const bool want_two = T && c->tune.fp64_two_lanes > 0 && t.has_next && pivots_fit_beside_update(c, N - t.nx) &&
                              (N - t.nx) > c->tune.chain_pipeline_below && cw >= c->tune.fp64_two_lanes;
        if (!want_two) L.cm = -1;
        const bool resplit = want_two && lane_split(c, t.nx + t.pc2, L.ce, L.cm);
        if (L.cm >= 0) rc = rm_turn_two_lanes(f, v, L, t, resplit);
        else {
            rc = rm_turn_one_lane(f, v, L, t);
            if (!t.has_next) break;
        }
    }
    if (!rc && L.lp && L.lseg < L.lp->nseg) rc = fail(c, -1, "factor_lookahead_rm: a late column segment was never brought up to date (plan beyond the matrix)");
    if (T) stream_join(ev, T, S);   // the last U write-backs / lane B
    stream_join(ev, P, S);
    return factor_epilogue(f, rc, L.sink, 1, true);
}
