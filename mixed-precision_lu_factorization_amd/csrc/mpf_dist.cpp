// Multi-GPU MPF behind the C ABI: 1-D block-cyclic column layout, one process per GPU, ONE broadcast per panel.
//
// The reference is single-device (MPF.cu:77); this partition is the build's extension (BASELINE north_star
// "1-D block-column layout and RCCL broadcast of the factored panel over xGMI").  A column block of nb columns lives
// entirely on one rank (global block b on rank b % world, local index b / world), so the fp16 pivot panel, its pivot
// search and the fp64 no-pivot panel are local to the owner -- there is no cross-GPU argmax.  Per panel the only exchange
// is one broadcast owner -> all of {factored panel (rows k..N x nb, fp64), nb pivots (int32), the panel's moved-row list};
// every rank then interchanges / TRSMs / GEMMs the columns it owns.  Per element the arithmetic is that of the 1-GPU path
// (the partition only changes WHO computes a column block): IPIV and LU are bit-identical to mpf_factor_dev.
//
// Schedule = the look-ahead schedule of mpf_factor.cpp with column indices translated: the owner of panel b+1 updates that
// block first ("strip"), runs its chain and posts the broadcast on the side stream P while every rank finishes update b on
// the main stream S.  Columns LEFT of a panel are interchanged once at the end (composite maps, laswp.hip).
//
// The broadcast is a callback (mpf_dist.bcast) so that any transport can carry it; the built-in one is RCCL
// (mpf_rccl_init: ncclBroadcast / ncclAllReduce on the context's communicator, resolved with dlopen so that single-GPU
// users never load RCCL).  Tests drive the same loop through a gloo-backed callback with several ranks on one GPU.
#include "solve_common.h"
#include "factor_common.h"
#include <dlfcn.h>
#include <climits>
#include <cstdio>
#include <cstring>
#include <cmath>
#include <algorithm>

// ---------------------------------------------------------------------------------------------------------------------
// RCCL through dlopen
// ---------------------------------------------------------------------------------------------------------------------
namespace {
struct NcclId { char internal[128]; };
struct Rccl {
    void *h = nullptr;
    int (*GetUniqueId)(NcclId *) = nullptr;
    int (*CommInitRank)(void **, int, NcclId, int) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*Broadcast)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*Send)(const void *, size_t, int, int, void *, hipStream_t) = nullptr;   // optional: the chain of the distributed triangular solves
    int (*Recv)(void *, size_t, int, int, void *, hipStream_t) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    int (*GetVersion)(int *) = nullptr;
    int (*CommCount)(void *, int *) = nullptr;       // optional (the bench line's record that RCCL saw N ranks)
    int (*CommUserRank)(void *, int *) = nullptr;
};
Rccl *rccl_load(std::string &err) {
    static Rccl r;
    static bool tried = false;
    if (r.h) return &r;
    if (tried) { err = "librccl not loadable"; return nullptr; }
    tried = true;
    const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char *n : names) { r.h = dlopen(n, RTLD_NOW | RTLD_NOLOAD); if (r.h) break; } // the copy torch already loaded, if any
    if (!r.h) for (const char *n : names) { r.h = dlopen(n, RTLD_NOW | RTLD_GLOBAL); if (r.h) break; }
    if (!r.h) { err = std::string("dlopen(librccl) failed: ") + dlerror(); return nullptr; }
#define RSYM(field, name) r.field = (decltype(r.field))dlsym(r.h, name); if (!r.field) { err = std::string("librccl lacks ") + name; r.h = nullptr; return nullptr; }
    RSYM(GetUniqueId, "ncclGetUniqueId") RSYM(CommInitRank, "ncclCommInitRank") RSYM(CommDestroy, "ncclCommDestroy")
    RSYM(Broadcast, "ncclBroadcast") RSYM(AllReduce, "ncclAllReduce") RSYM(GetErrorString, "ncclGetErrorString")
    RSYM(GetVersion, "ncclGetVersion")
#undef RSYM
    r.Send = (decltype(r.Send))dlsym(r.h, "ncclSend");
    r.Recv = (decltype(r.Recv))dlsym(r.h, "ncclRecv");
    r.CommCount = (decltype(r.CommCount))dlsym(r.h, "ncclCommCount");
    r.CommUserRank = (decltype(r.CommUserRank))dlsym(r.h, "ncclCommUserRank");
    return &r;
}
constexpr int NCCL_CHAR = 0, NCCL_DOUBLE = 8, NCCL_SUM = 0;

int rccl_bcast(void *user, void *d_buf, int64_t bytes, int32_t root, void *stream) {
    mpf_ctx *c = (mpf_ctx *)user;
    std::string err;
    Rccl *r = rccl_load(err);
    if (!r || !c->rccl_comm) { c->err = "RCCL communicator not initialised (mpf_rccl_init)"; return -5; }
    const int rc = r->Broadcast(d_buf, d_buf, (size_t)bytes, NCCL_CHAR, root, c->rccl_comm, (hipStream_t)stream);
    if (rc != 0) { c->err = std::string("ncclBroadcast: ") + r->GetErrorString(rc); return -5; }
    c->rccl_bcast_calls++; c->rccl_bcast_bytes += bytes;
    return 0;
}
int rccl_allreduce(void *user, double *d_buf, int64_t count, void *stream) {
    mpf_ctx *c = (mpf_ctx *)user;
    std::string err;
    Rccl *r = rccl_load(err);
    if (!r || !c->rccl_comm) { c->err = "RCCL communicator not initialised (mpf_rccl_init)"; return -5; }
    const int rc = r->AllReduce(d_buf, d_buf, (size_t)count, NCCL_DOUBLE, NCCL_SUM, c->rccl_comm, (hipStream_t)stream);
    if (rc != 0) { c->err = std::string("ncclAllReduce: ") + r->GetErrorString(rc); return -5; }
    c->rccl_allreduce_calls++;
    return 0;
}

int rccl_p2p(void *user, void *d_buf, int64_t bytes, int32_t peer, int32_t send, void *stream) {
    mpf_ctx *c = (mpf_ctx *)user;
    std::string err;
    Rccl *r = rccl_load(err);
    if (!r || !c->rccl_comm || !r->Send || !r->Recv) { c->err = "RCCL point-to-point not available"; return -5; }
    const int rc = send ? r->Send(d_buf, (size_t)bytes, NCCL_CHAR, peer, c->rccl_comm, (hipStream_t)stream)
                        : r->Recv(d_buf, (size_t)bytes, NCCL_CHAR, peer, c->rccl_comm, (hipStream_t)stream);
    if (rc != 0) { c->err = std::string(send ? "ncclSend: " : "ncclRecv: ") + r->GetErrorString(rc); return -5; }
    c->rccl_p2p_calls++; c->rccl_p2p_bytes += bytes;
    return 0;
}
bool rccl_has_p2p() { std::string err; Rccl *r = rccl_load(err); return r && r->Send && r->Recv; }

// ---- layout ----------------------------------------------------------------------------------------------------------
struct Layout {
    int64_t N; int nb, rank, world, nblocks;
    Layout(int64_t N_, int nb_, int rank_, int world_) : N(N_), nb(nb_), rank(rank_), world(world_), nblocks((int)((N_ + nb_ - 1) / nb_)) {}
    int owner(int b) const { return b % world; }
    bool mine(int b) const { return b % world == rank; }
    int width(int b) const { const int64_t w = N - (int64_t)b * nb; return (int)(w < nb ? w : nb); }
    int64_t lcol(int b) const { return (int64_t)(b / world) * nb; }           // first local column of (owned) block b
    int64_t local_cols() const { int64_t s = 0; for (int b = rank; b < nblocks; b += world) s += width(b); return s; }
    int64_t first_local_col_after(int b) const {                                // local columns whose global block is > b
        const int64_t cnt = b < rank ? 0 : (int64_t)(b - rank) / world + 1;
        const int64_t c0 = cnt * nb, lc = local_cols();
        return c0 < lc ? c0 : lc;
    }
    bool live(int b) const { return b < nblocks && N - (int64_t)b * nb > 1; }
};
// Panel message: the factored panel (rows k..N) with leading dimension ldp = rows + PANEL_PAD -- the padding at the bottom of
// column 32 q holds the 32 pivots (int32, global, 1-based) of sub-panel q, so a 32-column instalment of the message is ONE
// contiguous range that carries its own pivots -- then the panel's moved-row list.
constexpr int PANEL_PAD = 16;   // doubles = 128 bytes = 32 int32 pivots
size_t panel_buf_bytes(int64_t N, int nb) { return (size_t)(N + PANEL_PAD) * nb * 8 + sizeof(MovedList); }

int ensure_dist_bufs(mpf_ctx *c, int64_t N, int nb) {
    static_assert(sizeof(MovedList) % sizeof(double) == 0, "a panel message is a whole number of doubles");
    const int64_t need = (int64_t)(panel_buf_bytes(N, nb) / sizeof(double));
    for (auto &b : c->dist_buf) MPF_HIP_TRY(c, b.grow(need));
    return 0;
}

// ---- factorization: one call's state and steps -----------------------------------------------------------------------------
// The steps are the single-GPU schedules' (factor_common.h) on views of this rank's storage: a panel's columns in the local matrix,
// its L in the panel message; the far columns in the local matrix and an fp32 working copy, their super-panel's L in a store.
struct DistFactor {
    mpf_ctx *c; const mpf_opts &o; const Layout L;
    double *A; const int64_t lda, N; const int nb; int32_t *ipiv;   // the local matrix, the global order
    mpf_bcast_fn bcast_fn; void *user;
    const int64_t lcols;
    const bool f64, split, generic;   // generic: pivot_path = 1 / safe_pivots, as mpf_factor_dev (GPUs shared with other processes)
    mpf_stats st{}; EvPool ev; const FactorArgs f;
    hipStream_t S, P, X;              // main; the next panel's chain; the exchange of a message in instalments
    bool two = false, rm = false;
    int sb = 1, far_img = 1;          // panels per super-panel (1: one-level schedule); which L image the next K = sb * nb update reads
    bool inst_ok = false, fused_form_all = false; long long inst_min_bytes = 0, lds_rows_max = 0;   // agreed by the ranks (agree)
    RmView rv{};                                           // the local columns and their row-major copy (fp64 mode, rm)
    double *SPL = nullptr;                                 // the super-panel's panels, ld N
    float *W = nullptr;                                    // fp32 row-major working copy of the local far columns
    int64_t ldw = 1; ImageGeom g{};
    bool image_ready = false;         // the current panel's L21 image (fp16 modes) / row-major L21 (rm) is there
    std::vector<hipEvent_t> ev_piece;

    DistFactor(mpf_ctx *c_, const mpf_opts &o_, const mpf_dist *d, double *A_, int64_t lda_, int64_t N_, int nb_, int32_t *ipiv_)
        : c(c_), o(o_), L(N_, nb_, d->rank, d->world), A(A_), lda(lda_), N(N_), nb(nb_), ipiv(ipiv_), bcast_fn(d->bcast ? d->bcast : rccl_bcast),
          user(d->bcast ? d->user : (void *)c_), lcols(L.local_cols()), f64(o_.trailing == MPF_TRAIL_FP64), split(o_.trailing == MPF_TRAIL_FP16X3),
          generic(o_.pivot_path == 1 || safe_pivots(c_)), ev(c_), f{c_, ev, st, o_, A_, lda_, N_, nb_, ipiv_}, S(c_->stream), P(c_->stream), X(c_->stream) {
        ev.keep = &st.ms_gemm; st.n = N; st.nb = nb; st.superpanel = 1;
        st.fp16_fused = c->tune.fp16_fused != 0;   // (every rank's own option: the ranks must agree on it, include/mpf_c.h)
    }
    int bcast(void *buf, size_t bytes, int root, hipStream_t s) {
        if (L.world == 1) return 0;
        const int e = bcast_fn(user, buf, (int64_t)bytes, root, (void *)s);
        return e ? (e < 0 ? e : -5) : 0;
    }
    // message buffer of panel b (PANEL_PAD above)
    char *buf_of(int b) const { return (char *)c->dist_buf[b & 1].get(); }
    int64_t rows_of(int b) const { return N - (int64_t)b * nb; }
    int64_t ldp_of(int b) const { return rows_of(b) + PANEL_PAD; }
    size_t list_off(int b) const { return (size_t)ldp_of(b) * L.width(b) * 8; }
    int *piv_ptr(int b, int q) const { return (int *)((double *)buf_of(b) + (size_t)(32 * q) * ldp_of(b) + rows_of(b)); }   // pivots of sub-panel q
    PanelView panel(int b) const { return {A + L.lcol(b) * lda, lda, (int64_t)b * nb, (int)rows_of(b), L.width(b), c->lists + b, ipiv + (int64_t)b * nb}; }
    // super-panels: first block of b's, one past its last block, one past its look-ahead block, this rank's first far column
    int sp_first(int b) const { return (b / sb) * sb; }
    int sp_end(int b) const { const int e = sp_first(b) + sb; return e < L.nblocks ? e : L.nblocks; }
    int inner_end_blk(int b) const { const int e = sp_end(b) + 1; return e < L.nblocks ? e : L.nblocks; }
    int64_t far0(int b) const { return sb > 1 ? L.first_local_col_after(inner_end_blk(b) - 1) : lcols; }
    FarView far_view(int b) const { return {A + far0(b) * lda, lda, W + far0(b), ldw, lcols - far0(b), SPL, N, (const double *)buf_of(b), ldp_of(b)}; }

    // every call starts here: info and the pivot kernel's give-up counter reset (lists: + moved-row lists, left-hand scratch), the clock
    int begin(bool lists) {
        const int rc = mpf_factor_setup(c, N, nb, L.nblocks, lists);
        if (!rc) MPF_HIP_TRY(c, hipEventRecord(c->ev0, S));
        return rc;
    }
    // ---- what every rank must decide alike ------------------------------------------------------------------------------
    // How many broadcasts a panel message travels in, and the one- / two-level choice, follow from rank-local state: which streams
    // could be created, what this device's pivot kernel can hold, per-context options.  Ranks that disagreed would issue different
    // collectives (a hang) or factor with different roundings.  Every rank's values go round once (one 64-byte broadcast per rank)
    // and everyone takes the minimum; `sb` differing is an error on every rank (the buffers were sized for the local value).
    int agree() {
        hp_query_residency(c);
        // rows this device's pivot kernel can take beside the workgroups of the pipelined chain's gated interchange kernel (which wait for it)
        const long long lds_rows = hgetf2_capacity_rows(c, laswp_gated_grid(nb)), cap = HP_R * (long long)HP_MAXG;
        long long mine[8] = {two && c->tune.chain_pipeline != 0 && c->tstream != nullptr && !generic && c->tune.dist_instalments && c->xstream ? 1 : 0,
                             sb, -(long long)c->tune.dist_instalment_min_bytes, c->tune.dpanel_fused_form ? 1 : 0, lds_rows < cap ? lds_rows : cap,
                             two ? 1 : 0, 0, 0}, agreed[8];
        memcpy(agreed, mine, sizeof mine);
        long long *dv = (long long *)c->dist_buf[0].get();   // (free until the first panel message)
        for (int root = 0; root < L.world && L.world > 1; ++root) {
            if (root == L.rank) MPF_HIP_TRY(c, hipMemcpyAsync(dv, mine, sizeof mine, hipMemcpyHostToDevice, c->stream));
            const int e = bcast(dv, sizeof mine, root, c->stream);
            if (e) return e;
            long long got[8];
            MPF_HIP_TRY(c, hipMemcpyAsync(got, dv, sizeof got, hipMemcpyDeviceToHost, c->stream));
            MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));
            for (int i = 0; i < 8; ++i) if (got[i] < agreed[i]) agreed[i] = got[i];
        }
        if (agreed[1] != sb) { c->err = "mpf_factor_dist: the ranks disagree on the super-panel width (options superpanel_fp16 / fp16_work32 / safe_pivots must be the same on every rank)"; return -1; }
        inst_ok = agreed[0] != 0; inst_min_bytes = -agreed[2]; fused_form_all = agreed[3] != 0; lds_rows_max = agreed[4];
        return 0;
    }
    // Two-level schedule of the fp16 modes (factor_superpanel in mpf_factor.cpp, carried over to the block-cyclic layout): sb panels
    // form a super-panel; a panel updates only the INNER blocks (the super-panel's own and the next super-panel's first one) of
    // this rank, panel by panel, in fp64; this rank's FAR columns live in an fp32 row-major working copy and get one update with
    // K = sb * nb per super-panel, after the U block-row tasks.  What the single-GPU schedule reads from the matrix left of the
    // panel -- the super-panel's earlier panels -- every rank keeps in a store of its own, assembled from the panel messages.
    int set_up() {
        // the width is the single-GPU rule's; the gate is this loop's own: the inner region holds the look-ahead block too
        const int want_sb = wanted_superpanel(c, o, N);
        sb = (!f64 && !generic && c->tune.fp16_work32 != 0 && hgetf2_lds_eligible(c, (int)N, (int)(nb < N ? nb : N)) &&
              (int64_t)(want_sb + 1) * nb < N) ? want_sb : 1;
        const int64_t sbw = (int64_t)sb * nb;
        int rc = 0;
        if (!f64) {
            const int64_t kimg = sbw < 8 * HP_MAXCOLS ? sbw : 8 * HP_MAXCOLS;
            rc = sb > 1 ? mpf_ensure_h_images(c, N + HP_MAXCOLS + 64, (int)kimg, true) : mpf_ensure_h_images(c, N, nb, false);
            if (rc) return rc;
        }
        if (sb > 1) {
            MPF_HIP_TRY(c, c->dist_w32.grow(N * (lcols > 0 ? lcols : 1)));
            MPF_HIP_TRY(c, c->dist_spl.grow(N * sbw));
        }
        if (!c->xstream && L.world > 1 && c->tune.dist_instalments) {   // exchange stream of the panel's instalments
            int lo = 0, hi = 0;
            hipDeviceGetStreamPriorityRange(&lo, &hi);
            if (hipStreamCreateWithPriority(&c->xstream, hipStreamNonBlocking, hi) != hipSuccess) c->xstream = nullptr;
        }
        if (!o.no_lookahead && c->pstream) P = c->pstream;
        two = P != S;
        rc = agree();
        if (rc) return rc;
        // fp64 mode: this rank's columns right of the current panel live in a ROW-major working copy (as factor_lookahead_rm's): an
        // interchange moves contiguous row segments instead of one 64-byte sector per moved row and column; the update is the same MFMA
        // kernel on the transposed problem (c = fma(-u, l, c), kk ascending: the same bits).  Rank-local choice: results do not depend on it.
        rm = f64 && lcols > 0 && c->tune.fp64_rowmajor && N >= c->tune.fp64_rowmajor_min_n && N > nb && mpf_ensure_rowmajor_copy(c, N, lcols, nb) == 0;
        W = c->dist_w32; SPL = c->dist_spl;
        ldw = lcols > 0 ? lcols : 1;
        rv = {A, lda, rm ? c->r64.get() : nullptr, ldw};
        st.superpanel = sb;
        g = image_geom(N, sb > 1 ? lcols - L.first_local_col_after(sb) : 0, sb, nb, c->h_kmax, f64);
        rc = begin(true);
        if (rc) return rc;
        X = c->xstream ? c->xstream : P;   // (the owner's P runs the pivot kernel meanwhile)
        if (two) stream_join(ev, S, P);
        return 0;
    }
    // Number of 32-column instalments the message of panel b travels in (0: one broadcast after the whole chain).  A function
    // of the shape and of options that must be the same on every rank (chain_pipeline, pivot_path / safe_pivots, dist_instalments).
    // Small panels go in one piece: an instalment costs a collective's latency.
    int pieces_of(int b) const {
        const int64_t pc = L.width(b), pr = rows_of(b);
        if (!inst_ok || pc > HP_MAXCOLS || pr > lds_rows_max) return 0;           // (every rank's pivot kernel can hold the panel)
        if (pr * pc * 8 < inst_min_bytes) return 0;
        return (fused_form_all && pc % 32 == 0 && pc >= 64) ? (int)(pc / 32) : 0;        // = dgetf2_npv_pieces with the agreed option
    }
    // columns [c0, c0 + nc) of the panel + their sub-panels' pivots into the message
    int pack(int b, const PanelView &v, hipStream_t ps, int c0, int nc) {
        const int64_t ldp = ldp_of(b);
        MPF_HIP_TRY(c, hipMemcpy2DAsync(buf_of(b) + (size_t)c0 * ldp * 8, (size_t)ldp * 8, v.A + v.k + (int64_t)c0 * lda, (size_t)lda * 8, (size_t)v.pr * 8,
                                        (size_t)nc, hipMemcpyDeviceToDevice, ps));
        for (int q = c0 / 32; q * 32 < c0 + nc; ++q) {
            const int w = (v.pc - 32 * q) < 32 ? (v.pc - 32 * q) : 32;
            MPF_HIP_TRY(c, hipMemcpyAsync(piv_ptr(b, q), v.ipiv + 32 * q, (size_t)w * 4, hipMemcpyDeviceToDevice, ps));
        }
        return 0;
    }
    // owner only: pivots, interchange of the panel's own columns, fp64 panel, pack -- on stream s (and T).  With instalments
    // (np > 0) ev_piece[q] is recorded once instalment q (32 packed columns + their pivots; the last one: + the moved-row list)
    // is complete in the message buffer.
    int chain(int b, hipStream_t s, int np) {
        const PanelView v = panel(b);
        const int64_t ldp = ldp_of(b);
        char *buf = buf_of(b);
        StreamSwap sw(c, s);
        hipEvent_t before_pivots = ev.get();
        hipEventRecord(before_pivots, s);
        const bool lds = !generic && hgetf2_lds_eligible(c, v.pr, v.pc);
        // the fp64 panel follows the pivot kernel 32 columns behind on the helper stream (see chain_behind in mpf_factor.cpp) -- where
        // the panel's workgroups fit beside the gated interchange kernel's, which wait for it while sitting on CUs
        const int waiters = (c->tune.gate_wait_value && c->hp_signal) ? 0 : laswp_gated_grid(v.pc);
        const bool will_pipe = c->tune.chain_pipeline != 0 && c->tstream != nullptr && lds && hgetf2_fits_beside(c, v.pr, v.pc, waiters);
        int e = panel_pivots(f, v, s, will_pipe ? waiters : 0, !lds);
        if (e) return e;
        hipEvent_t pivots_done = ev.get();
        hipEventRecord(pivots_done, s);
        const int npp = will_pipe ? dgetf2_npv_pieces(c, v.pc) : 0;
        if (np > 0 && npp != np) { c->err = "mpf_factor_dist: instalment count differs from the agreed one"; return -1; }
        if (npp > 0) {
            hipStream_t T = c->tstream;
            hipStreamWaitEvent(T, before_pivots, 0);
            {
                StreamSwap swt(c, T);
                hipEvent_t t0 = ev.get(), t1 = ev.get();   // (the pieces run under ms_dpanel only where every region is timed)
                hipEventRecord(t0, T);
                e = panel_pieces(f, v, npp, [&](int q) -> int {
                    if (np == 0) return 0;
                    int e2 = pack(b, v, T, 32 * q, 32);   // instalment q leaves as it is: the interchanges still to come are applied to the message copy
                    // (the matrix holds the UNfactored diagonal tile until the last piece has run: dpanel.hip)
                    if (!e2 && q < np - 1) e2 = launch_dpanel_tile_copy(c, (double *)buf + (size_t)(32 * q) * ldp + 32 * q, ldp, q);
                    if (!e2 && q == np - 1) {
                        hipStreamWaitEvent(T, pivots_done, 0);   // the moved-row list is complete when the pivot kernel has ended
                        MPF_HIP_TRY(c, hipMemcpyAsync(buf + list_off(b), v.ml, sizeof(MovedList), hipMemcpyDeviceToDevice, T));
                    }
                    if (!e2) { ev_piece[(size_t)q] = ev.get(); hipEventRecord(ev_piece[(size_t)q], T); }
                    return e2; });
                hipEventRecord(t1, T);
                if (c->tune.timeline || c->tune.event_timers >= 2) ev.pairs.push_back({t0, t1, &st.ms_dpanel, nullptr});
            }
            stream_join(ev, T, s);
        } else e = panel_tail(f, v, s);
        if (e) return e;
        if (np == 0) {   // the whole message at once, from the finished panel
            e = pack(b, v, s, 0, v.pc);
            if (!e) MPF_HIP_TRY(c, hipMemcpyAsync(buf + list_off(b), v.ml, sizeof(MovedList), hipMemcpyDeviceToDevice, s));
        }
        st.panels++;
        return e;
    }
    // every rank: the exchange of panel b on stream s, then (non-owners) pivots and moved list out of the message.
    // np == 0: ONE broadcast.  np > 0: np instalments; after instalment q every rank applies sub-panel q's 32 interchanges to
    // the instalments already there (what the owner's matrix got from laswp_block while the later instalments were still being
    // factored): the assembled message is the finished panel.
    int exchange(int b, hipStream_t s, int np) {
        const int pc = L.width(b);
        const int64_t k = (int64_t)b * nb, ldp = ldp_of(b);
        char *buf = buf_of(b);
        int e = 0;
        if (np == 0) e = bcast(buf, list_off(b) + sizeof(MovedList), L.owner(b), s);
        else {
            StreamSwap sw(c, s);
            for (int q = 0; q < np && !e; ++q) {
                if (L.mine(b)) hipStreamWaitEvent(s, ev_piece[(size_t)q], 0);
                const size_t off = (size_t)(32 * q) * ldp * 8;
                e = bcast(buf + off, q == np - 1 ? list_off(b) + sizeof(MovedList) - off : (size_t)32 * ldp * 8, L.owner(b), s);
                // rows of the message are rows k.. of the matrix: address it from the matrix' row 0
                if (!e && q > 0) e = launch_laswp_block(c, (double *)buf - k, ldp, 32 * q, (int)k + 32 * q, 32, piv_ptr(b, q), N);
            }
        }
        if (e || L.mine(b)) return e;
        const int nq = (pc + 31) / 32;
        MPF_HIP_TRY(c, hipMemcpy2DAsync(ipiv + k, 128, piv_ptr(b, 0), (size_t)32 * ldp * 8, 128, (size_t)(pc / 32), hipMemcpyDeviceToDevice, s));
        if (pc % 32) MPF_HIP_TRY(c, hipMemcpyAsync(ipiv + k + 32 * (nq - 1), piv_ptr(b, nq - 1), (size_t)(pc % 32) * 4, hipMemcpyDeviceToDevice, s));
        MPF_HIP_TRY(c, hipMemcpyAsync(c->lists + b, buf + list_off(b), sizeof(MovedList), hipMemcpyDeviceToDevice, s));
        return 0;
    }
    // interchange + TRSM + trailing update of panel b on the local columns [c0, c0 + nc) (all right of block b)
    int update(int b, int64_t c0, int64_t nc) {
        if (nc <= 0) return 0;
        const int64_t k = (int64_t)b * nb, ldp = ldp_of(b);
        const int pc = L.width(b);
        const int64_t m = N - k - pc;
        const double *Pb = (const double *)buf_of(b);
        if (rm) {
            // interchange of contiguous row segments, TRSM through strides, L21 row-major once per panel, the update on the transposed
            // problem, then the finished U rows of these columns go home to the column-major matrix
            double *LT = c->rm_lt;
            int e = rm_swap(f, rv, S, c0, nc, {c->lists + b}, 0);
            if (!e) e = rm_solve_u(f, rv, S, Pb, ldp, k, pc, c0, nc);
            if (!e && m > 0) {
                if (!image_ready) { e = rm_l_image(f, S, Pb + pc, ldp, m, pc, LT, pc); image_ready = true; }
                if (!e) e = rm_update(f, rv, S, k, pc, k + pc, m, c0, nc, LT, pc);
            }
            if (!e) e = rm_home(f, rv, S, k, pc, c0, nc);
            return e;
        }
        int e = ev.timed(st.ms_laswp, S, [&] { return launch_laswp_from_list(c, A + c0 * lda, lda, nc, c->lists + b); });
        double *U12 = A + c0 * lda + k;
        if (!e) e = ev.timed(st.ms_trsm, S, [&] { return launch_dtrsm_llnu(c, pc, nc, Pb, ldp, U12, lda); });
        if (e || m <= 0) return e;
        e = ev.timed(st.ms_gemm, S, [&] {
            int e2 = 0;
            if (!f64 && !image_ready) { e2 = launch_cvt_l21(c, Pb + pc, ldp, m, pc, split); image_ready = true; } // once per panel
            if (!f64 && sb == 1) return e2 ? e2 : launch_hgemm_minus(c, m, nc, pc, U12, lda, U12 + pc, lda, split);
            if (!f64 && !e2) e2 = launch_inner_u_image(c, o, U12, lda, pc, nc, g.inner_u_off);
            return e2 ? e2 : launch_inner_gemm(c, o, m, nc, pc, Pb + pc, ldp, U12, lda, g.inner_u_off); });
        count_gemm(st, o, m, nc, pc);
        return e;
    }
    // ---- two-level schedule: this rank's far columns (sb > 1) -------------------------------------------------------------
    // the super-panel's panels as received: eager interchanges of panel b on the earlier ones, then panel b itself
    int spl_add(int b) {
        const int p = b - sp_first(b);
        const int64_t k = (int64_t)b * nb;
        int e = 0;
        if (p > 0) e = ev.timed(st.ms_laswp, S, [&] { return launch_laswp_from_list(c, SPL, N, (int64_t)p * nb, c->lists + b); });
        if (!e) MPF_HIP_TRY(c, hipMemcpy2DAsync(SPL + (int64_t)p * nb * N + k, (size_t)N * 8, buf_of(b), (size_t)ldp_of(b) * 8, (size_t)(N - k) * 8, (size_t)L.width(b),
                                                hipMemcpyDeviceToDevice, S));
        return e;
    }
    int far_task(int b) {   // block-row task of panel b on the far columns (T_p of factor_superpanel)
        if (far0(b) >= lcols) return 0;
        const int e = spl_add(b);
        return e ? e : far_block_row(f, far_view(b), g, (int64_t)sp_first(b) * nb, b - sp_first(b));
    }
    int superpanel_begin(int b) { return far_zero_padding(f, lcols - far0(b), g); }
    // end of b's super-panel: the operand image of L[s1.., s0..s1) once, the K = s1 - s0 update on the columns that join the next inner
    // region first (they return to fp64), then on the rest
    int superpanel_end(int b) {
        const int64_t f0 = far0(b), f0n = far0(sp_end(b));            // first far column of this and of the next super-panel
        if (f0 >= lcols) return 0;
        const int64_t s0 = (int64_t)sp_first(b) * nb, s1 = (int64_t)sp_end(b) * nb;
        const FarView v = far_view(b);
        int e = ev.timed(st.ms_cvt, S, [&] { return launch_cvt_l21(c, SPL + s1, N, N - s1, (int)(s1 - s0), split, far_img); });
        if (!e) e = far_big_update(f, v, g, s0, s1, 0, f0n - f0, far_img);
        if (!e && f0n > f0) e = ev.timed(st.ms_cvt, S, [&] { return launch_cvt_f32_f64(c, W + s1 * ldw + f0, ldw, A + f0 * lda + s1, lda, N - s1, f0n - f0); });
        if (!e) e = far_big_update(f, v, g, s0, s1, f0n - f0, lcols - f0n, far_img);
        far_img = 3 - far_img;
        return e;
    }
    // Schedule = the look-ahead schedule of mpf_factor.cpp with column indices translated (top of this file)
    int run() {
        int rc = 0;
        if (sb > 1 && far0(0) < lcols)   // this rank's far columns of the first super-panel go into the working copy
            rc = ev.timed(st.ms_cvt, S, [&] { return launch_cvt_f64_f32(c, A + far0(0) * lda, lda, W + far0(0), ldw, N, lcols - far0(0)); });
        if (!rc && L.live(0)) {
            if (L.mine(0)) rc = chain(0, S, 0);
            if (!rc) rc = exchange(0, S, 0);
        }
        if (!rc && rm)   // everything this rank owns goes into the row-major copy (block 0, if it is here, is finished: its copy is never read)
            rc = rm_l_image(f, S, rv.a(0, 0), lda, N, lcols, rv.r(0, 0), rv.ldr);
        for (int b = 0; L.live(b) && rc == 0; ++b) {
            const int64_t k = (int64_t)b * nb;
            const int pc = L.width(b);
            const int nxt = b + 1;
            const bool has_next = L.live(nxt), own_next = has_next && L.mine(nxt), trailing = k + pc < N;
            int64_t rest0 = L.first_local_col_after(b);
            image_ready = false;
            hipEvent_t e2 = nullptr;
            if (trailing && own_next) { // my block of panel b+1 first, then its chain on the side stream
                rc = update(b, L.lcol(nxt), L.width(nxt));
                if (!rc && rm)   // the next panel's columns return to the column-major matrix before its chain (rows k + pc ..; its U rows went with the update)
                    rc = rm_home(f, rv, S, k + pc, N - k - pc, L.lcol(nxt), L.width(nxt));
                if (rc) break;
                rest0 = L.lcol(nxt) + L.width(nxt);
            }
            if (has_next) {
                const int np = pieces_of(nxt);
                hipStream_t xs = np > 0 ? X : P;
                if (two) { // strip done; receive buffer free (its last reader was update b - 1, in front of this event on S)
                    hipEvent_t e1 = ev.get(); hipEventRecord(e1, S); hipStreamWaitEvent(P, e1, 0);
                    if (xs != P) hipStreamWaitEvent(xs, e1, 0);
                }
                ev_piece.assign((size_t)(np > 0 ? np : 1), nullptr);
                if (own_next) rc = chain(nxt, P, np);
                if (!rc) rc = exchange(nxt, xs, np);
                if (rc) break;
                if (two) {
                    e2 = ev.get(); hipEventRecord(e2, xs);
                    if (xs != P && own_next) stream_join(ev, P, S);   // the owner's chain itself
                }
            }
            if (sb == 1) { if (trailing && rest0 < lcols) rc = update(b, rest0, lcols - rest0); }
            else if (trailing) {
                // inner blocks right of the strip, panel by panel in fp64; far columns: block-row task now, K = sb * nb update at the
                // end of the super-panel (it runs under the chain of the next super-panel's first panel, launched above)
                if (b == sp_first(b)) rc = superpanel_begin(b);
                if (!rc && rest0 < far0(b)) rc = update(b, rest0, far0(b) - rest0);
                if (!rc) rc = far_task(b);
                if (!rc && b + 1 == sp_end(b)) rc = superpanel_end(b);
            }
            if (e2) hipStreamWaitEvent(S, e2, 0);
            if (o.verbose) printf("[rank %d] panel %d (k=%lld) owner %d\n", L.rank, b, (long long)k, L.owner(b));
        }
        if (!rc) rc = ev.timed(st.ms_laswp, S, [&] { return launch_lazy_left_swaps(c, A, lda, N, nb, L.nblocks, c->lists, 1, L.world, L.rank); });
        return rc;
    }
    // Panels wider than 256 columns (the LDS pivot kernel and the moved-row lists stop there): the reference's own order, panel by
    // panel on one stream, with the generic (global-memory) pivot kernels and the sequential interchange of ALL local columns
    // (MPF.cu:145-162) -- no look-ahead, no deferred left-hand side.  Message = the factored panel (leading dimension = its rows)
    // followed by its pivots.  Per element the operations are those of factor_generic (mpf_factor.cpp): identical bits.
    int run_wide() {
        int rc = f64 ? 0 : mpf_ensure_h_images(c, N, nb < 8 * HP_MAXCOLS ? nb : 8 * HP_MAXCOLS, false);
        for (int b = 0; L.live(b) && rc == 0; ++b) {
            const int64_t k = (int64_t)b * nb;
            const int pc = L.width(b), pr = (int)(N - k);
            double *buf = c->dist_buf[0];
            int *piv = (int *)(buf + (size_t)pr * pc);
            if (L.mine(b)) {
                double *Ap = A + L.lcol(b) * lda + k;
                st.pivot_path = 1;
                rc = ev.timed(st.ms_hpanel, S, [&] { return launch_hgetf2_generic(c, Ap, lda, nullptr, 0, pr, pc, (int)k, ipiv + k, nullptr, 0); });
                if (!rc) rc = ev.timed(st.ms_laswp, S, [&] { return launch_laswp_seq(c, A, lda, lcols, (int)k, pc, ipiv + k, N); });
                if (!rc) rc = ev.timed(st.ms_dpanel, S, [&] { return launch_dgetf2_npv(c, Ap, lda, pr, pc, o.fused_panel, (int)k); });
                if (rc) break;
                MPF_HIP_TRY(c, hipMemcpy2DAsync(buf, (size_t)pr * 8, Ap, (size_t)lda * 8, (size_t)pr * 8, (size_t)pc, hipMemcpyDeviceToDevice, S));
                MPF_HIP_TRY(c, hipMemcpyAsync(piv, ipiv + k, (size_t)pc * 4, hipMemcpyDeviceToDevice, S));
                st.panels++;
            }
            rc = bcast(buf, (size_t)pr * pc * 8 + (size_t)pc * 4, L.owner(b), S);
            if (rc) break;
            if (!L.mine(b)) {
                MPF_HIP_TRY(c, hipMemcpyAsync(ipiv + k, piv, (size_t)pc * 4, hipMemcpyDeviceToDevice, S));
                if (lcols > 0) rc = ev.timed(st.ms_laswp, S, [&] { return launch_laswp_seq(c, A, lda, lcols, (int)k, pc, ipiv + k, N); });
                if (rc) break;
            }
            const int64_t c0 = L.first_local_col_after(b), nc = lcols - c0, m = (int64_t)pr - pc;
            if (k + pc < N && nc > 0) {
                double *U12 = A + c0 * lda + k;
                rc = ev.timed(st.ms_trsm, S, [&] { return launch_dtrsm_llnu(c, pc, nc, buf, pr, U12, lda); });
                if (!rc && m > 0) {
                    rc = ev.timed(st.ms_gemm, S, [&] { return launch_generic_update(c, o, m, nc, pc, buf + pc, pr, U12, lda); });
                    count_gemm(st, o, m, nc, pc);
                }
            }
            if (o.verbose) printf("[rank %d] panel %d (k=%lld) owner %d (wide panels: generic schedule)\n", L.rank, b, (long long)k, L.owner(b));
        }
        return rc;
    }
    // the end of every call: the host waits for every stream; info covers this rank's panels only (the caller combines: min over the positive values)
    int report(int rc) {
        return factor_report(c, st, rc, [&] {
            hipError_t e = hipStreamSynchronize(S);
            for (hipStream_t s : {P, c->xstream, c->tstream})
                if (two && s) { const hipError_t e2 = hipStreamSynchronize(s); if (e == hipSuccess) e = e2; }
            if (!rc && e == hipSuccess) { ev.collect(); st.lookahead = two ? 1 : 0; }
            return e; }, "distributed factorization", "fp16 pivot kernel: inter-workgroup hand-off timed out (buffers invalid; use pivot_path = 1)");
    }
};
} // namespace

extern "C" {

int mpf_rccl_unique_id(void *out128) {
    if (!out128) return -1;
    std::string err;
    Rccl *r = rccl_load(err);
    if (!r) return -5;
    NcclId id;
    if (r->GetUniqueId(&id) != 0) return -5;
    memcpy(out128, id.internal, 128);
    return 0;
}

int mpf_rccl_init(mpf_ctx *c, const void *id128, int32_t rank, int32_t world) {
    if (!c || !id128 || world < 1 || rank < 0 || rank >= world) return -1;
    std::string err;
    Rccl *r = rccl_load(err);
    if (!r) { c->err = err; return -5; }
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    if (c->rccl_comm) { r->CommDestroy(c->rccl_comm); c->rccl_comm = nullptr; }
    NcclId id;
    memcpy(id.internal, id128, 128);
    const int rc = r->CommInitRank(&c->rccl_comm, world, id, rank);
    if (rc != 0) { c->rccl_comm = nullptr; c->err = std::string("ncclCommInitRank: ") + r->GetErrorString(rc); return -5; }
    c->rccl_rank = rank; c->rccl_world = world;
    c->rccl_bcast_calls = c->rccl_bcast_bytes = c->rccl_allreduce_calls = c->rccl_p2p_calls = c->rccl_p2p_bytes = 0;
    return 0;
}

int mpf_rccl_destroy(mpf_ctx *c) {
    if (!c) return -1;
    if (c->rccl_comm) {
        std::string err;
        Rccl *r = rccl_load(err);
        if (r) r->CommDestroy(c->rccl_comm);
        c->rccl_comm = nullptr;
    }
    return 0;
}

// one broadcast and one all-reduce of a small device buffer on the context's communicator: checks the whole RCCL call path
// (symbols, communicator, stream ordering) independently of the factorization; every rank of the communicator must call it
int mpf_rccl_selftest(mpf_ctx *c) {
    if (!c) return -1;
    if (!c->rccl_comm) { c->err = "RCCL communicator not initialised (mpf_rccl_init)"; return -5; }
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    double h[4] = {1.0 + c->rccl_rank, 2.0, 3.0, 4.0}, back[4] = {0, 0, 0, 0};
    Buf<double> d;
    MPF_HIP_TRY(c, d.grow(4));
    int rc = 0;
    if (hipMemcpyAsync(d, h, sizeof h, hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = -2;
    if (!rc) rc = rccl_bcast(c, d, sizeof h, 0, c->stream);
    if (!rc) rc = rccl_allreduce(c, d, 4, c->stream);
    if (!rc && hipMemcpyAsync(back, d, sizeof h, hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = -2;
    if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = -2;
    if (rc) return rc;
    const double w = (double)c->rccl_world;
    if (back[0] != 1.0 * w || back[1] != 2.0 * w || back[3] != 4.0 * w) { c->err = "RCCL self-test: wrong values"; return -5; }
    return 0;
}

// What the context's communicator is and what has gone over it since mpf_rccl_init (the multi-GPU bench line's `rccl` object: the
// record that RCCL itself saw N ranks, not only the launcher).  Counters are host-side counts of the calls this library issued.
int mpf_rccl_info(mpf_ctx *c, mpf_rccl_info_t *out) {
    if (!c || !out) return -1;
    memset(out, 0, sizeof *out);
    std::string err;
    Rccl *r = rccl_load(err);
    out->version = -1; out->comm_count = -1; out->comm_rank = -1;
    if (r) { int v = 0; if (r->GetVersion(&v) == 0) out->version = v; }
    if (r && c->rccl_comm) {
        int v = 0;
        if (r->CommCount && r->CommCount(c->rccl_comm, &v) == 0) out->comm_count = v;
        if (r->CommUserRank && r->CommUserRank(c->rccl_comm, &v) == 0) out->comm_rank = v;
    }
    out->has_comm = c->rccl_comm ? 1 : 0;
    out->has_p2p = rccl_has_p2p() ? 1 : 0;
    out->device = c->device;
    out->bcast_calls = c->rccl_bcast_calls; out->bcast_bytes = c->rccl_bcast_bytes;
    out->allreduce_calls = c->rccl_allreduce_calls;
    out->p2p_calls = c->rccl_p2p_calls; out->p2p_bytes = c->rccl_p2p_bytes;
    // link to every other visible device: 0 = none / unknown, else hipExtGetLinkTypeAndHopCount's link type (xGMI = 4 on ROCm) and hops
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess) {
        out->visible_devices = ndev;
        for (int d = 0; d < ndev && d < 16; ++d) {
            if (d == c->device) continue;
            uint32_t lt = 0, hops = 0;
            int can = 0;
            if (hipExtGetLinkTypeAndHopCount(c->device, d, &lt, &hops) == hipSuccess) { out->link_type[d] = (int32_t)lt; out->link_hops[d] = (int32_t)hops; }
            if (hipDeviceCanAccessPeer(&can, c->device, d) == hipSuccess) out->peer_access[d] = can;
        }
    }
    return 0;
}
// `reps` broadcasts of `bytes` from `root` on the context's communicator, timed with HIP events on the context's stream (every rank
// calls it): milliseconds per broadcast -- the cost of one panel message of that size, apart from the factorization
int mpf_rccl_bcast_probe(mpf_ctx *c, int64_t bytes, int32_t root, int32_t reps, double *ms_per_bcast) {
    if (!c || !ms_per_bcast || bytes <= 0 || reps <= 0) return -1;
    if (!c->rccl_comm) { c->err = "RCCL communicator not initialised (mpf_rccl_init)"; return -5; }
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    Buf<char> d;
    MPF_HIP_TRY(c, d.grow(bytes));
    hipMemsetAsync(d, 0, (size_t)bytes, c->stream);
    const long long calls0 = c->rccl_bcast_calls, bytes0 = c->rccl_bcast_bytes;
    int rc = rccl_bcast(c, d, bytes, root, c->stream);   // warm-up (connection set-up)
    hipEventRecord(c->ev0, c->stream);
    for (int i = 0; i < reps && !rc; ++i) rc = rccl_bcast(c, d, bytes, root, c->stream);
    hipEventRecord(c->ev1, c->stream);
    if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = -2;
    float ms = 0;
    hipEventElapsedTime(&ms, c->ev0, c->ev1);
    *ms_per_bcast = ms / reps;
    c->rccl_bcast_calls = calls0; c->rccl_bcast_bytes = bytes0;   // (the probe is not part of a factorization's traffic)
    return rc;
}

int mpf_rccl_version(void) {
    std::string err;
    Rccl *r = rccl_load(err);
    int v = 0;
    if (!r || r->GetVersion(&v) != 0) return -5;
    return v;
}

// ---- factorization ---------------------------------------------------------------------------------------------------
int mpf_factor_dist(mpf_ctx *c, double *d_Aloc, int64_t ldloc, int64_t N, int32_t nb, int32_t *d_ipiv, const mpf_dist *dist,
                    const mpf_opts *opts) {
    if (!c || !d_ipiv || !dist) return -1;
    mpf_opts o{};
    if (opts) o = *opts;
    if (factor_check_args(c, "mpf_factor_dist", "ldloc", N, nb, ldloc, o)) return -1;
    if (dist->world < 1 || dist->rank < 0 || dist->rank >= dist->world) { c->err = "mpf_factor_dist: bad rank / world"; return -1; }
    if (o.pivot_search != 0 || c->tune.pivot_fp64) {
        c->err = "mpf_factor_dist: the fp64 pivot rules (mpf_opts.pivot_search = 1 or 2, option pivot_fp64) are single-GPU only; use mpf_factor_dev";
        return -1;
    }
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    // One rank owns every column: the local matrix IS the matrix, and the single-GPU driver's schedules (row-major working copy in
    // two column lanes for fp64, three lanes for the fp16 modes) are the ones to run -- the N = 1 point of a scaling curve is the
    // single-GPU number.  (Option dist_world1_loop = 1 keeps one rank in the distributed loop: tests of that loop.)
    if (dist->world == 1 && !c->tune.dist_world1_loop) {
        if (!d_Aloc) return -1;
        return mpf_factor_dev(c, d_Aloc, ldloc, N, nb, d_ipiv, &o);
    }
    if (!dist->bcast && dist->world > 1 && (!c->rccl_comm || c->rccl_world != dist->world || c->rccl_rank != dist->rank)) {
        c->err = "mpf_factor_dist: no broadcast callback and no matching RCCL communicator (mpf_rccl_init)"; return -5;
    }
    DistFactor d(c, o, dist, d_Aloc, ldloc, N, nb, d_ipiv);
    if (d.lcols > 0 && !d_Aloc) return -1;
    int rc = ensure_dist_bufs(c, N, nb);
    if (rc) return rc;
    const bool wide = nb > HP_MAXCOLS;   // wide panels: the generic schedule (reference order, one stream)
    rc = wide ? d.begin(false) : d.set_up();
    if (rc) return rc;
    return d.report(wide ? d.run_wide() : d.run());
}

int mpf_dist_set_p2p(mpf_ctx *c, mpf_p2p_fn fn, void *user) {
    if (!c) return -1;
    c->p2p_fn = fn; c->p2p_user = user;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// distributed refinement solve: residual = local GEMV + all-reduce; triangular solves walk the column blocks, the owner
// of a block applies it to the (replicated) vector and broadcasts the vector on
// ---------------------------------------------------------------------------------------------------------------------
int mpf_solve_ir_dist(mpf_ctx *c, const double *d_Aloc, int64_t lda, const double *d_LUloc, int64_t ldlu, const int32_t *d_ipiv,
                      int64_t N, int32_t nb, const double *d_b, double *d_x, int32_t max_iter, double tol, const mpf_dist *dist,
                      mpf_ir_stats *stats) {
    if (!c || !d_ipiv || !d_b || !d_x || !dist) return -1;
    if (N <= 0 || nb <= 0) { c->err = "solve_dist: bad N / nb"; return -1; }
    if (max_iter > 31) max_iter = 31;
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    mpf_bcast_fn bcast_fn = dist->bcast ? dist->bcast : rccl_bcast;
    mpf_allreduce_fn ar_fn = dist->allreduce ? dist->allreduce : rccl_allreduce;
    void *user = (dist->bcast || dist->allreduce) ? dist->user : (void *)c;
    const Layout L(N, nb, dist->rank, dist->world);
    const int64_t lcols = L.local_cols();
    int rc = mpf_ensure_solve_buf(c, N);
    if (rc) return rc;
    const int64_t SN = c->solve_n;
    double *r = c->solve_buf, *d = c->solve_buf + SN, *xloc = c->solve_buf + 2 * SN, *scal = c->solve_buf + 4 * SN;
    hipStream_t S = c->stream;
    std::vector<int32_t> ip((size_t)N), perm((size_t)N);
    MPF_HIP_TRY(c, hipMemcpyAsync(ip.data(), d_ipiv, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost, S));
    MPF_HIP_TRY(c, hipStreamSynchronize(S));
    for (int64_t i = 0; i < N; ++i) perm[(size_t)i] = (int32_t)i;
    for (int64_t i = 0; i < N; ++i) {
        const int64_t p = (int64_t)ip[(size_t)i] - 1;
        if (p < 0 || p >= N) { c->err = "solve_dist: ipiv entry out of range"; return -1; }
        if (p != i) std::swap(perm[(size_t)i], perm[(size_t)p]);
    }
    MPF_HIP_TRY(c, hipMemcpyAsync(c->perm_buf, perm.data(), (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice, S));
    mpf_ir_stats st{};
    hipEventRecord(c->ev0, S);
    // inverted diagonal blocks of the factors, for the blocks this rank owns (global block-of-64 index = position in trsv_inv)
    for (int b = L.rank; b < L.nblocks; b += L.world) {
        rc = launch_trsv_prepare_cols(c, d_LUloc + L.lcol(b) * ldlu, ldlu, N, (int64_t)b * nb, L.width(b));
        if (rc) return rc;
    }
    auto vec_bcast = [&](double *v, int64_t off, int64_t cnt, int root) -> int {
        if (L.world == 1 || cnt <= 0) return 0;
        const int e = bcast_fn(user, v + off, cnt * 8, root, (void *)S);
        return e ? (e < 0 ? e : -5) : 0;
    };
    // Point-to-point transport (round 4): the context's RCCL communicator (ncclSend / ncclRecv) with the built-in transport, or the
    // callback registered with mpf_dist_set_p2p next to the caller's own broadcast / all-reduce.
    mpf_p2p_fn p2p_fn = nullptr;
    void *p2p_user = nullptr;
    if (L.world > 1) {
        if (c->p2p_fn) { p2p_fn = c->p2p_fn; p2p_user = c->p2p_user; }
        else if (c->tune.dist_solve_p2p && !dist->bcast && !dist->allreduce && c->rccl_comm && rccl_has_p2p()) { p2p_fn = rccl_p2p; p2p_user = (void *)c; }
        // The choice follows from rank-local state (an option, a registered callback): ranks that chose differently would issue
        // different collectives and hang.  Every rank votes; the chain is taken only if ALL of them have it.
        double vote[2] = {p2p_fn ? 1.0 : 0.0, 1.0};
        MPF_HIP_TRY(c, hipMemcpyAsync(scal, vote, sizeof vote, hipMemcpyHostToDevice, S));
        { const int e = ar_fn(user, scal, 2, (void *)S); if (e) return e < 0 ? e : -5; }
        rc = read_scalars(c, scal, vote, 2);
        if (rc) return rc;
        if (vote[0] != vote[1]) { p2p_fn = nullptr; p2p_user = nullptr; }
    }
    double *up = xloc, *rbuf = c->solve_buf + 3 * SN;   // (xloc is only used by the residual, between two solves)
    auto p2p = [&](double *v, int64_t off, int64_t cnt, int peer, int send) -> int {
        if (cnt <= 0) return 0;
        const int e = p2p_fn(p2p_user, v + off, cnt * 8, peer, send, (void *)S);
        return e ? (e < 0 ? e : -5) : 0;
    };
    // out = U^-1 L^-1 P rhs, replicated on every rank.
    // With a point-to-point transport the running vector travels from owner to owner (a block's update needs nothing but what the
    // blocks before it have done to the rows below): 2 (nblocks - 1) sends of the tail / head + ONE all-reduce per solve, each rank
    // touching the wire only for its own blocks -- round 3 broadcast the vector to every rank after every block (2 nblocks
    // collectives per solve).  Lower sweep: the tail out[k + w .. N) goes on.  Upper sweep: every rank starts from its OWN segments
    // of y (zero elsewhere), adds what arrives, applies its block, sends the head [0, k) on and zeroes it locally (what has been sent
    // is the next owner's to hold); at the end the ranks' vectors are disjoint pieces of x: one all-reduce replicates it.
    auto lu_solve_chain = [&](const double *rhs, double *out) -> int {
        int e = launch_gather_rows(c, rhs, c->perm_buf, out, N);
        for (int b = 0; b < L.nblocks && !e; ++b) {
            if (!L.mine(b)) continue;
            const int64_t k = (int64_t)b * nb;
            const int w = L.width(b);
            if (b > 0 && L.owner(b - 1) != L.rank) e = p2p(out, k, N - k, L.owner(b - 1), 0);
            if (!e) e = launch_trsv_lower_cols(c, d_LUloc + L.lcol(b) * ldlu, ldlu, out, N, k, w);
            if (!e && b + 1 < L.nblocks && L.owner(b + 1) != L.rank) e = p2p(out, k + w, N - k - w, L.owner(b + 1), 1);
        }
        if (e) return e;
        MPF_HIP_TRY(c, hipMemsetAsync(up, 0, (size_t)N * 8, S));
        for (int b = L.rank; b < L.nblocks; b += L.world)
            MPF_HIP_TRY(c, hipMemcpyAsync(up + (int64_t)b * nb, out + (int64_t)b * nb, (size_t)L.width(b) * 8, hipMemcpyDeviceToDevice, S));
        for (int b = L.nblocks - 1; b >= 0 && !e; --b) {
            if (!L.mine(b)) continue;
            const int64_t k = (int64_t)b * nb;
            const int w = L.width(b);
            if (b + 1 < L.nblocks && L.owner(b + 1) != L.rank) {
                e = p2p(rbuf, 0, k + w, L.owner(b + 1), 0);
                if (!e) e = launch_axpy(c, 1.0, rbuf, up, k + w);
            }
            if (!e) e = launch_trsv_upper_cols(c, d_LUloc + L.lcol(b) * ldlu, ldlu, up, N, k, w);
            if (!e && b > 0 && L.owner(b - 1) != L.rank) {
                e = p2p(up, 0, k, L.owner(b - 1), 1);
                if (!e) MPF_HIP_TRY(c, hipMemsetAsync(up, 0, (size_t)k * 8, S));
            }
        }
        if (!e) { e = ar_fn(user, up, N, (void *)S); if (e) e = e < 0 ? e : -5; }
        if (!e) MPF_HIP_TRY(c, hipMemcpyAsync(out, up, (size_t)N * 8, hipMemcpyDeviceToDevice, S));
        return e;
    };
    auto lu_solve = [&](const double *rhs, double *out) -> int {
        if (p2p_fn) return lu_solve_chain(rhs, out);
        // broadcast-only transport: the owner applies a block to the replicated vector and broadcasts it on
        int e = launch_gather_rows(c, rhs, c->perm_buf, out, N);
        for (int b = 0; b < L.nblocks && !e; ++b) {
            const int64_t k = (int64_t)b * nb;
            if (L.mine(b)) e = launch_trsv_lower_cols(c, d_LUloc + L.lcol(b) * ldlu, ldlu, out, N, k, L.width(b));
            if (!e) e = vec_bcast(out, k, N - k, L.owner(b));
        }
        for (int b = L.nblocks - 1; b >= 0 && !e; --b) {
            const int64_t k = (int64_t)b * nb;
            if (L.mine(b)) e = launch_trsv_upper_cols(c, d_LUloc + L.lcol(b) * ldlu, ldlu, out, N, k, L.width(b));
            if (!e) e = vec_bcast(out, 0, k + L.width(b), L.owner(b));
        }
        return e;
    };
    auto norm = [&](const double *v, double &out) -> int { return vec_norm2(c, v, N, scal, out); };   // (S is c->stream)
    auto residual = [&](const double *x, double *rr) -> int { // rr = b - A x: own columns, then the sum over ranks
        int e = 0;
        for (int b = L.rank; b < L.nblocks && !e; b += L.world) // x restricted to the columns this rank owns
            MPF_HIP_TRY(c, hipMemcpyAsync(xloc + L.lcol(b), x + (int64_t)b * nb, (size_t)L.width(b) * 8, hipMemcpyDeviceToDevice, S));
        e = launch_residual_rect(c, d_Aloc, lda, xloc, L.rank == 0 ? d_b : nullptr, rr, N, lcols);
        if (!e && L.world > 1) { e = ar_fn(user, rr, N, (void *)S); if (e) e = e < 0 ? e : -5; }
        return e;
    };
    rc = refine_vector(c, N, d_b, d_x, max_iter, tol, st, r, d, norm, lu_solve, residual);
    if (rc) return rc;
    hipEventRecord(c->ev1, S);
    MPF_HIP_TRY(c, hipStreamSynchronize(S));
    float ms = 0;
    hipEventElapsedTime(&ms, c->ev0, c->ev1);
    st.ms_total = ms;
    if (stats) *stats = st;
    return 0;
}

} // extern "C"
