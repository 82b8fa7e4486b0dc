// What the factor schedules share (mpf_factor.cpp and factor_rm.cpp: the single-GPU driver, mpf_dist.cpp: the multi-rank loop, which
// runs the same steps on views of its block-cyclic storage): the argument checks, the wanted super-panel width, the bodies of a panel
// chain, the chain of the next panel and the end of a look-ahead schedule, the updates of the generic schedule and of an inner step,
// the far lane's steps, the steps on the fp64 row-major copy and the report that ends a call.  Host only; defined in mpf_factor.cpp
// (the row-major steps: factor_rm.cpp) unless inline.  The steps issue launches on the stream they are given (c->stream where none
// is): which stream waits for which event, and which schedule runs at a shape, stays with the callers.
#pragma once
#include "mpf_internal.h"
#include <initializer_list>

// what every schedule of one factorization works on (the entry point's arguments, the event pool, the statistics)
struct FactorArgs {
    mpf_ctx *c; EvPool &ev; mpf_stats &st; const mpf_opts &o;
    double *d_A; int64_t lda, N; int32_t nb; int32_t *d_ipiv;
};
// panel rows from which the pivot kernel takes its column-window form (launch_hgetf2's prefer_window_rows): the fp64 schedules only
inline int pref_window_rows(const mpf_opts &o) { return o.trailing == MPF_TRAIL_FP64 ? HP_FP64_WINDOW_ROWS : 0; }
// `into` goes on only behind everything queued on `from` so far
inline void stream_join(EvPool &ev, hipStream_t from, hipStream_t into) {
    hipEvent_t e = ev.get();
    hipEventRecord(e, from);
    hipStreamWaitEvent(into, e, 0);
}

// N, nb, the leading dimension (`ldname` in the text), N > INT_MAX / 2, nb > 65535, the trailing mode of entry `who`: 0, or -1 and the text
int factor_check_args(mpf_ctx *c, const char *who, const char *ldname, int64_t N, int32_t nb, int64_t ld, const mpf_opts &o);
// Panels per super-panel a call asks for: the mode's tuning value, 0 = automatic in the fp16 modes (a function of N and the mode only: the
// same on every rank, the same summation grouping in both drivers), mpf_opts.superpanel clamped to 8.  Whether it is USED: each driver's gate.
inline int wanted_superpanel(const mpf_ctx *c, const mpf_opts &o, int64_t N) {
    const bool f64 = o.trailing == MPF_TRAIL_FP64;
    int sb = f64 ? c->tune.superpanel_fp64 : c->tune.superpanel_fp16;
    if (!f64 && sb == 0) sb = (o.trailing == MPF_TRAIL_FP16 && N >= 24576) ? 6 : 4;   // (MpfTuning::superpanel_fp16)
    return o.superpanel > 0 ? (o.superpanel > 8 ? 8 : o.superpanel) : sb;
}
// The end of a factor call: ev1 on c->stream, the caller's wait for its streams, then ms_total, info and the pivot kernel's give-ups
// into st and st into c->stats.  rc (a failed launch) wins; a stream's error is -2 "<what> failed: ..."; a give-up is -4 with the
// caller's text; otherwise info.
int factor_report(mpf_ctx *c, mpf_stats &st, int rc, const std::function<hipError_t()> &wait, const char *what, const char *timeout_text);

// ---- panel chain: one panel's columns, wherever they live ----------------------------------------------------------------------------
struct PanelView {
    double *A; int64_t lda;    // row 0 of the panel's first column
    int64_t k; int pr, pc;     // first row, rows from there, columns
    MovedList *ml; int32_t *ipiv;   // the panel's moved-row list; where its pivots go
};
// (a) pivots, under ms_hpanel: the LDS kernel (waiters: workgroups of a gated interchange kernel that will wait for it on CUs), or with
// `generic` the global-memory kernel and its swap sequence resolved into the moved-row list (st.pivot_path = 1)
int panel_pivots(const FactorArgs &f, const PanelView &v, hipStream_t s, int waiters, bool generic = false);
// (b) the plain tail, under ms_dpanel: interchange of the panel's own columns, fp64 panel
int panel_tail(const FactorArgs &f, const PanelView &v, hipStream_t s);
// (c) the pipelined tail in np pieces of 32 columns (launches only): gated interchange of sub-panel q's pivots, piece q of the fp64
// panel, then after_piece(q)
int panel_pieces(const FactorArgs &f, const PanelView &v, int np, const std::function<int(int)> &after_piece = nullptr);
// single-GPU schedules (mpf_factor.cpp has the full story): the plain chain (a) + (b) of the matrix' panel at k on stream s; the chain of the
// NEXT panel (at nx) on the side streams behind e1, plain or pipelined (`b` is set), with the events that mark its end; the end of a
// look-ahead schedule -- the sink's last block rows or the deferred left-hand interchanges, then the host waits for the schedule's streams
int panel_chain(const FactorArgs &f, int64_t k, hipStream_t s);
struct ChainEnd { int rc = 0; hipEvent_t a = nullptr, b = nullptr; };
ChainEnd chain_behind(const FactorArgs &f, int64_t nx, hipEvent_t e1);
int factor_epilogue(const FactorArgs &f, int rc, bool sink, int sb, bool side_streams);

// ---- updates (launches only: the callers time and count them) ------------------------------------------------------------------------
// generic schedule, C = U12 + pc rows: one fp64 GEMM, or in the fp16 modes K cut to what the operand images hold
int launch_generic_update(mpf_ctx *c, const mpf_opts &o, int64_t m, int64_t n, int pc, const double *L21, int64_t ldl, double *U12, int64_t ldu);
// inner step of the two-level schedule in an fp16 mode: the U12 image behind the far columns' image, then (the L21 image being there)
// the image kernel; fp64: the GEMM alone
inline int launch_inner_u_image(mpf_ctx *c, const mpf_opts &o, const double *U12, int64_t ldu, int pc, int64_t n, int64_t inner_u_off) {
    return launch_cvt_u12(c, U12, ldu, pc, n, o.trailing == MPF_TRAIL_FP16X3, inner_u_off);
}
inline int launch_inner_gemm(mpf_ctx *c, const mpf_opts &o, int64_t m, int64_t n, int pc, const double *L21, int64_t ldl, double *U12, int64_t ldu, int64_t inner_u_off) {
    if (o.trailing == MPF_TRAIL_FP64) return launch_dgemm_minus(c, m, n, pc, L21, ldl, U12, ldu, U12 + pc, ldu);
    return launch_hgemm_images(c, m, n, pc, U12 + pc, ldu, false, o.trailing == MPF_TRAIL_FP16X3, 0, 0, inner_u_off);
}

// ---- far lane: the columns right of a super-panel's inner region, wherever they live -----------------------------------------------
struct FarView {
    double *A; int64_t lda;            // row 0 of the first far column in the fp64 matrix
    float *W; int64_t ldw, ncols;      // the same in the fp32 row-major working copy, or null: the update works on A; their count
    const double *Lsp; int64_t ldl;    // row 0 of the super-panel's first column of L: the matrix itself, or a rank's store of the panels
    const double *L11; int64_t ld11;   // the current panel's diagonal block: in the matrix, or in the panel message
};
struct ImageGeom { int kst; int64_t inner_u_off, brow_l_off; };   // row stride of the far U image; where the inner steps' U image and the block-row L images live
inline ImageGeom image_geom(int64_t N, int64_t far_cap, int sb, int nb, int h_kmax, bool f64) {   // far_cap: most far columns any super-panel has (here)
    const int kst = (int)(((int64_t)sb * nb + 63) & ~(int64_t)63);
    return {kst, (!f64 && far_cap > 0) ? far_cap * kst : 0, N * h_kmax};   // behind the far image; in the rows the image buffers hold beyond N
}
// image blocks of odd width: the padding the kernels read beyond a block must be zero
int far_zero_padding(const FactorArgs &f, int64_t ncols, const ImageGeom &g);
// Block-row task of panel p of the super-panel at s0 (full width nb): interchange; rows of block p lose L[p, < p] U[< p] (fp64: the
// MFMA GEMM, fp16 modes: the image kernel on A or W); back to fp64 from W; TRSM with L11; the finished U rows join the U image
int far_block_row(const FactorArgs &f, const FarView &v, const ImageGeom &g, int64_t s0, int p);
// the K = s1 - s0 update of the view's columns [col, col + ncols) below row s1 from L image `img`, with its statistics
int far_big_update(const FactorArgs &f, const FarView &v, const ImageGeom &g, int64_t s0, int64_t s1, int64_t col, int64_t ncols, int img);

// ---- fp64 row-major working copy (factor_rm.cpp; the multi-rank loop: a rank's local columns, ldr = their count) ----------------------
// Element (i, j) -- j a column of THIS storage -- lives at A[j * lda + i] and at R[i * ldr + j].  The two accessors are the only address
// arithmetic on R and on the U rows of A.
struct RmView {
    double *A; int64_t lda;
    double *R; int64_t ldr;
    double *a(int64_t i, int64_t j) const { return A + j * lda + i; }
    double *r(int64_t i, int64_t j) const { return R + i * ldr + j; }
};
// The steps of one panel on the columns [c, c + w) of the copy: each issues its launches on c->stream (the caller's StreamSwap scope) as ONE
// timed region booked on stream s.  rm_swap: interchange of contiguous row segments, list after list, under ms_laswp; scratch_off: where in
// the interchange scratch these columns' moved rows go (ranges in flight on different streams must not share it).  rm_solve_u: U[k : k + pc)
// = L11^-1 R[k : k + pc) through strides, under ms_trsm (L11: in the matrix, or in the panel message).  rm_update: R[r0 : r0 + rows) -=
// Limg U[ku : ku + K), the MFMA GEMM on the transposed problem under ms_gemm, and its count_gemm (Limg: row-major L image of the rows r0..).
// rm_home: the rows [row, row + rows) go home to the column-major matrix, under ms_cvt (split > 0: two launches, `split` rows first).
// rm_l_image: the other direction, a column-major block (of L21, of the matrix) into a row-major image (an L image, the copy itself).
int rm_swap(const FactorArgs &f, const RmView &v, hipStream_t s, int64_t c, int64_t w, std::initializer_list<const MovedList *> lists, int64_t scratch_off);
int rm_solve_u(const FactorArgs &f, const RmView &v, hipStream_t s, const double *L11, int64_t ld11, int64_t k, int pc, int64_t c, int64_t w);
int rm_update(const FactorArgs &f, const RmView &v, hipStream_t s, int64_t ku, int K, int64_t r0, int64_t rows, int64_t c, int64_t w, const double *Limg, int64_t ldimg);
int rm_home(const FactorArgs &f, const RmView &v, hipStream_t s, int64_t row, int64_t rows, int64_t c, int64_t w, int64_t split = 0);
int rm_l_image(const FactorArgs &f, hipStream_t s, const double *src, int64_t lds, int64_t rows, int64_t cols, double *img, int64_t ldimg);
bool pivots_fit_beside_update(const mpf_ctx *c, int64_t rows);   // the pivot kernel of a panel of `rows` rows fits beside a running update
// the schedule itself (mpf_factor_dev's fp64 default from fp64_rowmajor_min_n on)
int factor_lookahead_rm(mpf_ctx *c, double *d_A, int64_t lda, int64_t N, int32_t nb, int32_t *d_ipiv, const mpf_opts &o, mpf_stats &st, bool pairs);
