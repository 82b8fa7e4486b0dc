/*
 * mpf_c.h -- C ABI of the MI355X-native MPF hot path (libmpf_amd.so).
 *
 * Plain pointers and sizes only; no torch / C++ types.  Every entry point cites the piece of
 * the reference (paths relative to the reference repo) it replaces.  All `d_` pointers are
 * device (HBM) pointers; all matrices are fp64 column-major.  Calls are asynchronous on the
 * context's HIP stream unless stated otherwise.  Return value: 0 on success, < 0 on error
 * (mpf_last_error() gives the text), > 0 LAPACK-style "first zero pivot" where documented.
 */
#ifndef MPF_C_H
#define MPF_C_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct mpf_ctx mpf_ctx;

enum { MPF_TRAIL_FP64 = 0, MPF_TRAIL_FP16 = 1, MPF_TRAIL_FP16X3 = 2 };

typedef struct mpf_opts {
    int32_t trailing;    /* MPF_TRAIL_FP64: reference arithmetic (MPF.cu:215-239 in fp64).
                            MPF_TRAIL_FP16: fp16-in / fp32-accumulate MFMA trailing update.
                            MPF_TRAIL_FP16X3: the same with operands split hi + 2^-11 lo (three fp16 MFMA
                            products, ~22-bit operands): fp32-class factors at the same HBM-bound cost.
                            Both fp16 modes keep the matrix right of the current super-panel in an fp32 working
                            copy owned by the context (4 N^2 bytes of device memory, allocated at the first such
                            call; option fp16_work32 = 0 updates the fp64 matrix in place instead); panels, TRSMs and
                            the factors returned in d_A are fp64. */
    int32_t verbose;     /* 1: per-panel line on stdout like MPF.cu:137 */
    int32_t fused_panel; /* 0: separate fp64 mul/sub in the no-pivot panel (contract C3); 1: FMA */
    int32_t sync_timing; /* 1: no look-ahead, synchronise after every phase and fill the per-phase timers */
    int32_t no_lookahead;/* 1: single-stream schedule (panel k+1 only after the whole update k)   */
    int32_t superpanel;    /* 0: default (fp64: 1 = one-level loop; fp16 modes: 4); n > 1: n panels per super-panel, one
                              K = n * nb update of the matrix right of it (two-level schedule).  In the fp64 mode every
                              element keeps its fma chain, so the result does not depend on this value. */
    int32_t pivot_path;    /* 0: automatic -- the LDS-resident fp16 pivot kernel (its workgroups hand candidates to each other
                              inside one launch and must all be resident: one per CU) wherever the panel fits it, the generic
                              global-memory path otherwise (panels wider than 256 columns or taller than 256 rows x #CUs).
                              1: generic path and generic schedule always -- no kernel ever waits for another workgroup; for GPUs
                              shared with other processes (also option safe_pivots / MPF_SAFE_PIVOTS=1).  Results do not depend on this value. */
    int32_t pivot_search;  /* 0: the reference's rule -- pivots from an fp16 image of the panel (double_to_fp16 clamps at +-65504 and flushes
                              below 2^-14, so entries outside that range, or within one fp16 ulp of each other, tie).  Default.
                              1: LAPACK's partial pivoting -- the pivot search runs in fp64 on the numbers being eliminated (see
                              mpf_dgetf2_piv): |l_ij| <= 1, the pivots do not change when the matrix is scaled by a power of two, fp16's
                              range plays no part.  Runs the generic schedule's loop in every trailing mode (single stream, no kernel
                              waits for another workgroup, -4 cannot occur), any nb and lda: per panel mpf_dgetf2_piv, the interchange of
                              the columns left and right of the panel, then the TRSM and the update as they are.  In the fp64 trailing
                              mode IPIV and the factors equal, bit for bit, what the same loop gives through the step operators
                              mpf_dgetf2_piv, mpf_laswp, mpf_dtrsm_llnu, mpf_dgemm_minus.  Also option pivot_fp64 / MPF_PIVOT_FP64=1, which
                              turns it on for every entry point that factors internally.  Not available in mpf_factor_dist.
                              2: tournament pivoting (the panel of communication-avoiding LU) in fp64 -- the rule of mpf_dgetf2_tp: every
                              256-row slab of a 32-column sub-panel picks its own 32 best rows by partial pivoting, the winners are merged
                              eight slabs at a time, the sub-panel is factored without pivoting on the rows that won.  1 + ceil(log8(slabs))
                              selection launches per 32 columns instead of 33.  Scale-invariant like 1; |l_ij| <= 1 is NOT promised (a
                              panel of at most 256 rows gives exactly the pivots and bits of 1).  The same loop as 1 with mpf_dgetf2_tp as
                              the panel, the same bit statement against the step operators (mpf_dgetf2_tp, mpf_laswp, mpf_dtrsm_llnu,
                              mpf_dgemm_minus).  Also option pivot_fp64 = 2 / MPF_PIVOT_FP64=2; an explicit pivot_search of 1 or 2 wins over
                              the option.  Not available in mpf_factor_dist. */
} mpf_opts;

typedef struct mpf_stats {
    double ms_total;  /* device time of the last mpf_factor_dev (hipEvents)        */
    double ms_h2d, ms_d2h; /* only mpf_factor_host (ms_d2h: wall clock after the factorization's end) */
    /* per-phase device time.  sync_timing=1: each phase alone.  Look-ahead schedule: HIP-event pairs
     * around the launches as they ran (ms_hpanel = whole panel chain on the side stream, ms_dpanel = 0;
     * ms_gemm = sum over the gemm_launches trailing-update kernel launches, concurrent panel work included; conversions of
     * operands / working-copy windows are booked under ms_cvt). */
    double ms_hpanel, ms_laswp, ms_dpanel, ms_trsm, ms_gemm;
    int64_t n;
    int32_t nb, panels;
    int32_t hpanel_timeouts; /* spin give-ups inside the fp16 pivot kernel (must be 0) */
    int32_t info;            /* first zero pivot (1-based) or 0                        */
    int32_t gemm_launches;   /* number of dgemm launches behind ms_gemm                */
    int32_t lookahead;       /* 1 if the look-ahead schedule ran                       */
    int32_t superpanel;      /* panels per super-panel the schedule really used (1 = one-level loop) */
    int32_t pivot_path;      /* 0: LDS-resident pivot kernel on every panel; 1: some panel took the generic (global-memory) one */
    double gemm_flops;       /* flops of the launches timed under ms_gemm (2 m n k each; fp16x3: counted once, not 3x) */
    double gemm_bytes;       /* algorithmic HBM bytes of the same launches: 16 per updated fp64 element + operand reads */
    /* fp16 trailing modes, two-level schedule: the K = sb * nb update launches ALONE (the fp16 MFMA kernel, no conversion, no
     * inside-super-panel update): HIP-event time, flops (2 m n K), algorithmic HBM bytes (C read + write at 4 or 8 bytes per
     * element + the fp16 operand images once) and number of launches -- what bench.py's mxp.roofline is made of. */
    double ms_gemm_big, gemm_big_flops, gemm_big_bytes;
    double ms_cvt;           /* operand-image conversions and fp32 <-> fp64 window conversions (not part of ms_gemm) */
    double ms_blockrow;      /* U block-row of the super-panels (part of ms_trsm) */
    int32_t gemm_big_launches;
    int32_t host_rows_streamed; /* mpf_factor_host: block rows (panels) that went to the caller's matrix WHILE the factorization ran (0: the
                                   matrix went back in one piece afterwards, as MPF.cu:245-247 does; ms_d2h is then that copy, otherwise
                                   what was left of the way home after the last kernel) */
    int32_t host_late_segments; /* mpf_factor_host: column segments of the matrix that went UP while the factorization had started on the
                                   first part (0: the whole matrix first, as MPF.cu:82; ms_h2d is then the whole upload, otherwise the first part's) */
    int32_t pivot_search;       /* the pivot rule that ran: 0 fp16 image (the reference's), 1 fp64 partial pivoting, 2 fp64 tournament
                                   pivoting -- for 1 and 2 lookahead = 0, superpanel = 1, ms_hpanel = 0 and ms_dpanel is the pivoting panel
                                   (event_timers = 2 for the phase timers) */
    int32_t fp16_fused;         /* the fp16 pivot panel's elimination that ran: 0 rounded product, rounded difference (contract C2), 1 one fused
                                   multiply-add (contract C2f, option fp16_fused); 0 under pivot_search 1 and 2, which run no fp16 panel */
    int32_t lazy_onepass_blocks; /* look-ahead schedules: column blocks whose deferred left-hand interchanges ran in one pass, in place (option
                                   lazy_gather = 2; the others went through the temporary: option lazy_onepass_max_rows) */
} mpf_stats;

/* ---- lifetime -------------------------------------------------------------------------- */
/* Replaces the per-call cudaSetDevice/cudaMalloc/cublasCreate block, reference MPF.cu:69-97. */
int mpf_create(mpf_ctx **out, int device);
int mpf_destroy(mpf_ctx *ctx); /* reference MPF.cu:250-255 */
/* Use a caller-owned hipStream_t (e.g. torch's current stream) instead of the context's own. */
int mpf_set_stream(mpf_ctx *ctx, void *hip_stream);
int mpf_synchronize(mpf_ctx *ctx);
const char *mpf_last_error(mpf_ctx *ctx);
int mpf_get_stats(mpf_ctx *ctx, mpf_stats *out);
/* Per-context behaviour switches (schedule and kernel choices; results never depend on them unless stated).  A context takes
 * its defaults from the environment once, at mpf_create (variable MPF_<NAME>, upper case; e.g. MPF_SUPERPANEL for
 * "superpanel_fp16", see csrc/mpf_internal.h MpfTuning for the list); afterwards only these calls change them, so contexts
 * on different host threads are independent.  Names: safe_pivots, chain_pipeline, chain_pipeline_below, fp16_work32,
 * superpanel_fp16, superpanel_fp64, no_lookahead, verbose, timeline, hp_spin_limit, hp_gate_ticks, hp_acq_fence, hgemm_pad,
 * hgemm_split_pad, hgemm_big, hgemm_big_tile, dgemm_dma, generic_fused, pivot_fp64 (0 .. 2: the pivot_search every driver that factors internally uses), fp64_rowmajor, fp64_rowmajor_min_n, dist_instalments, dist_instalment_min_bytes, lazy_gather (0 .. 2), lazy_onepass_max_rows, dpanel_fused_form, trsm_laswp_fused,
 * fp16_fused (0 / 1, MPF_FP16_FUSED; default 0.  RESULTS DEPEND ON IT.  The rank-1 step of the fp16 pivot panel, hgetf2_kernel.cu:113
 * `panel[k*ld+row] -= multiplier * panel[k*ld+j]`: 0 = contract C2, the product rounded to fp16, then the difference rounded to fp16 -- what the
 * reference computes when nvcc does not contract, as under the `-G -O0` recipe this project's parity is stated for; 1 = contract C2f,
 * a[row][k] <- fma(-m, a[j][k], a[row][k]) rounded ONCE to fp16, round-to-nearest-even, subnormals kept, zeros / infinities / NaN by IEEE rules --
 * v_pk_fma_f16 here, CUDA's fma.rn.f16, what an optimised nvcc build may make of that line; negating m is exact.  Nothing else changes: the
 * conversion (C1), the pivot search and its tie-break, the division (IEEE fp32 quotient rounded once), the interchanges, the fp64 panel
 * (mpf_opts.fused_panel is independent), the trailing updates.  The fp16 panel's only output is IPIV, so the other setting is another
 * factorization: other pivots, other bits.  Read at each launch of a pivot kernel: mpf_hgetf2_pivots, mpf_hgetf2, mpf_factor_dev (every schedule
 * and trailing mode), mpf_factor_host, MPF(), mpf_gesv, mpf_gesvx, mpf_gesvx_block, mpf_gesvxx_block, mpf_factor_dist -- whose ranks MUST all hold
 * the same value (every rank factors panels with its own context's setting; ranks that disagree produce an inconsistent factorization, and nothing
 * checks it).  No effect under pivot_search = 1 or 2 (no fp16 panel runs).  mpf_stats.fp16_fused says what ran.),
 * gmres_group_tiles (tiles of 32 columns mpf_solve_gmres_ir_block takes together; 0 = automatic; same bits).  mpf_option_name enumerates them (returns the count). */
/* Rows of the tallest panel the LDS-resident pivot kernel takes -- all its workgroups must be resident at once -- beside `waiters`
 * workgroups of kernels that wait for its progress (0: alone; a negative value -w: beside the pipelined chain's gated interchange
 * kernel on a panel of w columns).  Derived from the kernels' LDS / register footprints and the occupancy API (csrc/fp16_panel.hip):
 * taller panels run unpipelined, or on the generic path.  form: 0 = the better of the two forms, 1 = the full-slab form (a CU per
 * 256 rows), 2 = the column-window form (two workgroups per CU). */
int64_t mpf_hgetf2_capacity_rows(mpf_ctx *ctx, int32_t waiters, int32_t form);
int mpf_set_option(mpf_ctx *ctx, const char *name, int64_t value);
int mpf_get_option(mpf_ctx *ctx, const char *name, int64_t *value);
int mpf_option_name(int32_t index, char *buf, int64_t buflen);
/* HIP analogue of the reference's capability probe, check_cooperative_groups.cu:4-48.
 * Writes a human-readable report into buf; returns the number of HIP devices or < 0. */
int mpf_device_report(char *buf, int64_t buflen);


/* ---- whole path ------------------------------------------------------------------------ */
/* The body of the reference's MPF() (MPF.cu:66-256) on HOST buffers: H2D, factor, D2H.
 * ipiv_host follows MPF.h:3 semantics (caller pre-initialises to identity).  The device copy of the matrix (N x N doubles) and of
 * the pivots stays in the context and only grows -- the reference allocates and frees it inside every call, MPF.cu:80-94,250-255 --
 * next to the fp64 mode's row-major working copy (another N x N doubles, mpf_factor_dev): a context that has factored an N x N host
 * matrix holds 2 x 8 N^2 bytes until mpf_trim or mpf_destroy.
 * Round 5: in the fp64 mode's look-ahead schedules (what MPF() runs) the transfers overlap the factorization -- from N = 4096 on
 * finished block rows of the factors go to A_host while it still runs (options host_sink, host_sink_min_n), from N = 16384 on only
 * the first quarter of the matrix goes up before the first panel (host_late_parts, host_first_pct, host_late_min_n); same bits
 * (csrc/rowsink.hip).  The call then starts short-lived host threads of its own, keeps ~330 MB of pinned memory and two
 * more N x N device buffers (staging of the block rows; the matrix as uploaded, from which the call repeats itself on the generic
 * pivot path if a pivot kernel gives up (-4) after rows have left).  mpf_stats.host_rows_streamed / host_late_segments say what ran.
 * On a negative return: with host_sink = 0 nothing has been copied back; otherwise A_host may hold finished block rows beside
 * untouched ones. */
int mpf_factor_host(mpf_ctx *ctx, double *A_host, int64_t N, int32_t nb, int32_t *ipiv_host,
                    const mpf_opts *opts);
/* Gives the context's large cached buffers back to the device (host-path copies, row-major / fp32 working copies); they are
 * allocated again on demand. */
int mpf_trim(mpf_ctx *ctx);
/* The panel loop MPF.cu:100-242 on a DEVICE-resident matrix (lda >= N).  d_ipiv: N int32,
 * entries for a skipped 1x1 tail are left untouched (MPF.cu:104).  Synchronises at the end.
 * Any panel width 1 <= nb <= 65535 (the tuned schedules cover nb <= 256 and N <= 256 x #CUs; the rest runs the generic
 * schedule -- same results, see mpf_opts.pivot_path).
 * Returns -4 when the LDS pivot kernel's bounded inter-workgroup wait gave up (only possible when something else holds
 * CUs for seconds, e.g. another process on the same GPU): d_A and d_ipiv are then INVALID (partially factored with
 * unusable pivots; nothing outside them was touched); call again on a fresh copy with pivot_path = 1. */
int mpf_factor_dev(mpf_ctx *ctx, double *d_A, int64_t lda, int64_t N, int32_t nb, int32_t *d_ipiv,
                   const mpf_opts *opts);

/* ---- step operators (each replaces one reference kernel / library call) ------------------ */
/* double_to_fp16_block, MPF.cu:20-25 (+ fp16_utils.h:15-23): out[i] = double_to_fp16(in[i]). */
int mpf_double_to_fp16(mpf_ctx *ctx, const double *d_in, uint16_t *d_out, int64_t n);
/* Element-wise fp16 division with the contract's IEEE semantics (the '/' of
 * hgetf2_kernel.cu:108); exposed so the division can be tested exhaustively. */
int mpf_hdiv(mpf_ctx *ctx, const uint16_t *d_a, const uint16_t *d_b, uint16_t *d_q, int64_t n);
/* Steps 1.1-3.2 of MPF.cu (:108-159) fused: read the fp64 panel d_A[0:rows, 0:cols] (leading
 * dimension lda), convert with double_to_fp16, run the fp16 partial-pivot LU of
 * HGETF2_kernel (hgetf2_kernel.cu:15-120) with the panel resident in LDS, and write
 * d_ipiv[j] = panel-local pivot + ipiv_offset (1-based; MPF.cu:152 uses ipiv_offset = k).
 * d_panel16_out (optional, may be NULL): receives the factored fp16 panel, rows x cols, ld =
 * rows, rows physically swapped as the reference leaves them -- for parity tests. */
int mpf_hgetf2_pivots(mpf_ctx *ctx, const double *d_A, int64_t lda, int32_t rows, int32_t cols,
                      int32_t ipiv_offset, int32_t *d_ipiv, uint16_t *d_panel16_out);
/* HGETF2_kernel itself (hgetf2_kernel.cu:15): fp16 panel in, factored in place, 1-based
 * panel-local pivots out. */
int mpf_hgetf2(mpf_ctx *ctx, uint16_t *d_panel16, int64_t ld, int32_t rows, int32_t cols,
               int32_t *d_ipiv_panel);
/* LASWP_kernel, MPF.cu:42-59: apply `cols` sequential swaps (row k+pc <-> d_ipiv_global[pc]-1)
 * to ncols columns of d_A. */
int mpf_laswp(mpf_ctx *ctx, double *d_A, int64_t lda, int64_t ncols, int32_t k, int32_t cols,
              const int32_t *d_ipiv_global);
/* dgetf2_native_npv, dgetf2_native_npv.cu:11-36, in place with leading dimension ld (no packed
 * copy: replaces the extract / write-back memcpy loops MPF.cu:168-200 too). */
int mpf_dgetf2_npv(mpf_ctx *ctx, double *d_P, int64_t ld, int32_t rows, int32_t cols, int32_t fused);
/* LAPACK dgetf2 on a panel (build extension; the reference has no fp64 pivot search): partial pivoting in fp64, in place on
 * d_P[rows x cols] with leading dimension ld; any rows >= 1, 1 <= cols <= 65535.
 * Pivot rule (idamax): for column j the pivot is the smallest row index p >= j with |a_pj| largest over rows j .. rows-1 of the
 * column as updated by the columns < j; comparison is a strict >, so the first maximum wins; a NaN never beats a number; a column
 * whose remaining part is all zero or all NaN keeps p = j.  d_ipiv[j] = p + 1 + ipiv_offset for j < min(rows, cols) (the convention
 * of mpf_hgetf2_pivots); rows j and p are exchanged in all columns of the panel.
 * Arithmetic: that of mpf_dgetf2_npv (contract C3), honouring `fused`: the multiplier is a_ij / a_jj, each element is then updated
 * once per k in ascending order (separate multiply and subtract, or one FMA).  Bit contract: the factored panel equals, bit for bit,
 * mpf_dgetf2_npv applied to the same panel with its rows pre-permuted by the returned pivots.
 * info (host, optional): first zero pivot, 1-based, or 0; when given the call synchronises, otherwise it is asynchronous.
 * One or two ordinary launches per column (csrc/dpivot.hip); the kernel boundary is the only inter-workgroup synchronisation: no
 * spinning, no bounded waits, no LDS-residency or co-residency requirement. */
int mpf_dgetf2_piv(mpf_ctx *ctx, double *d_P, int64_t ld, int32_t rows, int32_t cols, int32_t fused,
                   int32_t ipiv_offset, int32_t *d_ipiv, int32_t *info /* host, optional */);
/* The same panel with TOURNAMENT pivoting (build extension; the panel of CALU: Grigori, Demmel, Xiang): the same arguments and
 * limits as mpf_dgetf2_piv.  The rule is this project's own contract:
 * The panel goes by sub-panels of 32 columns.  At the sub-panel that starts at panel column j0, of width w = min(32, kmax - j0),
 * kmax = min(rows, cols), columns j0 .. j0+w-1 have received the updates of all earlier sub-panels and the active rows are j0 .. rows-1.
 * select(S), on a stack S of m <= 256 rows x w columns, is dgetf2's pivot choice on a private copy; it returns an ordered list of
 *   min(m, w) rows of S.  At step s = 0, 1, ... the row not yet chosen with the largest |x_s| is taken (a NaN counts as 0;
 *   comparison is a strict >, so the smallest position wins a tie; if every key is 0 that is the smallest position not yet
 *   chosen), and it changes places with the row at position s -- positions are the private copy's CURRENT ones, as in dgetf2, so
 *   the row a pivot displaced stands where that pivot was, and an all-zero column keeps position s.  Then every row not chosen
 *   computes m = x_s / pivot_s and x_c <- x_c - m u_c for c = s+1 .. w-1, product and difference rounded separately -- ALWAYS
 *   unfused, so the pivots do not depend on `fused`.
 * Tournament: level 0 groups the active rows by 256 consecutive rows counted from j0 (group g = rows j0 + 256 g ..) and runs select
 *   on each group.  Level l >= 1 stacks the lists of up to 8 consecutive groups (in group order, each list in its ranking order; the
 *   rows' values AS THEY WERE ON ENTRY to the sub-panel, not the eliminated ones) into <= 256 rows and runs select again, until one
 *   list is left: the winners q_0 .. q_{w-1}.  With one group at level 0 (at most 256 active rows) this is LAPACK's partial pivoting.
 * Interchanges: for s = 0 .. w-1, with p the row at which original row q_s stands after the interchanges 0 .. s-1,
 *   d_ipiv[j0+s] = p + 1 + ipiv_offset, and rows j0+s and p are exchanged in ALL columns of the panel.
 * Factorization: the sub-panel is then factored WITHOUT pivoting in mpf_dgetf2_npv's arithmetic (contract C3), honouring `fused`:
 *   the multiplier is a_ij / a_jj, each element is updated once per k in ascending order; the columns right of it follow as in
 *   mpf_dgetf2_piv.
 * Bit contract (mpf_dgetf2_piv's): the factored panel equals, bit for bit, mpf_dgetf2_npv applied to the panel with its rows
 * pre-permuted by the returned pivots.  info: the first zero diagonal entry the no-pivot factorization met, 1-based, or 0.
 * Consequences: the pivots of A 2^k are those of A; where rows - j0 <= 256 at every sub-panel (e.g. rows <= 256) pivots and bits are
 * mpf_dgetf2_piv's; |l_ij| <= 1 is NOT promised (growth as in every communication-avoiding LU: in practice as stable as partial pivoting).
 * Launches per sub-panel: 1 + ceil(log8(ceil((rows - j0) / 256))) selections (at most 4 up to 1 M rows), then the interchange, the
 * factorization, the U row-block and the update -- all ordinary launches, no kernel waits for another workgroup (csrc/dpivot.hip). */
int mpf_dgetf2_tp(mpf_ctx *ctx, double *d_P, int64_t ld, int32_t rows, int32_t cols, int32_t fused,
                  int32_t ipiv_offset, int32_t *d_ipiv, int32_t *info /* host, optional */);
/* cublasDtrsm(LEFT, LOWER, N, UNIT, m, n, 1.0, L, ldl, B, ldb), call site MPF.cu:215-225. */
int mpf_dtrsm_llnu(mpf_ctx *ctx, int32_t m, int64_t n, const double *d_L, int64_t ldl, double *d_B,
                   int64_t ldb);
/* cublasDgemm(N, N, m, n, k, -1.0, A, lda, B, ldb, 1.0, C, ldc), call site MPF.cu:230-239. */
int mpf_dgemm_minus(mpf_ctx *ctx, int64_t m, int64_t n, int32_t k, const double *d_A, int64_t lda,
                    const double *d_B, int64_t ldb, double *d_C, int64_t ldc);

/* Build-added speed mode of the same update (BASELINE north_star): C -= fp16(A) * fp16(B) with
 * v_mfma_f32_32x32x16_f16, fp32 accumulation over k, one fp64 subtraction per element. */
int mpf_hgemm_minus(mpf_ctx *ctx, int64_t m, int64_t n, int32_t k, const double *d_A, int64_t lda,
                    const double *d_B, int64_t ldb, double *d_C, int64_t ldc, int32_t split /* 0: fp16, 1: fp16x3 */);

/* The same update on an fp32 matrix: C (float, column-major) -= fp16(A) * fp16(B).  This is the operation the two-level
 * schedule of the fp16 trailing modes runs on its fp32 working copy of the trailing matrix (8 instead of 16 bytes of HBM per
 * updated element); exposed as a step operator so that it can be tested against the oracle's tolerance formula. */
int mpf_hgemm_minus_f32(mpf_ctx *ctx, int64_t m, int64_t n, int32_t k, const double *d_A, int64_t lda,
                        const double *d_B, int64_t ldb, float *d_C, int64_t ldc, int32_t split);

/* The fp32 working copy itself (row-major: element (i, j) at d_W[i * ldw + j]; the fp64 matrix is column-major), as step
 * operators: conversion of a rows x cols window in both directions, and LASWP_kernel's interchange (MPF.cu:42-59: `cols`
 * sequential swaps row k + pc <-> d_ipiv_global[pc] - 1) on ncols columns of the copy.  mpf_w32_laswp needs scratch of
 * 8 * N * max(cols, 256) bytes, which mpf_factor_dev allocates; stand-alone calls allocate it themselves. */
int mpf_w32_from_f64(mpf_ctx *ctx, const double *d_A, int64_t lda, float *d_W, int64_t ldw, int64_t rows, int64_t cols);
int mpf_w32_to_f64(mpf_ctx *ctx, const float *d_W, int64_t ldw, double *d_A, int64_t lda, int64_t rows, int64_t cols);
int mpf_w32_laswp(mpf_ctx *ctx, float *d_W, int64_t ldw, int64_t ncols, int32_t k, int32_t cols, const int32_t *d_ipiv_global);

/* ---- the reference generator's stream on the device (matrix_generator.cpp:55-80 as benchmark.cpp:192-194 reads it) ----
 * d_A[col * lda + row] = (rand() % 100) / 10.0 for t = col * N + row = 0 .. N^2-1 in order, rand() = glibc's default
 * generator, never seeded, after `skip` earlier draws (`matgen f N (N-2) lin` emits a 2 x 2 first: skip = 4).  Bit-identical
 * to the reference binary's file as benchmark.cpp parses it; no host-side N^2 work.  Synchronous.
 * _cols_: only columns [col0, col0 + ncols) of that N x N matrix, written to d_A's columns 0 .. ncols-1 (1-D block-column
 * layouts generate their own blocks).  mpf_matgen_state: host-only check of the jump-ahead (31 raw words in front of
 * rand() call number `call`). */
int mpf_matgen_dev(mpf_ctx *ctx, double *d_A, int64_t lda, int64_t N, int64_t skip);
int mpf_matgen_cols_dev(mpf_ctx *ctx, double *d_A, int64_t lda, int64_t N, int64_t skip, int64_t col0, int64_t ncols);
int mpf_matgen_state(int64_t call, uint32_t *out31);

/* ---- the reference's acceptance test at scale (benchmark.cpp:106-144: get_LU, L * U, row_permute, |A - P L U| <= 1e-10) ----
 * The reference multiplies L * U on the host with CBLAS (benchmark.cpp:77-82): 7e13 flops at N = 32768.  Here P^T A - L U is
 * formed on the device with the library's fp64 MFMA GEMM.  max_abs_err is the reference's criterion (compare with 1e-10),
 * fro_rel_err = ||A - P L U||_F / ||A||_F.  Needs 3 N^2 doubles of device scratch.  _host: host buffers (ld = N), device 0. */
int mpf_check_plu_dev(mpf_ctx *ctx, const double *d_A, int64_t lda, const double *d_LU, int64_t ldlu, const int32_t *d_ipiv,
                      int64_t N, double *max_abs_err, double *fro_rel_err);
int mpf_check_plu_host(const double *A, const double *LU, const int32_t *ipiv, int64_t N, double *max_abs_err, double *fro_rel_err);

/* ---- build-added solve (no reference counterpart; BASELINE north_star) -------------------- */
typedef struct mpf_ir_stats {
    int32_t iterations;   /* correction steps taken */
    int32_t converged;
    double rel_residual;  /* ||b - A x||_2 / ||b||_2 at exit */
    double history[32];   /* residual after step i (history[0] = after the first solve) */
    double ms_total;
    int32_t stalled;      /* 1: stopped early because the residual stopped shrinking (ratio > 0.7 twice in a row) */
    int32_t reserved;
} mpf_ir_stats;
/* Solve A x = b with the factors produced by mpf_factor_dev and fp64 iterative refinement:
 * x0 = U^-1 L^-1 P b; repeat r = b - A x (fp64), x += U^-1 L^-1 P r until
 * ||r||/||b|| <= tol or max_iter corrections.  d_A is the ORIGINAL matrix, d_LU the factors. */
int mpf_solve_ir(mpf_ctx *ctx, const double *d_A, int64_t lda, const double *d_LU, int64_t ldlu,
                 const int32_t *d_ipiv, int64_t N, const double *d_b, double *d_x, int32_t max_iter,
                 double tol, mpf_ir_stats *stats);

/* The same for nrhs right-hand sides: d_B / d_X are N x nrhs column-major (ldb, ldx >= N); stats = array of nrhs entries (or NULL).
 * The factors' diagonal-block inverses and the pivot gather index are prepared once. */
int mpf_solve_ir_nrhs(mpf_ctx *ctx, const double *d_A, int64_t lda, const double *d_LU, int64_t ldlu, const int32_t *d_ipiv,
                      int64_t N, int32_t nrhs, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t max_iter,
                      double tol, mpf_ir_stats *stats);

/* GMRES-IR (Carson & Higham): refinement whose correction equation A d = r is solved by GMRES (restart `restart`, <= 100)
 * preconditioned with the factors, everything in fp64.  Converges where plain refinement does not contract -- the
 * generator's own matrices with MPF_TRAIL_FP16 factors -- at the price of one factor solve + one matrix-vector product per
 * inner iteration.  history[i] = ||b - A x|| / ||b|| before outer step i. */
typedef struct mpf_gmres_stats {
    int32_t outer_iterations, inner_iterations, converged;
    int32_t budget_expired;   /* 1: stopped by the wall-clock limit mpf_gesv gives it (the estimated time of an fp64 refactorization) */
    double rel_residual;
    double history[32];
    double ms_total;
} mpf_gmres_stats;
int mpf_solve_gmres_ir(mpf_ctx *ctx, const double *d_A, int64_t lda, const double *d_LU, int64_t ldlu, const int32_t *d_ipiv,
                       int64_t N, const double *d_b, double *d_x, int32_t max_outer, int32_t restart, double tol,
                       mpf_gmres_stats *stats);

/* Solve A x = b end to end with the fastest path that reaches the tolerance: (1) factor a copy of A in the fp16
 * trailing mode and refine in fp64; (2) if the refinement stalls or diverges (ill-conditioned input: kappa * 2^-11
 * is not << 1), factor again with the fp64 trailing update (the reference arithmetic) and solve with that.
 * d_A is preserved; d_work is an N x N fp64 scratch (ld = N) that holds the factors on return; d_ipiv N int32. */
typedef struct mpf_gesv_stats {
    int32_t path;            /* 1: fp16 trailing + refinement, 2: fp64 fallback, 3: fp16 trailing + GMRES-IR */
    int32_t info;
    double ms_factor_fp16, ms_ir_fp16, ms_factor_fp64, ms_ir_fp64, ms_total;
    mpf_ir_stats ir_fp16, ir_final;
    double gmres_budget_ms;  /* try_fp16 = 3: the wall-clock limit GMRES-IR ran under (0: it did not run) */
    int32_t gmres_budget_expired, reserved;
} mpf_gesv_stats;
int mpf_gesv(mpf_ctx *ctx, const double *d_A, int64_t lda, int64_t N, int32_t nb, double *d_work, int32_t *d_ipiv,
             const double *d_b, double *d_x, int32_t max_iter, double tol,
             int32_t try_fp16 /* 0: fp64 only, 1: fp16, 2: fp16x3, 3: fp16 and, if plain refinement stalls, GMRES-IR on the same factors --
                                  for at most the time an fp64 refactorization is estimated to take (from this context's last measured
                                  fp64 factorization rate, option gesv_fp64_tflops to override), then the fp64 path;
                                  GMRES-IR with the caller's own limits: mpf_solve_gmres_ir */,
             mpf_gesv_stats *stats);

/* ---- expert solve driver (build extension; LAPACK dgetrs('T') / dlange / dgeequ / dgecon / dgesvx analogues) ----------------
 * Every reduction below has one fixed order (no floating-point atomics): a second call on the same data returns the same bits. */

/* mpf_solve_ir_nrhs for A^T X = B: the factors of A (P A = L U, from mpf_factor_dev) give x0 = P^T L^-T U^-T b through
 * U^T w = b (forward), L^T z = w (backward), x[perm[i]] = z[i]; refinement takes r = b - A^T x in fp64 and stops, stalls and
 * diverges by the rules of the plain solve.  Same arguments, stats per right-hand side.  Synchronises; -4 as the plain solve. */
int mpf_solve_ir_trans(mpf_ctx *ctx, const double *d_A, int64_t lda, const double *d_LU, int64_t ldlu, const int32_t *d_ipiv,
                       int64_t N, int32_t nrhs, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t max_iter,
                       double tol, mpf_ir_stats *stats);

/* LAPACK dlange of the M x N matrix d_A: norm '1' / 'O' max column abs sum, 'I' max row abs sum, 'M' max |a_ij|, 'F' Frobenius
 * (ordered sum of squares, then sqrt: no rescaling, so entries beyond ~1e154 overflow -- out of scope).  *out on the host;
 * synchronises. */
int mpf_lange(mpf_ctx *ctx, const double *d_A, int64_t lda, int64_t M, int64_t N, char norm, double *out);

/* Equilibration factors of the N x N matrix d_A as LAPACK dgeequb computes them, powers of two so that scaling is exact:
 *   r_i = 2^-floor(log2 max_j |a_ij|),  c_j = 2^-floor(log2 max_i |a_ij| r_i)   (exponents clamped to [-1022, 1022]);
 * rowcnd / colcnd / amax as dgeequ: rowcnd = max(min_i m_i, smlnum) / min(max_i m_i, bignum) over the row maxima m_i (colcnd
 * the same over the scaled column maxima), amax = max |a_ij|; smlnum = DBL_MIN, bignum = 1 / smlnum.  d_r, d_c: N doubles each
 * on the device.  Returns 0; i + 1 when row i (0-based) is zero (then d_c, colcnd are not set); N + j + 1 when column j is.
 * Synchronises. */
int mpf_geequ(mpf_ctx *ctx, const double *d_A, int64_t lda, int64_t N, double *d_r, double *d_c, double *rowcnd, double *colcnd,
              double *amax);

/* Reciprocal condition number of the factored matrix, as LAPACK dgecon: ||(L U)^-1|| is estimated by dlacn2 (Hager / Higham,
 * ITMAX = 5) on the device's triangular solves (no P, which changes neither norm): norm '1' / 'O': its B-products are L-then-U
 * solves, its B^T-products U^T-then-L^T solves; 'I': the two swapped.  rcond = 1 / (anorm * ainvnm), anorm = the same norm of
 * the matrix (mpf_lange).  rcond = 0 without a NaN when anorm == 0, when U has a zero diagonal entry (checked before any solve)
 * or when the estimate is not finite.  Synchronises; -4 as the solves. */
typedef struct mpf_gecon_stats {
    int32_t solves;       /* L-then-U solves (A^-1 products) */
    int32_t solves_t;     /* U^T-then-L^T solves (A^-T products) */
    int32_t iterations;   /* dlacn2's iteration count (2 .. 5; 1 for N = 1) */
    int32_t reserved;
    double ainvnm;        /* the estimate of ||(L U)^-1|| */
    double ms_total;
} mpf_gecon_stats;
int mpf_gecon(mpf_ctx *ctx, const double *d_LU, int64_t ldlu, int64_t N, char norm, double anorm, double *rcond,
              mpf_gecon_stats *stats);

/* Expert driver (LAPACK dgesvx's shape, one right-hand side): solve A x = b (trans = 0) or A^T x = b (trans = 1).
 *   1. equilibrate: 0 never; 1 by dlaqge's rule (rows if rowcnd < 0.1 or amax outside [smlnum, bignum], smlnum = DBL_MIN / 2^-52;
 *      columns if colcnd < 0.1); 2 always; nothing when mpf_geequ reports a zero row or column.  d_work = Dr A Dc (ld = N).
 *      In the low-precision modes an equilibrated matrix gets one more global power of two, folded into Dr (equed then includes
 *      rows), so that max |Dr A Dc| lies in [2^13, 2^14): the fp16 operands saturate at 65504 and go subnormal below 2^-14.
 *      (With option pivot_fp64 the pivots are searched in fp64, but this step stays: the update operands of these modes are still fp16.)
 *   2. factor d_work in the mode try_fp16 asks for (0: fp64, 1: fp16, 2: fp16x3), 3. mpf_gecon on those factors (norm '1',
 *      'I' for trans = 1), 4. if 1 / rcond > kappa_max (0: 1e4 for fp16, 1e6 for fp16x3) factor again in fp64 at once;
 *   5. otherwise refine against the ORIGINAL A: r = b - A x (or b - A^T x) in fp64, correction Dc (L U)^-1 P (Dr r) (trans = 1:
 *      Dr P^T (L U)^-T (Dc r)), with mpf_solve_ir's stop / stall rules; 6. not converged: fp64 factors of the same equilibrated
 *      matrix, refined the same way.
 * d_A is preserved; d_work (N x N) holds the factors used on return, d_ipiv (N int32) their pivots; d_r / d_c (N doubles each,
 * optional) receive the scale factors (valid where equed says they were applied).  Returns 0 when the answer converged, 1 when
 * not, < 0 on error.  Synchronises. */
typedef struct mpf_gesvx_stats {
    int32_t path;             /* 1: low-precision factors + refinement, 2: fp64 factors */
    int32_t info;             /* first zero pivot of the last factorization (1-based) or 0 */
    int32_t equed;            /* 0 none, 1 rows, 2 columns, 3 both */
    int32_t skipped_by_rcond; /* 1: the low-precision factors' rcond sent the solve to fp64 without refining */
    double rowcnd, colcnd, amax;   /* mpf_geequ's (0 when equilibrate = 0) */
    double anorm;             /* norm of the equilibrated matrix gecon used */
    double kappa_max;         /* the threshold applied */
    double rcond_lowp;        /* rcond of the low-precision factors (0: none) */
    double rcond;             /* rcond of the factors the answer was refined with */
    double ms_equilibrate, ms_factor, ms_gecon, ms_ir, ms_total;
    mpf_ir_stats ir_lowp, ir_final;
} mpf_gesvx_stats;
int mpf_gesvx(mpf_ctx *ctx, const double *d_A, int64_t lda, int64_t N, int32_t nb, double *d_work, int32_t *d_ipiv,
              const double *d_b, double *d_x, int32_t trans, int32_t equilibrate, int32_t try_fp16, double kappa_max,
              int32_t max_iter, double tol, double *d_r, double *d_c, mpf_gesvx_stats *stats);

/* ---- blocked multi-right-hand-side solve (build extension; LAPACK dgetrs and block refinement) -----------------------------
 * The right-hand sides go through the device in tiles of 32 columns: every triangular step reads its factor block once per tile
 * (several tiles in one launch) and every residual reads A once per tile, on fp64 MFMA.  Each column's arithmetic has one fixed
 * order and reads no other column: X[:, j] (and its stats) has the same bits whatever the other columns, nrhs or j's position,
 * and two calls return the same bits.  The bits differ from the per-column solves' (another summation order). */

/* LAPACK dgetrs: B := A^-1 B (trans = 0) or A^-T B (trans = 1), in place, with the factors of mpf_factor_dev
 * (P A = L U).  d_B is N x nrhs column-major, ldb >= N; rows N .. ldb-1 are not touched.  nrhs = 0: returns 0, no work.
 * Synchronises; -4 when a bounded wait of the step kernel gave up (as the other solves). */
int mpf_getrs(mpf_ctx *ctx, int32_t trans, const double *d_LU, int64_t ldlu, const int32_t *d_ipiv, int64_t N,
              int32_t nrhs, double *d_B, int64_t ldb);

/* Refinement of all nrhs columns together: the same per-column rules and stats as mpf_solve_ir_nrhs / _trans.
 * x0 = getrs(b); r = b - op(A) x in fp64; stop at ||r||/||b|| <= tol, at max_iter, on NaN, or on the stall rule.
 * The residual, the corrections and the norms are computed for a whole tile of columns per pass over A and over the factors.
 * A column that has stopped gets no further correction.  stats: nrhs entries (or NULL); ms_total is the wall time of the whole
 * call and the same for every column.  Synchronises. */
int mpf_solve_ir_block(mpf_ctx *ctx, int32_t trans, const double *d_A, int64_t lda, const double *d_LU, int64_t ldlu,
                       const int32_t *d_ipiv, int64_t N, int32_t nrhs, const double *d_B, int64_t ldb, double *d_X,
                       int64_t ldx, int32_t max_iter, double tol, mpf_ir_stats *stats);

/* GMRES-IR for all nrhs columns together, op(A) X = B with op(A) = A (trans = 0) or A^T (trans = 1): mpf_solve_gmres_ir's method on the
 * tiles of the blocked solve, for factors on which classical refinement does not contract.  Per column, with M^-1 = getrs on the factors:
 *   nb2 = ||b||_2 (0 reads 1); x = M^-1 b; outer step 0, 1, ...: r = b - op(A) x in fp64, rel = ||r||_2 / nb2, history[outer] = rel;
 *   stop converged at rel <= tol, stop not converged at max_outer steps or on a NaN; z = M^-1 r, beta = ||z||_2 (0 or NaN: stop),
 *   v_0 = z / beta, inner tolerance max(1e-14, min(1e-2, 0.1 tol / rel)); inner step k < restart: w = M^-1 op(A) v_k, orthogonalised
 *   against v_0 .. v_k by CLASSICAL Gram-Schmidt applied TWICE (h = V^T w, w -= V h, h' = V^T w, w -= V h', H[0..k, k] = h + h',
 *   H[k+1, k] = ||w||_2), Givens rotations on the host as mpf_solve_gmres_ir; the inner loop ends when the rotated residual is at
 *   most inner tolerance x beta or ||w|| = 0; then x += V y.
 * restart and max_outer are clamped as mpf_solve_gmres_ir clamps them (restart < 1: 30, at most 100; max_outer 1 .. 31).
 * The columns of a group (option gmres_group_tiles) take every outer and every inner step together -- one pass over A and one over
 * the factors per product for the whole group, one orthogonalisation of three sweeps over the basis and ONE host read-back per inner
 * step whatever k is; a column whose inner loop has ended is frozen until the group's longest one ends.  Every sum has one fixed
 * order and no column reads another: X[:, j] and its stats (but ms_total) have the same bits whatever the other columns, nrhs, j's
 * position or the group width, and two calls return the same bits.  They are NOT the bits of mpf_solve_gmres_ir, which
 * orthogonalises by modified Gram-Schmidt and sums in another order (as mpf_solve_ir_block's are not those of the per-column solves).
 * d_B is preserved; rows N .. ldx-1 of d_X are not touched.  stats: nrhs host entries or NULL; budget_expired stays 0 (there is no
 * wall-clock limit: a column's bits would depend on timing); ms_total is the wall time of the whole call, the same for every column.
 * Returns 0 when every column converged, 1 when some column did not (the stats say which), < 0 on error.  nrhs = 0: returns 0, no
 * work.  Synchronises; -4 as the other solves. */
int mpf_solve_gmres_ir_block(mpf_ctx *ctx, int32_t trans, const double *d_A, int64_t lda, const double *d_LU, int64_t ldlu,
                             const int32_t *d_ipiv, int64_t N, int32_t nrhs, const double *d_B, int64_t ldb, double *d_X, int64_t ldx,
                             int32_t max_outer, int32_t restart, double tol, mpf_gmres_stats *stats /* nrhs host entries or NULL */);

/* ---- error bounds for solves (build extension; LAPACK dgerfs on the tiles of the blocked solve) -----------------------------------
 * Refines a solution of op(A) X = B in place and returns, per column, the componentwise backward error berr and a bound ferr on
 * max_i |x_i - xtrue_i| / max_i |x_i|.  d_X holds a solution on entry (from the blocked solve above, for example); ferr and berr are
 * HOST arrays of nrhs doubles; stats: nrhs host entries or NULL.  itmax = 0 means LAPACK's 5; larger values are clamped to 31 (fp16
 * factors can need more than 5 corrections).  The arithmetic is dgerfs's, column by column, with eps = 2^-53, safmin = DBL_MIN,
 * nz = N + 1, safe1 = nz safmin, safe2 = safe1 / eps:
 *   r = b - op(A) x, w = |b| + |op(A)| |x| (ONE pass over op(A) for both, on fp64 MFMA);
 *   berr = max_i (w_i > safe2 ? |r_i| / w_i : (|r_i| + safe1) / (w_i + safe1));
 *   while berr > eps, 2 berr <= the previous berr (3 at first) and fewer than itmax corrections: x += op(A)^-1 r, again; a NaN berr
 *   stops the column and is returned;
 *   w_i <- |r_i| + nz eps w_i (+ safe1 where w_i was <= safe2); est = dlacn2's estimate of || op(A)^-1 diag(w) ||_inf;
 *   ferr = est / max_i |x_i| (est when that is 0).
 * All columns of a group run the refinement and dlacn2 in lock-step: every product is one pass over the factors for the group, a
 * column that has stopped is frozen.  Every sum has one fixed order: X[:, j], ferr[j], berr[j], iterations and lacn2_iterations
 * have the same bits whatever the other columns, nrhs or j's position, and two calls return the same bits.
 * nrhs = 0: returns 0, no work.  Rows N .. ld - 1 of d_X are not touched.  Synchronises; -4 as the other solves. */
typedef struct mpf_gerfs_stats {
    int32_t iterations;        /* corrections this column received (0 .. itmax) */
    int32_t lacn2_iterations;  /* dlacn2's count for this column (2 .. 5; 1 for N = 1) */
    int32_t solves;            /* tile solves (op(A)^-1 or op(A)^-T passes) the column's group went through */
    int32_t reserved;
    double ms_total;           /* wall time of the whole call, the same for every column */
} mpf_gerfs_stats;
int mpf_gerfs(mpf_ctx *ctx, int32_t trans, const double *d_A, int64_t lda, const double *d_LU, int64_t ldlu,
              const int32_t *d_ipiv, int64_t N, int32_t nrhs, const double *d_B, int64_t ldb, double *d_X, int64_t ldx,
              int32_t itmax, double *ferr, double *berr, mpf_gerfs_stats *stats);

/* ---- extra-precise refinement (build extension; LAPACK dgerfsx / dla_gerfsx_extended with the XBLAS residual) ---------------------
 * Every other solve here takes its residual from an fp64 MFMA product, so it stops at a forward error of about kappa(A) 2^-53.  These
 * two entry points add the precision above fp64: the residual is accumulated in twice the working precision, and refinement is
 * steered by the size of the corrections, not of the residual.
 *
 * mpf_residual_x, the step operator: R = B - op(A) X (op(A) = A or A^T), all matrices column-major on the device (lda, ldx, ldb,
 * ldr >= N).  Every element is accumulated as an unevaluated pair (hi, lo) from (b, 0): for each k, p = a x, e = fma(a, x, -p) (the
 * product's exact error), (hi, t) = TwoSum(hi, -p) (Knuth's six operations), lo += t - e; partials of 4096 columns of op(A) are pairs
 * and are added by the same pair addition in ascending order; the element returned is hi + lo, rounded once.  Its error is at most
 * 2^-53 |r| + about (N + 1)^2 2^-106 (|b| + |op(A)| |x|)_i.  A non-finite operand makes that element NaN or +-Inf.  One fixed order per
 * element, the same for every column: R[:, j] has the same bits whatever stands beside it, and two calls return the same bits.
 * This is fp64 VALU work, about ten instructions per product: several times the cost of the MFMA residual.
 * Rows N .. ldr - 1 of d_R are not touched.  nrhs = 0: returns 0, no work.  Synchronises. */
int mpf_residual_x(mpf_ctx *ctx, int32_t trans, const double *d_A, int64_t lda, int64_t N, int32_t nrhs,
                   const double *d_X, int64_t ldx, const double *d_B, int64_t ldb, double *d_R, int64_t ldr);

/* mpf_gerfsx: refines a solution X of op(A) X = B in place (X as mpf_gerfs takes it) and returns, per column, a normwise and a
 * componentwise forward error bound without a dlacn2 run.  err_norm and err_comp are HOST arrays of nrhs doubles, both required;
 * stats: nrhs host entries or NULL.  ithresh = 0 means LAPACK's 10; larger values are clamped to 31.
 * The rule is dla_gerfsx_extended's with the residual precision fixed at "extra" (where LAPACK would raise the precision, the state
 * becomes NOPROG instead).  eps = 2^-53, rthresh = 0.5, dz_ub = 0.25, HUGE = DBL_MAX.  Per column: x_state = WORKING, z_state =
 * UNSTABLE, dxratmax = dzratmax = 0, final_dx_x = final_dz_z = prev_dx = prev_dz = HUGE.  Iteration cnt = 0, 1, .. < ithresh:
 *   r = b - op(A) x as mpf_residual_x forms it; d = op(A)^-1 r on the factors;
 *   normx = max_i |x_i|, normdx = max_i |d_i|, dz = max_i |d_i| / |x_i| (HUGE where x_i = 0 != d_i, 0 where both are 0);
 *   a NaN among the three, or an infinite normx or normdx: x_state = NAN, stop;
 *   dx_x = normdx / normx (normx = 0: 0 if normdx = 0, else HUGE); dxrat = normdx / prev_dx; dzrat = dz / prev_dz;
 *   x_state NOPROG and dxrat <= rthresh: WORKING again;
 *   x_state WORKING: dx_x <= eps: CONV; else dxrat > rthresh: NOPROG; else dxratmax = max(dxratmax, dxrat); on leaving WORKING
 *     final_dx_x = dx_x;
 *   z_state UNSTABLE and dz <= dz_ub: WORKING;  z_state NOPROG and dzrat <= rthresh: WORKING;
 *   z_state WORKING: dz <= eps: CONV; else dz > dz_ub: UNSTABLE, dzratmax = 0, final_dz_z = HUGE; else dzrat > rthresh: NOPROG; else
 *     dzratmax = max(dzratmax, dzrat); in NOPROG or CONV final_dz_z = dz;
 *   neither state WORKING: stop, and this iteration's d is NOT applied (as in LAPACK); else prev_dx = normdx, prev_dz = dz, x += d.
 * At the end a state still WORKING takes the last dx_x / dz as its final value, and
 *   err_norm = final_dx_x / (1 - dxratmax),  err_comp = final_dz_z / (1 - dzratmax),  both at least max(10, sqrt(N)) eps;
 * a column in state NAN returns +Inf for both.  err_norm bounds max_i |x_i - xtrue_i| / max_i |x_i|, err_comp bounds
 * max_i |x_i - xtrue_i| / |x_i|; err_comp means something where z_state ends CONV.
 * All columns of a group of 512 take every step together: one residual, one pass over the factors, one reduction launch with one
 * read-back and one masked update per step; a column that has stopped is frozen.  A column's arithmetic depends on nothing but its own
 * data: X[:, j], both bounds and the stats (but ms_total) have the same bits whatever the other columns, nrhs, j's position or the
 * group, and two calls return the same bits.
 * What it is not: it keeps no doubled-precision x (LAPACK's last escalation stage) and is not wired into mpf_gesvx_block or mpf_gesv;
 * berr and scale vectors are mpf_gerfsx_scaled's, the driver around both is mpf_gesvxx_block (below).
 * Returns 0 when every column ended with x_state = CONV, 1 otherwise (the stats say which), < 0 on error.  nrhs = 0: returns 0, no
 * work.  Rows N .. ldx - 1 of d_X are not touched; d_B is preserved.  Synchronises; -4 as the other solves. */
typedef struct mpf_gerfsx_stats {
    int32_t iterations;        /* corrections applied to this column (0 .. ithresh) */
    int32_t x_state;           /* 0 WORKING (ithresh reached), 1 NOPROG, 2 CONV, 3 NAN */
    int32_t z_state;           /* -1 UNSTABLE, 0 WORKING, 1 NOPROG, 2 CONV */
    int32_t solves;            /* tile solves that entered this column's decisions: iterations, + 1 when the last d was not applied */
    double final_dx_x, final_dz_z, dxratmax, dzratmax;
    double ms_total;           /* wall time of the whole call, the same for every column */
} mpf_gerfsx_stats;
int mpf_gerfsx(mpf_ctx *ctx, int32_t trans, const double *d_A, int64_t lda, const double *d_LU, int64_t ldlu,
               const int32_t *d_ipiv, int64_t N, int32_t nrhs, const double *d_B, int64_t ldb, double *d_X, int64_t ldx,
               int32_t ithresh, double *err_norm, double *err_comp, mpf_gerfsx_stats *stats);

/* ---- expert driver for many right-hand sides (build extension; mpf_gesvx's steps on the tiles of the blocked solve) -----------------
 * Solves op(A) X = B for nrhs columns with ONE factorization: steps 1 .. 4 are mpf_gesvx's, from the same code (equilibrate, factor
 * d_work in the mode try_fp16 asks for, rcond of those factors, the kappa_max gate).  They depend on A only: for the same A and
 * arguments path, equed, rcond, rcond_lowp, skipped_by_rcond, anorm, d_work and d_ipiv are mpf_gesvx's, bit for bit.
 *   5. All columns are refined together against the ORIGINAL A by mpf_solve_ir_block's per-column rules (max_iter, tol, the stall
 *      rule, stats), with the equilibrated factors as the preconditioner: op(A)^-1 v ~ Dc (L U)^-1 P (Dr v) (trans = 1:
 *      Dr P^T (L U)^-T (Dc v)).  The scale vectors ride on the tile loads and stores, so a solve costs what mpf_getrs costs.
 *   6. If ANY column has not converged on low-precision factors, the whole call goes to fp64 factors of the same equilibrated matrix
 *      and ALL columns are solved and refined again (path = 2).  A column's bits therefore depend only on A, on its own b and on
 *      the path the call took, not on which other columns converged; the price is that one hard column costs every column the
 *      fp64 path.
 *   7. With ferr and berr given (HOST arrays of nrhs doubles; both NULL: no bounds stage) mpf_gerfs's loop runs on the factors that
 *      produced the answer: X is refined further in place by dgerfs's rule (itmax as in mpf_gerfs: 0 means 5, clamped to 31) and
 *      berr, ferr are those of the ORIGINAL system for the returned X: the residual and the weights are taken on A, B, X as given,
 *      the corrections and dlacn2's products go through the scaled solves (the op(A)^-T product with the two scale vectors
 *      swapped).  This departs from LAPACK's dgesvx on purpose: LAPACK bounds the equilibrated system and divides ferr by colcnd
 *      or rowcnd.  Every scale factor here is an exact power of two, so the residual and the weights of the original system are
 *      the equilibrated ones times Dr^-1 without rounding: berr is the same number, and the direct ferr bounds the error of the X
 *      the caller gets instead of a bound loosened by a condition number.
 * d_B (N x nrhs, ldb >= N) is preserved; d_X (ldx >= N) receives the solution, rows N .. ldx - 1 are not touched; d_A, d_work,
 * d_ipiv, d_r, d_c as mpf_gesvx.  stats: the call (path, equed, rcond, rcond_lowp, times; ir_lowp / ir_final: the column with the
 * largest final rel_residual of the respective attempt; ms_ir includes the bounds stage, whose own time is rfs[0].ms_total).
 * ir, rfs: nrhs host entries each of the attempt that produced X, or NULL.  A column has the same bits alone, among others and at
 * another position, within the same path.  Returns 0 when every column converged, 1 when some column did not (ir says which),
 * < 0 on error; nrhs = 0 returns 0 and does no work, not even the factorization.  Synchronises. */
int mpf_gesvx_block(mpf_ctx *ctx, const double *d_A, int64_t lda, int64_t N, int32_t nb, double *d_work, int32_t *d_ipiv,
                    int32_t nrhs, const double *d_B, int64_t ldb, double *d_X, int64_t ldx,
                    int32_t trans, int32_t equilibrate, int32_t try_fp16, double kappa_max, int32_t max_iter, double tol,
                    int32_t itmax, double *d_r, double *d_c,
                    double *ferr, double *berr,             /* host, nrhs each; both NULL: no bounds stage */
                    mpf_gesvx_stats *stats,                 /* the call: path, equed, rcond, rcond_lowp, times */
                    mpf_ir_stats *ir, mpf_gerfs_stats *rfs  /* host, nrhs each, optional */);

/* ---- extra-precise expert solve (build extension; LAPACK dgesvxx's driver, dla_gerpvgrw and dgerfsx on equilibrated factors) ---------
 * Three entry points; the third is a composition of public operators, so that it can be compared bit for bit with them. */

/* Reciprocal pivot growth, LAPACK dla_gerpvgrw: d_LU (N x N, ldlu >= N) holds the factors of Dr A Dc, d_r / d_c (device, N doubles each,
 * optional) the diagonals of Dr / Dc; NULL means the identity.  Per column j
 *   amax_j = max_i (|a_ij| r_i) c_j,   umax_j = max_{i <= j} |u_ij|,
 *   *rpvgrw = min(1, min over the j with umax_j != 0 of amax_j / umax_j)          (the initial value 1 is LAPACK's).
 * A value well below 1 says that the factorization grew: the default pivot rule takes its pivots from an fp16 image and
 * pivot_search = 2 does not promise |l_ij| <= 1, so neither bounds the growth by itself.  A NaN in A's or U's part of a column makes the
 * result NaN.  Maxima have no order to fix and the quotient is one division: the result equals the formula above evaluated in fp64 in
 * any order, and two calls return the same bits.  One pass over A and half a pass over LU: 8 N^2 + 4 N (N + 1) bytes (12.9 GB at
 * N = 32768), each column read once, coalesced.  *rpvgrw on the host.  Returns 0, < 0 on error.  Synchronises. */
int mpf_gerpvgrw(mpf_ctx *ctx, const double *d_A, int64_t lda, const double *d_LU, int64_t ldlu, int64_t N,
                 const double *d_r, const double *d_c /* device, N each, optional */, double *rpvgrw /* host */);

/* mpf_gerfsx on the factors of an equilibrated copy, with berr.  d_LU / d_ipiv are the factors of Dr A Dc (d_r, d_c: device, N doubles
 * each, exact powers of two as mpf_geequ returns them; NULL: the identity).  The rule, the three measures and the residual are
 * mpf_gerfsx's, taken on the ORIGINAL A, B and X; only the correction changes:
 *   d = Dc (L U)^-1 P Dr r      (trans = 1:  d = Dr P^T (L U)^-T Dc r),
 * the scale vectors riding on the tile loads and stores of the solve as in mpf_gesvx_block, so a correction costs what mpf_getrs costs.
 * err_norm and err_comp (host, nrhs each, required) therefore bound the error of the caller's X in the original system.
 * berr (host, nrhs doubles, optional): the componentwise backward error of the X that is returned, taken once after the loop:
 *   r = b - op(A) x as mpf_residual_x forms it (one more pair residual), w = |b| + |op(A)| |x| from mpf_gerfs's fp64 MFMA pass,
 *   berr = max_i (w_i > safe2 ? |r_i| / w_i : (|r_i| + safe1) / (w_i + safe1)),  safe1 = (N + 1) DBL_MIN, safe2 = safe1 / 2^-53
 * (mpf_gerfs's quotient and constants); a NaN is kept.  It is within (N + 2) 2^-53 relative + 8 (N + 1) 2^-106 of the exact quotient
 * (w is a sum of N + 1 non-negative terms; r has the pair residual's error).  The cost is one pair residual and one MFMA pass per group
 * of 512 columns, after the loop only; with berr NULL neither runs.
 * With d_r, d_c and berr all NULL the call returns mpf_gerfsx's bits in X, both bounds and the stats.  Column independence as
 * mpf_gerfsx: X[:, j], both bounds, berr[j] and the stats (but ms_total) have the same bits whatever stands beside column j and at any
 * position.  Return value, nrhs = 0, ithresh, stats and the untouched rows as mpf_gerfsx.  Synchronises; -4 as the other solves. */
int mpf_gerfsx_scaled(mpf_ctx *ctx, int32_t trans, const double *d_A, int64_t lda, const double *d_LU, int64_t ldlu,
                      const int32_t *d_ipiv, int64_t N, int32_t nrhs, const double *d_B, int64_t ldb, double *d_X, int64_t ldx,
                      int32_t ithresh, const double *d_r, const double *d_c,   /* device, optional: LU = factors of Dr A Dc */
                      double *err_norm, double *err_comp, double *berr /* host, nrhs, optional */, mpf_gerfsx_stats *stats);

/* The extra-precise expert driver for many right-hand sides (LAPACK dgesvxx's shape): mpf_gesvx_block with mpf_gerfsx's refinement and
 * bounds in place of dgerfs's, and the pivot growth.
 *   Steps 1 .. 4 are mpf_gesvx's / mpf_gesvx_block's, from the same code: equilibrate, factor d_work in the mode try_fp16 asks for
 *   (option pivot_fp64 applies as there), rcond of those factors, the kappa_max gate.  For the same A and arguments equed, rcond_lowp,
 *   skipped_by_rcond, anorm, the scale vectors and the low-precision factors are theirs, bit for bit.
 *   One attempt on the factors in d_work has two stages:
 *     (a) mpf_solve_ir_block's refinement (x0 from the factors, the fp64 MFMA residual, max_iter, tol, the stall rule), exactly as
 *         mpf_gesvx_block's step 5.  Its `converged` flags decide nothing here: the stage is a warm start that takes the cheap steps
 *         with the cheap residual (several times cheaper than the pair residual).
 *     (b) mpf_gerfsx_scaled's loop (ithresh, a fresh rule state, berr when asked) on that X, with the same scale vectors.
 *   The attempt stands iff EVERY column ends stage (b) with x_state = CONV.  A low-precision attempt that does not stand sends ALL
 *   columns to fp64 factors of the same equilibrated matrix (path = 2), for mpf_gesvx_block's reason: a column's bits depend on A, on
 *   its own b and on the path only.  There is no per-column fall-back.
 * With equilibrate = 0 and try_fp16 = 0 the call returns, bit for bit, mpf_factor_dev, then mpf_solve_ir_block, then mpf_gerfsx_scaled
 * with NULL scales; with scales the same holds with the driver's d_r / d_c and the factors it leaves in d_work.
 * err_norm, err_comp (host, nrhs each, required), berr (host, nrhs, optional): mpf_gerfsx_scaled's, of the ORIGINAL system and the
 * caller's X (the argument of mpf_gesvx_block's step 7 holds: the scale factors are exact powers of two).  rpvgrw (host, one double,
 * optional): mpf_gerpvgrw on A, the factors in d_work and the scales equed says were applied.  stats as mpf_gesvx_block's: ir_lowp /
 * ir_final hold the worst column of stage (a) of the respective attempt, ms_ir includes stage (b).  ir, xr (host, nrhs each, optional):
 * the per-column stats of stages (a) and (b) of the attempt that produced X; ir[j].ms_total is the attempt's time, xr[j].ms_total
 * stage (b)'s.  d_A, d_B, d_work, d_ipiv, d_r, d_c, the untouched rows of d_X and the argument checks as mpf_gesvx_block.
 * The measures are taken on the caller's x = post .* y (y: the equilibrated system's solution).  The blocked solves are stable normwise
 * in y, not per component, so with scale vectors spread over many orders of magnitude the loop contracts to 2^-53 where x's large
 * components are those with a large scale (a solution that follows the column scaling) and ends NOPROG, return value 1, where a
 * solution of uniform size meets such scales (measured: errors of 3 .. 16 x 2^-53 at a spread of 2^60).
 * What it is not: no Skeel condition numbers and no trust flags (dgesvxx's err_bnds(:, 1) and (:, 3)); no doubled-precision x (on a
 * host model of LAPACK's y_tail stage it changed no final state and no error by more than one ulp up to kappa = 3e15); no per-column
 * fall-back; not used by mpf_gesv or the distributed path.
 * Returns 0 when every column ended with x_state = CONV, 1 otherwise (xr says which), < 0 on error; nrhs = 0 returns 0 and does no
 * work, not even the factorization.  Synchronises. */
int mpf_gesvxx_block(mpf_ctx *ctx, const double *d_A, int64_t lda, int64_t N, int32_t nb, double *d_work, int32_t *d_ipiv,
                     int32_t nrhs, const double *d_B, int64_t ldb, double *d_X, int64_t ldx,
                     int32_t trans, int32_t equilibrate, int32_t try_fp16, double kappa_max, int32_t max_iter, double tol,
                     int32_t ithresh, double *d_r, double *d_c,
                     double *err_norm, double *err_comp,   /* host, nrhs each, required */
                     double *berr, double *rpvgrw,         /* host, nrhs / 1, optional */
                     mpf_gesvx_stats *stats, mpf_ir_stats *ir, mpf_gerfsx_stats *xr /* host, optional */);

/* ---- inverse and determinant from the factors (build extension; LAPACK dgetri, LINPACK dgedi's determinant) ---------------------------
 * Inverse: d_LU / d_ipiv are the factors P A' = L U of A' = Dr A Dc as mpf_factor_dev leaves them (d_r, d_c: device, N doubles each,
 * exact powers of two as mpf_geequ returns them; NULL: the identity).  d_inv (N x N column-major, ldinv >= N) receives
 *   inv(A) = Dc inv(A') Dr = Dc inv(U) inv(L) P Dr,
 * out of place: d_LU and d_ipiv are preserved, rows N .. ldinv - 1 of d_inv are not touched, and d_inv must not overlap d_LU (-1).
 * Any factors are accepted: on fp16 or fp16x3 factors the result is the inverse of the matrix those factors multiply to, no more
 * accurate than they are; the call does no refinement.
 * Algorithm: right-looking over d_inv itself in blocks of 256, about 4/3 N^3 flops as dgetri, the O(N^3) part on mpf_dgemm_minus's
 * fp64 MFMA kernel with K = 256 (no solve against an identity, no N x N workspace: the scratch is ceil(N / 256) 256^2 doubles beside
 * the solves' 256 x 256 block inverses).
 *   1. d_inv = I.  Block row k from the last one up: X(k, k:) = inv(U_kk) R(k, k:), then R(0:k, k:) -= U(0:k, k) X(k, k:): inv(U) in
 *      the upper triangle, N^3 / 3 flops, none on the zero triangle.
 *   2. X L = inv(U).  Block column j from the last one down: X(:, j) = R(:, j) inv(L_jj), then R(:, 0:j) -= X(:, j) L(j, 0:j): N^3 flops.
 *   3. dgetri's column interchanges (j = N - 2 .. 0: columns j and ipiv[j] - 1), composed into one permutation, and the scales
 *      x_ij <- (c_i x_ij) r_j in one pass.
 * Contract: every element has one fixed operation order (the block-inverse products: one accumulator from zero, k ascending; the
 * updates: mpf_dgemm_minus's chain); two calls return the same bits; the bits do not depend on ldlu or ldinv; with scales the result
 * equals (c_i y_ij) r_j bit for bit, Y the call without scales, as long as nothing over- or underflows.
 * Returns 0; i + 1 when u_ii is the first zero on U's diagonal -- checked before anything is written to d_inv, which is then left
 * untouched (dgetri's / dtrtri's rule; only the context's own solve scratch may have been allocated); < 0 on error.  N = 0: returns 0, no work.  Synchronises. */
int mpf_getri(mpf_ctx *ctx, const double *d_LU, int64_t ldlu, const int32_t *d_ipiv, int64_t N,
              const double *d_r, const double *d_c,   /* device, N each, optional: LU = factors of Dr A Dc */
              double *d_inv, int64_t ldinv);

/* Determinant of A from the same factors and scales: det(A) = *mant 2^*expo with |*mant| in [0.5, 1) or *mant = 0 (LINPACK's form: no
 * over- or underflow at any N).  One fixed order, every step exact but the products of two numbers in [0.5, 1):
 *   (m_i, e_i) = frexp(u_ii); with scales e_i is reduced by the exponents of r_i and c_i (log2 of a power of two);
 *   chunks of 256 consecutive i, ascending; inside a chunk from p = 1, e = 0:  p = p m_i, (p, k) = frexp(p), e += k + e_i;
 *   the chunk results are combined in ascending order from (1, 0) by the same step;
 *   the sign flips once per i with ipiv[i] != i + 1.
 * Any non-finite u_ii gives (NaN, 0); otherwise a zero u_ii gives (0, 0) and return value 0.  N = 0 gives (0.5, 1).  A restatement in
 * any IEEE arithmetic gives the same bits (tests/getri_model.py).  One launch, N loads.  *mant, *expo on the host.  Returns 0, < 0 on
 * error.  Synchronises. */
int mpf_getdet(mpf_ctx *ctx, const double *d_LU, int64_t ldlu, const int32_t *d_ipiv, int64_t N,
               const double *d_r, const double *d_c, double *mant, int64_t *expo /* host */);

/* ---- LU of many small matrices (build extension; LAPACK dgetrf / dgetrs per matrix of a strided batch) ---------------------------------
 * Every other entry point works on ONE matrix and is tuned for N >= 4096; these take `batch` matrices of one size n <= 128 in one
 * launch (csrc/batched.hip).  fp64 only, LAPACK partial pivoting: the fp16-image pivot rule and the fp16 trailing modes have no meaning
 * at these sizes.  No driver uses them; the inverse and the determinant from the factors are mpf_getri_batched and mpf_getdet_batched
 * below; matrices of different orders in one call: the mpf_*_vbatched entries after them; refinement, error bounds and rcond for these
 * batches: the mpf_*_batched expert entries after mpf_getdet_batched, and for one order up to 1024 the mpf_*_batched_blocked expert
 * entries after mpf_getdet_batched_blocked, and for a descriptor of different orders the mpf_*_vbatched expert entries after
 * mpf_getdet_vbatched.
 *
 * Layout: A[b] = d_A + b * strideA, n x n column-major, lda >= n, strideA >= lda * n (or batch == 1);
 * ipiv[b] = d_ipiv + b * strideP, strideP >= n (or batch == 1), 1-based as LAPACK; d_info: batch int32 on the device, optional.
 *
 * Factorization.  For every b, A[b] and ipiv[b][0 .. n-1] on return equal, bit for bit, what
 * mpf_dgetf2_piv(ctx, A[b], lda, n, n, fused, 0, ipiv[b], ...) leaves:
 *   idamax with a strict >, so the first maximum wins; a NaN never beats a number; a column whose remaining part is all zero or all
 *   NaN keeps p = j; the multiplier is a_ij / a_jj (IEEE division); each element is then updated once per k in ascending order, as a
 *   separate product and difference (fused = 0) or as one FMA (fused = 1; contract C3); all n pivot entries are written, so the last
 *   one is n; a zero pivot is divided by, as there (Inf / NaN follow); d_info[b] = the first zero pivot, 1-based, or 0.
 * Matrix b's bits do not depend on batch, on b's position, on lda, strideA or strideP, or on which kernel form took it (n <= 32: 8, 16
 * or 32 lanes of a wave per matrix, the matrix in registers; above: one workgroup per matrix, the matrix in LDS).  Rows n .. lda-1 and the bytes between
 * matrices are not touched.  Every launch is an ordinary launch: no kernel waits for another workgroup, no bounded spin, no
 * co-residency requirement.
 * Returns 0, or < 0 with a message: -1 for n > 128 (use mpf_factor_dev), negative sizes, lda < n, strides too small, NULL d_A or
 * d_ipiv.  n == 0 or batch == 0: returns 0, no work.  Per-matrix singularity is reported through d_info only.  Asynchronous on the
 * context's stream. */
int mpf_getrf_batched(mpf_ctx *ctx, double *d_A, int64_t lda, int64_t strideA, int32_t n, int64_t batch,
                      int32_t *d_ipiv, int64_t strideP, int32_t *d_info, int32_t fused);
/* B[b] = d_B + b * strideB, n x nrhs column-major, ldb >= n, strideB >= ldb * nrhs (or batch == 1):
 * B[b] := A[b]^-1 B[b] (trans = 0) or A[b]^-T B[b] (trans = 1), in place, with the factors and pivots mpf_getrf_batched leaves.
 * LAPACK dgetrs per matrix with ONE fixed order per element, always unfused (the product is rounded, then the difference):
 *   trans = 0: for j = 0 .. n-1 rows j and ipiv[j] - 1 of B change places; for i ascending b_i <- b_i - l_ij b_j, j = 0 .. i-1
 *              ascending; for i descending b_i <- b_i - u_ij b_j, j = n-1 down to i+1, then b_i <- b_i / u_ii.
 *   trans = 1: with U^T, for i ascending b_i <- b_i - u_ji b_j, j ascending, then b_i <- b_i / u_ii; with L^T, for i descending
 *              b_i <- b_i - l_ji b_j, j = n-1 down to i+1; then the interchanges in reverse order, j = n-1 .. 0.
 * Columns do not read each other, and matrix b's result depends on nothing but its own LU, ipiv and B (tests/batched_model.py restates
 * the chains).  No singularity check, as in dgetrs.  Rows n .. ldb-1 of B are not touched.
 * Returns 0, or < 0 with a message (n > 128, negative sizes, trans not 0 or 1, leading dimensions < n, strides too small, NULL
 * pointers).  n == 0, batch == 0 or nrhs == 0: returns 0, no work.  Asynchronous on the context's stream. */
int mpf_getrs_batched(mpf_ctx *ctx, int32_t trans, const double *d_LU, int64_t ldlu, int64_t strideLU, int32_t n, int64_t batch,
                      const int32_t *d_ipiv, int64_t strideP, int32_t nrhs, double *d_B, int64_t ldb, int64_t strideB);
/* inv[b] = d_inv + b * strideInv, n x n column-major, ldinv >= n, strideInv >= ldinv * n (or batch == 1):
 * inv[b] := A[b]^-1 from the factors and pivots mpf_getrf_batched leaves, out of place: d_LU and d_ipiv are preserved, rows
 * n .. ldinv-1 of every inv[b] and the bytes between matrices are not touched, and the address range of the d_inv batch must not
 * overlap that of the d_LU batch (-1; mpf_getri's rule).
 * Contract: for a matrix whose factors are finite and whose U has no zero on the diagonal, inv[b] equals, bit for bit, what
 * mpf_getrs_batched(trans = 0) returns for B[b] = I with the same factors (tests/batched_model.py: getrs_model(LU, ipiv, eye(n))).
 * Per element, column k
 *   starts as e_q, q the position row k reaches under the interchanges j = 0 .. n-1;
 *   then x_i <- x_i - l_ij x_j for j ascending;
 *   then for i descending x_i <- x_i - u_ij x_j, j = n-1 down to i+1, and x_i <- x_i / u_ii;
 * every step unfused (the product is rounded, then the difference).  No identity is formed or read.
 * Structural zeros: above and below its one the column holds +0 until forward step q, so a forward step j < q subtracts
 * l_ij (+0) = +-0 from +0, and +0 - (+-0) = +0 in round-to-nearest: a kernel form may skip those steps (rows above q stay +0) without
 * changing a bit, the signs of zeros included, as long as the factors are finite.  Nothing is skipped in the backward sweep.
 * (tests/batched_inv_model.py states the chain both ways and checks that they agree.)
 * Singular matrices: d_info[b] (optional, batch int32 on the device) = i + 1 for the first u_ii == 0.0, else 0; such a matrix leaves
 * inv[b] untouched (mpf_getri's and dgetri's rule), whether or not d_info is given.
 * Not promised: the values of a matrix's result when its factors are not finite.  Even then every access stays in range (an ipiv
 * entry outside 1 .. n reads as "no interchange", as in mpf_getrs_batched) and no other matrix is affected.  A matrix's bits depend on
 * nothing but its own LU and ipiv: not on batch, its position, any ld or stride, or the kernel form (n <= 32: 8, 16 or 32 lanes of a
 * wave per matrix, from registers; above: one workgroup per matrix, the factors in LDS).  Every launch is an ordinary launch.
 * Returns 0, or < 0 with a message (n > 128: use mpf_factor_dev and mpf_getri; negative sizes, leading dimensions < n, strides too
 * small, NULL d_LU, d_ipiv or d_inv, overlap).  n == 0 or batch == 0: returns 0, no work.  Asynchronous on the context's stream. */
int mpf_getri_batched(mpf_ctx *ctx, const double *d_LU, int64_t ldlu, int64_t strideLU, int32_t n, int64_t batch,
                      const int32_t *d_ipiv, int64_t strideP,
                      double *d_inv, int64_t ldinv, int64_t strideInv, int32_t *d_info /* optional */);
/* det(A[b]) = d_mant[b] 2^d_expo[b] from the same factors, |d_mant[b]| in [0.5, 1) or 0: mpf_getdet's order and special cases on
 * every matrix.  n <= 128 is a single chunk of that order: (m_i, e_i) = frexp(u_ii); from p = 1, e = 0, i ascending: p = p m_i,
 * (p, k) = frexp(p), e += k + e_i; the one combining step from (1, 0); the sign flips once per ipiv[i] != i + 1 -- the bits of
 * tests/getri_model.py: getdet_model(diag(U), ipiv).  Any non-finite u_ii gives (NaN, 0); otherwise a zero u_ii gives (0, 0).
 * d_expo is int32 (|expo| <= 128 * 1075).  No scale vectors: the batched factorization has no equilibration.  Reads n of the n^2
 * doubles of a matrix.
 * Returns 0, or < 0 with a message (as above; NULL d_mant or d_expo).  n == 0 or batch == 0: returns 0, no work, nothing written.
 * Asynchronous on the context's stream. */
int mpf_getdet_batched(mpf_ctx *ctx, const double *d_LU, int64_t ldlu, int64_t strideLU, int32_t n, int64_t batch,
                       const int32_t *d_ipiv, int64_t strideP,
                       double *d_mant, int32_t *d_expo /* device, batch each */);

/* ---- the expert layer for the same batches (build extension; csrc/batched_refine.hip) -----------------------------------------------------
 * A reciprocal condition number per matrix, dgerfs's refinement with berr and ferr per matrix and column, and the two step operators
 * they need, for strided batches of ONE order n <= 128.  The layout rules, argument checks, error style and asynchrony are
 * mpf_getrs_batched's: everything runs on the device in ordinary launches on the context's stream, nothing is read back, every result
 * is a device array.  n > 128 is refused with -1 (use mpf_gecon / mpf_gerfs on one matrix at a time); n == 0, batch == 0 or nrhs == 0
 * return 0 with no work; rows n .. ld-1 and the bytes between matrices are neither read nor written.
 *
 * THESE ARE NOT LAPACK'S ESTIMATES.  dgecon and dgerfs estimate || A^-1 || and || |op(A)^-1| g || with dlacn2, 4 to 11 single-vector
 * solves each.  At these sizes one such solve is bound by the latency of a 2 n-step chain, and all n columns of the inverse, side by
 * side, cost about as much.  So both quantities are computed EXACTLY: the kernels form the columns or rows of the inverse in registers
 * by the chains of mpf_getrs_batched / mpf_getri_batched, reduce them on the fly and never store them.  Both are true norms of the
 * computed inverse, not lower bounds: rcond is <= dgecon's (by a factor of at most about n) and ferr is >= dgerfs's.
 *
 * Shared rules (tests/batched_refine_model.py restates every entry in numpy, bit for bit):
 *   tree sum   every sum over a row or column index is a halving tree, + rounded once per step: the terms are padded to 128 with +0,
 *              then v = v[0..63] + v[64..127], v[0..31] + v[32..63], and so on down to one element.  Every term is >= +0, so the
 *              padding is exact and the result depends on neither n's padding nor the kernel form.
 *   maxima     order-free; a NaN among the terms gives NaN.
 *   fusion     every multiply-subtract and multiply-add is unfused: the product is rounded, then the sum or difference.
 *   constants  mpf_gerfs's: eps = 2^-53, safmin = DBL_MIN, nz = n + 1, safe1 = nz safmin, safe2 = safe1 / eps.
 * A matrix's (and a column's) results depend on nothing but its own data: not on batch, its position, nrhs, any ld or stride, or the
 * kernel form (n <= 8, 16, 32: that many lanes of a wave per matrix; above: one workgroup per matrix).  Non-finite data stays inside
 * its own matrix.  Two calls return the same bits.
 *
 * mpf_lange_batched: d_out[b] = '1' / 'O': max_j tree_i |a_ij|; 'I': max_i tree_j |a_ij|; 'M': max |a_ij|.  Any other letter: -1. */
int mpf_lange_batched(mpf_ctx *ctx, char norm, const double *d_A, int64_t lda, int64_t strideA, int32_t n, int64_t batch,
                      double *d_out /* device, batch */);
/* d_rcond[b] = (1 / ainvnm) / d_anorm[b] with ainvnm the norm of (L[b] U[b])^-1 from the packed factors; like mpf_gecon it takes no P.
 *   '1' / 'O': ainvnm = max_k tree_i |x_ik|, column k formed from e_k by the trans = 0 chains of mpf_getrs_batched without
 *              interchanges (as a set, mpf_getri_batched's columns for ipiv = 1 .. n);
 *   'I':       ainvnm = max_i tree_k |y_k|, y the trans = 1 chains from e_i without interchanges (row i of the same inverse).
 * A kernel may skip the forward steps before a chain's one, as mpf_getri_batched does (they meet zeros only; finite factors).
 * d_rcond[b] = 0, never NaN, when d_anorm[b] == 0, when U[b] has a zero on its diagonal (checked before any arithmetic; d_ainvnm[b]
 * is then +Inf) or when ainvnm is not finite (or 0, as mpf_gecon has it).  d_ainvnm (optional): ainvnm per matrix.  d_anorm: what mpf_lange_batched returns for
 * the same letter on the matrices that were factored. */
int mpf_gecon_batched(mpf_ctx *ctx, char norm, const double *d_LU, int64_t ldlu, int64_t strideLU, int32_t n, int64_t batch,
                      const double *d_anorm /* device, batch */, double *d_rcond /* device, batch */,
                      double *d_ainvnm /* optional: device, batch */);
/* The step operator.  R[b] = B[b] - op(A[b]) X[b] and, when d_W is given (R's layout: ldr, strideR), W[b] = |B[b]| + |op(A[b])| |X[b]|
 * (op(A) = A for trans = 0, A^T for trans = 1; X, B, R are n x nrhs as mpf_getrs_batched's B).  Per element, for j ascending:
 * r_i starts as b_i and has op(A)_ij x_j subtracted; w_i starts as |b_i| and has |op(A)_ij| |x_j| added.  One pass over A serves both.
 * d_R may be d_B (same layout); d_R and d_W must not overlap d_A or d_X. */
int mpf_residual_batched(mpf_ctx *ctx, int32_t trans, const double *d_A, int64_t lda, int64_t strideA, int32_t n, int64_t batch,
                         int32_t nrhs, const double *d_X, int64_t ldx, int64_t strideX, const double *d_B, int64_t ldb, int64_t strideB,
                         double *d_R, int64_t ldr, int64_t strideR, double *d_W /* optional */);
/* dgerfs per (matrix, column), exactly as mpf_gerfs's text above states it, with the factors and pivots mpf_getrf_batched leaves:
 * d_X holds a solution of op(A[b]) X[b] = B[b] on entry (from mpf_getrs_batched) and is refined in place.
 *   r and w are the step operator's; berr = max_i (w_i > safe2 ? |r_i| / w_i : (|r_i| + safe1) / (w_i + safe1));
 *   while berr > eps, 2 berr <= the previous berr (3 at first) and fewer than itmax corrections: x <- x + dx, dx = the chain of
 *   mpf_getrs_batched with the same trans applied to r.  itmax <= 0 means 5; larger values are clamped to 31.  A NaN berr stops the column and
 *   is returned.
 * With d_ferr given, from the last r and w: g_i = |r_i| + (nz eps) w_i, plus safe1 where w_i <= safe2; for every i,
 * f_i = tree_k |y_k| g_k with y what the chain of mpf_getrs_batched with the other trans (1 - trans) leaves for e_i, interchanges
 * included, so that y_k = (op(A)^-1)_ik; ferr = max_i f_i / max_i |x_i|, or the numerator alone when the denominator is 0.
 * Results per (matrix b, column c) at index b * nrhs + c of d_berr, d_ferr (optional) and d_iters (optional: the corrections made).
 * d_A, d_LU, d_ipiv and d_B are preserved; rows n .. ldx-1 of X are not touched.  Without d_ferr the call costs one residual per
 * column that is already converged; with it, n more chains per matrix (and per eight columns). */
int mpf_gerfs_batched(mpf_ctx *ctx, int32_t trans, const double *d_A, int64_t lda, int64_t strideA, const double *d_LU, int64_t ldlu,
                      int64_t strideLU, int32_t n, int64_t batch, const int32_t *d_ipiv, int64_t strideP, int32_t nrhs,
                      const double *d_B, int64_t ldb, int64_t strideB, double *d_X, int64_t ldx, int64_t strideX, int32_t itmax,
                      double *d_ferr /* optional */, double *d_berr, int32_t *d_iters /* optional */);

/* ---- the same for ONE order up to 1024 (blocked; csrc/batched_blocked.hip) ----------------------------------------------------------------
 * mpf_getrf_batched and mpf_getrs_batched above stop at n = 128, where a matrix still fits one workgroup's LDS, and stay as they are.
 * These take 0 <= n <= 1024 with the same layout, argument checks, error style and asynchrony, and mpf_getri_batched_blocked and
 * mpf_getdet_batched_blocked below do the same for mpf_getri_batched and mpf_getdet_batched; fp64 only, one n per call, no driver
 * uses them; refinement, error bounds and rcond above 128: the mpf_*_batched_blocked expert entries after mpf_getdet_batched_blocked.  Matrices of different orders up to 1024 in one call: a descriptor from mpf_vbatch_create_blocked
 * below (the descriptor from mpf_vbatch_create stays at n <= 128).
 *
 * Factorization.  mpf_getrf_batched's contract, word for word, with the larger limit: for every b, A[b], ipiv[b][0 .. n-1] and
 * d_info[b] equal, bit for bit, what mpf_dgetf2_piv(ctx, A[b], lda, n, n, fused, 0, ...) leaves; for n <= 128 that is also
 * mpf_getrf_batched's result.  The kernels are a right-looking blocked LU -- panel (mpf_dgetf2_piv's rule), the panel's interchanges
 * outside it, the U row block by forward substitution with k ascending, the trailing update with k ascending (fused = 1: a chain of
 * v_mfma_f64_16x16x4_f64, contract C5; fused = 0: a rounded product and a rounded difference) -- which applies to every element the
 * updates of contract C3 in their order, whatever the panel width (tests/batched_blocked_model.py restates the loop and checks it
 * against the unblocked model).  So a matrix's bits depend on nothing but the matrix and `fused`: not on batch, position, lda, the
 * strides, the panel width (option batched_blocked_nb: 8, 16, 32, or 0 = automatic) or the path (option batched_blocked_min_n,
 * default 129: smaller n are handed to mpf_getrf_batched; 0 sends every n through the blocked kernels).  Rows n .. lda-1 and the
 * bytes between matrices are neither written nor read.  Three ordinary launches per panel step for the whole batch: no kernel waits
 * for another workgroup, no bounded spin, no co-residency requirement.
 * Returns 0, or < 0 with a message: -1 for n > 1024 (use mpf_factor_dev), negative sizes, lda < n, strides too small, NULL d_A or
 * d_ipiv.  n == 0 or batch == 0: returns 0, no work, nothing written.  Asynchronous on the context's stream. */
int mpf_getrf_batched_blocked(mpf_ctx *ctx, double *d_A, int64_t lda, int64_t strideA, int32_t n, int64_t batch,
                              int32_t *d_ipiv, int64_t strideP, int32_t *d_info /* optional */, int32_t fused);
/* mpf_getrs_batched's chains, element orders and layout (above; tests/batched_model.py: getrs_model) for n <= 1024: always unfused,
 * trans = 0 or 1, in place on B, rows n .. ldb-1 untouched.  Columns do not read each other: a column solved alone gives the same
 * bits, as does any tiling of the columns.  n below option batched_blocked_min_n (and <= 128) is handed to mpf_getrs_batched.
 * Returns 0, or < 0 with a message (n > 1024: use mpf_factor_dev and mpf_getrs; the other cases as there).  n == 0, batch == 0 or
 * nrhs == 0: returns 0, no work.  Asynchronous on the context's stream. */
int mpf_getrs_batched_blocked(mpf_ctx *ctx, int32_t trans, const double *d_LU, int64_t ldlu, int64_t strideLU, int32_t n, int64_t batch,
                              const int32_t *d_ipiv, int64_t strideP, int32_t nrhs, double *d_B, int64_t ldb, int64_t strideB);
/* Inverse.  mpf_getri_batched's contract, word for word, with 0 <= n <= 1024: out of place (d_LU and d_ipiv are preserved; a d_inv
 * batch whose address range overlaps the d_LU batch's is refused with -1), rows n .. ldinv-1 and the bytes between matrices neither
 * written nor read.  For finite factors with no zero on U's diagonal inv[b] equals, bit for bit, mpf_getrs_batched_blocked(trans = 0)
 * on B[b] = I (tests/batched_model.py: getrs_model(LU, ipiv, eye(n))); for n <= 128 that is also mpf_getri_batched's result.  Every
 * step is unfused.  inv(A) = inv(U) inv(L) P: column k of the result is column q(k) of inv(L) -- q(k) the position row k reaches
 * under the interchanges -- taken through the backward sweep, so the interchanges are no arithmetic: the workgroup that forms
 * columns q .. q + ct - 1 of inv(L) stores them at columns k(q).  The forward sweep of a tile starts at the 32-row block that holds
 * its smallest q (the steps before it subtract l (+0) from +0: +0 - (+-0) = +0); rows above a column's q are stored as +0; nothing
 * is skipped in the backward sweep (tests/batched_blocked_inv_model.py restates the blocked algorithm).
 * d_info[b] = i + 1 for the first u_ii == 0.0, else 0; such a matrix's inv[b] is left untouched whether or not d_info is given
 * (every workgroup reads its matrix's diagonal before its first store; there is no workspace).  Non-finite factors: the values are
 * not promised, every access stays in range (an ipiv entry outside 1 .. n reads as "no interchange") and no other matrix changes.
 * A matrix's bits depend on nothing but its LU and ipiv: not on batch, position, any ld or stride, the tile width (option
 * batched_blocked_inv_ct: 8, 16, or 0 = automatic) or the path (n <= 128 and n < option batched_blocked_min_n: handed to
 * mpf_getri_batched).  One ordinary launch per 32768 matrices: no kernel waits for another workgroup.
 * Returns 0, or < 0 with a message: -1 for n > 1024 (use mpf_factor_dev and mpf_getri), negative sizes, ld < n, strides too small,
 * NULL d_LU, d_ipiv or d_inv, overlap.  n == 0 or batch == 0: returns 0, no work.  Asynchronous on the context's stream. */
int mpf_getri_batched_blocked(mpf_ctx *ctx, const double *d_LU, int64_t ldlu, int64_t strideLU, int32_t n, int64_t batch,
                              const int32_t *d_ipiv, int64_t strideP,
                              double *d_inv, int64_t ldinv, int64_t strideInv, int32_t *d_info /* optional */);
/* Determinant.  det(A[b]) = d_mant[b] * 2^d_expo[b] in mpf_getdet's order per matrix (no scales): for n <= 1024 up to four chunks of
 * 256 consecutive diagonal entries, each from (1, 0) ascending, the chunk results combined ascending from (1, 0) by the same step;
 * the sign flips once per ipiv[i] != i + 1 (tests/getri_model.py: getdet_model(diag(U), ipiv)) -- the bits of mpf_getdet on each
 * matrix and, for n <= 128, of mpf_getdet_batched.  Any non-finite u_ii gives (NaN, 0), otherwise a zero gives (0, 0).  d_expo is
 * int32 (|expo| <= 1024 * 1075).  Reads n of a matrix's n^2 doubles; one ordinary launch per 32768 matrices.  n <= 128 and n <
 * option batched_blocked_min_n: handed to mpf_getdet_batched.  n == 0 or batch == 0: returns 0 and writes nothing.  Errors as above
 * (n > 1024: use mpf_factor_dev and mpf_getdet). */
int mpf_getdet_batched_blocked(mpf_ctx *ctx, const double *d_LU, int64_t ldlu, int64_t strideLU, int32_t n, int64_t batch,
                               const int32_t *d_ipiv, int64_t strideP, double *d_mant, int32_t *d_expo);
/* The expert layer for ONE order up to 1024 (csrc/batched_refine_blocked.hip): mpf_lange_batched, mpf_gecon_batched,
 * mpf_residual_batched and mpf_gerfs_batched above with 0 <= n <= 1024 -- the argument lists word for word, the layout rules, checks,
 * error style and asynchrony of mpf_getrs_batched_blocked, the factors and pivots mpf_getrf_batched_blocked leaves.  Everything runs on
 * the device in ordinary launches on the context's stream, nothing is read back, no kernel waits for another workgroup and nothing
 * spins; rows n .. ld-1 and the bytes between matrices are neither read nor written; batches above 32768 go in chunks.
 * The contract is the small layer's with the larger limit (tests/batched_refine_blocked_model.py restates every entry in numpy):
 *   tree sum   the halving tree on the terms padded with +0 to 1024: v[0..511] + v[512..1023], then + 256, .. + 1.  Every term is
 *              >= +0, so padding to any power of two >= n gives the same bits: for n <= 128 this IS the tree padded to 128.
 *   maxima     order-free; a NaN among the terms gives NaN.
 *   fusion     every multiply-subtract and multiply-add is unfused.
 *   constants  mpf_gerfs's, nz = n + 1.
 *   lange      '1' / 'O', 'I', 'M' as mpf_lange_batched; any other letter: -1.
 *   gecon      no P.  '1': the columns the trans = 0 chains of mpf_getrs_batched_blocked leave for e_k without interchanges; 'I': the
 *              vectors its trans = 1 chains leave for e_i.  rcond = 0, never NaN, for anorm == 0, a zero on U's diagonal (checked before
 *              any arithmetic; ainvnm is then +Inf) or an ainvnm that is not finite (or 0).  d_ainvnm is optional.
 *   residual   r_i from b_i, op(A)_ij x_j subtracted for j ascending; w_i from |b_i|, |op(A)_ij| |x_j| added; one pass over A serves
 *              both; trans 0 or 1; d_R may be d_B, d_R and d_W must not overlap d_A or d_X.
 *   gerfs      mpf_gerfs_batched's rule, stop reasons, itmax (<= 0 means 5, clamped to 31) and outputs (berr, optional ferr and iters
 *              at b * nrhs + c).  The correction is the chain of mpf_getrs_batched_blocked with the same trans applied to r; ferr
 *              comes from the last r and w with the chains of the other trans for every e_i, interchanges included, as a tree over k
 *              of |y_k| g_k (the product rounded before the sum).  A NaN stops its column with berr = NaN and touches no neighbour.
 * A kernel may skip steps that meet only zeros, as mpf_getri_batched_blocked does (finite factors; the sign of a zero reaches no
 * | |).  A matrix's and a column's results depend on nothing but its own data: not on batch, position, nrhs, any ld or stride, a
 * tile width or the path (n <= 128 and n < option batched_blocked_min_n: handed to the entry above).  For n <= 128 the results equal
 * the small entries' bit for bit; two calls give the same bits.
 * Workspace (the context's, grow-only): gecon one double per (matrix, tile of 16 chains); gerfs with d_ferr n + 1 doubles per
 * (matrix, column) and one per (matrix, column, tile), at most 256 MB: a call with d_ferr goes in chunks of as many matrices as fit
 * (and at most 32768).  Nothing is proportional to n^2.
 * Return 0, or < 0 with a message (n > 1024: use mpf_lange, mpf_gecon / mpf_gerfs on one matrix at a time; negative sizes, a bad
 * letter or trans, leading dimensions < n, strides too small, NULL pointers).  n == 0, batch == 0 or nrhs == 0: 0, no work. */
int mpf_lange_batched_blocked(mpf_ctx *ctx, char norm, const double *d_A, int64_t lda, int64_t strideA, int32_t n, int64_t batch,
                              double *d_out /* device, batch */);
int mpf_gecon_batched_blocked(mpf_ctx *ctx, char norm, const double *d_LU, int64_t ldlu, int64_t strideLU, int32_t n, int64_t batch,
                              const double *d_anorm /* device, batch */, double *d_rcond /* device, batch */,
                              double *d_ainvnm /* optional: device, batch */);
int mpf_residual_batched_blocked(mpf_ctx *ctx, int32_t trans, const double *d_A, int64_t lda, int64_t strideA, int32_t n, int64_t batch,
                                 int32_t nrhs, const double *d_X, int64_t ldx, int64_t strideX, const double *d_B, int64_t ldb,
                                 int64_t strideB, double *d_R, int64_t ldr, int64_t strideR, double *d_W /* optional */);
int mpf_gerfs_batched_blocked(mpf_ctx *ctx, int32_t trans, const double *d_A, int64_t lda, int64_t strideA, const double *d_LU,
                              int64_t ldlu, int64_t strideLU, int32_t n, int64_t batch, const int32_t *d_ipiv, int64_t strideP,
                              int32_t nrhs, const double *d_B, int64_t ldb, int64_t strideB, double *d_X, int64_t ldx, int64_t strideX,
                              int32_t itmax, double *d_ferr /* optional */, double *d_berr, int32_t *d_iters /* optional */);

/* ---- the same for matrices of DIFFERENT orders (vbatched; csrc/vbatched.hip, host plan in csrc/vbatch_plan.h) ---------------------------
 * One descriptor says where `batch` matrices of orders 0 <= n[b] <= 128 lie inside ONE allocation; four entry points then factor, solve,
 * invert and take determinants of all of them in a handful of ordinary launches (one per size class that is not empty).  For every b the
 * result equals, bit for bit, what the fixed-size entry above returns for that matrix alone with n = n[b]: a matrix's bits do not depend
 * on the batch, its position, the orders of its neighbours (the matrices that share its wave included), ld, off, the class order or the
 * kernel form.
 *
 * Matrix layout (A / LU, and the inverse): matrix b is n[b] x n[b] column-major at base + off[b] (an element offset) with leading
 * dimension ld[b].  ld == NULL: ld[b] = n[b].  off == NULL: packed, off[b] = sum_{i<b} ld[i] n[i].  extent = the doubles the operand
 * spans = max_b off[b] + (n[b] - 1) ld[b] + n[b] (matrices of order 0 span nothing).
 * Vector layout (always packed): offV[b] = sum_{i<b} n[i], total_n = sum n.  Pivots of matrix b: d_ipiv + offV[b] (1-based).  The
 * right-hand sides of all matrices form one tall total_n x nrhs column-major matrix, ldb >= total_n; B[b] is its rows offV[b] ..
 * offV[b] + n[b] - 1: the block-diagonal solve D^-1 B.  d_info, d_mant, d_expo: one entry per matrix.
 *
 * mpf_vbatch_create checks on the host and refuses with a message (< 0): negative batch or n[b]; n[b] > 128 (use mpf_factor_dev);
 * ld[b] < n[b]; off[b] < 0; an extent past 2^62; two matrices whose footprints [off, off + (n-1) ld + n) overlap (footprints that only
 * touch are accepted); batch >= 2^31.  n[b] == 0 and batch == 0 are allowed.  It then bins the matrices into size classes by n[b] alone --
 * n <= 8, 16, 32: 8, 16 or 32 lanes of a wave per matrix; n <= 48, 64: a 256-thread workgroup per matrix; n <= 96, 128: a 1024-thread
 * one (two classes per workgroup form, so that a launch asks only for the LDS its largest matrix needs) -- orders every class by n
 * (stable) and uploads n, off, ld, offV and the class lists (synchronous copies; the descriptor owns the device memory).  Matrices of
 * order 0 are in no class: they are kept in a list of their own, for d_info and the determinant.
 * mpf_vbatch_destroy synchronises the context's stream first; destroy every descriptor before its context.
 * mpf_vbatch_info / mpf_vbatch_offsets: what creation computed (any output may be NULL); offM = the matrix offsets, offV the vector ones.
 *
 * Not here: pointer arrays to separate allocations, n > 128 (mpf_vbatch_create_blocked below), a per-matrix nrhs, sizes given on the
 * device, a block-diagonal matrix-vector product with the inverses, fp16.  Refinement, error bounds and rcond: the expert entries
 * after mpf_getdet_vbatched.  No driver uses these. */
typedef struct mpf_vbatch mpf_vbatch;
int mpf_vbatch_create(mpf_ctx *ctx, int64_t batch, const int32_t *n /* host */, const int64_t *ld /* host, optional */,
                      const int64_t *off /* host, optional */, mpf_vbatch **out);
/* The same descriptor for orders 0 <= n[b] <= 1024 (csrc/vbatched_blocked.hip, bodies in csrc/batched_blocked_body.h): the same layout
 * rules, checks, messages and descriptor type; n[b] > 1024 is refused (use mpf_factor_dev).  The four mpf_*_vbatched entries below take
 * either kind of descriptor; for one from mpf_vbatch_create they issue exactly the launches they always did.
 * Contract: for every b the result equals, bit for bit, what the fixed-size BLOCKED entry above (mpf_getrf_batched_blocked,
 * mpf_getrs_batched_blocked, mpf_getri_batched_blocked, mpf_getdet_batched_blocked) returns for that matrix alone with n = n[b] -- A / LU,
 * pivots, d_info, the in-place solve on rows offV[b] .. of the tall B, the inverse in the descriptor's layout, (mant, expo).  A matrix's
 * bits depend on nothing but the matrix and `fused`: not on the batch, its position, the orders of the matrices launched with it, ld,
 * off, the panel width (option batched_blocked_nb), the inverse tile (option batched_blocked_inv_ct) or the path it took.  Rows n[b] ..
 * ld[b]-1 and every byte between matrices are neither read nor written; a matrix with a zero on U's diagonal leaves its inverse
 * untouched and disturbs no neighbour; out-of-range pivots read as "no interchange".
 * Path: a matrix with n[b] <= 128 and n[b] < option batched_blocked_min_n goes into the seven size classes above and runs their
 * kernels -- the rule by which the fixed-size blocked entries forward.  Every other matrix goes into the large list, ordered by n
 * (stable) and cut into launch groups by order (tops 256, 512, 1024), and runs the ragged forms of the blocked kernels: grids and
 * blocks sized for the largest matrix of a launch, and each panel step of the factorization launched only over the matrices still
 * active at that column (a suffix of the ordered group).  The option is read ONCE, at creation, and stored in the descriptor: changing
 * it later does not move a matrix of an existing descriptor.  batched_blocked_min_n = 0 sends every order >= 1 through the blocked
 * kernels; matrices of order 0 stay in the list of their own.
 * Asynchronous on the context's stream, no workspace beyond the descriptor, nothing read back; every launch is an ordinary launch (no
 * kernel waits for another workgroup, no bounded spin, no co-residency requirement); a group with more than 32768 matrices is launched
 * in chunks.
 * Not here: pointer arrays, a per-matrix nrhs, sizes given on the device, fp16; no driver uses it.  Refinement, error bounds and
 * rcond: the expert entries after mpf_getdet_vbatched. */
int mpf_vbatch_create_blocked(mpf_ctx *ctx, int64_t batch, const int32_t *n /* host */, const int64_t *ld /* host, optional */,
                              const int64_t *off /* host, optional */, mpf_vbatch **out);
void mpf_vbatch_destroy(mpf_vbatch *vb);
int mpf_vbatch_info(const mpf_vbatch *vb, int64_t *batch, int64_t *total_n, int64_t *extent);
int mpf_vbatch_offsets(const mpf_vbatch *vb, int64_t *offM /* host, batch */, int64_t *offV /* host, batch */);
/* mpf_getrf_batched's contract per matrix (pivots and bits of mpf_dgetf2_piv, fused or not); d_info[b] (optional) = the first zero
 * pivot or 0, 0 for n[b] == 0.  Rows n[b] .. ld[b]-1 and every byte between matrices are not touched.  Returns 0, or < 0 with a message
 * (NULL ctx, descriptor, d_A or d_ipiv; a descriptor of another context).  batch == 0 or total_n == 0: no work on the matrices.
 * These four calls are asynchronous on the context's stream, use no workspace beyond the descriptor and read nothing back; a class
 * with more matrices than one grid takes is launched in chunks. */
int mpf_getrf_vbatched(mpf_ctx *ctx, const mpf_vbatch *vb, double *d_A, int32_t *d_ipiv, int32_t *d_info /* optional */, int32_t fused);
/* mpf_getrs_batched's chains per matrix on rows offV[b] .. of the tall B, in place; rows of B outside 0 .. total_n-1 are not touched.
 * Refused: NULL pointers, trans not 0 or 1, nrhs < 0, ldb < total_n, a descriptor of another context.  nrhs == 0: no work. */
int mpf_getrs_vbatched(mpf_ctx *ctx, const mpf_vbatch *vb, int32_t trans, const double *d_LU, const int32_t *d_ipiv, int32_t nrhs,
                       double *d_B, int64_t ldb);
/* mpf_getri_batched's contract per matrix, the inverse in the descriptor's matrix layout at d_inv, out of place: refused when
 * [d_LU, + extent) and [d_inv, + extent) overlap.  A matrix with a zero on U's diagonal: d_info[b] = the first such i + 1, its inverse
 * is left untouched, no neighbour is affected; ipiv entries out of range read as "no interchange".  d_info[b] = 0 for n[b] == 0. */
int mpf_getri_vbatched(mpf_ctx *ctx, const mpf_vbatch *vb, const double *d_LU, const int32_t *d_ipiv, double *d_inv,
                       int32_t *d_info /* optional */);
/* mpf_getdet_batched's (mant, expo) per matrix; n[b] == 0 gives (0.5, 1), mpf_getdet's N = 0 case. */
int mpf_getdet_vbatched(mpf_ctx *ctx, const mpf_vbatch *vb, const double *d_LU, const int32_t *d_ipiv, double *d_mant, int32_t *d_expo);
/* The expert layer on a descriptor of EITHER kind (csrc/vbatched_refine.hip, bodies in csrc/batched_refine_blocked_body.h): norms, exact
 * reciprocal condition numbers, the residual step operator and the refinement with berr and an exact ferr for all matrices of the
 * descriptor in a handful of ordinary launches.
 * Layouts: the matrices (A, LU) in the descriptor's layout; X, B, R and W tall total_n x nrhs column-major matrices, matrix b's rows at
 * offV[b] .., every leading dimension >= total_n (mpf_getrs_vbatched's B); the pivots at offV[b]; per-matrix outputs (d_out, d_anorm,
 * d_rcond, d_ainvnm) at b, per-column outputs (d_ferr, d_berr, d_iters) at b * nrhs + c.
 * Contract: for every b every output equals, bit for bit, what the fixed-size BLOCKED expert entry above (mpf_lange_batched_blocked,
 * mpf_gecon_batched_blocked, mpf_residual_batched_blocked, mpf_gerfs_batched_blocked) returns for that matrix alone with n = n[b], and
 * so, for n[b] <= 128, what the small expert entry returns.  The result depends on nothing but the matrix, its factors and its
 * columns: not on the batch or the position, the orders launched beside it, ld, off or nrhs, the chunk or the kind of descriptor.  The
 * rule, constants and stop reasons of the refinement, the itmax handling, the rcond = 0 cases and the NaN behaviour are the fixed
 * entries', word for word; rows n[b] .. ld[b]-1 and every byte between matrices are neither read nor written, nor are rows of X, B, R,
 * W outside 0 .. total_n-1.  d_R may be d_B.
 * Path: every matrix of order >= 1 runs the ragged forms of the blocked expert kernels, whatever the descriptor's kind and option
 * batched_blocked_min_n (the tree padded to 1024 is the tree padded to 128, so the small entries' bits come out for n <= 128).  The
 * list ordered by n is cut into launch groups at the orders 64, 128, 256, 512, 1024, a group into chunks of at most 32768 matrices;
 * grids and blocks are sized for the largest matrix of a launch.  Matrices of order 0 own no rows; their outputs are norm 0, rcond 1 and
 * ainvnm 0 (dgecon's quick return), berr = ferr = 0 and iters = 0 for each column.
 * Asynchronous on the context's stream, nothing read back, no kernel waits for another workgroup and nothing spins.  Workspace (the
 * context's, grow-only): gecon one double per (matrix, tile of 16 chains); gerfs with d_ferr n[b] + 1 doubles per (matrix, column) and
 * one per (matrix, column, tile), at most 256 MB: such a call goes in chunks of as many matrices as fit (at least one).  Nothing is
 * proportional to n^2.
 * Return 0, or < 0 with a message: NULL pointers, a descriptor of another context, a bad letter or trans, nrhs < 0, a leading
 * dimension < total_n.  batch == 0, total_n == 0 and nrhs == 0 do no work on matrices.
 * Not here: forms of the small expert kernels' 8 / 16 / 32 lanes per matrix (orders <= 32 run a workgroup each), equilibration,
 * dlacn2 estimates, an extra-precise residual, a per-matrix nrhs, pointer arrays; no driver uses these. */
int mpf_lange_vbatched(mpf_ctx *ctx, const mpf_vbatch *vb, char norm, const double *d_A, double *d_out /* device, batch */);
int mpf_gecon_vbatched(mpf_ctx *ctx, const mpf_vbatch *vb, char norm, const double *d_LU, const double *d_anorm /* device, batch */,
                       double *d_rcond /* device, batch */, double *d_ainvnm /* optional: device, batch */);
int mpf_residual_vbatched(mpf_ctx *ctx, const mpf_vbatch *vb, int32_t trans, const double *d_A, int32_t nrhs, const double *d_X, int64_t ldx,
                          const double *d_B, int64_t ldb, double *d_R, int64_t ldr, double *d_W /* optional, ldr */);
int mpf_gerfs_vbatched(mpf_ctx *ctx, const mpf_vbatch *vb, int32_t trans, const double *d_A, const double *d_LU, const int32_t *d_ipiv,
                       int32_t nrhs, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t itmax, double *d_ferr /* optional */,
                       double *d_berr, int32_t *d_iters /* optional */);

/* ---- equilibration of the batched layouts (csrc/batched_equil.hip) ---------------------------------------------------------
 * mpf_geequ's power-of-two factors, dlaqge's scaling and the diagonal scaling of right-hand sides for the three batched layouts: a
 * strided batch of one order n <= 128 (mpf_*_batched), of one order n <= 1024 (mpf_*_batched_blocked) and a descriptor of either kind
 * (mpf_*_vbatched).  Layout rules, argument checks, error style and asynchrony are mpf_getrs_batched's, mpf_getrs_batched_blocked's and
 * mpf_getrs_vbatched's: ordinary launches on the context's stream, nothing read back, every result a device array, rows n .. ld-1 and
 * the bytes between matrices neither read nor written, n == 0 or batch == 0 returns 0 with no work.  The small entries refuse n > 128,
 * the blocked ones n > 1024 (a matrix that large: mpf_geequ / mpf_gesvx, mpf_factor_dev); a blocked entry hands n below option
 * batched_blocked_min_n to the small kernels; batches longer than one launch go in chunks.
 * Every product below is a product with a power of two and every extreme is a maximum or minimum, so a matrix's results are the same
 * bits on every path: they depend on the matrix and `rule` alone, not on batch, position, ld, stride, off, the orders launched beside it,
 * the kernel form, batched_blocked_min_n or the kind of descriptor.  tests/batched_equil_model.py restates all of it in numpy.
 *
 * mpf_geequ_*: per matrix mpf_geequ's definitions -- r_i = 2^-floor(log2 max_j |a_ij|), c_j = 2^-floor(log2 max_i |a_ij| r_i) (the
 * rounded product), exponents clamped to [-1022, 1022]; with rmax / rmin the largest / smallest row maximum and smlnum = DBL_MIN,
 * rowcnd = max(rmin, smlnum) / min(rmax, 1 / smlnum), colcnd the same of the scaled column maxima, amax = the largest |a_ij|.
 * d_r and d_c hold n doubles per matrix -- strided layouts at b n, descriptors at offV[b]; d_rowcnd, d_colcnd, d_amax (double) and
 * d_info (int32) one per matrix; all six are required.  d_info[b]:
 *   0           a clean matrix: everything is set.
 *   i + 1       row i is the first zero row: amax is set, rowcnd is 0, r is set (1 for a zero row); c and colcnd are not written.
 *   n + j + 1   column j is the first zero column of the row-scaled matrix: r, rowcnd and amax are set; c and colcnd are not written.
 *   2 n + 1     the matrix holds a NaN or +-Inf: amax is that NaN or Inf (a NaN wherever one is present); the check comes before any
 *               scale is formed, and r, c, rowcnd and colcnd are not written.
 * A matrix of order 0 (descriptors): rowcnd = colcnd = 1, amax = 0, info = 0 (dgeequ's quick return).
 *
 * mpf_laqge_*: d_out[b] = Dr A[b] Dc by `rule`, decided per matrix on the device: 0 never (a copy); 1 dlaqge's rule as mpf_gesvx
 * states it -- rows if rowcnd < 0.1 or amax outside [small, 1 / small] with small = DBL_MIN / DBL_EPSILON, columns if colcnd < 0.1; 2
 * always both; any other rule returns -1.  A matrix with d_info[b] != 0 is never scaled under any rule (its rowcnd / colcnd are not
 * looked at).  d_out may be d_A (in place: a matrix that is not scaled is then not touched); otherwise it has d_A's layout (lda,
 * strideA / the descriptor) and must not overlap d_A.  Each element is (r_i a_ij) c_j, two rounded products in that order; a side that
 * is not scaled contributes no product.  d_equed[b] (int32, required): 0 none, 1 rows, 2 columns, 3 both (mpf_gesvx_stats.equed's
 * values).  d_spread (optional, 2 doubles per matrix): [2 b] = max_i r_i / min_i r_i if the rows were scaled, else 1; [2 b + 1] the
 * same of c -- exact powers of two (Inf past 2^1023), what a driver multiplies ferr by.  Order 0: equed 0, spread 1.
 *
 * mpf_lascl2_*: V[b] = diag(s[b]) V[b] in place on the matrices with d_equed == NULL or d_equed[b] & bit; a matrix whose bit is clear
 * is not touched.  V is n x nrhs per matrix laid out as mpf_getrs_batched's B (ldv, strideV), for a descriptor the tall total_n x nrhs
 * matrix of mpf_getrs_vbatched with s at offV[b].  A driver needs multiplications only: B' = Dr B and X = Dc X' for trans = 0,
 * B' = Dc B and X = Dr X' for trans = 1.
 *
 * Paths: n <= 32 runs 8 / 16 / 32 lanes of a wave per matrix, 33 .. 128 a workgroup per matrix, both reading A once; the blocked
 * entries spread a matrix over ceil(n / 64) workgroups for the row maxima and ceil(n / 16) for the scaled column maxima, with one small
 * launch after each (four launches, A read twice); a descriptor runs the ragged forms of those four for every order >= 1, launch
 * group by launch group of its ordered list (the expert layer's groups).  Workspace (the context's, grow-only): two words per row of a
 * chunk for the blocked and descriptor forms.  No kernel waits for another workgroup.
 * Return 0, or < 0 with a message: NULL pointers, negative sizes, n over the limit, a leading dimension or stride too small, a bad
 * rule, d_out overlapping d_A, a descriptor of another context.
 * Not here: scaling fused into the loads of getrf / getrs; a C driver (the Python gesvx_batched composes these entries with the
 * existing ones, refining on the equilibrated system); the 8 / 16 / 32-lane forms for the small matrices of a descriptor; mpf_geequ and
 * the large-matrix drivers are unchanged. */
int mpf_geequ_batched(mpf_ctx *ctx, const double *d_A, int64_t lda, int64_t strideA, int32_t n, int64_t batch, double *d_r, double *d_c,
                      double *d_rowcnd, double *d_colcnd, double *d_amax, int32_t *d_info);
int mpf_laqge_batched(mpf_ctx *ctx, int32_t rule, const double *d_A, int64_t lda, int64_t strideA, int32_t n, int64_t batch,
                      const double *d_r, const double *d_c, const double *d_rowcnd, const double *d_colcnd, const double *d_amax,
                      const int32_t *d_info, double *d_out, int32_t *d_equed, double *d_spread /* optional: 2 per matrix */);
int mpf_lascl2_batched(mpf_ctx *ctx, const double *d_s, int32_t n, int64_t batch, int32_t nrhs, double *d_V, int64_t ldv, int64_t strideV,
                       const int32_t *d_equed /* optional */, int32_t bit);
int mpf_geequ_batched_blocked(mpf_ctx *ctx, const double *d_A, int64_t lda, int64_t strideA, int32_t n, int64_t batch, double *d_r,
                              double *d_c, double *d_rowcnd, double *d_colcnd, double *d_amax, int32_t *d_info);
int mpf_laqge_batched_blocked(mpf_ctx *ctx, int32_t rule, const double *d_A, int64_t lda, int64_t strideA, int32_t n, int64_t batch,
                              const double *d_r, const double *d_c, const double *d_rowcnd, const double *d_colcnd, const double *d_amax,
                              const int32_t *d_info, double *d_out, int32_t *d_equed, double *d_spread /* optional */);
int mpf_lascl2_batched_blocked(mpf_ctx *ctx, const double *d_s, int32_t n, int64_t batch, int32_t nrhs, double *d_V, int64_t ldv,
                               int64_t strideV, const int32_t *d_equed /* optional */, int32_t bit);
int mpf_geequ_vbatched(mpf_ctx *ctx, const mpf_vbatch *vb, const double *d_A, double *d_r, double *d_c, double *d_rowcnd, double *d_colcnd,
                       double *d_amax, int32_t *d_info);
int mpf_laqge_vbatched(mpf_ctx *ctx, const mpf_vbatch *vb, int32_t rule, const double *d_A, const double *d_r, const double *d_c,
                       const double *d_rowcnd, const double *d_colcnd, const double *d_amax, const int32_t *d_info, double *d_out,
                       int32_t *d_equed, double *d_spread /* optional */);
int mpf_lascl2_vbatched(mpf_ctx *ctx, const mpf_vbatch *vb, const double *d_s, int32_t nrhs, double *d_V, int64_t ldv,
                        const int32_t *d_equed /* optional */, int32_t bit);

/* ---- multi-GPU (build extension; the reference is single-device, MPF.cu:77) ------------------------------------
 * One process per GPU.  1-D block-cyclic columns: global column block b (nb columns) lives on rank b % world as local block
 * b / world; d_Aloc is the rank's N x (local columns) column-major matrix (ldloc >= N), d_ipiv the full pivot vector (N int32,
 * identity-initialised like MPF.h:3 wants it), replicated on every rank on return.  Per panel ONE exchange: the owner
 * broadcasts the factored panel + pivots + moved-row list; everything else is local.  Results are bit-identical to
 * mpf_factor_dev.  Panel width <= 256.
 * The exchange goes through callbacks so any transport can carry it (both are called on every rank, in the same order,
 * with a HIP stream the transfer must be ordered on; return 0 on success):
 *   bcast(user, d_buf, bytes, root, stream)        d_buf is the message on the root and the landing buffer elsewhere
 *   allreduce(user, d_buf, count, stream)          in-place sum of `count` doubles (refinement residual only)
 * NULL callbacks select the context's RCCL communicator (mpf_rccl_init: ncclBroadcast / ncclAllReduce over xGMI). */
typedef int (*mpf_bcast_fn)(void *user, void *d_buf, int64_t bytes, int32_t root, void *hip_stream);
typedef int (*mpf_allreduce_fn)(void *user, double *d_buf, int64_t count, void *hip_stream);
typedef struct mpf_dist {
    int32_t rank, world;
    mpf_bcast_fn bcast;
    mpf_allreduce_fn allreduce;
    void *user;
} mpf_dist;
/* RCCL communicator owned by the context (librccl is resolved with dlopen at the first call: single-GPU users never load it).
 * mpf_rccl_unique_id: 128 bytes to be produced on one rank and handed to all (e.g. through torch.distributed / MPI). */
int mpf_rccl_unique_id(void *out128);
int mpf_rccl_init(mpf_ctx *ctx, const void *id128, int32_t rank, int32_t world);
int mpf_rccl_destroy(mpf_ctx *ctx);
int mpf_rccl_version(void); /* ncclGetVersion(), or < 0 when librccl cannot be loaded */
/* What the context's communicator is (ncclCommCount / ncclCommUserRank: what RCCL itself says) and what this library has sent over
 * it since mpf_rccl_init; link_type / link_hops / peer_access: hipExtGetLinkTypeAndHopCount and hipDeviceCanAccessPeer from the
 * context's device to each visible device (index = device ordinal, up to 16). */
typedef struct mpf_rccl_info_t {
    int32_t version, has_comm, comm_count, comm_rank, has_p2p, device, visible_devices, reserved;
    int64_t bcast_calls, bcast_bytes, allreduce_calls, p2p_calls, p2p_bytes;
    int32_t link_type[16], link_hops[16], peer_access[16];
} mpf_rccl_info_t;
int mpf_rccl_info(mpf_ctx *ctx, mpf_rccl_info_t *out);
/* `reps` broadcasts of `bytes` from `root` on the communicator, timed on the context's stream: ms per broadcast (every rank calls it) */
int mpf_rccl_bcast_probe(mpf_ctx *ctx, int64_t bytes, int32_t root, int32_t reps, double *ms_per_bcast);
int mpf_rccl_selftest(mpf_ctx *ctx); /* one small broadcast + all-reduce on the communicator (every rank calls it) */
/* The panel loop MPF.cu:100-242 over the block-cyclic layout (look-ahead schedule: the owner of panel k+1 updates that block
 * first, runs its chain and posts the broadcast on a side stream under everybody's update k).  Returns this rank's info.
 * The fp64 pivot rules (mpf_opts.pivot_search = 1 or 2, option pivot_fp64) are single-GPU only: -1 with a message here. */
int mpf_factor_dist(mpf_ctx *ctx, double *d_Aloc, int64_t ldloc, int64_t N, int32_t nb, int32_t *d_ipiv, const mpf_dist *dist,
                    const mpf_opts *opts);
/* Optional point-to-point transport next to the caller's own broadcast / all-reduce callbacks (with NULL callbacks in mpf_dist the
 * context's RCCL communicator supplies ncclSend / ncclRecv by itself):
 *   p2p(user, d_buf, bytes, peer, send, stream)    send != 0: d_buf goes to rank `peer`; send == 0: bytes from `peer` land in d_buf
 * Every send has exactly one matching receive, issued in the same order on both ranks. */
typedef int (*mpf_p2p_fn)(void *user, void *d_buf, int64_t bytes, int32_t peer, int32_t send, void *hip_stream);
int mpf_dist_set_p2p(mpf_ctx *ctx, mpf_p2p_fn fn, void *user);
/* mpf_solve_ir over the same layout: d_Aloc = the rank's columns of the ORIGINAL matrix, d_LUloc = of the factors; d_b and
 * d_x (N each) replicated.  Residual = local GEMV + all-reduce.  The triangular solves walk the column blocks; with a point-to-point
 * transport the running vector travels from owner to owner (2 (N / nb - 1) sends + one all-reduce per factor solve), otherwise the
 * owner applies a block to the replicated vector and broadcasts it on (2 N / nb broadcasts).  nb must be a multiple of 64. */
int mpf_solve_ir_dist(mpf_ctx *ctx, const double *d_Aloc, int64_t lda, const double *d_LUloc, int64_t ldlu, const int32_t *d_ipiv,
                      int64_t N, int32_t nb, const double *d_b, double *d_x, int32_t max_iter, double tol, const mpf_dist *dist,
                      mpf_ir_stats *stats);

#ifdef __cplusplus
}
#endif
#endif
