// Internal declarations shared by the HIP kernels and the C++ host driver of libmpf_amd.so.
// gfx950 (MI355X) only: 64-lane wavefronts, 160 KiB LDS per CU, 8 XCDs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include <functional>
#include "../../include/mpf_c.h"

// ---- fp16 pivot panel geometry (fp16_panel.hip) ---------------------------------------------
constexpr int HP_R = 256;              // panel rows owned by one workgroup (its LDS slab)
constexpr int HP_T = 512;              // threads per workgroup
constexpr int HP_MAXG = 256;           // max workgroups = CUs: all must be co-resident
constexpr int HP_MAXCOLS = 256;        // max panel width
constexpr int LASWP_MAXMOVED = 2 * HP_MAXCOLS;

// Rows that really move under one panel's interchanges: content of row src[i] goes to row dst[i] (global rows).
struct MovedList {
    int n;
    int pad[3];
    int src[LASWP_MAXMOVED];
    int dst[LASWP_MAXMOVED];
};

// Device workspace owned by a context, zeroed once at mpf_create.  Hand-off granules carry the launch sequence number of the
// pivot kernel in their tags, so nothing here is cleared between launches.
struct MpfWorkspace {
    unsigned long long cand[2][HP_MAXG];   // {tag:31 | abs:15 | ~tiekey:17} per workgroup, tag = launch sequence << 9 | column + 1
    int flags[16];                         // [0]: give-ups of the triangular solves' bounded waits (ir.hip; must stay 0); rest spare
    unsigned long long rowbuf[2][HP_MAXG][HP_MAXCOLS / 2]; // candidate pivot rows: {tag32 | 2 x fp16} granules
    int hp_timeouts;                       // spin give-ups inside the pivot kernel (must stay 0)
    int pad0[3];
    MovedList list0;                       // moved-row list of the stand-alone mpf_laswp (built by laswp_plan)
    int info;                              // first zero pivot in the fp64 panel (1-based) or INT_MAX
    int pad[3];
    unsigned long long hp_stamps[8];       // diagnostic build of the pivot kernel (MPF_HP_STAMP=1): cycles per segment
    unsigned long long hp_progress;        // {launch sequence:32 | columns whose pivots are final:32}, published by workgroup 0
    unsigned long long hp_xcd_target;      // single-XCD form of the pivot kernel: {launch sequence:32 | XCC id + 1} of the XCD whose workgroups take the panel
    unsigned long long hp_xcd_roles;       // ... {launch sequence:32 | workgroups of that XCD that have taken a slab}
};

// Behaviour switches of a context.  Defaults come from the environment ONCE, at mpf_create (the MPF_* variable named with
// each field); after that they are plain per-context state, changed through mpf_set_option (include/mpf_c.h) -- two contexts
// on two host threads never share or race on them.
struct MpfTuning {
    int safe_pivots = 0;                 // MPF_SAFE_PIVOTS=1: generic (never-waiting) pivot path and schedule always
    int pivot_fp64 = 0;                  // MPF_PIVOT_FP64=1: every factorization searches its pivots in fp64 (mpf_opts.pivot_search = 1; dpivot.hip);
                                         // 2: by tournament pivoting (mpf_opts.pivot_search = 2; dpivot.hip)
    int chain_pipeline = 1;              // MPF_CHAIN_PIPELINE=0: the fp64 panel waits for the whole pivot kernel
    long long chain_pipeline_below = 10240; // MPF_CHAIN_PIPELINE_BELOW: fp64 mode pipelines the chain only below this trailing size (re-tuned in round 4
                                            // after the pivot kernel got faster: 8192 .. 14336 within 1 ms of each other, 18432 + 3 ms, 0 + 9 ms)
    int fp16_work32 = 1;                 // MPF_FP16_WORK32=0: fp16 modes update the fp64 matrix in place (no fp32 working copy)
    int superpanel_fp16 = 0;             // MPF_SUPERPANEL: panels per super-panel of the fp16 modes (mpf_opts.superpanel = 0): 1 .. 8, or 0 = automatic --
                                         // plain fp16 operands from N = 24576 on: 6, else 4 (fp16x3: 4; mpf_factor_dist: the same rule).  A wider super-panel feeds
                                         // the big-K update a longer K (fewer passes over the fp32 copy: 520 -> 628 TFLOP/s per launch in the schedule
                                         // at N = 32768) and costs fp64 work in the inner region (125.4 -> 127.9 ms there, 467.9 -> 456.9 at N = 65536;
                                         // fp16x3 loses at every width above 4): profiles/r05_superpanel_width.log
    int superpanel_fp64 = 1;             // MPF_SUPERPANEL_FP64: the same for the fp64 mode
    int no_lookahead = 0;                // MPF_NO_LOOKAHEAD=1: single-stream schedule
    int verbose = 0;                     // MPF_VERBOSE=1: per-panel line (MPF.cu:137) from the drop-in MPF()
    int timeline = 0;                    // MPF_TIMELINE=1: every timed region as (start, end) on stderr
    long long hp_spin_limit = 1ll << 21; // MPF_HP_SPIN_LIMIT: bound of every cross-workgroup spin of the LDS pivot kernel (polls)
    long long hp_gate_ticks = 200000000ll; // MPF_HP_GATE_TICKS: bound of a gate's wait for the pivot kernel (100 MHz ticks: 2 s)
    int hp_window = -1;                  // MPF_HP_WINDOW: pivot panels on the column-window kernel (76 KB of LDS, shares its CU) instead of the
                                         // full-slab one (a CU per workgroup): 0 never, n >= 1 for panels of at least n rows, -1 automatic --
                                         // 20 000 rows under an fp64 trailing update (whose 68-KB workgroups fit beside it: -1 % factor time), under the fp16
                                         // ones only for panels that leave fewer than 72 CUs free (above (CUs - 72) x 256 = 47 104 rows), where the
                                         // full-slab form deadlocks against the chain's gated kernels (measured)
    int hp_acq_fence = 0;                // MPF_HP_ACQ_FENCE=1: agent-scope acquire after the hand-off poll (debug aid)
    int hgemm_pad = 0;                   // MPF_HGEMM_PAD: unused dynamic LDS (bytes) of the plain fp16 update kernel (occupancy cap)
    int hgemm_split_pad = 32768;         // MPF_HGEMM_SPLIT_PAD: the same for the split-operand kernel (two workgroups per CU)
    int hgemm_big = 1;                   // MPF_HGEMM_BIG=0: the 128 x 128-tile fp16 update kernel for every shape (A/B switch)
    int hgemm_mfma16 = 1;                // MPF_HGEMM_MFMA16=0: plain-operand fp16 updates on round 4's v_mfma_f32_32x32x16_f16 kernels (trailing_f16.hip,
                                         // hgemm_pp.hip) instead of the 16x16x32 ones (hgemm16.hip); A/B switch -- the two families differ in bits
                                         // (different summation order inside an MFMA), each is self-consistent across its kernels
    int hgemm_big_tile = 0;              // MPF_HGEMM_BIG_TILE: form of the big-K fp16 update (launch_hgemm_ptrs): 0 = automatic, 1 / 2 = 128 x 256 tiles (one / two
                                         // workgroups per CU), 3 = round 3's kernel, 4 = hgemm_big_kernel everywhere, 5 = hgemm_pp_kernel everywhere
    int dgemm_dma = 1;                   // MPF_DGEMM_DMA=0: register-staged eight-wave fp64 update kernel (same bits)
    int lazy_gather = 2;                 // MPF_LAZY_GATHER: deferred left-hand interchanges (laswp.hip) 2 = in one pass, in place: one map launch + a few apply launches;
                                         // 1 = panel by panel through a temporary, as gathered reads; 0 = the same as scattered writes.  Same bits
    int lazy_onepass_max_rows = 32768;   // MPF_LAZY_ONEPASS_MAX_ROWS: lazy_gather = 2 takes a column block in one pass while its segment has at most that many rows
                                         // (a workgroup's registers hold 32768); longer segments go through the temporary
    int dpanel_fused_form = 1;           // MPF_DPANEL_FUSED=0: fp64 panel without the fused update + sub-panel launches
    int dist_instalments = 1;            // MPF_DIST_INSTALMENTS=0: the panel message of mpf_factor_dist always travels in one broadcast
    long long dist_instalment_min_bytes = 8ll << 20; // MPF_DIST_INSTALMENT_MIN_BYTES: panels below this go in one broadcast
    int fp16_fused = 0;                  // MPF_FP16_FUSED=1: the fp16 pivot panel eliminates with ONE fused multiply-add per element, fma(-m, u, x) rounded once (contract C2f)
                                         // instead of a rounded product and a rounded difference (C2): other pivots, other factors.  Read at each launch of a pivot kernel
    int generic_fused = 1;               // MPF_GENERIC_FUSED=0: generic pivot path with four launches per column instead of two
    int fp64_rowmajor = 1;               // MPF_FP64_ROWMAJOR=0: fp64 mode updates the column-major matrix in place (no row-major working copy)
    long long fp64_rowmajor_min_n = 8192;// MPF_FP64_ROWMAJOR_MIN_N: smaller matrices stay in place (the copy's extra launches cost more than they save)
    int trsm_laswp_fused = 1;            // MPF_TRSM_LASWP_FUSED=0: interchange and TRSM right of the strip as two launches
    int fp64_two_lanes = 8192;           // MPF_FP64_TWO_LANES: fp64 row-major schedule splits the update over two lanes while at least this many
                                         // columns lie right of the strip and the chain is not pipelined (0: always one lane)
    int dist_solve_p2p = 0;              // MPF_DIST_SOLVE_P2P=1: the distributed triangular solves pass the vector from owner to owner over ncclSend / ncclRecv
                                         // instead of broadcasting after every block.  Off by default until a run on two or more GPUs has covered it
                                         // (ADVICE r4); the ranks vote, and the chain is taken only when every rank has it
    int host_sink = 1;                   // MPF_HOST_SINK=0: mpf_factor_host / MPF() copy the factors back in one piece after the factorization (as the
                                         // reference does) instead of block row by block row while it runs (rowsink.hip)
    int hp_local_xcd = 1;                // MPF_HP_LOCAL_XCD: panels of at most (CUs / 8) slabs run their pivot kernel on the workgroups of ONE XCD (hand-offs through that
                                         // XCD's L2: plain stores; fp16_panel.hip): 0 never, 1 in the fp16 modes' schedules and the step operator, 2 always
    int hp_half_slabs = 1;               // MPF_HP_HALF_SLABS=0: the pivot kernel keeps 256-row slabs everywhere (1: 128-row slabs for 256-column panels of <= 16384 rows in the
                                         // fp16 modes' schedules and the step operator; fp16_panel.hip)
    int hp_half_slabs_rows = 16384;      // MPF_HP_HALF_SLABS_ROWS: ... up to this many rows
    int sink_trace = 0;                  // MPF_SINK_TRACE=1: the block-row sink prints one line per block row on stderr (when final, when home)
    int host_late_parts = 3;             // MPF_HOST_LATE_PARTS: column segments of the matrix that go up WHILE mpf_factor_host's factorization has started on the
                                         // first part (0: the whole matrix first, as MPF.cu:82); fp64 row-major schedule only
    long long host_late_min_n = 16384;   // MPF_HOST_LATE_MIN_N: ... and from this size on
    int host_first_pct = 25;             // MPF_HOST_FIRST_PCT: share of the columns in that first part
    int host_late_q_pct = 110;           // MPF_HOST_LATE_Q_PCT: percent of the estimated arrival time of a late segment at which it is planned in (mpf_factor_host)
    long long host_sink_min_n = 4096;    // MPF_HOST_SINK_MIN_N: smaller matrices always go back in one piece
    int gate_wait_value = 0;             // MPF_GATE_WAIT_VALUE=1: the pipelined chain's gated interchange as hipStreamWaitValue64 on the pivot kernel's progress
                                         // word (signal memory) + an ungated kernel, instead of a kernel that spins on CUs (measured round 5: DESIGN 4.1)
    int gesv_fp64_tflops = 0;            // MPF_GESV_FP64_TFLOPS: fp64 factorization rate mpf_gesv(try_fp16 = 3) prices GMRES-IR's time limit with; 0 = this
                                         // context's last measured fp64-mode factorization (N >= 8192), 50 before there is one
    int dist_world1_loop = 0;            // MPF_DIST_WORLD1_LOOP=1: mpf_factor_dist with ONE rank runs the distributed loop (tests) instead of handing over to mpf_factor_dev
    int event_timers = 1;                // MPF_EVENT_TIMERS: HIP-event pairs around 2 = every timed region (mpf_stats.ms_hpanel ... ms_cvt), 1 = the
                                         // trailing updates only (ms_gemm, ms_gemm_big; default), 0 = none; option timeline implies 2
    int fp64_lane_a_pct = 50;            // MPF_FP64_LANE_A_PCT: share of those columns in lane A at a (re-)split; re-split 10 points below.  Lane B's
                                         // update has to cover lane A's small launches of the next panel (measured: 60 % and more lose)
    int fp64_pair = 1;                   // MPF_FP64_PAIR=0: fp64 row-major schedule passes over the far columns once per panel (K = nb) everywhere; 1: once per
                                         // panel PAIR (K = 2 nb) while the update is the longer side (factor_rm_pairs; same bits)
    long long fp64_pair_min_n = 16384;   // MPF_FP64_PAIR_MIN_N: ... that is, while the trailing matrix of the pair's first panel is larger than this (measured at
                                         // N = 32768: 9216 .. 16384 within 1.5 ms of each other, profiles/pair_ab.log; below, the pair's two chains no longer fit under its update)
    int gmres_group_tiles = 0;           // MPF_GMRES_GROUP_TILES: 32-column tiles mpf_solve_gmres_ir_block takes through the device together: n >= 1 exactly n
                                         // (at most 16), 0 = automatic -- the most (<= 16, >= 1) whose restart + 1 basis sets and six working sets fit in
                                         // 2 GiB.  The results do not depend on it (every column's arithmetic is its own)
    int batched_blocked_min_n = 129;     // MPF_BATCHED_BLOCKED_MIN_N: mpf_getrf_batched_blocked / mpf_getrs_batched_blocked hand matrices of n below this (and <= 128)
                                         // to the one-workgroup kernels of batched.hip (same bits by contract); 0: every n through the blocked kernels.
                                         // mpf_vbatch_create_blocked reads it once, at creation: which matrices go into the small classes
    int batched_blocked_nb = 0;          // MPF_BATCHED_BLOCKED_NB: panel width of the blocked batched LU: 8, 16 or 32; 0 (or any other value) = automatic.  Same bits
    int batched_blocked_inv_ct = 0;      // MPF_BATCHED_BLOCKED_INV_CT: columns per workgroup of the blocked batched inverse: 8 or 16; 0 (or any other value) = automatic.  Same bits
#ifdef MPF_PROBE                         // libmpf_probe.so only (tools/): measured-slower variants and diagnostics
    int batched_blocked_valu = 0;        // MPF_BATCHED_BLOCKED_VALU=1: the blocked batched LU's fused trailing update on the VALU kernel instead of the MFMA one (cross-check)
    int batched_blocked_stages = 7;      // MPF_BATCHED_BLOCKED_STAGES: stages the blocked batched LU launches, bit 0 panel, 1 row block, 2 update (per-stage timing; results wrong unless 7)
    int hp_stamp = 0;                    // MPF_HP_STAMP=1: cycle-stamped build of the pivot kernel
    int hp_r256_upto = 1 << 30;          // MPF_HP_R256_UPTO: panels above that many rows use 128-row workgroups
    int dgemm_w8 = 1;                    // MPF_DGEMM_W8=0: four-wave fp64 update kernel everywhere
    int gemm_lds_pad = 0;                // MPF_GEMM_LDS_PAD: extra dynamic LDS of the fp64 update kernels
    int hgemm_dbg = 0;                   // MPF_HGEMM_DBG: big fp16 update 1 = K loop only, 2 = C stream only (timing probes; results wrong)
    int hgemm_big_reg = 0;               // MPF_HGEMM_BIG_REG=1: the big fp16 update stages its operands through registers instead of by LDS-DMA
#endif
};

// Grow-only scratch buffer (device memory, or pinned host memory when Pinned) owned by whoever holds it; freed when that is destroyed.
// grow(n) reallocates only when n elements do not fit, and keeps no contents; on failure the buffer is empty and the error is returned
// (the caller decides whether that is fatal and whether to clear HIP's sticky error).
template <class T, bool Pinned = false>
struct Buf {
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    ~Buf() { release(); }
    hipError_t grow(int64_t n) {
        if (n <= cap_) return hipSuccess;
        release();
        void *q = nullptr;
        const hipError_t e = Pinned ? hipHostMalloc(&q, (size_t)n * sizeof(T)) : hipMalloc(&q, (size_t)n * sizeof(T));
        if (e != hipSuccess) return e;
        p_ = (T *)q;
        cap_ = n;
        return hipSuccess;
    }
    void release() {
        if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        cap_ = 0;
    }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    int64_t cap() const { return cap_; }   // elements
private:
    T *p_ = nullptr;
    int64_t cap_ = 0;
};

struct mpf_ctx {
    MpfTuning tune;
    unsigned attr_done = 0;            // hipFuncSetAttribute done for this context's device, one bit per kernel family
    unsigned attr_big = 0;             // the same for the instantiations of hgemm_big_kernel (bit = launch slot, + 8 for the fp32 copy)
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipStream_t pstream = nullptr;     // high-priority stream of the look-ahead panel chain
    hipStream_t tstream = nullptr;     // second chain stream: the fp64 panel follows the pivot kernel 32 columns behind
    hipStream_t xstream = nullptr;     // mpf_factor_dist: exchange stream of the panel message's instalments (created on demand)
    std::vector<hipEvent_t> ev_pool;   // reusable events (dependencies + per-launch timing)
    MpfWorkspace *ws = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::string err;
    mpf_stats stats{};
    int num_cus = 0;
    // scratch for the solve path (grown on demand)
    Buf<double> solve_buf;
    int64_t solve_n = 0;
    Buf<unsigned short> h_L, h_U;      // fp16 operand images of the fp16 trailing mode
    int64_t h_rows = 0;
    Buf<unsigned short> h_Lb[2];       // L images of the deferred K = sb * nb updates (two super-panels in flight)
    int h_kmax = 0;                     // K capacity (columns) of the fp16 operand images
    unsigned hp_seq = 0;               // launch sequence number of the pivot kernel (row-granule tags)
    unsigned long long *hp_signal = nullptr;   // 8 bytes of signal memory (hipMallocSignalMemory): the progress word for hipStreamWaitValue64
    Buf<int32_t> perm_buf;
    Buf<MovedList> lists;              // one moved-row list per panel of the running factorization
    Buf<int> Fmap;                     // composite row map of the deferred left-hand interchanges (the map and its inverse)
    Buf<double> perm_tmp;              // N x nb scratch of the same
    Buf<int> lazy_snap;                // one-pass form of the same: the inverse map's snapshots, one per (super-)panel, triangular (about N^2 / (2 nb) ints)
    int lazy_onepass_blocks = 0;       // column blocks the last launch_lazy_left_swaps took in one pass (mpf_stats.lazy_onepass_blocks)
    Buf<double> trsv_inv;              // inverted 64x64 diagonal blocks of L then of U (solve path)
    Buf<double> trsv_inv256;           // full inverses of the 256 x 256 diagonal blocks of L then of U (single-GPU solve)
    Buf<int> trsv_cnt;                 // per-step counters of the solve's launches (near workgroups done), L steps then U steps
    Buf<double> krylov;                // GMRES-IR: (restart + 1) basis vectors
    Buf<double> res_part;              // per-column-chunk partial sums of the residual (deterministic reduction)
    // expert driver (mpf_expert.cpp, solve_ext.hip): partials of the column / row reductions, of the vector reductions, and its vectors
    Buf<double> ext_part, ext_red, ext_vec;
    // blocked multi-right-hand-side solve (mpf_block.cpp, solve_block.hip): right-hand-side tiles, the residual's partial products, the
    // per-column refinement mask
    Buf<double> blk_tiles, blk_part;
    Buf<int> blk_mask;
    // error bounds (mpf_gerfs, solve_bounds.hip): results + partials of the per-column reductions, per-column arguments of the dlacn2 steps
    Buf<double> blk_red;
    Buf<int> blk_colarg;
    // blocked GMRES-IR (blk_gmres_core, solve_gmres.hip; its basis lives in `krylov`): partials of the orthogonalisation, its results
    // [h | h' | ||w||^2], and what the host sends per step ([scale | live] per column; [y | counts] per outer step)
    Buf<double> gm_part, gm_out, gm_ctl;
    // inverse and determinant (mpf_getri.cpp, getri.hip): ceil(N / 256) x 256 x 256 doubles -- L's block inverses transposed, then the
    // 256-row panel of the interchange pass; mpf_getdet's chunk results
    Buf<double> getri_buf;
    // blocked batched expert layer (batched_refine_blocked.hip, vbatched_refine.hip): g per (matrix, column, row) and max |x| per (matrix, column) between
    // the refinement and its bound; the tile maxima of the reduced chains per (matrix[, column], tile)
    Buf<double> rb_g, rb_xm, rb_part;
    // factored 32x32 diagonal tiles of the fp64 panel, parked here until every workgroup of the sub-panel launches has
    // read the UNfactored tile from the matrix (dpanel.hip); one tile per 32 panel columns, grown on demand
    Buf<double> dtiles;
    Buf<float> w32;                    // fp32 working copy of the trailing matrix (fp16 trailing modes, two-level schedule)
    Buf<double> r64;                   // fp64 ROW-major working copy of the trailing matrix (fp64 mode, factor_lookahead_rm)
    bool hgemm_standalone = false;     // set around the fp16 update of a step operator (no panel chain beside it: the persistent kernel may take every CU)
    mpf_p2p_fn p2p_fn = nullptr;       // point-to-point transport of the distributed solves (mpf_dist_set_p2p); null: RCCL's, or none
    void *p2p_user = nullptr;
    double gmres_budget_ms = 0;        // wall-clock limit of mpf_solve_gmres_ir while mpf_gesv runs it (0: none)
    double fp64_rate_tflops = 0;       // last measured fp64-mode factorization rate of this context (N >= 8192; 0: none yet)
    Buf<double> host_A;                // mpf_factor_host's device copy of the caller's matrix, kept between calls
    Buf<int32_t> host_P;               // ... and of the pivot vector
    Buf<double> host_A0;               // ... and the matrix (then the pivot vector) as uploaded, while block rows leave during the factorization
                                       // (rowsink.hip): what a repeated call on the generic pivot path starts from when the caller's buffer is
                                       // already partly results
    Buf<unsigned, true> late_flags;    // 16 pinned host words: LatePlan::flags
    unsigned late_seq = 0;
    struct ColFeed *feed = nullptr;    // mpf_factor_host's upload of late column segments (rowsink.hip)
    struct LatePlan *late = nullptr;   // set by mpf_factor_host around mpf_factor_dev: column segments still on their way up (factor_lookahead_rm takes it)
    struct RowSink *sink = nullptr;    // mpf_factor_host's block-row copies (rowsink.hip); null until the first call that uses it
    Buf<double> rm_tmp;                // its scratch: moved rows of an interchange (2 * HP_MAXCOLS x N) / the panel's L21 row-major
    Buf<double> rm_lt;                 // L21 of the current panel, row-major [rows][nb]
    Buf<double> rm_pair;               // paired phase (factor_rm_pairs): two row-major images [rows][2 nb] of a panel pair's [L(k) | L(k + nb)]
    // generic (global-memory) fp16 pivot path, fp16_panel_generic.hip: packed fp16 panel + per-block candidates
    Buf<unsigned short> g16;
    Buf<unsigned long long> gcand;
    // pivoting fp64 panel, dpivot.hip: per-workgroup candidates with their rows, two launch parities
    Buf<unsigned long long> dpiv;
    // tournament-pivoting fp64 panel, dpivot.hip: two alternating candidate buffers (32 rows with their indices per group) + the winners
    Buf<double> dtp;
    // distributed path (mpf_dist.cpp): RCCL communicator (dlopen'ed), two panel message buffers
    void *rccl_comm = nullptr;
    int rccl_rank = 0, rccl_world = 0;
    long long rccl_bcast_calls = 0, rccl_bcast_bytes = 0, rccl_allreduce_calls = 0, rccl_p2p_calls = 0, rccl_p2p_bytes = 0;   // since mpf_rccl_init
    Buf<double> dist_buf[2];
    // mpf_factor_dist, two-level schedule of the fp16 modes: this rank's fp32 working copy (N rows x local columns, row-major) and
    // the current super-panel's panels as every rank received them (N x sb * nb doubles, column-major, leading dimension N)
    Buf<float> dist_w32;
    Buf<double> dist_spl;
    int hp_resident_per_cu = -1;       // occupancy query of the LDS pivot kernel (cached)
    int hp_win_per_cu = 0;             // ... of its column-window form
    int hp_full_beside_waiter = 0;     // pivot workgroups (full-slab / column-window form) that still fit on a CU that holds one workgroup of
    int hp_win_beside_waiter = 0;      // the gated interchange kernel (from the kernels' own LDS / register footprints)
};

#define MPF_HIP_TRY(ctx, expr)                                                        \
    do {                                                                              \
        hipError_t e_ = (expr);                                                       \
        if (e_ != hipSuccess) {                                                       \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);           \
            return -2;                                                                \
        }                                                                             \
    } while (0)
// a call's error text and code: into the context, or -- a call without one -- into the calling thread's slot (mpf_host.cpp) that
// mpf_last_error(nullptr) reads
std::string &noctx_error();
inline int fail(mpf_ctx *c, int code, const std::string &msg) {
    (c ? c->err : noctx_error()) = msg;
    return code;
}

enum { ATTR_HP = 1, ATTR_DGEMM = 2, ATTR_HGEMM = 4, ATTR_HGEMM256 = 8, ATTR_HGEMM_PP = 16, ATTR_HGEMM16_BIG32 = 32, ATTR_HGEMM16_BIG64 = 64, ATTR_BATCHED = 128, ATTR_VBATCHED = 256, ATTR_BATCHED_REFINE = 512 };
inline bool safe_pivots(const mpf_ctx *c) { return c->tune.safe_pivots != 0; }

// ---- launchers implemented in the .hip files (all asynchronous on `s`) -----------------------
int launch_double_to_fp16(mpf_ctx *c, const double *in, uint16_t *out, int64_t n);
int launch_hdiv(mpf_ctx *c, const uint16_t *a, const uint16_t *b, uint16_t *q, int64_t n);
// LDS-resident pivot kernel (cols <= 256, rows <= 256 x resident workgroups); hgetf2_lds_eligible says whether it may run
// waiters: workgroups of kernels that will WAIT for this launch's progress while it runs (the pipelined chain's gated interchange:
// laswp_gated_grid); they hold CUs the pivot kernel's workgroups -- which must all be resident at once -- cannot use.
// prefer_window_rows > 0: panels of at least that many rows take the column-window form where it fits (fp64 schedules: it leaves
// half of each CU to the update).  The form is chosen per call from these and the occupancy figures: no state is kept between calls.
int launch_hgetf2(mpf_ctx *c, const double *A64, int64_t lda, uint16_t *P16, int64_t ld16, int rows,
                  int cols, int ipiv_offset, int *d_ipiv, uint16_t *out16, int64_t ldo, MovedList *moved, int waiters = 0, int prefer_window_rows = 0);
bool hgetf2_lds_eligible(mpf_ctx *c, int rows, int cols);
// can a panel of that shape run (in either form) beside `waiters` waiting workgroups?  Rows either form can take beside them.
bool hgetf2_fits_beside(mpf_ctx *c, int rows, int cols, int waiters);
long long hgetf2_capacity_rows(mpf_ctx *c, int waiters, int form = 0);
int laswp_gated_footprint(int *lds_bytes, int *vgprs, int *threads);
int laswp_gated_grid(int64_t ncols);
constexpr int HP_FP64_WINDOW_ROWS = 20000;   // fp64 schedules: the column-window form from that many panel rows on (-1 % factor time at N = 32768)
int hp_query_residency(mpf_ctx *c);
// generic pivot path (any shape, no cross-workgroup spinning) and the reference-style sequential interchange that goes with it
// wait (on c->stream, bounded) until the most recent launch_hgetf2 of this context has fixed the pivots of `target` columns
int launch_hgetf2_gate(mpf_ctx *c, int target);
// cols (<= 256) sequential swaps (row k + j <-> d_ipiv[j] - 1) on ncols columns, resolved and applied in one launch
int launch_laswp_block(mpf_ctx *c, double *A, int64_t lda, int64_t ncols, int k, int cols, const int *d_ipiv, int64_t nrows);
int launch_laswp_block_gated(mpf_ctx *c, double *A, int64_t lda, int64_t ncols, int k, int cols, const int *d_ipiv, int64_t nrows, int target);
// one piece of launch_dgetf2_npv: piece 0 = the first 32-column sub-panel, piece s = fused update + sub-panel s; the last piece
// also puts the parked diagonal tiles back.  Only for cols % 32 == 0, cols >= 64 (dgetf2_npv_pieces(cols) > 0).
int dgetf2_npv_pieces(mpf_ctx *c, int cols);
int launch_dgetf2_npv_piece(mpf_ctx *c, double *P, int64_t ld, int rows, int cols, int fused, int info_base, int piece);
int launch_dpanel_tile_copy(mpf_ctx *c, double *dst, int64_t ld, int piece);   // parked factored diagonal tile of a finished piece
int launch_hgetf2_generic(mpf_ctx *c, const double *A64, int64_t lda, uint16_t *P16, int64_t ld16, int rows, int cols,
                          int ipiv_offset, int *d_ipiv, uint16_t *out16, int64_t ldo);
int launch_laswp_seq(mpf_ctx *c, double *A, int64_t lda, int64_t ncols, int k, int cols, const int *d_ipiv, int64_t nrows);
// row interchange of `ncols` columns from a moved-row list left by the pivot kernel (fused LASWP plan)
int launch_laswp_from_list(mpf_ctx *c, double *A, int64_t lda, int64_t ncols, const MovedList *ml);
int launch_laswp_from_list_hole(mpf_ctx *c, double *A, int64_t lda, int64_t ncols, const MovedList *ml, int64_t hole_from, int64_t hole_len);
// deferred interchanges of everything LEFT of each panel: one composite permutation per column block, applied at
// the end of the factorization (lists[p] = moved rows of panel p, p = 0..npanels-1)
int launch_lazy_left_swaps(mpf_ctx *c, double *A, int64_t lda, int64_t N, int nb, int npanels, const MovedList *lists, int sb = 1,
                           int world = 1, int rank = 0);
int64_t lazy_snap_elems(int64_t N, int nb, int npanels, int sb);   // ints of mpf_ctx::lazy_snap its one-pass form needs
// mpf_factor_host -> factor_lookahead_rm: the matrix's columns from c0[0] on are still being uploaded when the factorization starts.
// Segment i = columns [c0[i], c0[i + 1]) (the last one ends at N); the panels [0, q[i]) are factored on the columns left of it, then
// the segment -- in d_A once flags[i] == seq -- receives those panels' interchange / TRSM / update one after the other (per element
// the same operations in the same order: same bits), and the loop goes on with the wider matrix.
struct LatePlan {
    int nseg = 0;
    int64_t c0[4] = {0, 0, 0, 0};
    int q[4] = {0, 0, 0, 0};
    unsigned *flags = nullptr;         // pinned host words the device can read
    unsigned seq = 0;
    double *snapshot = nullptr;        // where the uploaded matrix is kept (mpf_ctx::host_A0), or null
    bool taken = false;
    bool snapped[4] = {false, false, false, false};
};
int launch_late_wait(mpf_ctx *c, const unsigned *flag, unsigned seq);   // the stream waits (bounded) until *flag == seq; a give-up lands in ws->flags[1]
int feed_start(mpf_ctx *c, const double *A_host, double *d_A, int64_t N, LatePlan *lp);   // uploads the plan's segments from a thread of its own
int feed_finish(mpf_ctx *c);           // joins it; 0 or -2
void feed_destroy(mpf_ctx *c);
void feed_trim(mpf_ctx *c);
// rowsink.hip: finished block rows of the factors to the caller's host matrix while the factorization runs (mpf_factor_host)
int sink_attach(mpf_ctx *c, double *A_host, int64_t N, int nb);
bool sink_take(mpf_ctx *c, const double *d_A, int64_t lda, int64_t N, int nb);
void sink_notify(mpf_ctx *c, int upto_panel, hipStream_t stream);
hipError_t sink_stream_wait(mpf_ctx *c, hipStream_t stream);   // hipStreamSynchronize, or polling while the sink's thread copies
int sink_finish(mpf_ctx *c, int *panels_sent);
void sink_destroy(mpf_ctx *c);
void sink_trim(mpf_ctx *c);
int launch_laswp(mpf_ctx *c, double *A, int64_t lda, int64_t ncols, int k, int cols, const int *d_ipiv);
// resolve a panel's sequential swap list (<= 256 swaps, global 1-based pivots) into a moved-row list
int launch_laswp_plan(mpf_ctx *c, const int *d_ipiv, int k, int cols, MovedList *out);
int launch_dgetf2_npv(mpf_ctx *c, double *P, int64_t ld, int rows, int cols, int fused, int info_base);
// dpivot.hip: LAPACK dgetf2 on the panel (fp64 pivot search, launch_dgetf2_npv's arithmetic); d_ipiv[j] = pivot row + 1 + ipiv_offset
// for j < min(rows, cols); first zero pivot into the workspace's info word as launch_dgetf2_npv.  _reserve: its scratch for panels of
// up to `rows` rows, so that a factorization allocates once, before its first launch
int launch_dgetf2_piv(mpf_ctx *c, double *P, int64_t ld, int rows, int cols, int fused, int info_base, int ipiv_offset, int *d_ipiv);
int dgetf2_piv_reserve(mpf_ctx *c, int rows);
// dpivot.hip: the same panel with tournament pivoting (mpf_dgetf2_tp's rule): the same arguments, the same info word
int launch_dgetf2_tp(mpf_ctx *c, double *P, int64_t ld, int rows, int cols, int fused, int info_base, int ipiv_offset, int *d_ipiv);
int dgetf2_tp_reserve(mpf_ctx *c, int rows);
int launch_dtrsm_llnu(mpf_ctx *c, int m, int64_t n, const double *L, int64_t ldl, double *B, int64_t ldb);
int launch_dgemm_minus(mpf_ctx *c, int64_t m, int64_t n, int k, const double *A, int64_t lda,
                       const double *B, int64_t ldb, double *C, int64_t ldc);
// fp16-in / fp32-accumulate trailing update (trailing_f16.hip); operand images live in c->h_L / c->h_U
int launch_cvt_l21(mpf_ctx *c, const double *A, int64_t lda, int64_t m, int K, int split, int img = 0, int64_t elem_off = 0);
int launch_hgemm_minus(mpf_ctx *c, int64_t m, int64_t n, int K, const double *B, int64_t ldb, double *C, int64_t ldc,
                       int split, int img = 0, int64_t elem_off = 0);
int launch_hgemm_minus_w32(mpf_ctx *c, int64_t m, int64_t n, int K, const double *B, int64_t ldb, float *C, int64_t ldc,
                           int split, int img = 0, int64_t elem_off = 0);
// the two halves of launch_hgemm_minus[_w32]: U12 -> fp16 image in c->h_U, then the MFMA kernel on ready images
// (images may be blocks of wider ones: element offsets into the buffers and row strides; 0 = the padded K itself)
int launch_cvt_u12(mpf_ctx *c, const double *B, int64_t ldb, int K, int64_t n, int split, int64_t elem_off = 0, int kstride = 0);
int launch_hgemm_images(mpf_ctx *c, int64_t m, int64_t n, int K, void *C, int64_t ldc, bool c32, int split, int img = 0, int64_t elem_off = 0,
                        int64_t u_off = 0, int ksL = 0, int ksU = 0);
struct HgemmImages { const unsigned short *Lh = nullptr, *Ll = nullptr, *Uh = nullptr, *Ul = nullptr; int ksL = 0, ksU = 0; };
int launch_hgemm_ptrs(mpf_ctx *c, int64_t m, int64_t n, int K, const HgemmImages &im, void *C, int64_t ldc, bool c32, int split);
// hgemm16.hip: the plain-operand updates on v_mfma_f32_16x16x32_f16 (big-K tile kernel; fp32 copy or fp64 matrix)
int launch_hgemm16_big(mpf_ctx *c, int64_t m, int64_t n, int Kp, const HgemmImages &im, void *C, int64_t ldc, bool c32);
int launch_hgemm16_ring(mpf_ctx *c, int64_t m, int64_t n, int Kp, const HgemmImages &im, void *C, int64_t ldc, bool c32);
// hgemm_pp.hip: the big-K update on the fp32 copy (persistent workgroups, ping-pong wave groups); Kp = padded K
int launch_hgemm_pp(mpf_ctx *c, int64_t m, int64_t n, int Kp, const HgemmImages &im, float *C, int64_t ldc);
// C is ROW-major fp32 (element (i, j) at Crm[i * ldrow + j]): the fp32 working copy of the two-level schedule
int launch_hgemm_images_rowmajor(mpf_ctx *c, int64_t m, int64_t n, int K, float *Crm, int64_t ldrow, int split, int img = 0, int64_t elem_off = 0,
                                 int64_t u_off = 0, int ksL = 0, int ksU = 0);
int launch_laswp_from_list_f32(mpf_ctx *c, float *A, int64_t lda, int64_t ncols, const MovedList *ml);
// fp64 row-major working copy of the fp64 mode (factor_lookahead_rm): interchange of contiguous rows, window transposes
int launch_laswp_from_list_rm64(mpf_ctx *c, double *R, int64_t ldr, int64_t ncols, const MovedList *ml, int64_t scratch_off = 0);
int launch_transpose64(mpf_ctx *c, double *A, int64_t lda, double *R, int64_t ldr, int64_t rows, int64_t cols, bool to_rowmajor);
// dtrsm_llnu on a right-hand side with arbitrary strides: element (row, col) at B[row * rs + col * cs]
int launch_dtrsm_llnu_strided(mpf_ctx *c, int m, int64_t n, const double *L, int64_t ldl, double *B, int64_t rs, int64_t cs);
int launch_cvt_f64_f32(mpf_ctx *c, const double *A, int64_t lda, float *W, int64_t ldw, int64_t rows, int64_t cols);
int launch_cvt_f32_f64(mpf_ctx *c, const float *W, int64_t ldw, double *A, int64_t lda, int64_t rows, int64_t cols);
// solve helpers (ir.hip)
int launch_gather_rows(mpf_ctx *c, const double *in, const int *perm, double *out, int64_t n);
int launch_residual(mpf_ctx *c, const double *A, int64_t lda, const double *x, const double *b, double *r,
                    int64_t n);
int launch_residual_rect(mpf_ctx *c, const double *A, int64_t lda, const double *x, const double *b, double *r, int64_t n, int64_t ncols);
int launch_trsv_prepare_cols(mpf_ctx *c, const double *LUb, int64_t ld, int64_t n, int64_t k0, int w);
int launch_trsv_lower_cols(mpf_ctx *c, const double *LUb, int64_t ld, double *x, int64_t n, int64_t k0, int w);
int launch_trsv_upper_cols(mpf_ctx *c, const double *LUb, int64_t ld, double *x, int64_t n, int64_t k0, int w);
extern "C" {
int mpf_ensure_h_images(mpf_ctx *c, int64_t rows, int kmax, bool big); // internal (not in mpf_c.h): fp16 operand images
int mpf_ensure_solve_buf(mpf_ctx *c, int64_t n);                        // internal: solve scratch
int mpf_ensure_rowmajor_copy(mpf_ctx *c, int64_t rows, int64_t cols, int32_t nb);   // internal: fp64 row-major working copy + its scratch (non-zero: no room)
// internal: before a factorization (mpf_factor_dev, mpf_factor_dist) -- with `lists`, the per-panel moved-row lists (cleared) and the scratch
// of the deferred left-hand interchanges; always the first-zero-pivot word (INT_MAX) and the pivot kernel's give-up counter (0)
int mpf_factor_setup(mpf_ctx *c, int64_t N, int32_t nb, int32_t npanels, bool lists);
}
int launch_trsv_prepare(mpf_ctx *c, const double *LU, int64_t ld, int64_t n);
int launch_trsv_lower_unit(mpf_ctx *c, const double *LU, int64_t ld, double *x, int64_t n);
int launch_trsv_upper(mpf_ctx *c, const double *LU, int64_t ld, double *x, int64_t n);
int launch_axpy(mpf_ctx *c, double alpha, const double *x, double *y, int64_t n);
int launch_norm2(mpf_ctx *c, const double *x, int64_t n, double *d_out);
int launch_dot(mpf_ctx *c, const double *x, const double *y, int64_t n, double *d_out);
int launch_scal(mpf_ctx *c, double alpha, double *x, int64_t n);
// shared by the solve entry points (mpf_solve.cpp, mpf_expert.cpp): the pivot sequence as a gather index in c->perm_buf and the
// factors' inverted diagonal blocks (launch_trsv_prepare); after the stream has been synchronised, -4 if a bounded wait gave up
int solve_setup(mpf_ctx *c, const double *d_LU, int64_t ldlu, const int32_t *d_ipiv, int64_t N);
int solve_check_waits(mpf_ctx *c);
// expert driver kernels (solve_ext.hip).  Transposed solves with the packed factors, in place on x (prepared as for the plain ones):
int launch_trsv_upper_t(mpf_ctx *c, const double *LU, int64_t ld, double *x, int64_t n);        // U^T w = x
int launch_trsv_lower_unit_t(mpf_ctx *c, const double *LU, int64_t ld, double *x, int64_t n);   // L^T z = x
int launch_scatter_rows(mpf_ctx *c, const double *in, const int *perm, double *out, int64_t n); // out[perm[i]] = in[i]
int launch_residual_t(mpf_ctx *c, const double *A, int64_t lda, const double *x, const double *b, double *r, int64_t n);   // r = b - A^T x
int launch_col_abs_sums(mpf_ctx *c, const double *A, int64_t lda, int64_t m, int64_t n, double *out);
int launch_col_sumsq(mpf_ctx *c, const double *A, int64_t lda, int64_t m, int64_t n, double *out);
int launch_col_max_abs(mpf_ctx *c, const double *A, int64_t lda, int64_t m, int64_t n, const double *rs, double *out);   // max_i |a_ij| rs_i
int launch_row_abs_sums(mpf_ctx *c, const double *A, int64_t lda, int64_t m, int64_t n, double *out);
int launch_row_max_abs(mpf_ctx *c, const double *A, int64_t lda, int64_t m, int64_t n, double *out);
int launch_vec_sum(mpf_ctx *c, const double *x, int64_t n, double *d_out);
int launch_vec_max(mpf_ctx *c, const double *x, int64_t n, double *d_out);
int launch_dasum(mpf_ctx *c, const double *x, int64_t n, double *d_out);
int launch_lacn2_sign(mpf_ctx *c, const double *x, const double *isgn, int64_t n, double *xs, double *d_out);
int launch_idamax(mpf_ctx *c, const double *x, int64_t n, double *d_out);
int launch_lacn2_fill(mpf_ctx *c, double *x, int64_t n, int kind, int64_t j);
int launch_diag_zero(mpf_ctx *c, const double *LU, int64_t ld, int64_t n, double *d_out);
int launch_pow2_scale(mpf_ctx *c, const double *m, int64_t n, double *s, double *d_stats);
int launch_scaled_copy(mpf_ctx *c, const double *A, int64_t lda, const double *r, const double *cs, double *W, int64_t ldw, int64_t m, int64_t n);
int launch_vscale(mpf_ctx *c, const double *x, const double *s, double alpha, double *y, int64_t n);
// reciprocal pivot growth (mpf_gerpvgrw).  launch_pivot_growth_cols: q[j] = amax_j / umax_j with amax_j = max_i (|a_ij| r_i) c_j (r / cs
// null: 1) and umax_j = max_{i <= j} |lu_ij|; 1 where umax_j = 0 (the column is skipped), NaN where either maximum is.
// launch_vec_min1: d_out[0] = min(1, min_j q[j]), a NaN kept
int launch_pivot_growth_cols(mpf_ctx *c, const double *A, int64_t lda, const double *LU, int64_t ldlu, int64_t n, const double *r,
                             const double *cs, double *q);
int launch_vec_min1(mpf_ctx *c, const double *q, int64_t n, double *d_out);
// blocked multi-right-hand-side solve (solve_block.hip).  Tiles: BLK_T columns each, column-major with ld = N rounded up to 256, rows
// beyond N zero.  launch_blk_tri: which 0 = L, 1 = U, 2 = U^T, 3 = L^T on x (consumed) -> y, factors prepared by launch_trsv_prepare
constexpr int BLK_T = 32;
int launch_blk_tri(mpf_ctx *c, const double *LU, int64_t ld, int64_t n, int which, double *x, double *y, int64_t ldt, int ntiles);
int launch_blk_residual(mpf_ctx *c, const double *A, int64_t lda, int64_t n, bool trans, const double *X, const double *B, double *R,
                        int64_t ldt, int ntiles);   // R = B - op(A) X
// load / store: `scale` (optional, n doubles, powers of two) multiplies each element by the scale of its MATRIX row, perm[i] or i;
// null is the unscaled kernel (a template instance of its own)
int launch_blk_load(mpf_ctx *c, const double *src, int64_t lds, const int *perm, int64_t n, int64_t ncols, double *t, int64_t ldt, int ntiles,
                    const double *scale = nullptr);
int launch_blk_store(mpf_ctx *c, const double *t, int64_t ldt, const int *perm, int64_t n, int64_t ncols, double *dst, int64_t ldd,
                     const double *scale = nullptr);
int launch_blk_masked_axpy(mpf_ctx *c, const double *d, const int *mask, double *x, int64_t ldt, int ntiles);
// error bounds (mpf_gerfs).  R = B - op(A) X, W = |B| + |op(A)| |X|, Q = dgerfs's backward-error ratio per element: one pass over op(A)
int launch_blk_residual_bound(mpf_ctx *c, const double *A, int64_t lda, int64_t n, bool trans, const double *X, const double *B, double *R,
                              double *W, double *Q, int64_t ldt, int ntiles, double safe1, double safe2);
// solve_bounds.hip: per-column reductions into c->blk_red (what: 0 max |t|, 1 sum |t| + sign mismatches against sg, 2 first argmax |t| +
// T[at[col], col]) and the elementwise steps of the batched dlacn2
int launch_blk_col_reduce(mpf_ctx *c, int what, const double *T, int64_t ldt, int64_t n, int64_t ncols, const double *sg, const int *at);
int launch_blk_scale(mpf_ctx *c, double *v, const double *w, int64_t ldt, int ntiles);
int launch_blk_ferr_weight(mpf_ctx *c, const double *r, double *w, int64_t n, int64_t ncols, int64_t ldt, double nzeps, double safe1, double safe2);
int launch_blk_lacn2_fill(mpf_ctx *c, double *v, int64_t n, int64_t ncols, int64_t ldt, const int *kind, const int *at);
int launch_blk_lacn2_sign(mpf_ctx *c, double *v, double *isgn, int64_t n, int64_t ncols, int64_t ldt, const int *live);
// extra-precise refinement (solve_xr.hip).  launch_blk_residual_x: launch_blk_residual with every element accumulated as an unevaluated
// pair of doubles (its partial pairs take 2 x the plain residual's room in c->blk_part).  launch_blk_xr_measure: max |x|, max |d| and
// max |d_i| / |x_i| (DBL_MAX where x_i = 0 != d_i) per column of the tiles X and D, one launch, into c->blk_red (3 x ncols doubles)
int launch_blk_residual_x(mpf_ctx *c, const double *A, int64_t lda, int64_t n, bool trans, const double *X, const double *B, double *R,
                          int64_t ldt, int ntiles);
int launch_blk_xr_measure(mpf_ctx *c, const double *X, const double *D, int64_t ldt, int64_t n, int64_t ncols);
// launch_blk_xr_berr: dgerfs's componentwise backward error per column of the tiles R (residual) and W (|b| + |op(A)| |x|):
// max_i (w_i > safe2 ? |r_i| / w_i : (|r_i| + safe1) / (w_i + safe1)), a NaN kept, one launch, into c->blk_red (ncols doubles)
int launch_blk_xr_berr(mpf_ctx *c, const double *R, const double *W, int64_t ldt, int64_t n, int64_t ncols, double safe1, double safe2);
// mpf_block.cpp: what every core of the blocked solve layer receives.  BlkSys: op(A) = A or A^T (tr), the ORIGINAL matrix and its
// prepared factors (solve_setup) with the preconditioner
//     op(A)^-1 v ~ post .* op(L U, P)^-1 (pre .* v)        (pre / post: scale vectors of the factored matrix Dr A Dc, or null)
// tr = 0: pre = Dr, post = Dc; tr = 1: pre = Dc, post = Dr.  BlkRhs: the right-hand sides and the solutions, column-major.
struct BlkSys { mpf_ctx *c; bool tr; const double *A; int64_t lda; const double *LU; int64_t ldlu; int64_t N; const double *pre, *post; };
struct BlkRhs { int32_t nrhs; const double *B; int64_t ldb; double *X; int64_t ldx; };
// The bodies of mpf_solve_ir_block, mpf_gerfs and mpf_gerfsx / mpf_gerfsx_scaled (ithresh clamped by the caller) after the argument
// checks and solve_setup; `st` holds nrhs zeroed entries; no core synchronises at its end or sets ms_total.  blk_xrefine_core with
// `berr` (host, nrhs doubles): after the loop, dgerfs's backward error of the X it returns (one more pair residual and one ABS pass
// per group); without it the core is mpf_gerfsx's, launch for launch.
int blk_refine_core(const BlkSys &s, const BlkRhs &r, int32_t max_iter, double tol, mpf_ir_stats *st);
int blk_bounds_core(const BlkSys &s, const BlkRhs &r, int32_t itmax, double *ferr, double *berr, mpf_gerfs_stats *st);
int blk_xrefine_core(const BlkSys &s, const BlkRhs &r, int32_t ithresh, double *err_norm, double *err_comp, mpf_gerfsx_stats *st,
                     double *berr = nullptr);
// solve_gmres.hip: the orthogonalisation (classical Gram-Schmidt twice) and the vector updates of the blocked GMRES-IR; basis slot i at
// V + i * vs, tiles as above.  launch_gmres_ortho: W = -W orthogonalised against the slots 0 .. ns - 1 on the columns with live[j] != 0,
// out = [h (ns x tc) | h' (ns x tc) | ||w||^2 (tc)], tc = BLK_T * ntiles; part: gmres_ortho_chunks(ldt) * max(ns, 4) * tc doubles
int gmres_ortho_chunks(int64_t ldt);
int launch_gmres_ortho(mpf_ctx *c, const double *V, int64_t vs, int ns, double *W, int64_t ldt, int64_t n, int ntiles, const int *live,
                       double *part, double *out);
int launch_gmres_append(mpf_ctx *c, const double *src, const double *scale, double *dst, int64_t ldt, int64_t n, int ntiles);   // dst = src * scale[j] where scale[j] != 0
int launch_gmres_xupdate(mpf_ctx *c, const double *V, int64_t vs, const double *y, const int *cnt, double *X, int64_t ldt, int64_t n,
                         int ntiles);   // X[:, j] += sum_{i < cnt[j]} y[i * tc + j] V_i[:, j]
// inverse and determinant from the factors (getri.hip; driver in mpf_getri.cpp).  launch_getri_tri: the block-inverse products in place
// on W -- left: W[r0 .. r0 + w, c0 .. c0 + extent) = G W[same]; right: W[r0 .. r0 + extent, c0 .. c0 + w) = W[same] G^T, G the
// 256 x 256 upper triangular operand (inv(U_kk), or inv(L_jj) transposed by launch_getri_transpose).  launch_getri_permute:
// W[:, j] <- cs .* W[:, src[j]] r[j] through the 256 x n panel T
int launch_getri_init(mpf_ctx *c, double *W, int64_t ld, int64_t n);
int launch_getri_transpose(mpf_ctx *c, const double *inv, double *out, int64_t nblk);
int launch_getri_tri(mpf_ctx *c, bool right, const double *G, double *W, int64_t ld, int64_t r0, int64_t c0, int w, int64_t extent);
int launch_getri_permute(mpf_ctx *c, double *W, int64_t ld, int64_t n, const int *src, const double *r, const double *cs, double *T);
int launch_getdet(mpf_ctx *c, const double *LU, int64_t ld, const int *ipiv, int64_t n, const double *r, const double *cs, double *part,
                  double *out);
// the one step of every determinant's running product (mpf_getdet's order, include/mpf_c.h): (p, e) times m 2^em, p back in [0.5, 1)
template <class E>
__device__ __forceinline__ void mpf_det_step(double &p, E &e, double m, E em) {
    int k;
    p = frexp(p * m, &k);
    e += k + em;
}
// LU of many small matrices (batched.hip; argument checks and chunks in mpf_batched.cpp): one launch each on at most BT_MAX_LAUNCH
// matrices of 1 <= n <= 128.  launch_getrf_batched: mpf_dgetf2_piv's pivots and bits per matrix (n <= 32: 8, 16 or 32 lanes per matrix from
// registers; above: a workgroup per matrix from LDS), info[b] = first zero pivot or 0 when info is not null.  launch_getrs_batched:
// dgetrs per matrix, in place on B, always unfused
constexpr int64_t BT_MAX_LAUNCH = 1 << 22;
int launch_getrf_batched(mpf_ctx *c, double *A, int64_t lda, int64_t strideA, int n, int64_t batch, int *ipiv, int64_t strideP, int *info,
                         int fused);
int launch_getrs_batched(mpf_ctx *c, int trans, const double *LU, int64_t ldlu, int64_t strideLU, int n, int64_t batch, const int *ipiv,
                         int64_t strideP, int nrhs, double *B, int64_t ldb, int64_t strideB);
// launch_getri_batched: inv[b] = launch_getrs_batched(trans = 0)'s bits on an identity, out of place; a matrix with a zero on U's
// diagonal is left untouched, info[b] (when not null) = the first such i + 1 or 0.  launch_getdet_batched: mpf_getdet's order per matrix
int launch_getri_batched(mpf_ctx *c, const double *LU, int64_t ldlu, int64_t strideLU, int n, int64_t batch, const int *ipiv, int64_t strideP,
                         double *inv, int64_t ldinv, int64_t strideInv, int *info);
int launch_getdet_batched(mpf_ctx *c, const double *LU, int64_t ldlu, int64_t strideLU, int n, int64_t batch, const int *ipiv, int64_t strideP,
                          double *mant, int *expo);
// The expert layer on the same strided batches (batched_refine.hip; checks and chunks in mpf_batched.cpp), 1 <= n <= 128, one launch each.
// launch_lange_batched: mode 0 = '1', 1 = 'I', 2 = 'M'.  launch_gecon_batched: the exact norm of (L U)^-1 (inf = 0: '1', 1: 'I'), rcond
// and, when not null, ainvnm per matrix.  launch_residual_batched: at most BR_MAX_UNITS (matrix, column) pairs; W may be null.
// launch_gerfs_batched: itmax already resolved (1 .. 31); ferr and iters may be null.
constexpr int64_t BR_MAX_UNITS = 1 << 30;
int launch_lange_batched(mpf_ctx *c, int mode, const double *A, int64_t lda, int64_t strideA, int n, int64_t batch, double *out);
int launch_gecon_batched(mpf_ctx *c, int inf, const double *LU, int64_t ldlu, int64_t strideLU, int n, int64_t batch, const double *anorm,
                         double *rcond, double *ainvnm);
int launch_residual_batched(mpf_ctx *c, int trans, const double *A, int64_t lda, int64_t strideA, int n, int64_t batch, int nrhs,
                            const double *X, int64_t ldx, int64_t strideX, const double *B, int64_t ldb, int64_t strideB, double *R,
                            int64_t ldr, int64_t strideR, double *W);
int launch_gerfs_batched(mpf_ctx *c, int trans, const double *A, int64_t lda, int64_t strideA, const double *LU, int64_t ldlu,
                         int64_t strideLU, int n, int64_t batch, const int *ipiv, int64_t strideP, int nrhs, const double *B, int64_t ldb,
                         int64_t strideB, double *X, int64_t ldx, int64_t strideX, int itmax, double *ferr, double *berr, int *iters);
// The same for matrices of different orders (vbatched.hip; descriptor and chunks in mpf_batched.cpp, host plan in vbatch_plan.h): one
// launch each on `count` <= BT_MAX_LAUNCH entries of one class list.  BtRagged: the descriptor's device arrays, indexed by matrix;
// idx[i] = the matrix of list entry i; top = the class's largest order (8, 16, 32: wave forms; 48, 64, 96, 128: workgroup forms),
// nmax = the largest order in the list (sizes the dynamic LDS).  The vectors (ipiv, B's rows) lie at offv[b].
struct BtRagged { const int32_t *n; const int64_t *off, *ld, *offv; };
int launch_getrf_vbatched(mpf_ctx *c, const BtRagged &v, const int32_t *idx, int64_t count, int top, int nmax, double *A, int *ipiv, int *info,
                          int fused);
int launch_getrs_vbatched(mpf_ctx *c, const BtRagged &v, const int32_t *idx, int64_t count, int top, int nmax, int trans, const double *LU,
                          const int *ipiv, int nrhs, double *B, int64_t ldb);
int launch_getri_vbatched(mpf_ctx *c, const BtRagged &v, const int32_t *idx, int64_t count, int top, int nmax, const double *LU,
                          const int *ipiv, double *inv, int *info);
int launch_getdet_vbatched(mpf_ctx *c, const BtRagged &v, const int32_t *idx, int64_t count, int top, const double *LU, const int *ipiv,
                           double *mant, int *expo);
// the matrices of order 0: info[b] = 0 (when info is not null), (mant[b], expo[b]) = (0.5, 1) (when mant is not null)
int launch_vbatched_empty(mpf_ctx *c, const int32_t *idx, int64_t count, int *info, double *mant, int *expo);
// Blocked LU of many matrices of 1 <= n <= 1024 (batched_blocked.hip, bodies in batched_blocked_body.h; checks, chunks and forwarding
// in mpf_batched.cpp on the rules of batch_args.h): at most
// BB_MAX_LAUNCH matrices per call (the batch is a grid's second dimension).  launch_getrf_batched_blocked: the right-looking loop over
// panels of nb = 8, 16 or 32 columns -- panel, row block, trailing update, each ONE launch for the whole batch; valu != 0: the fused
// update on the VALU kernel; stages: bit 0 panel, 1 row block, 2 update (7 everywhere but in the probe library's per-stage timing).
// launch_getrs_batched_blocked: launch_getrs_batched's chains, one workgroup per (matrix, column tile).
constexpr int64_t BB_MAX_LAUNCH = 1 << 15;
constexpr int BB_MAXN = 1024;
int launch_getrf_batched_blocked(mpf_ctx *c, double *A, int64_t lda, int64_t strideA, int n, int64_t batch, int *ipiv, int64_t strideP,
                                 int *info, int fused, int nb, int valu, int stages);
int launch_getrs_batched_blocked(mpf_ctx *c, int trans, const double *LU, int64_t ldlu, int64_t strideLU, int n, int64_t batch,
                                 const int *ipiv, int64_t strideP, int nrhs, double *B, int64_t ldb, int64_t strideB);
// launch_getri_batched_blocked: launch_getrs_batched_blocked(trans = 0)'s bits on an identity that is never formed, out of place, one
// workgroup per (matrix, tile of ct = 8 or 16 columns of inv(L); anything else: automatic); a matrix with a zero on U's diagonal is
// left untouched, info[b] (when not null) = the first such i + 1 or 0.  launch_getdet_batched_blocked: mpf_getdet's order per matrix
// (up to four chunks of 256), one workgroup per matrix.
int launch_getri_batched_blocked(mpf_ctx *c, const double *LU, int64_t ldlu, int64_t strideLU, int n, int64_t batch, const int *ipiv,
                                 int64_t strideP, double *inv, int64_t ldinv, int64_t strideInv, int *info, int ct);
int launch_getdet_batched_blocked(mpf_ctx *c, const double *LU, int64_t ldlu, int64_t strideLU, int n, int64_t batch, const int *ipiv,
                                  int64_t strideP, double *mant, int *expo);
// The expert layer on those batches (batched_refine_blocked.hip): launch_lange_batched's, launch_gecon_batched's,
// launch_residual_batched's and launch_gerfs_batched's arguments and bits for 1 <= n <= 1024, at most BB_MAX_LAUNCH matrices per call.
// Workspace (grow-only, in the context): gecon one double per (matrix, tile of chains); gerfs with ferr n + 1 doubles per (matrix,
// column) and one per (matrix, column, tile).  Nothing is proportional to n^2.
int launch_lange_batched_blocked(mpf_ctx *c, int mode, const double *A, int64_t lda, int64_t strideA, int n, int64_t batch, double *out);
int launch_gecon_batched_blocked(mpf_ctx *c, int inf, const double *LU, int64_t ldlu, int64_t strideLU, int n, int64_t batch,
                                 const double *anorm, double *rcond, double *ainvnm);
int launch_residual_batched_blocked(mpf_ctx *c, int trans, const double *A, int64_t lda, int64_t strideA, int n, int64_t batch, int nrhs,
                                    const double *X, int64_t ldx, int64_t strideX, const double *B, int64_t ldb, int64_t strideB, double *R,
                                    int64_t ldr, int64_t strideR, double *W);
int launch_gerfs_batched_blocked(mpf_ctx *c, int trans, const double *A, int64_t lda, int64_t strideA, const double *LU, int64_t ldlu,
                                 int64_t strideLU, int n, int64_t batch, const int *ipiv, int64_t strideP, int nrhs, const double *B,
                                 int64_t ldb, int64_t strideB, double *X, int64_t ldx, int64_t strideX, int itmax, double *ferr, double *berr,
                                 int *iters);
// The same for matrices of different orders (vbatched_blocked.hip, on the same bodies of batched_blocked_body.h; descriptor, groups
// and chunks in mpf_batched.cpp): `count` <= BB_MAX_LAUNCH entries of a list ordered by n, idx[i] = the matrix of entry i, nmax = the
// largest order among them.  launch_getrf_vbatched_blocked_step: ONE panel step of the right-looking loop at column j0 (a multiple of nb = 8, 16 or
// 32, as vbatched_blocked_nb resolves the option) over the entries still active there (n > j0; vbatch_plan.h: factor_steps) -- panel,
// row block, trailing update, each one launch sized for nmax.  The other three: one launch each, sized for nmax.
int vbatched_blocked_nb(int nb);
int launch_getrf_vbatched_blocked_step(mpf_ctx *c, const BtRagged &v, const int32_t *idx, int64_t count, int nmax, int j0, int nb, double *A,
                                       int *ipiv, int *info, int fused, int valu, int stages);
int launch_getrs_vbatched_blocked(mpf_ctx *c, const BtRagged &v, const int32_t *idx, int64_t count, int nmax, int trans, const double *LU,
                                  const int *ipiv, int nrhs, double *B, int64_t ldb);
int launch_getri_vbatched_blocked(mpf_ctx *c, const BtRagged &v, const int32_t *idx, int64_t count, int nmax, const double *LU,
                                  const int *ipiv, double *inv, int *info, int ct);
int launch_getdet_vbatched_blocked(mpf_ctx *c, const BtRagged &v, const int32_t *idx, int64_t count, const double *LU, const int *ipiv,
                                   double *mant, int *expo);
// The expert layer for matrices of different orders (vbatched_refine.hip, on the bodies of batched_refine_blocked_body.h that
// batched_refine_blocked.hip calls too; launch groups: vbatch_plan.h refine_chunks): `count` <= BB_MAX_LAUNCH entries of a list ordered
// by n, every order >= 1, nmax the largest.  RbvWork: where the launch's chunk keeps its workspace -- row / tile point at the chunk's first
// entry of the descriptor's prefix sums (orders and tiles of 16 chains of the entries before a list position), row0 / tile0 are their
// values there; part: one double per tile (gecon) or nrhs per tile (ferr), g: nrhs per row, xm: nrhs per entry of the chunk.
// launch_refine_vbatched_empty: the order-0 matrices' outputs, whichever are not null (norm 0, rcond 1, ainvnm 0, berr = ferr = iters = 0)
struct RbvWork { const int64_t *row, *tile; int64_t row0, tile0; double *part, *g, *xm; };
int launch_lange_vbatched(mpf_ctx *c, const BtRagged &v, const int32_t *idx, int64_t count, int nmax, int mode, const double *A, double *out);
int launch_gecon_vbatched(mpf_ctx *c, const BtRagged &v, const int32_t *idx, const RbvWork &w, int64_t count, int nmax, int inf, const double *LU,
                          const double *anorm, double *rcond, double *ainvnm);
int launch_residual_vbatched(mpf_ctx *c, const BtRagged &v, const int32_t *idx, int64_t count, int nmax, int trans, const double *A, int nrhs,
                             const double *X, int64_t ldx, const double *B, int64_t ldb, double *R, int64_t ldr, double *W);
int launch_gerfs_vbatched(mpf_ctx *c, const BtRagged &v, const int32_t *idx, const RbvWork &w, int64_t count, int nmax, int trans, const double *A,
                          const double *LU, const int *ipiv, int nrhs, const double *B, int64_t ldb, double *X, int64_t ldx, int itmax,
                          double *ferr, double *berr, int *iters);
int launch_refine_vbatched_empty(mpf_ctx *c, const int32_t *idx, int64_t count, int nrhs, double *norm, double *rcond, double *ainvnm,
                                 double *berr, double *ferr, int *iters);
// Equilibration of those batches (batched_equil.hip; checks and chunks in mpf_batched.cpp).  launch_geequ_batched: 1 <= n <= 128, at most
// BT_MAX_LAUNCH matrices, A read once.  launch_geequ_batched_blocked / launch_geequ_vbatched: any order up to 1024, at most BB_MAX_LAUNCH
// matrices or list entries (every order >= 1), four launches; rk, ck: one double-sized word per row of the launch each (ragged: entry i's
// at row[i] - row0, the descriptor's prefix sums as in RbvWork).  launch_laqge_decide: equed and, when not null, spread of `count` matrices
// (idx null: matrices 0 .. count-1 of order n; else list entries of any order, v the descriptor's arrays).  launch_laqge_batched and
// launch_lascl2_batched: one thread per element, fewer than 2^31 elements per call.  out may be A itself.
int launch_geequ_batched(mpf_ctx *c, const double *A, int64_t lda, int64_t stride, int n, int64_t batch, double *r, double *cs, double *rowcnd,
                         double *colcnd, double *amax, int *info);
int launch_geequ_batched_blocked(mpf_ctx *c, const double *A, int64_t lda, int64_t stride, int n, int64_t batch, double *r, double *cs,
                                 double *rowcnd, double *colcnd, double *amax, int *info, double *rk, double *ck);
int launch_geequ_vbatched(mpf_ctx *c, const BtRagged &v, const int32_t *idx, const int64_t *row, int64_t row0, int64_t count, int nmax,
                          const double *A, double *r, double *cs, double *rowcnd, double *colcnd, double *amax, int *info, double *rk, double *ck);
int launch_geequ_vbatched_empty(mpf_ctx *c, const int32_t *idx, int64_t count, double *rowcnd, double *colcnd, double *amax, int *info);
int launch_laqge_decide(mpf_ctx *c, int rule, int n, int64_t count, const int32_t *idx, const BtRagged *v, const double *r, const double *cs,
                        const double *rowcnd, const double *colcnd, const double *amax, const int *info, int *equed, double *spread);
int launch_laqge_batched(mpf_ctx *c, const double *A, int64_t lda, int64_t stride, int n, int64_t batch, const double *r, const double *cs,
                         const int *equed, double *out);
int launch_laqge_batched_blocked(mpf_ctx *c, const double *A, int64_t lda, int64_t stride, int n, int64_t batch, const double *r, const double *cs,
                                 const int *equed, double *out);
int launch_laqge_vbatched(mpf_ctx *c, const BtRagged &v, const int32_t *idx, int64_t count, int nmax, const double *A, const double *r,
                          const double *cs, const int *equed, double *out);
int launch_lascl2_batched(mpf_ctx *c, const double *s, int n, int64_t batch, int nrhs, double *V, int64_t ldv, int64_t stride, const int *equed,
                          int bit);
int launch_lascl2_vbatched(mpf_ctx *c, const BtRagged &v, const int32_t *idx, int64_t count, int nmax, const double *s, int nrhs, double *V,
                           int64_t ldv, const int *equed, int bit);
// mpf_block.cpp: the body of mpf_solve_gmres_ir_block, as the cores above (no scales); restart and max_outer clamped (gmres_clamp)
int blk_gmres_core(const BlkSys &s, const BlkRhs &r, int32_t max_outer, int32_t restart, double tol, mpf_gmres_stats *st);

// ---- host-side helpers shared by the schedules (mpf_factor.cpp, factor_rm.cpp, mpf_dist.cpp) --------------------------------------------
struct StreamSwap { // launch_* helpers use c->stream: point it at another stream for a scope
    mpf_ctx *c; hipStream_t saved;
    StreamSwap(mpf_ctx *c_, hipStream_t s) : c(c_), saved(c_->stream) { c->stream = s; }
    ~StreamSwap() { c->stream = saved; }
};
struct EvPool { // events are recycled across calls; timing pairs are read after the final synchronise
    mpf_ctx *c; size_t next = 0;
    struct Pair { hipEvent_t a, b; double *acc, *acc2; };
    std::vector<Pair> pairs;
    const double *keep = nullptr;   // the timer that stays on at event_timers = 1 (the schedule's ms_gemm)
    explicit EvPool(mpf_ctx *c_) : c(c_) {}
    hipEvent_t get() {
        if (next == c->ev_pool.size()) { hipEvent_t e; hipEventCreate(&e); c->ev_pool.push_back(e); }
        return c->ev_pool[next++];
    }
    int timed(double &acc, hipStream_t s, const std::function<int()> &fn, double *also = nullptr) {
        // option event_timers: 2 = every region, 1 = only the trailing updates (default: what the roofline needs), 0 = none.  A pair of
        // events around every small launch of the chain costs ~8 ms per factorization at N = 32768 (fp16 mode: 152 -> 145 ms)
        const int lvl = c->tune.timeline ? 2 : c->tune.event_timers;
        if (lvl == 0 || (lvl == 1 && &acc != keep)) return fn();
        hipEvent_t a = get(), b = get();
        hipEventRecord(a, s);
        int rc = fn();
        hipEventRecord(b, s);
        pairs.push_back({a, b, &acc, also});   // `also`: a second timer the same region is booked under (a sub-total)
        return rc;
    }
    void collect() {
        for (auto &p : pairs) { float ms = 0; if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) { *p.acc += ms; if (p.acc2) *p.acc2 += ms; } }
        if (!pairs.empty() && c->tune.timeline) { // diagnostic: every timed region as (start, end) in ms since the first one
            const double *base = pairs[0].acc;
            for (auto &p : pairs) if (p.acc < base) base = p.acc;
            for (auto &p : pairs) {
                float t0 = 0, t1 = 0;
                hipEventElapsedTime(&t0, pairs[0].a, p.a);
                hipEventElapsedTime(&t1, pairs[0].a, p.b);
                fprintf(stderr, "TL %d %.4f %.4f\n", (int)(p.acc - base), t0, t1);
            }
        }
    }
};

// bookkeeping of one trailing-update launch timed under ms_gemm: flops and algorithmic HBM bytes (every fp64 element of the
// block read and written once + the operands in the form the kernel reads them: fp64, fp16 images, or hi + lo images)
inline void count_gemm(mpf_stats &st, const mpf_opts &o, int64_t m, int64_t n, int64_t k, double c_bytes = 16.0) {
    if (m <= 0 || n <= 0 || k <= 0) return;
    st.gemm_flops += 2.0 * (double)m * (double)n * (double)k;
    const double opb = o.trailing == MPF_TRAIL_FP64 ? 8.0 : (o.trailing == MPF_TRAIL_FP16X3 ? 4.0 : 2.0);
    st.gemm_bytes += c_bytes * (double)m * (double)n + opb * (double)k * (double)(m + n);   // c_bytes = 8: fp32 working copy
    st.gemm_launches++;
}

