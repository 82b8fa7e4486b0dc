// Blocked multi-right-hand-side solve (no reference counterpart; LAPACK dgetrs and block refinement):
//   mpf_getrs            B := A^-1 B or A^-T B with the factors of mpf_factor_dev
//   mpf_solve_ir_block   fp64 refinement of all columns together, per-column rules and stats of mpf_solve_ir_nrhs / _trans
//   mpf_gerfs            LAPACK dgerfs: refinement by the componentwise backward error, berr and the forward bound ferr per column
//   mpf_solve_gmres_ir_block   GMRES-IR (mpf_solve_gmres_ir's method) on all columns of a group in lock-step, op(A) = A or A^T
//   mpf_residual_x, mpf_gerfsx   LAPACK dgerfsx: the residual in pairs of doubles, refinement steered by the corrections' size
//   mpf_gerfsx_scaled    the same on the factors of an equilibrated copy Dr A Dc, with dgerfs's berr of the returned X
// Each of the four refinements is a core (blk_refine_core, blk_bounds_core, blk_xrefine_core, blk_gmres_core) on a system (BlkSys:
// A, its prepared factors, optional scale vectors for the factors of an equilibrated copy Dr A Dc) and its right-hand sides (BlkRhs);
// mpf_gesvx_block and mpf_gesvxx_block (mpf_expert.cpp) call the first three with their scales, the public functions here with none
// (mpf_gerfsx_scaled: the caller's), through solve_entry.
// Around the per-column rules of solve_rules.h every core has the same three frames, each written once:
//   for_groups / for_rhs_groups   the right-hand sides go through the device in groups of at most GROUP_TILES tiles of BLK_T columns
//                                 (solve_block.hip); every triangular step and every residual is one pass over the factor block / over
//                                 A for the whole group
//   LockStep                      the columns of a group step together; a column whose rule has stopped it is frozen by a mask
//   solve_entry                   argument checks, solve_setup, the core, timing, stats, return value
#include "solve_common.h"
#include <algorithm>
#include <cstring>
#include <initializer_list>

namespace {
constexpr int GROUP_TILES = 16;   // 512 columns per group: six N x 512 tile sets of scratch at most (mpf_gerfs; 805 MB at N = 32768)

struct Group {
    int64_t ldt = 0;   // rows of a tile (N rounded up to 256)
    int ntiles = 0;
    double *base = nullptr;
    double *t(int i) const { return base + (int64_t)i * ldt * BLK_T * ntiles; }
    int64_t tcols() const { return (int64_t)BLK_T * ntiles; }
};
// `count` tile sets of `ntiles` tiles, zeroed (the rows beyond N and the columns beyond nrhs stay zero)
int group_tiles(mpf_ctx *c, int64_t N, int ntiles, int count, Group &g) {
    g.ldt = (N + 255) / 256 * 256;
    g.ntiles = ntiles;
    const int64_t len = (int64_t)count * g.ldt * BLK_T * ntiles;
    MPF_HIP_TRY(c, c->blk_tiles.grow(len));
    g.base = c->blk_tiles;
    MPF_HIP_TRY(c, hipMemsetAsync(g.base, 0, (size_t)len * sizeof(double), c->stream));
    return 0;
}
// The group walk: nrhs columns in groups of at most `width` tiles, `sets` zeroed tile sets each; body(g, j0, ncols).
template <class Body>
int for_groups(mpf_ctx *c, int64_t N, int32_t nrhs, int width, int sets, Body body) {
    for (int32_t j0 = 0; j0 < nrhs; j0 += width * BLK_T) {
        const int64_t ncols = std::min<int64_t>(nrhs - j0, (int64_t)width * BLK_T);
        Group g;
        int rc = group_tiles(c, N, (int)((ncols + BLK_T - 1) / BLK_T), sets, g);
        if (!rc) rc = body(g, j0, ncols);
        if (rc) return rc;
    }
    return 0;
}
// columns j0 .. j0 + ncols of a column-major matrix <-> a tile set, rows in the matrix's own order
int load_cols(mpf_ctx *c, const double *M, int64_t ld, int32_t j0, int64_t ncols, int64_t N, double *T, const Group &g) {
    return launch_blk_load(c, M + (int64_t)j0 * ld, ld, nullptr, N, ncols, T, g.ldt, g.ntiles);
}
int store_cols(mpf_ctx *c, const double *T, const Group &g, int64_t N, int32_t j0, int64_t ncols, double *M, int64_t ld) {
    return launch_blk_store(c, T, g.ldt, nullptr, N, ncols, M + (int64_t)j0 * ld, ld);
}
// The walk of a core: B goes into tile set 0 and X into tile set 1 before the body, X is stored from tile set 1 after it, each if asked.
enum { LOAD_B = 1, LOAD_X = 2, STORE_X = 4 };
template <class Body>
int for_rhs_groups(const BlkSys &s, const BlkRhs &r, int width, int sets, int io, Body body) {
    return for_groups(s.c, s.N, r.nrhs, width, sets, [&](const Group &g, int32_t j0, int64_t ncols) {
        int rc = 0;
        if (io & LOAD_B) rc = load_cols(s.c, r.B, r.ldb, j0, ncols, s.N, g.t(0), g);
        if (!rc && (io & LOAD_X)) rc = load_cols(s.c, r.X, r.ldx, j0, ncols, s.N, g.t(1), g);
        if (!rc) rc = body(g, j0, ncols);
        if (!rc && (io & STORE_X)) rc = store_cols(s.c, g.t(1), g, s.N, j0, ncols, r.X, r.ldx);
        return rc;
    });
}

// The columns of a group in lock-step: active[j] while column j's rule lets it go on, and the mask of a step (1 = the column takes
// part) over all tcols columns of the tiles, the padding columns 0.  All columns start active.
struct LockStep {
    mpf_ctx *c;
    std::vector<int> active, mask;
    LockStep(mpf_ctx *c_, int64_t ncols, int64_t tcols) : c(c_), active((size_t)ncols, 1), mask((size_t)tcols, 0) {
        std::fill(mask.begin(), mask.begin() + ncols, 1);
    }
    // rule(j) decides for every column that is still active whether it goes on; a stopped column is never asked again.  The mask
    // becomes the columns that go on; true if there is one.
    template <class Rule>
    bool step(Rule rule) {
        bool any = false;
        for (size_t j = 0; j < active.size(); ++j) {
            if (active[j]) active[j] = rule((int64_t)j) ? 1 : 0;
            mask[j] = active[j];
            any = any || active[j];
        }
        return any;
    }
    // The mask to c->blk_mask, asynchronously from the host vector.  No synchronisation follows it, and none is needed: every caller
    // writes `mask` only in step(), with the values of a read-back (read_back below) that has synchronised the stream after the
    // last upload, and leaves its loop only from such a step -- or says where it does not (blk_xrefine_core).
    int upload() {
        MPF_HIP_TRY(c, c->blk_mask.grow((int64_t)mask.size()));
        MPF_HIP_TRY(c, hipMemcpyAsync(c->blk_mask, mask.data(), mask.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
        return 0;
    }
};

// W <- op^-1 W on prepared factors: P^T-free forms, the permutation is applied by the loads and stores around it; Z scratch
int tile_solve(mpf_ctx *c, const double *LU, int64_t ldlu, int64_t N, bool trans, double *W, double *Z, const Group &g) {
    int rc = launch_blk_tri(c, LU, ldlu, N, trans ? 2 : 0, W, Z, g.ldt, g.ntiles);
    return rc ? rc : launch_blk_tri(c, LU, ldlu, N, trans ? 3 : 1, Z, W, g.ldt, g.ntiles);
}
// out (tiles) <- post .* op(L U, P)^-1 (pre .* src) (tiles), through W / Z: op(A)^-1 src for the factors of A itself (pre = post = null)
// and for those of Dr A Dc (trans = 0: Dc (L U)^-1 P Dr, pre = Dr, post = Dc; trans = 1: Dr P^T (L U)^-T Dc, pre = Dc, post = Dr).
// The scales ride on the load and the store, indexed by the matrix row as the permutation is.  `transposed`: op(A)^-T instead, the
// scales swapped with it.
int tile_getrs(const BlkSys &s, const double *src, double *out, double *W, double *Z, const Group &g, bool transposed = false) {
    mpf_ctx *c = s.c;
    const bool trans = s.tr != transposed;
    const double *pre = transposed ? s.post : s.pre, *post = transposed ? s.pre : s.post;
    int rc = launch_blk_load(c, src, g.ldt, trans ? nullptr : c->perm_buf, s.N, g.tcols(), W, g.ldt, g.ntiles, pre);
    if (!rc) rc = tile_solve(c, s.LU, s.ldlu, s.N, trans, W, Z, g);
    if (!rc) rc = launch_blk_store(c, W, g.ldt, trans ? c->perm_buf : nullptr, s.N, g.tcols(), out, g.ldt, post);
    return rc;
}
// n doubles of a step's result back on the host; the one synchronisation of a step
int read_back(mpf_ctx *c, const double *d_src, size_t n, double *out) {
    MPF_HIP_TRY(c, hipMemcpyAsync(out, d_src, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return 0;
}
int col_norms(mpf_ctx *c, const double *T, const Group &g, int64_t N, int64_t ncols, std::vector<double> &out) {
    int rc = launch_col_sumsq(c, T, g.ldt, N, ncols, c->blk_part);
    out.resize((size_t)ncols);
    if (!rc) rc = read_back(c, c->blk_part, out.size(), out.data());
    if (rc) return rc;
    for (auto &v : out) v = std::sqrt(v);
    return 0;
}
// one per-column reduction of a step (launch_blk_col_reduce) back on the host: `nvals` values per column, out[v * ncols + j]
int col_reduce(mpf_ctx *c, int what, const double *T, const Group &g, int64_t N, int64_t ncols, const double *sg, const int *at, int nvals,
               std::vector<double> &out) {
    int rc = launch_blk_col_reduce(c, what, T, g.ldt, N, ncols, sg, at);
    out.resize((size_t)(nvals * ncols));
    return rc ? rc : read_back(c, c->blk_red, out.size(), out.data());
}

// The argument checks of every entry point, in their order: trans, N / nrhs, the leading dimensions, nrhs == 0, the pointers.
// True: go on.  False: the entry point returns `ret` -- -1 with c->err set, or 0 for nrhs == 0 (nothing to do, nothing is written).
using Ptrs = std::initializer_list<const void *>;
bool blk_args(mpf_ctx *c, const char *who, int32_t trans, int64_t N, int32_t nrhs, std::initializer_list<int64_t> lds, Ptrs ptrs,
              Ptrs more, int &ret) {
    const auto bad = [&](const char *what) { c->err = std::string(who) + what; ret = -1; return false; };
    if (trans != 0 && trans != 1) return bad(": trans must be 0 or 1");
    if (N <= 0 || nrhs < 0) return bad(": N must be positive, nrhs >= 0");
    for (int64_t ld : lds) if (ld < N) return bad(": leading dimension < N");
    ret = 0;
    if (nrhs == 0) return false;
    for (Ptrs l : {ptrs, more})
        for (const void *p : l) if (!p) return bad(": null pointer");
    return true;
}
// The body of an entry point around its core: the checks (A, the factors, B, X and `more` must not be null), the factors' set-up,
// core(st) on nrhs zeroed stats, the wall time into every column's ms_total, the stats out.  Returns an error, else 0 if
// done(st[j]) holds for every column and 1 if not.
template <class Stats, class Core, class Done>
int solve_entry(const char *who, int32_t trans, const BlkSys &s, const BlkRhs &r, const int32_t *d_ipiv, Ptrs more, Stats *stats,
                Core core, Done done) {
    mpf_ctx *c = s.c;
    if (!c) return -1;
    int rc;
    if (!blk_args(c, who, trans, s.N, r.nrhs, {s.ldlu, r.ldb, s.lda, r.ldx}, {s.A, s.LU, d_ipiv, r.B, r.X}, more, rc)) return rc;
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    const auto t0 = std::chrono::steady_clock::now();
    rc = solve_setup(c, s.LU, s.ldlu, d_ipiv, s.N);
    if (rc) return rc;
    std::vector<Stats> st((size_t)r.nrhs);
    rc = core(st.data());
    if (rc) return rc;
    MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));
    const double ms = ms_since(t0);
    bool all = true;
    for (auto &q : st) { q.ms_total = ms; all = all && done(q); }
    if (stats) std::copy(st.begin(), st.end(), stats);
    rc = solve_check_waits(c);
    return rc ? rc : (all ? 0 : 1);
}
} // namespace

// The body of mpf_solve_ir_block (mpf_internal.h): x0 and every correction go through the scaled tile_getrs, the residual is taken
// against the original A; rules, stats and masking per column as documented for mpf_solve_ir_block.
int blk_refine_core(const BlkSys &s, const BlkRhs &r, int32_t max_iter, double tol, mpf_ir_stats *st) {
    mpf_ctx *c = s.c;
    const int64_t N = s.N;
    if (max_iter > 31) max_iter = 31;
    return for_rhs_groups(s, r, GROUP_TILES, 5, LOAD_B | STORE_X, [&](const Group &g, int32_t j0, int64_t ncols) {
        double *Bt = g.t(0), *Xt = g.t(1), *R = g.t(2), *W = g.t(3), *Z = g.t(4);
        MPF_HIP_TRY(c, c->blk_part.grow(g.tcols()));   // (the column norms' output)
        std::vector<double> nb2, nr;
        int rc = col_norms(c, Bt, g, N, ncols, nb2);
        if (!rc) rc = tile_getrs(s, Bt, Xt, W, Z, g);   // x0
        if (rc) return rc;
        for (auto &v : nb2) if (v == 0) v = 1;
        LockStep ls(c, ncols, g.tcols());
        for (int it = 0;; ++it) {
            rc = launch_blk_residual(c, s.A, s.lda, N, s.tr, Xt, Bt, R, g.ldt, g.ntiles);
            if (!rc) rc = col_norms(c, R, g, N, ncols, nr);
            if (rc) return rc;
            // ir_step's rules, column by column; a stopped column is frozen
            if (!ls.step([&](int64_t j) { return ir_step(st[(size_t)(j0 + j)], it, nr[(size_t)j] / nb2[(size_t)j], max_iter, tol); })) break;
            rc = ls.upload();
            if (!rc) rc = tile_getrs(s, R, R, W, Z, g);   // correction d = op^-1 r (into R: r is consumed)
            if (!rc) rc = launch_blk_masked_axpy(c, R, c->blk_mask, Xt, g.ldt, g.ntiles);
            if (rc) return rc;
        }
        return 0;
    });
}

// The body of mpf_gerfs (mpf_internal.h): residual, weights and berr of the ORIGINAL system; corrections and dlacn2's KASE 2 product
// through the scaled tile_getrs, KASE 1 through the transposed one.
int blk_bounds_core(const BlkSys &s, const BlkRhs &r, int32_t itmax, double *ferr, double *berr, mpf_gerfs_stats *st) {
    mpf_ctx *c = s.c;
    const int64_t N = s.N;
    if (itmax <= 0) itmax = 5;
    if (itmax > 31) itmax = 31;
    const double eps = LAPACK_EPS, nz = (double)(N + 1), safe1 = gerfs_safe1(N), safe2 = gerfs_safe2(N);
    // (X is stored in the middle, before the forward bound's kernels, not by the frame)
    return for_rhs_groups(s, r, GROUP_TILES, 6, LOAD_B | LOAD_X, [&](const Group &g, int32_t j0, int64_t ncols) {
        const int64_t tcols = g.tcols();
        // Bt and R are free once the weights of the forward bound stand in Wt: dlacn2's vector and its stored signs take their place
        double *Bt = g.t(0), *Xt = g.t(1), *R = g.t(2), *Wt = g.t(3), *S1 = g.t(4), *S2 = g.t(5), *V = Bt, *Isgn = R;
        MPF_HIP_TRY(c, c->blk_colarg.grow(2 * tcols));
        int *d_kind = c->blk_colarg, *d_at = d_kind + tcols;
        std::vector<int> arg((size_t)(2 * tcols), 0);
        int *kind = arg.data(), *at = kind + tcols;
        std::vector<double> red;
        int solves = 0, rc;

        // ---- refinement (dgerfs's loop, every column by its own berr; `count` is the same for all columns still refining) ----
        std::vector<double> lstres((size_t)ncols, 3.0);
        LockStep ls(c, ncols, tcols);
        for (int count = 1;; ++count) {
            rc = launch_blk_residual_bound(c, s.A, s.lda, N, s.tr, Xt, Bt, R, Wt, S1, g.ldt, g.ntiles, safe1, safe2);
            if (!rc) rc = col_reduce(c, 0, S1, g, N, ncols, nullptr, nullptr, 1, red);
            if (rc) return rc;
            const bool any = ls.step([&](int64_t j) {
                const double be = red[(size_t)j];
                berr[j0 + j] = be;
                if (!(be > eps && 2.0 * be <= lstres[(size_t)j] && count <= itmax)) return false;   // (also for a NaN)
                lstres[(size_t)j] = be;
                st[(size_t)(j0 + j)].iterations = count;
                return true;
            });
            if (!any) break;
            rc = ls.upload();
            if (!rc) rc = tile_getrs(s, R, R, S1, S2, g);   // d = op(A)^-1 r (into R: the next pass rebuilds r)
            if (!rc) rc = launch_blk_masked_axpy(c, R, c->blk_mask, Xt, g.ldt, g.ntiles);
            if (rc) return rc;
            ++solves;
        }
        // a stopped column's x did not change any more, so the last pass left its last r and w (the same bits as when it stopped)
        rc = store_cols(c, Xt, g, N, j0, ncols, r.X, r.ldx);
        if (!rc) rc = col_reduce(c, 0, Xt, g, N, ncols, nullptr, nullptr, 1, red);
        if (rc) return rc;
        const std::vector<double> xmax(red.begin(), red.begin() + ncols);

        // ---- forward bound: dlacn2 on (op(A)^-1 diag(w))^T, all columns in lock-step ----------------------------------------
        rc = launch_blk_ferr_weight(c, R, Wt, N, ncols, g.ldt, nz * eps, safe1, safe2);
        if (rc) return rc;
        auto kase1 = [&]() {   // v <- w .* (op(A)^-T v)
            ++solves;
            int r2 = tile_getrs(s, V, V, S1, S2, g, true);
            return r2 ? r2 : launch_blk_scale(c, V, Wt, g.ldt, g.ntiles);
        };
        auto kase2 = [&]() {   // v <- op(A)^-1 (w .* v)
            ++solves;
            int r2 = launch_blk_scale(c, V, Wt, g.ldt, g.ntiles);
            return r2 ? r2 : tile_getrs(s, V, V, S1, S2, g);
        };
        std::vector<Lacn2Col> col((size_t)ncols);   // dlacn2's decisions per column (solve_rules.h)
        LockStep live(c, ncols, tcols);             // active = still in dlacn2's loop; what fill and sign send to the kernels
        for (int64_t j = ncols; j < tcols; ++j) kind[j] = -1;
        auto fill = [&](int stage) {   // 0: 1/N; 1: e_j for the live columns, 3 (zero) for the others; 2: the alternating vector
            for (int64_t j = 0; j < ncols; ++j) { kind[j] = stage == 1 && !live.active[(size_t)j] ? 3 : stage; at[j] = (int)col[(size_t)j].j; }
            // (as LockStep::upload: `arg` changes again only after the read-back of the product that follows)
            MPF_HIP_TRY(c, hipMemcpyAsync(d_kind, arg.data(), arg.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
            return launch_blk_lacn2_fill(c, V, N, ncols, g.ldt, d_kind, d_at);
        };
        auto sign = [&]() {   // live columns: v = isgn = sign(v); the others: v = 0
            int r2 = live.upload();
            return r2 ? r2 : launch_blk_lacn2_sign(c, V, Isgn, N, ncols, g.ldt, c->blk_mask);
        };
        rc = fill(0);
        if (!rc) rc = kase1();
        if (!rc) rc = col_reduce(c, 1, V, g, N, ncols, Isgn, nullptr, 2, red);
        if (rc) return rc;
        for (int64_t j = 0; j < ncols; ++j) col[(size_t)j].first_product(red[(size_t)j], N);
        if (N > 1) {
            rc = sign();
            if (!rc) rc = kase2();
            if (!rc) rc = col_reduce(c, 2, V, g, N, ncols, nullptr, d_at, 3, red);
            if (rc) return rc;
            for (int64_t j = 0; j < ncols; ++j) col[(size_t)j].first_transposed((int64_t)red[(size_t)(ncols + j)]);
            for (;;) {
                rc = fill(1);
                if (!rc) rc = kase1();
                if (!rc) rc = col_reduce(c, 1, V, g, N, ncols, Isgn, nullptr, 2, red);
                if (rc) return rc;
                if (!live.step([&](int64_t j) { return col[(size_t)j].product(red[(size_t)j], red[(size_t)(ncols + j)] == 0); })) break;
                rc = sign();
                if (!rc) rc = kase2();
                if (!rc) rc = col_reduce(c, 2, V, g, N, ncols, nullptr, d_at, 3, red);   // (d_at still holds jlast)
                if (rc) return rc;
                if (!live.step([&](int64_t j) {
                        return col[(size_t)j].transposed((int64_t)red[(size_t)(ncols + j)], red[(size_t)j], red[(size_t)(2 * ncols + j)]);
                    })) break;
            }
            rc = fill(2);   // final stage
            if (!rc) rc = kase1();
            if (!rc) rc = col_reduce(c, 1, V, g, N, ncols, Isgn, nullptr, 2, red);
            if (rc) return rc;
            for (int64_t j = 0; j < ncols; ++j) col[(size_t)j].final_stage(red[(size_t)j], N);
        }
        for (int64_t j = 0; j < ncols; ++j) {
            ferr[j0 + j] = xmax[(size_t)j] != 0 ? col[(size_t)j].est / xmax[(size_t)j] : col[(size_t)j].est;
            st[(size_t)(j0 + j)].lacn2_iterations = col[(size_t)j].iter;
            st[(size_t)(j0 + j)].solves = solves;
        }
        return 0;
    });
}

// The body of mpf_gerfsx (mpf_internal.h): dla_gerfsx_extended's loop on all columns of a group in lock-step.  Per step one residual in
// pairs of doubles (launch_blk_residual_x), one tile_getrs, one launch and one read-back of the three measures, XrCol's decision per
// column (solve_rules.h) and one masked update; a column that has stopped is frozen.  Tile sets: B, X, R (then in place d) and
// tile_getrs's two.  With `berr`, after the loop and for the X that is returned: w = |b| + |op(A)| |x| from mpf_gerfs's ABS pass (its
// plain residual and quotient land in scratch and are dropped), r once more in pairs, dgerfs's quotient and its column maximum.
int blk_xrefine_core(const BlkSys &s, const BlkRhs &r, int32_t ithresh, double *err_norm, double *err_comp, mpf_gerfsx_stats *st,
                     double *berr) {
    mpf_ctx *c = s.c;
    const int64_t N = s.N;
    return for_rhs_groups(s, r, GROUP_TILES, 5, LOAD_B | LOAD_X | STORE_X, [&](const Group &g, int32_t j0, int64_t ncols) {
        double *Bt = g.t(0), *Xt = g.t(1), *R = g.t(2), *W = g.t(3), *Z = g.t(4);
        std::vector<XrCol> col((size_t)ncols);
        std::vector<int> solves((size_t)ncols, 0);
        std::vector<double> red((size_t)(3 * ncols));
        LockStep ls(c, ncols, g.tcols());
        int cnt = 0;
        for (; cnt < ithresh; ++cnt) {
            int rc = launch_blk_residual_x(c, s.A, s.lda, N, s.tr, Xt, Bt, R, g.ldt, g.ntiles);
            if (!rc) rc = tile_getrs(s, R, R, W, Z, g);   // d = op(A)^-1 r (into R: the next step rebuilds r)
            if (!rc) rc = launch_blk_xr_measure(c, Xt, R, g.ldt, N, ncols);
            if (!rc) rc = read_back(c, c->blk_red, red.size(), red.data());
            if (rc) return rc;
            const bool any = ls.step([&](int64_t j) {
                ++solves[(size_t)j];
                return col[(size_t)j].step(red[(size_t)j], red[(size_t)(ncols + j)], red[(size_t)(2 * ncols + j)]);
            });
            if (!any) break;
            rc = ls.upload();
            if (!rc) rc = launch_blk_masked_axpy(c, R, c->blk_mask, Xt, g.ldt, g.ntiles);
            if (rc) return rc;
        }
        // out of steps with columns still going: the one way out of a lock-step loop that has no read-back behind the last upload
        if (cnt == ithresh) MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (berr) {   // (W and Z are free: no solve follows)
            const double safe1 = gerfs_safe1(N), safe2 = gerfs_safe2(N);
            int rc = launch_blk_residual_bound(c, s.A, s.lda, N, s.tr, Xt, Bt, R, W, Z, g.ldt, g.ntiles, safe1, safe2);
            if (!rc) rc = launch_blk_residual_x(c, s.A, s.lda, N, s.tr, Xt, Bt, R, g.ldt, g.ntiles);
            if (!rc) rc = launch_blk_xr_berr(c, R, W, g.ldt, N, ncols, safe1, safe2);
            if (!rc) rc = read_back(c, c->blk_red, (size_t)ncols, berr + j0);
            if (rc) return rc;
        }
        for (int64_t j = 0; j < ncols; ++j) {
            XrCol &cj = col[(size_t)j];
            cj.finish(N, err_norm[j0 + j], err_comp[j0 + j]);
            mpf_gerfsx_stats &q = st[(size_t)(j0 + j)];
            q.iterations = cj.corrections;
            q.x_state = cj.x_state;
            q.z_state = cj.z_state;
            q.solves = solves[(size_t)j];
            q.final_dx_x = cj.final_dx_x;
            q.final_dz_z = cj.final_dz_z;
            q.dxratmax = cj.dxratmax;
            q.dzratmax = cj.dzratmax;
        }
        return 0;
    });
}

// The body of mpf_solve_gmres_ir_block (mpf_internal.h).  Per column the rules are GmresCol's (solve_rules.h); the columns of a group
// take every outer step and every inner step together: one launch_blk_residual and one tile_getrs per product, one orthogonalisation
// (launch_gmres_ortho) and ONE read-back -- h, h', ||w||^2 of every column -- per inner step.  A column whose inner loop has ended
// waits (live = 0: the kernels leave its basis and its w alone) until the group's longest one ends, then every column applies its own
// x += V y.  Tile sets: B, X, R (the residual, then in place M^-1 of it: z and w), two of tile_getrs's scratch, and one that stays
// zero (the "b" of the product -op(A) v_k); the basis is restart + 1 more in c->krylov.
int blk_gmres_core(const BlkSys &s, const BlkRhs &r, int32_t max_outer, int32_t restart, double tol, mpf_gmres_stats *st) {
    mpf_ctx *c = s.c;
    const int64_t N = s.N;
    const int m = restart, WORK = 6;
    const int64_t ldt = (N + 255) / 256 * 256;
    int gt = c->tune.gmres_group_tiles;
    if (gt <= 0) {   // automatic: the widest group whose basis and working sets fit in 2 GiB
        const int64_t per_tile = (int64_t)(m + 1 + WORK) * ldt * BLK_T * (int64_t)sizeof(double);
        gt = (int)std::max<int64_t>(1, std::min<int64_t>(GROUP_TILES, (2ll << 30) / per_tile));
    }
    gt = std::min(gt, GROUP_TILES);
    // option timeline: event pairs around the factor solves (0), the residuals (1) and the orthogonalisation (2) of the inner steps
    const bool tl = c->tune.timeline != 0;
    EvPool pool(c);
    struct Pair { hipEvent_t a, b; int what; };
    std::vector<Pair> pairs;
    auto timed = [&](int what, int r2) {   // closes the pair opened by `open`
        if (tl) { pairs.back().what = what; hipEventRecord(pairs.back().b, c->stream); }
        return r2;
    };
    auto open = [&]() { if (tl) { pairs.push_back({pool.get(), pool.get(), 0}); hipEventRecord(pairs.back().a, c->stream); } };
    double inner_wall_ms = 0;
    long inner_steps = 0;
    // (B is loaded after the basis has been cleared, not by the frame)
    int rc = for_rhs_groups(s, r, gt, WORK, STORE_X, [&](const Group &g, int32_t j0, int64_t ncols) {
        const int64_t tc = g.tcols(), vs = g.ldt * tc;
        double *Bt = g.t(0), *Xt = g.t(1), *R = g.t(2), *S1 = g.t(3), *S2 = g.t(4), *Zero = g.t(5);
        MPF_HIP_TRY(c, c->krylov.grow((int64_t)(m + 1) * vs));
        MPF_HIP_TRY(c, c->blk_part.grow(tc));   // (the column norms' output)
        MPF_HIP_TRY(c, c->gm_part.grow((int64_t)gmres_ortho_chunks(g.ldt) * std::max(m, 4) * tc));
        MPF_HIP_TRY(c, c->gm_out.grow((2 * (int64_t)m + 1) * tc));
        MPF_HIP_TRY(c, c->gm_ctl.grow(((int64_t)m + 2) * tc));
        double *V = c->krylov;
        MPF_HIP_TRY(c, hipMemsetAsync(V, 0, (size_t)((int64_t)(m + 1) * vs) * sizeof(double), c->stream));
        // what the host sends: per step [scale (tc doubles) | live (tc ints)], per outer step [y (m x tc doubles) | counts (tc ints)]
        std::vector<double> ctl((size_t)((m + 1) * tc), 0.0), out((size_t)((2 * m + 1) * tc));
        const double *d_scale = c->gm_ctl, *d_y = c->gm_ctl;
        const int *d_live = (const int *)(c->gm_ctl + tc), *d_cnt = (const int *)(c->gm_ctl + (int64_t)m * tc);
        auto send_step = [&](const std::vector<int> &live) {   // (the next read-back synchronises before `ctl` changes again)
            std::memcpy(ctl.data() + tc, live.data(), (size_t)tc * sizeof(int));
            MPF_HIP_TRY(c, hipMemcpyAsync(c->gm_ctl, ctl.data(), (size_t)(tc + (tc + 1) / 2) * sizeof(double), hipMemcpyHostToDevice, c->stream));
            return 0;
        };
        int rc = load_cols(c, r.B, r.ldb, j0, ncols, N, Bt, g);
        std::vector<double> nb2, nr;
        if (!rc) rc = col_norms(c, Bt, g, N, ncols, nb2);
        if (!rc) rc = tile_getrs(s, Bt, Xt, S1, S2, g);   // x0
        if (rc) return rc;
        for (auto &v : nb2) if (v == 0) v = 1;
        std::vector<GmresCol> col((size_t)ncols, GmresCol(m));
        std::vector<int> cnt((size_t)tc, 0);
        LockStep outer_ls(c, ncols, tc);   // active = the column has not stopped for good
        for (int outer = 0;; ++outer) {
            rc = launch_blk_residual(c, s.A, s.lda, N, s.tr, Xt, Bt, R, g.ldt, g.ntiles);
            if (!rc) rc = col_norms(c, R, g, N, ncols, nr);
            if (rc) return rc;
            if (!outer_ls.step([&](int64_t j) {
                    return col[(size_t)j].outer_check(st[(size_t)(j0 + j)], outer, nr[(size_t)j] / nb2[(size_t)j], max_outer, tol);
                })) break;
            rc = tile_getrs(s, R, R, S1, S2, g);              // z = M^-1 r
            if (!rc) rc = col_norms(c, R, g, N, ncols, nr);   // beta
            if (rc) return rc;
            bool any = outer_ls.step([&](int64_t j) { return col[(size_t)j].begin_inner(nr[(size_t)j], st[(size_t)(j0 + j)].rel_residual, tol); });
            for (int64_t j = 0; j < ncols; ++j) {
                cnt[(size_t)j] = 0;
                ctl[(size_t)j] = outer_ls.active[(size_t)j] ? 1.0 / nr[(size_t)j] : 0.0;
            }
            if (!any) break;
            LockStep inner = outer_ls;   // active = live: the column's inner loop of this outer step has not ended
            rc = send_step(inner.mask);
            if (!rc) rc = launch_gmres_append(c, R, d_scale, V, g.ldt, N, g.ntiles);   // v_0 = z / beta
            if (rc) return rc;
            const auto t_inner = std::chrono::steady_clock::now();
            for (int k = 0; any; ++k) {
                const int64_t len = (int64_t)(k + 1) * tc;
                open();
                rc = timed(1, launch_blk_residual(c, s.A, s.lda, N, s.tr, V + (int64_t)k * vs, Zero, R, g.ldt, g.ntiles));   // -op(A) v_k
                open();
                if (!rc) rc = timed(0, tile_getrs(s, R, R, S1, S2, g));                                                      // -M^-1 op(A) v_k
                open();
                if (!rc) rc = timed(2, launch_gmres_ortho(c, V, vs, k + 1, R, g.ldt, N, g.ntiles, d_live, c->gm_part, c->gm_out));
                if (!rc) rc = read_back(c, c->gm_out, (size_t)(2 * len + tc), out.data());
                if (rc) return rc;
                ++inner_steps;
                std::fill(ctl.begin(), ctl.begin() + ncols, 0.0);
                any = inner.step([&](int64_t j) {
                    double *h = out.data() + j;
                    for (int i = 0; i <= k; ++i) h[(size_t)i * tc] += h[(size_t)(len + i * tc)];   // H[0 .. k, k] = h + h'
                    const double hn = std::sqrt(out[(size_t)(2 * len + j)]);
                    const bool live = col[(size_t)j].inner_step(st[(size_t)(j0 + j)], h, (size_t)tc, hn);
                    if (live && hn > 0) ctl[(size_t)j] = 1.0 / hn;
                    return live;
                });
                if (!any) break;
                rc = send_step(inner.mask);
                if (!rc) rc = launch_gmres_append(c, R, d_scale, V + (int64_t)(k + 1) * vs, g.ldt, N, g.ntiles);   // v_{k+1} = w / hn
                if (rc) return rc;
            }
            inner_wall_ms += ms_since(t_inner);
            std::fill(ctl.begin(), ctl.end(), 0.0);
            for (int64_t j = 0; j < ncols; ++j) {   // every column that ran this outer step: its own y, its own count
                if (!outer_ls.active[(size_t)j]) continue;
                GmresCol &cj = col[(size_t)j];
                cj.solve_y();
                cnt[(size_t)j] = cj.k;
                for (int i = 0; i < cj.k; ++i) ctl[(size_t)(i * tc + j)] = cj.y[(size_t)i];
            }
            std::memcpy(ctl.data() + (int64_t)m * tc, cnt.data(), (size_t)tc * sizeof(int));
            MPF_HIP_TRY(c, hipMemcpyAsync(c->gm_ctl, ctl.data(), (size_t)(m * tc + (tc + 1) / 2) * sizeof(double), hipMemcpyHostToDevice, c->stream));
            rc = launch_gmres_xupdate(c, V, vs, d_y, d_cnt, Xt, g.ldt, N, g.ntiles);
            if (rc) return rc;
            MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));   // `ctl` is refilled right here, before any read-back
            std::fill(ctl.begin(), ctl.end(), 0.0);
        }
        return 0;
    });
    if (rc) return rc;
    if (tl) {   // factor solves, residuals, orthogonalisation (device time between the events), the inner loops' wall time, their steps
        MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));
        double acc[3] = {0, 0, 0};
        for (auto &p : pairs) { float ms = 0; if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) acc[p.what] += ms; }
        fprintf(stderr, "GMRES_TL %.4f %.4f %.4f %.4f %ld\n", acc[0], acc[1], acc[2], inner_wall_ms, inner_steps);
    }
    return 0;
}

extern "C" {

int mpf_getrs(mpf_ctx *c, int32_t trans, const double *d_LU, int64_t ldlu, const int32_t *d_ipiv, int64_t N, int32_t nrhs, double *d_B,
              int64_t ldb) {
    if (!c) return -1;
    int rc;
    if (!blk_args(c, "getrs", trans, N, nrhs, {ldlu, ldb}, {d_LU, d_ipiv, d_B}, {}, rc)) return rc;
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    rc = solve_setup(c, d_LU, ldlu, d_ipiv, N);
    if (rc) return rc;
    const bool tr = trans == 1;
    // in place on B, the permutation in the load or in the store
    rc = for_groups(c, N, nrhs, GROUP_TILES, 2, [&](const Group &g, int32_t j0, int64_t ncols) {
        double *W = g.t(0), *Z = g.t(1), *B = d_B + (int64_t)j0 * ldb;
        int r2 = launch_blk_load(c, B, ldb, tr ? nullptr : c->perm_buf, N, ncols, W, g.ldt, g.ntiles);
        if (!r2) r2 = tile_solve(c, d_LU, ldlu, N, tr, W, Z, g);
        return r2 ? r2 : launch_blk_store(c, W, g.ldt, tr ? c->perm_buf : nullptr, N, ncols, B, ldb);
    });
    if (rc) return rc;
    MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return solve_check_waits(c);
}

int mpf_solve_ir_block(mpf_ctx *c, int32_t trans, const double *d_A, int64_t lda, const double *d_LU, int64_t ldlu, const int32_t *d_ipiv,
                       int64_t N, int32_t nrhs, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t max_iter, double tol,
                       mpf_ir_stats *stats) {
    const BlkSys s{c, trans == 1, d_A, lda, d_LU, ldlu, N};
    const BlkRhs r{nrhs, d_B, ldb, d_X, ldx};
    return solve_entry("solve_ir_block", trans, s, r, d_ipiv, {}, stats,
                       [&](mpf_ir_stats *st) { return blk_refine_core(s, r, max_iter, tol, st); },
                       [](const mpf_ir_stats &) { return true; });
}

int mpf_gerfs(mpf_ctx *c, int32_t trans, const double *d_A, int64_t lda, const double *d_LU, int64_t ldlu, const int32_t *d_ipiv,
              int64_t N, int32_t nrhs, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t itmax, double *ferr,
              double *berr, mpf_gerfs_stats *stats) {
    const BlkSys s{c, trans == 1, d_A, lda, d_LU, ldlu, N};
    const BlkRhs r{nrhs, d_B, ldb, d_X, ldx};
    return solve_entry("gerfs", trans, s, r, d_ipiv, {ferr, berr}, stats,
                       [&](mpf_gerfs_stats *st) { return blk_bounds_core(s, r, itmax, ferr, berr, st); },
                       [](const mpf_gerfs_stats &) { return true; });
}

int mpf_residual_x(mpf_ctx *c, int32_t trans, const double *d_A, int64_t lda, int64_t N, int32_t nrhs, const double *d_X, int64_t ldx,
                   const double *d_B, int64_t ldb, double *d_R, int64_t ldr) {
    if (!c) return -1;
    int rc;
    if (!blk_args(c, "residual_x", trans, N, nrhs, {lda, ldb, ldx, ldr}, {d_A, d_X, d_B, d_R}, {}, rc)) return rc;
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    rc = for_groups(c, N, nrhs, GROUP_TILES, 3, [&](const Group &g, int32_t j0, int64_t ncols) {
        double *Bt = g.t(0), *Xt = g.t(1), *R = g.t(2);
        int r2 = load_cols(c, d_B, ldb, j0, ncols, N, Bt, g);
        if (!r2) r2 = load_cols(c, d_X, ldx, j0, ncols, N, Xt, g);
        if (!r2) r2 = launch_blk_residual_x(c, d_A, lda, N, trans == 1, Xt, Bt, R, g.ldt, g.ntiles);
        return r2 ? r2 : store_cols(c, R, g, N, j0, ncols, d_R, ldr);
    });
    if (rc) return rc;
    MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return 0;
}

// mpf_gerfsx and mpf_gerfsx_scaled: d_r / d_c (the scales of the factored matrix Dr A Dc, or null) become tile_getrs's pre / post as
// gesvx_steps maps them (mpf_expert.cpp)
static int gerfsx_entry(const char *who, mpf_ctx *c, int32_t trans, const double *d_A, int64_t lda, const double *d_LU, int64_t ldlu,
                        const int32_t *d_ipiv, int64_t N, int32_t nrhs, const double *d_B, int64_t ldb, double *d_X, int64_t ldx,
                        int32_t ithresh, const double *d_r, const double *d_c, double *err_norm, double *err_comp, double *berr,
                        mpf_gerfsx_stats *stats) {
    if (ithresh <= 0) ithresh = 10;
    if (ithresh > 31) ithresh = 31;
    const bool tr = trans == 1;
    const BlkSys s{c, tr, d_A, lda, d_LU, ldlu, N, tr ? d_c : d_r, tr ? d_r : d_c};
    const BlkRhs r{nrhs, d_B, ldb, d_X, ldx};
    return solve_entry(who, trans, s, r, d_ipiv, {err_norm, err_comp}, stats,
                       [&](mpf_gerfsx_stats *st) { return blk_xrefine_core(s, r, ithresh, err_norm, err_comp, st, berr); },
                       [](const mpf_gerfsx_stats &q) { return q.x_state == XrCol::X_CONV; });
}

int mpf_gerfsx(mpf_ctx *c, int32_t trans, const double *d_A, int64_t lda, const double *d_LU, int64_t ldlu, const int32_t *d_ipiv,
               int64_t N, int32_t nrhs, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t ithresh, double *err_norm,
               double *err_comp, mpf_gerfsx_stats *stats) {
    return gerfsx_entry("gerfsx", c, trans, d_A, lda, d_LU, ldlu, d_ipiv, N, nrhs, d_B, ldb, d_X, ldx, ithresh, nullptr, nullptr, err_norm,
                        err_comp, nullptr, stats);
}

int mpf_gerfsx_scaled(mpf_ctx *c, int32_t trans, const double *d_A, int64_t lda, const double *d_LU, int64_t ldlu, const int32_t *d_ipiv,
                      int64_t N, int32_t nrhs, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t ithresh, const double *d_r,
                      const double *d_c, double *err_norm, double *err_comp, double *berr, mpf_gerfsx_stats *stats) {
    return gerfsx_entry("gerfsx_scaled", c, trans, d_A, lda, d_LU, ldlu, d_ipiv, N, nrhs, d_B, ldb, d_X, ldx, ithresh, d_r, d_c, err_norm,
                        err_comp, berr, stats);
}

int mpf_solve_gmres_ir_block(mpf_ctx *c, int32_t trans, const double *d_A, int64_t lda, const double *d_LU, int64_t ldlu,
                             const int32_t *d_ipiv, int64_t N, int32_t nrhs, const double *d_B, int64_t ldb, double *d_X, int64_t ldx,
                             int32_t max_outer, int32_t restart, double tol, mpf_gmres_stats *stats) {
    gmres_clamp(max_outer, restart);
    const BlkSys s{c, trans == 1, d_A, lda, d_LU, ldlu, N};
    const BlkRhs r{nrhs, d_B, ldb, d_X, ldx};
    return solve_entry("solve_gmres_ir_block", trans, s, r, d_ipiv, {}, stats,
                       [&](mpf_gmres_stats *st) { return blk_gmres_core(s, r, max_outer, restart, tol, st); },
                       [](const mpf_gmres_stats &q) { return q.converged != 0; });
}

} // extern "C"
