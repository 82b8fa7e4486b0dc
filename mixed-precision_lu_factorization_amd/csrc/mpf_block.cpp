// Blocked multi-right-hand-side solve (no reference counterpart; LAPACK dgetrs and block refinement):
//   mpf_getrs            B := A^-1 B or A^-T B with the factors of mpf_factor_dev
//   mpf_solve_ir_block   fp64 refinement of all columns together, per-column rules and stats of mpf_solve_ir_nrhs / _trans
//   mpf_gerfs            LAPACK dgerfs: refinement by the componentwise backward error, berr and the forward bound ferr per column
//   mpf_solve_gmres_ir_block   GMRES-IR (mpf_solve_gmres_ir's method) on all columns of a group in lock-step, op(A) = A or A^T
//   mpf_residual_x, mpf_gerfsx   LAPACK dgerfsx: the residual in pairs of doubles, refinement steered by the corrections' size (blk_xrefine_core)
// The bodies of the second and third are cores (blk_refine_core, blk_bounds_core) that take optional scale vectors for the factors of an
// equilibrated copy Dr A Dc: mpf_gesvx_block (mpf_expert.cpp) calls them with its scales, the public functions with none.
// The right-hand sides go through the device in groups of at most GROUP_TILES tiles of BLK_T columns (solve_block.hip); every
// triangular step and every residual is one pass over the factor block / over A for the whole group.
#include "solve_common.h"
#include <algorithm>
#include <cstring>

namespace {
constexpr int GROUP_TILES = 16;   // 512 columns per group: six N x 512 tile sets of scratch at most (mpf_gerfs; 805 MB at N = 32768)

struct Group {
    int64_t ldt = 0;   // rows of a tile (N rounded up to 256)
    int ntiles = 0;
    double *base = nullptr;
    double *t(int i) const { return base + (int64_t)i * ldt * BLK_T * ntiles; }
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
// W <- op^-1 W on prepared factors: P^T-free forms, the permutation is applied by the loads and stores around it; Z scratch
int tile_solve(mpf_ctx *c, const double *LU, int64_t ldlu, int64_t N, bool trans, double *W, double *Z, const Group &g) {
    int rc = launch_blk_tri(c, LU, ldlu, N, trans ? 2 : 0, W, Z, g.ldt, g.ntiles);
    return rc ? rc : launch_blk_tri(c, LU, ldlu, N, trans ? 3 : 1, Z, W, g.ldt, g.ntiles);
}
// out (tiles) <- post .* op(L U, P)^-1 (pre .* src) (tiles), through W / Z: op(A)^-1 src for the factors of A itself (pre = post = null)
// and for those of Dr A Dc (trans = 0: Dc (L U)^-1 P Dr, pre = Dr, post = Dc; trans = 1: Dr P^T (L U)^-T Dc, pre = Dc, post = Dr).
// The scales ride on the load and the store, indexed by the matrix row as the permutation is.
int tile_getrs(mpf_ctx *c, const double *LU, int64_t ldlu, int64_t N, bool trans, const double *src, double *out, double *W, double *Z,
               const Group &g, const double *pre = nullptr, const double *post = nullptr) {
    const int64_t cols = (int64_t)BLK_T * g.ntiles;
    int rc = launch_blk_load(c, src, g.ldt, trans ? nullptr : c->perm_buf, N, cols, W, g.ldt, g.ntiles, pre);
    if (!rc) rc = tile_solve(c, LU, ldlu, N, trans, W, Z, g);
    if (!rc) rc = launch_blk_store(c, W, g.ldt, trans ? c->perm_buf : nullptr, N, cols, out, g.ldt, post);
    return rc;
}
int col_norms(mpf_ctx *c, const double *T, const Group &g, int64_t N, int64_t ncols, std::vector<double> &out) {
    int rc = launch_col_sumsq(c, T, g.ldt, N, ncols, c->blk_part);
    if (rc) return rc;
    out.resize((size_t)ncols);
    MPF_HIP_TRY(c, hipMemcpyAsync(out.data(), c->blk_part, (size_t)ncols * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (auto &v : out) v = std::sqrt(v);
    return 0;
}
// one per-column reduction of a step (launch_blk_col_reduce) back on the host: `nvals` values per column, out[v * ncols + j]
int col_reduce(mpf_ctx *c, int what, const double *T, const Group &g, int64_t N, int64_t ncols, const double *sg, const int *at, int nvals,
               std::vector<double> &out) {
    int rc = launch_blk_col_reduce(c, what, T, g.ldt, N, ncols, sg, at);
    if (rc) return rc;
    out.resize((size_t)(nvals * ncols));
    MPF_HIP_TRY(c, hipMemcpyAsync(out.data(), c->blk_red, out.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return 0;
}
int check_args(mpf_ctx *c, const char *who, int32_t trans, int64_t N, int32_t nrhs, int64_t ldlu, int64_t ldb) {
    if (trans != 0 && trans != 1) c->err = std::string(who) + ": trans must be 0 or 1";
    else if (N <= 0 || nrhs < 0) c->err = std::string(who) + ": N must be positive, nrhs >= 0";
    else if (ldlu < N || ldb < N) c->err = std::string(who) + ": leading dimension < N";
    else return 0;
    return -1;
}
} // namespace

// The body of mpf_solve_ir_block (mpf_internal.h): x0 and every correction go through the scaled tile_getrs, the residual is taken
// against the original A; rules, stats and masking per column as documented for mpf_solve_ir_block.
int blk_refine_core(mpf_ctx *c, bool tr, const double *d_A, int64_t lda, const double *d_LU, int64_t ldlu, int64_t N, int32_t nrhs,
                    const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t max_iter, double tol, const double *pre,
                    const double *post, mpf_ir_stats *st) {
    if (max_iter > 31) max_iter = 31;
    int rc;
    for (int32_t j0 = 0; j0 < nrhs; j0 += GROUP_TILES * BLK_T) {
        const int64_t ncols = std::min<int64_t>(nrhs - j0, GROUP_TILES * BLK_T);
        Group g;
        rc = group_tiles(c, N, (int)((ncols + BLK_T - 1) / BLK_T), 5, g);
        if (rc) return rc;
        const int64_t tcols = (int64_t)BLK_T * g.ntiles;
        double *Bt = g.t(0), *Xt = g.t(1), *R = g.t(2), *W = g.t(3), *Z = g.t(4);
        MPF_HIP_TRY(c, c->blk_mask.grow(tcols));
        MPF_HIP_TRY(c, c->blk_part.grow(tcols));   // (also the column norms' output)
        rc = launch_blk_load(c, d_B + (int64_t)j0 * ldb, ldb, nullptr, N, ncols, Bt, g.ldt, g.ntiles);
        std::vector<double> nb2, nr;
        if (!rc) rc = col_norms(c, Bt, g, N, ncols, nb2);
        if (!rc) rc = tile_getrs(c, d_LU, ldlu, N, tr, Bt, Xt, W, Z, g, pre, post);   // x0
        if (rc) return rc;
        for (auto &v : nb2) if (v == 0) v = 1;
        std::vector<int> active((size_t)ncols, 1), mask((size_t)tcols, 0);
        for (int it = 0;; ++it) {
            rc = launch_blk_residual(c, d_A, lda, N, tr, Xt, Bt, R, g.ldt, g.ntiles);
            if (!rc) rc = col_norms(c, R, g, N, ncols, nr);
            if (rc) return rc;
            bool any = false;
            for (int64_t j = 0; j < ncols; ++j) {   // ir_step's rules, column by column; a stopped column is frozen
                if (active[(size_t)j]) active[(size_t)j] = ir_step(st[(size_t)(j0 + j)], it, nr[(size_t)j] / nb2[(size_t)j], max_iter, tol);
                mask[(size_t)j] = active[(size_t)j];
                any = any || active[(size_t)j];
            }
            if (!any) break;
            MPF_HIP_TRY(c, hipMemcpyAsync(c->blk_mask, mask.data(), (size_t)tcols * sizeof(int), hipMemcpyHostToDevice, c->stream));
            rc = tile_getrs(c, d_LU, ldlu, N, tr, R, R, W, Z, g, pre, post);   // correction d = op^-1 r (into R: r is consumed)
            if (!rc) rc = launch_blk_masked_axpy(c, R, c->blk_mask, Xt, g.ldt, g.ntiles);
            if (rc) return rc;
            MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));   // `mask` is a host vector reused by the next step
        }
        rc = launch_blk_store(c, Xt, g.ldt, nullptr, N, ncols, d_X + (int64_t)j0 * ldx, ldx);
        if (rc) return rc;
    }
    return 0;
}

// The body of mpf_gerfs (mpf_internal.h): residual, weights and berr of the ORIGINAL system; corrections and dlacn2's KASE 2 product
// through the scaled tile_getrs, KASE 1 through the transposed one with pre and post swapped.
int blk_bounds_core(mpf_ctx *c, bool tr, const double *d_A, int64_t lda, const double *d_LU, int64_t ldlu, int64_t N, int32_t nrhs,
                    const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t itmax, double *ferr, double *berr, const double *pre,
                    const double *post, mpf_gerfs_stats *st) {
    if (itmax <= 0) itmax = 5;
    if (itmax > 31) itmax = 31;
    int rc;
    const double eps = LAPACK_EPS, nz = (double)(N + 1), safe1 = gerfs_safe1(N), safe2 = gerfs_safe2(N);
    for (int32_t j0 = 0; j0 < nrhs; j0 += GROUP_TILES * BLK_T) {
        const int64_t ncols = std::min<int64_t>(nrhs - j0, GROUP_TILES * BLK_T);
        Group g;
        rc = group_tiles(c, N, (int)((ncols + BLK_T - 1) / BLK_T), 6, g);
        if (rc) return rc;
        const int64_t tcols = (int64_t)BLK_T * g.ntiles;
        // Bt and R are free once the weights of the forward bound stand in Wt: dlacn2's vector and its stored signs take their place
        double *Bt = g.t(0), *Xt = g.t(1), *R = g.t(2), *Wt = g.t(3), *S1 = g.t(4), *S2 = g.t(5), *V = Bt, *Isgn = R;
        MPF_HIP_TRY(c, c->blk_mask.grow(tcols));
        MPF_HIP_TRY(c, c->blk_colarg.grow(2 * tcols));
        int *d_kind = c->blk_colarg, *d_at = d_kind + tcols;
        std::vector<int> mask((size_t)tcols, 0), arg((size_t)(2 * tcols), 0);
        int *kind = arg.data(), *at = kind + tcols;
        std::vector<double> red;
        int solves = 0;
        auto upload = [&](int *dst, const std::vector<int> &src) {   // (the step's read-back synchronises before `src` changes again)
            MPF_HIP_TRY(c, hipMemcpyAsync(dst, src.data(), src.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
            return 0;
        };
        rc = launch_blk_load(c, d_B + (int64_t)j0 * ldb, ldb, nullptr, N, ncols, Bt, g.ldt, g.ntiles);
        if (!rc) rc = launch_blk_load(c, d_X + (int64_t)j0 * ldx, ldx, nullptr, N, ncols, Xt, g.ldt, g.ntiles);
        if (rc) return rc;

        // ---- refinement (dgerfs's loop, every column by its own berr; `count` is the same for all columns still refining) ----
        std::vector<double> lstres((size_t)ncols, 3.0);
        std::vector<int> active((size_t)ncols, 1);
        for (int count = 1;; ++count) {
            rc = launch_blk_residual_bound(c, d_A, lda, N, tr, Xt, Bt, R, Wt, S1, g.ldt, g.ntiles, safe1, safe2);
            if (!rc) rc = col_reduce(c, 0, S1, g, N, ncols, nullptr, nullptr, 1, red);
            if (rc) return rc;
            bool any = false;
            for (int64_t j = 0; j < ncols; ++j) {
                mask[(size_t)j] = 0;
                if (!active[(size_t)j]) continue;
                const double be = red[(size_t)j];
                berr[j0 + j] = be;
                if (be > eps && 2.0 * be <= lstres[(size_t)j] && count <= itmax) {   // (false for a NaN)
                    lstres[(size_t)j] = be;
                    st[(size_t)(j0 + j)].iterations = count;
                    mask[(size_t)j] = 1;
                    any = true;
                } else active[(size_t)j] = 0;
            }
            if (!any) break;
            rc = upload(c->blk_mask, mask);
            if (!rc) rc = tile_getrs(c, d_LU, ldlu, N, tr, R, R, S1, S2, g, pre, post);   // d = op(A)^-1 r (into R: the next pass rebuilds r)
            if (!rc) rc = launch_blk_masked_axpy(c, R, c->blk_mask, Xt, g.ldt, g.ntiles);
            if (rc) return rc;
            ++solves;
        }
        // a stopped column's x did not change any more, so the last pass left its last r and w (the same bits as when it stopped)
        rc = launch_blk_store(c, Xt, g.ldt, nullptr, N, ncols, d_X + (int64_t)j0 * ldx, ldx);
        if (!rc) rc = col_reduce(c, 0, Xt, g, N, ncols, nullptr, nullptr, 1, red);
        if (rc) return rc;
        const std::vector<double> xmax(red.begin(), red.begin() + ncols);

        // ---- forward bound: dlacn2 on (op(A)^-1 diag(w))^T, all columns in lock-step ----------------------------------------
        rc = launch_blk_ferr_weight(c, R, Wt, N, ncols, g.ldt, nz * eps, safe1, safe2);
        if (rc) return rc;
        auto kase1 = [&]() {   // v <- w .* (op(A)^-T v): the transposed solve, its scales swapped
            ++solves;
            int r2 = tile_getrs(c, d_LU, ldlu, N, !tr, V, V, S1, S2, g, post, pre);
            return r2 ? r2 : launch_blk_scale(c, V, Wt, g.ldt, g.ntiles);
        };
        auto kase2 = [&]() {   // v <- op(A)^-1 (w .* v)
            ++solves;
            int r2 = launch_blk_scale(c, V, Wt, g.ldt, g.ntiles);
            return r2 ? r2 : tile_getrs(c, d_LU, ldlu, N, tr, V, V, S1, S2, g, pre, post);
        };
        std::vector<Lacn2Col> col((size_t)ncols);   // dlacn2's decisions per column (solve_rules.h); live = still in its loop
        for (int64_t j = ncols; j < tcols; ++j) kind[j] = -1;
        auto fill = [&](int stage) {   // 0: 1/N; 1: e_j for the live columns, 3 (zero) for the others; 2: the alternating vector
            for (int64_t j = 0; j < ncols; ++j) { kind[j] = stage == 1 && !col[(size_t)j].live ? 3 : stage; at[j] = (int)col[(size_t)j].j; }
            int r2 = upload(d_kind, arg);
            return r2 ? r2 : launch_blk_lacn2_fill(c, V, N, ncols, g.ldt, d_kind, d_at);
        };
        auto sign = [&]() {   // live columns: v = isgn = sign(v); the others: v = 0
            for (int64_t j = 0; j < ncols; ++j) mask[(size_t)j] = col[(size_t)j].live;
            int r2 = upload(c->blk_mask, mask);
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
                bool any = false;
                for (int64_t j = 0; j < ncols; ++j) any = col[(size_t)j].product(red[(size_t)j], red[(size_t)(ncols + j)] == 0) || any;
                if (!any) break;
                rc = sign();
                if (!rc) rc = kase2();
                if (!rc) rc = col_reduce(c, 2, V, g, N, ncols, nullptr, d_at, 3, red);   // (d_at still holds jlast)
                if (rc) return rc;
                any = false;
                for (int64_t j = 0; j < ncols; ++j)
                    any = col[(size_t)j].transposed((int64_t)red[(size_t)(ncols + j)], red[(size_t)j], red[(size_t)(2 * ncols + j)]) || any;
                if (!any) break;
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
    }
    return 0;
}

// The body of mpf_gerfsx (mpf_internal.h): dla_gerfsx_extended's loop on all columns of a group in lock-step.  Per step one residual in
// pairs of doubles (launch_blk_residual_x), one tile_getrs, one launch and one read-back of the three measures, XrCol's decision per
// column (solve_rules.h) and one masked update; a column that has stopped is frozen.  Tile sets: B, X, R (then in place d) and
// tile_getrs's two.
int blk_xrefine_core(mpf_ctx *c, bool tr, const double *d_A, int64_t lda, const double *d_LU, int64_t ldlu, int64_t N, int32_t nrhs,
                     const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t ithresh, double *err_norm, double *err_comp,
                     mpf_gerfsx_stats *st) {
    int rc;
    for (int32_t j0 = 0; j0 < nrhs; j0 += GROUP_TILES * BLK_T) {
        const int64_t ncols = std::min<int64_t>(nrhs - j0, GROUP_TILES * BLK_T);
        Group g;
        rc = group_tiles(c, N, (int)((ncols + BLK_T - 1) / BLK_T), 5, g);
        if (rc) return rc;
        const int64_t tcols = (int64_t)BLK_T * g.ntiles;
        double *Bt = g.t(0), *Xt = g.t(1), *R = g.t(2), *W = g.t(3), *Z = g.t(4);
        MPF_HIP_TRY(c, c->blk_mask.grow(tcols));
        rc = launch_blk_load(c, d_B + (int64_t)j0 * ldb, ldb, nullptr, N, ncols, Bt, g.ldt, g.ntiles);
        if (!rc) rc = launch_blk_load(c, d_X + (int64_t)j0 * ldx, ldx, nullptr, N, ncols, Xt, g.ldt, g.ntiles);
        if (rc) return rc;
        std::vector<XrCol> col((size_t)ncols);
        std::vector<int> active((size_t)ncols, 1), mask((size_t)tcols, 0), solves((size_t)ncols, 0);
        std::vector<double> red((size_t)(3 * ncols));
        for (int cnt = 0; cnt < ithresh; ++cnt) {
            rc = launch_blk_residual_x(c, d_A, lda, N, tr, Xt, Bt, R, g.ldt, g.ntiles);
            if (!rc) rc = tile_getrs(c, d_LU, ldlu, N, tr, R, R, W, Z, g);   // d = op(A)^-1 r (into R: the next step rebuilds r)
            if (!rc) rc = launch_blk_xr_measure(c, Xt, R, g.ldt, N, ncols);
            if (rc) return rc;
            MPF_HIP_TRY(c, hipMemcpyAsync(red.data(), c->blk_red, red.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));
            bool any = false;
            for (int64_t j = 0; j < ncols; ++j) {
                if (active[(size_t)j]) {
                    ++solves[(size_t)j];
                    active[(size_t)j] = col[(size_t)j].step(red[(size_t)j], red[(size_t)(ncols + j)], red[(size_t)(2 * ncols + j)]);
                }
                mask[(size_t)j] = active[(size_t)j];
                any = any || active[(size_t)j];
            }
            if (!any) break;
            MPF_HIP_TRY(c, hipMemcpyAsync(c->blk_mask, mask.data(), (size_t)tcols * sizeof(int), hipMemcpyHostToDevice, c->stream));
            rc = launch_blk_masked_axpy(c, R, c->blk_mask, Xt, g.ldt, g.ntiles);
            if (rc) return rc;
            MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));   // `mask` is a host vector reused by the next step
        }
        rc = launch_blk_store(c, Xt, g.ldt, nullptr, N, ncols, d_X + (int64_t)j0 * ldx, ldx);
        if (rc) return rc;
        for (int64_t j = 0; j < ncols; ++j) {
            XrCol &cj = col[(size_t)j];
            cj.finish(N, err_norm[j0 + j], err_comp[j0 + j]);
            mpf_gerfsx_stats &s = st[(size_t)(j0 + j)];
            s.iterations = cj.corrections;
            s.x_state = cj.x_state;
            s.z_state = cj.z_state;
            s.solves = solves[(size_t)j];
            s.final_dx_x = cj.final_dx_x;
            s.final_dz_z = cj.final_dz_z;
            s.dxratmax = cj.dxratmax;
            s.dzratmax = cj.dzratmax;
        }
    }
    return 0;
}

// The body of mpf_solve_gmres_ir_block (mpf_internal.h).  Per column the rules are GmresCol's (solve_rules.h); the columns of a group
// take every outer step and every inner step together: one launch_blk_residual and one tile_getrs per product, one orthogonalisation
// (launch_gmres_ortho) and ONE read-back -- h, h', ||w||^2 of every column -- per inner step.  A column whose inner loop has ended
// waits (live = 0: the kernels leave its basis and its w alone) until the group's longest one ends, then every column applies its own
// x += V y.  Tile sets: B, X, R (the residual, then in place M^-1 of it: z and w), two of tile_getrs's scratch, and one that stays
// zero (the "b" of the product -op(A) v_k); the basis is restart + 1 more in c->krylov.
int blk_gmres_core(mpf_ctx *c, bool tr, const double *d_A, int64_t lda, const double *d_LU, int64_t ldlu, int64_t N, int32_t nrhs,
                   const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t max_outer, int32_t restart, double tol,
                   mpf_gmres_stats *st) {
    const int m = restart, WORK = 6;
    const int64_t ldt = (N + 255) / 256 * 256;
    int gt = c->tune.gmres_group_tiles;
    if (gt <= 0) {   // automatic: the widest group whose basis and working sets fit in 2 GiB
        const int64_t per_tile = (int64_t)(m + 1 + WORK) * ldt * BLK_T * (int64_t)sizeof(double);
        gt = (int)std::max<int64_t>(1, std::min<int64_t>(GROUP_TILES, (2ll << 30) / per_tile));
    }
    gt = std::min(gt, GROUP_TILES);
    int rc;
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
    for (int32_t j0 = 0; j0 < nrhs; j0 += gt * BLK_T) {
        const int64_t ncols = std::min<int64_t>(nrhs - j0, (int64_t)gt * BLK_T);
        Group g;
        rc = group_tiles(c, N, (int)((ncols + BLK_T - 1) / BLK_T), WORK, g);
        if (rc) return rc;
        const int64_t tc = (int64_t)BLK_T * g.ntiles, vs = g.ldt * tc;
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
        rc = launch_blk_load(c, d_B + (int64_t)j0 * ldb, ldb, nullptr, N, ncols, Bt, g.ldt, g.ntiles);
        std::vector<double> nb2, nr;
        if (!rc) rc = col_norms(c, Bt, g, N, ncols, nb2);
        if (!rc) rc = tile_getrs(c, d_LU, ldlu, N, tr, Bt, Xt, S1, S2, g);   // x0
        if (rc) return rc;
        for (auto &v : nb2) if (v == 0) v = 1;
        std::vector<GmresCol> col((size_t)ncols, GmresCol(m));
        std::vector<int> active((size_t)ncols, 1), live((size_t)tc, 0), cnt((size_t)tc, 0);
        for (int outer = 0;; ++outer) {
            rc = launch_blk_residual(c, d_A, lda, N, tr, Xt, Bt, R, g.ldt, g.ntiles);
            if (!rc) rc = col_norms(c, R, g, N, ncols, nr);
            if (rc) return rc;
            bool any = false;
            for (int64_t j = 0; j < ncols; ++j) {
                if (active[(size_t)j]) active[(size_t)j] = col[(size_t)j].outer_check(st[(size_t)(j0 + j)], outer, nr[(size_t)j] / nb2[(size_t)j], max_outer, tol);
                any = any || active[(size_t)j];
            }
            if (!any) break;
            rc = tile_getrs(c, d_LU, ldlu, N, tr, R, R, S1, S2, g);   // z = M^-1 r
            if (!rc) rc = col_norms(c, R, g, N, ncols, nr);           // beta
            if (rc) return rc;
            any = false;
            for (int64_t j = 0; j < ncols; ++j) {
                if (active[(size_t)j]) active[(size_t)j] = col[(size_t)j].begin_inner(nr[(size_t)j], st[(size_t)(j0 + j)].rel_residual, tol);
                live[(size_t)j] = active[(size_t)j];
                cnt[(size_t)j] = 0;
                ctl[(size_t)j] = active[(size_t)j] ? 1.0 / nr[(size_t)j] : 0.0;
                any = any || active[(size_t)j];
            }
            if (!any) break;
            rc = send_step(live);
            if (!rc) rc = launch_gmres_append(c, R, d_scale, V, g.ldt, N, g.ntiles);   // v_0 = z / beta
            if (rc) return rc;
            const auto t_inner = std::chrono::steady_clock::now();
            for (int k = 0; any; ++k) {
                const int64_t len = (int64_t)(k + 1) * tc;
                open();
                rc = timed(1, launch_blk_residual(c, d_A, lda, N, tr, V + (int64_t)k * vs, Zero, R, g.ldt, g.ntiles));   // -op(A) v_k
                open();
                if (!rc) rc = timed(0, tile_getrs(c, d_LU, ldlu, N, tr, R, R, S1, S2, g));                              // -M^-1 op(A) v_k
                open();
                if (!rc) rc = timed(2, launch_gmres_ortho(c, V, vs, k + 1, R, g.ldt, N, g.ntiles, d_live, c->gm_part, c->gm_out));
                if (rc) return rc;
                MPF_HIP_TRY(c, hipMemcpyAsync(out.data(), c->gm_out, (size_t)(2 * len + tc) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
                MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));
                ++inner_steps;
                any = false;
                for (int64_t j = 0; j < ncols; ++j) {
                    ctl[(size_t)j] = 0.0;
                    if (!live[(size_t)j]) continue;
                    double *h = out.data() + j;
                    for (int i = 0; i <= k; ++i) h[(size_t)i * tc] += h[(size_t)(len + i * tc)];   // H[0 .. k, k] = h + h'
                    const double hn = std::sqrt(out[(size_t)(2 * len + j)]);
                    live[(size_t)j] = col[(size_t)j].inner_step(st[(size_t)(j0 + j)], h, (size_t)tc, hn);
                    if (live[(size_t)j] && hn > 0) ctl[(size_t)j] = 1.0 / hn;
                    any = any || live[(size_t)j];
                }
                if (!any) break;
                rc = send_step(live);
                if (!rc) rc = launch_gmres_append(c, R, d_scale, V + (int64_t)(k + 1) * vs, g.ldt, N, g.ntiles);   // v_{k+1} = w / hn
                if (rc) return rc;
            }
            inner_wall_ms += ms_since(t_inner);
            std::fill(ctl.begin(), ctl.end(), 0.0);
            for (int64_t j = 0; j < ncols; ++j) {   // every column that ran this outer step: its own y, its own count
                if (!active[(size_t)j]) continue;
                GmresCol &cj = col[(size_t)j];
                cj.solve_y();
                cnt[(size_t)j] = cj.k;
                for (int i = 0; i < cj.k; ++i) ctl[(size_t)(i * tc + j)] = cj.y[(size_t)i];
            }
            std::memcpy(ctl.data() + (int64_t)m * tc, cnt.data(), (size_t)tc * sizeof(int));
            MPF_HIP_TRY(c, hipMemcpyAsync(c->gm_ctl, ctl.data(), (size_t)(m * tc + (tc + 1) / 2) * sizeof(double), hipMemcpyHostToDevice, c->stream));
            rc = launch_gmres_xupdate(c, V, vs, d_y, d_cnt, Xt, g.ldt, N, g.ntiles);
            if (rc) return rc;
            MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));   // `ctl` is a host vector reused by the next step
            std::fill(ctl.begin(), ctl.end(), 0.0);
        }
        rc = launch_blk_store(c, Xt, g.ldt, nullptr, N, ncols, d_X + (int64_t)j0 * ldx, ldx);
        if (rc) return rc;
    }
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
    if (check_args(c, "getrs", trans, N, nrhs, ldlu, ldb)) return -1;
    if (nrhs == 0) return 0;
    if (!d_LU || !d_ipiv || !d_B) { c->err = "getrs: null pointer"; return -1; }
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    int rc = solve_setup(c, d_LU, ldlu, d_ipiv, N);
    if (rc) return rc;
    const bool tr = trans == 1;
    for (int32_t j0 = 0; j0 < nrhs; j0 += GROUP_TILES * BLK_T) {
        const int64_t ncols = std::min<int64_t>(nrhs - j0, GROUP_TILES * BLK_T);
        Group g;
        rc = group_tiles(c, N, (int)((ncols + BLK_T - 1) / BLK_T), 2, g);
        if (rc) return rc;
        double *W = g.t(0), *Z = g.t(1), *B = d_B + (int64_t)j0 * ldb;
        rc = launch_blk_load(c, B, ldb, tr ? nullptr : c->perm_buf, N, ncols, W, g.ldt, g.ntiles);
        if (!rc) rc = tile_solve(c, d_LU, ldlu, N, tr, W, Z, g);
        if (!rc) rc = launch_blk_store(c, W, g.ldt, tr ? c->perm_buf : nullptr, N, ncols, B, ldb);
        if (rc) return rc;
    }
    MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return solve_check_waits(c);
}

int mpf_solve_ir_block(mpf_ctx *c, int32_t trans, const double *d_A, int64_t lda, const double *d_LU, int64_t ldlu, const int32_t *d_ipiv,
                       int64_t N, int32_t nrhs, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t max_iter, double tol,
                       mpf_ir_stats *stats) {
    if (!c) return -1;
    if (check_args(c, "solve_ir_block", trans, N, nrhs, ldlu, ldb)) return -1;
    if (lda < N || ldx < N) { c->err = "solve_ir_block: leading dimension < N"; return -1; }
    if (nrhs == 0) return 0;
    if (!d_A || !d_LU || !d_ipiv || !d_B || !d_X) { c->err = "solve_ir_block: null pointer"; return -1; }
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    const auto t0 = std::chrono::steady_clock::now();
    int rc = solve_setup(c, d_LU, ldlu, d_ipiv, N);
    if (rc) return rc;
    std::vector<mpf_ir_stats> st((size_t)nrhs);
    rc = blk_refine_core(c, trans == 1, d_A, lda, d_LU, ldlu, N, nrhs, d_B, ldb, d_X, ldx, max_iter, tol, nullptr, nullptr, st.data());
    if (rc) return rc;
    MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));
    const double ms = ms_since(t0);
    for (auto &s : st) s.ms_total = ms;
    if (stats) std::copy(st.begin(), st.end(), stats);
    return solve_check_waits(c);
}

int mpf_gerfs(mpf_ctx *c, int32_t trans, const double *d_A, int64_t lda, const double *d_LU, int64_t ldlu, const int32_t *d_ipiv,
              int64_t N, int32_t nrhs, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t itmax, double *ferr,
              double *berr, mpf_gerfs_stats *stats) {
    if (!c) return -1;
    if (check_args(c, "gerfs", trans, N, nrhs, ldlu, ldb)) return -1;
    if (lda < N || ldx < N) { c->err = "gerfs: leading dimension < N"; return -1; }
    if (nrhs == 0) return 0;
    if (!d_A || !d_LU || !d_ipiv || !d_B || !d_X || !ferr || !berr) { c->err = "gerfs: null pointer"; return -1; }
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    const auto t0 = std::chrono::steady_clock::now();
    int rc = solve_setup(c, d_LU, ldlu, d_ipiv, N);
    if (rc) return rc;
    std::vector<mpf_gerfs_stats> st((size_t)nrhs);
    rc = blk_bounds_core(c, trans == 1, d_A, lda, d_LU, ldlu, N, nrhs, d_B, ldb, d_X, ldx, itmax, ferr, berr, nullptr, nullptr, st.data());
    if (rc) return rc;
    MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));
    const double ms = ms_since(t0);
    for (auto &s : st) s.ms_total = ms;
    if (stats) std::copy(st.begin(), st.end(), stats);
    return solve_check_waits(c);
}

int mpf_residual_x(mpf_ctx *c, int32_t trans, const double *d_A, int64_t lda, int64_t N, int32_t nrhs, const double *d_X, int64_t ldx,
                   const double *d_B, int64_t ldb, double *d_R, int64_t ldr) {
    if (!c) return -1;
    if (check_args(c, "residual_x", trans, N, nrhs, lda, ldb)) return -1;
    if (ldx < N || ldr < N) { c->err = "residual_x: leading dimension < N"; return -1; }
    if (nrhs == 0) return 0;
    if (!d_A || !d_X || !d_B || !d_R) { c->err = "residual_x: null pointer"; return -1; }
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    for (int32_t j0 = 0; j0 < nrhs; j0 += GROUP_TILES * BLK_T) {
        const int64_t ncols = std::min<int64_t>(nrhs - j0, GROUP_TILES * BLK_T);
        Group g;
        int rc = group_tiles(c, N, (int)((ncols + BLK_T - 1) / BLK_T), 3, g);
        if (rc) return rc;
        double *Bt = g.t(0), *Xt = g.t(1), *R = g.t(2);
        rc = launch_blk_load(c, d_B + (int64_t)j0 * ldb, ldb, nullptr, N, ncols, Bt, g.ldt, g.ntiles);
        if (!rc) rc = launch_blk_load(c, d_X + (int64_t)j0 * ldx, ldx, nullptr, N, ncols, Xt, g.ldt, g.ntiles);
        if (!rc) rc = launch_blk_residual_x(c, d_A, lda, N, trans == 1, Xt, Bt, R, g.ldt, g.ntiles);
        if (!rc) rc = launch_blk_store(c, R, g.ldt, nullptr, N, ncols, d_R + (int64_t)j0 * ldr, ldr);
        if (rc) return rc;
    }
    MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return 0;
}

int mpf_gerfsx(mpf_ctx *c, int32_t trans, const double *d_A, int64_t lda, const double *d_LU, int64_t ldlu, const int32_t *d_ipiv,
               int64_t N, int32_t nrhs, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, int32_t ithresh, double *err_norm,
               double *err_comp, mpf_gerfsx_stats *stats) {
    if (!c) return -1;
    if (check_args(c, "gerfsx", trans, N, nrhs, ldlu, ldb)) return -1;
    if (lda < N || ldx < N) { c->err = "gerfsx: leading dimension < N"; return -1; }
    if (nrhs == 0) return 0;
    if (!d_A || !d_LU || !d_ipiv || !d_B || !d_X || !err_norm || !err_comp) { c->err = "gerfsx: null pointer"; return -1; }
    if (ithresh <= 0) ithresh = 10;
    if (ithresh > 31) ithresh = 31;
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    const auto t0 = std::chrono::steady_clock::now();
    int rc = solve_setup(c, d_LU, ldlu, d_ipiv, N);
    if (rc) return rc;
    std::vector<mpf_gerfsx_stats> st((size_t)nrhs);
    rc = blk_xrefine_core(c, trans == 1, d_A, lda, d_LU, ldlu, N, nrhs, d_B, ldb, d_X, ldx, ithresh, err_norm, err_comp, st.data());
    if (rc) return rc;
    MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));
    const double ms = ms_since(t0);
    bool all = true;
    for (auto &s : st) { s.ms_total = ms; all = all && s.x_state == XrCol::X_CONV; }
    if (stats) std::copy(st.begin(), st.end(), stats);
    rc = solve_check_waits(c);
    return rc ? rc : (all ? 0 : 1);
}

int mpf_solve_gmres_ir_block(mpf_ctx *c, int32_t trans, const double *d_A, int64_t lda, const double *d_LU, int64_t ldlu,
                             const int32_t *d_ipiv, int64_t N, int32_t nrhs, const double *d_B, int64_t ldb, double *d_X, int64_t ldx,
                             int32_t max_outer, int32_t restart, double tol, mpf_gmres_stats *stats) {
    if (!c) return -1;
    if (check_args(c, "solve_gmres_ir_block", trans, N, nrhs, ldlu, ldb)) return -1;
    if (lda < N || ldx < N) { c->err = "solve_gmres_ir_block: leading dimension < N"; return -1; }
    if (nrhs == 0) return 0;
    if (!d_A || !d_LU || !d_ipiv || !d_B || !d_X) { c->err = "solve_gmres_ir_block: null pointer"; return -1; }
    gmres_clamp(max_outer, restart);
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    const auto t0 = std::chrono::steady_clock::now();
    int rc = solve_setup(c, d_LU, ldlu, d_ipiv, N);
    if (rc) return rc;
    std::vector<mpf_gmres_stats> st((size_t)nrhs);
    rc = blk_gmres_core(c, trans == 1, d_A, lda, d_LU, ldlu, N, nrhs, d_B, ldb, d_X, ldx, max_outer, restart, tol, st.data());
    if (rc) return rc;
    MPF_HIP_TRY(c, hipStreamSynchronize(c->stream));
    const double ms = ms_since(t0);
    bool all = true;
    for (auto &s2 : st) { s2.ms_total = ms; all = all && s2.converged; }
    if (stats) std::copy(st.begin(), st.end(), stats);
    rc = solve_check_waits(c);
    return rc ? rc : (all ? 0 : 1);
}

} // extern "C"
