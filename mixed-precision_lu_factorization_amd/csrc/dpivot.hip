// fp64 panel with partial pivoting (LAPACK dgetf2): the pivot of column j is searched in fp64 on the numbers being eliminated --
// the first row p >= j with the largest |a_pj| (idamax: strict >, a NaN never beats a number, an all-zero or all-NaN rest keeps
// p = j) -- instead of on an fp16 image of the panel (fp16_panel*.hip), so |l_ij| <= 1 holds, scaling the matrix by a power of
// two changes nothing, and fp16's range plays no part.
//
// The arithmetic is dpanel.hip's (contract C3: m = a_ij / a_jj, then per element one update per k in ascending order, separate
// multiply and subtract or one FMA): the factored panel equals, bit for bit, launch_dgetf2_npv on the same panel with its rows
// pre-permuted by the pivots returned here.
//
// The kernel boundary is the only inter-workgroup synchronisation: nothing spins, nothing waits, nothing has to be co-resident
// (the scheme of fp16_panel_generic.hip).  The panel goes by sub-panels of DV_IB = 32 columns:
//   dpv_step     ONE launch per column j of the sub-panel (+ one in front of the first).  A workgroup owns the same 256 rows for the
//                whole sub-panel, a thread one row.  Every workgroup picks the winner from the per-workgroup candidates the previous
//                launch left, divides its rows of column j by the pivot, applies the rank-1 update to the rest of the sub-panel and
//                leaves its candidate for column j + 1.  The two rows of the interchange never travel through the panel inside a
//                launch: a candidate's 32-wide row goes to a side buffer with the candidate, row j + 1 (the next "old row j") to
//                another one; the thread that owns row p computes on the old row j and stores it at p, workgroup 0 stores the
//                pivot row at j.  So nobody reads a row another workgroup of the same launch writes.  Side buffers alternate
//                between launches.
//   dpv_swap     the sub-panel's interchanges on the panel's other columns (left and right of it), one thread per column;
//   dpv_usolve   U row-block right of the sub-panel (unit-lower solve with the 32 x 32 tile), one thread per column;
//   dpv_update   rank-32 update of the rows below the tile right of the sub-panel, k ascending per element (dpanel_update's order).
// Launches per column: 1 + 4 / 32.  Algorithmic bytes of a column step at sub-panel column jj on `rows` rows: 16 (w - jj) rows
// (columns jj .. w-1 read and written once) + 288 bytes of candidates per workgroup.
//
// Tournament pivoting (launch_dgetf2_tp, the rule of mpf_dgetf2_tp in include/mpf_c.h; second half of this file) keeps dpv_usolve and
// dpv_update and replaces the w + 1 column steps of a sub-panel by
//   dtp_select   1 + ceil(log8(groups)) launches: a workgroup runs partial pivoting on a PRIVATE copy of its <= 256 rows (level 0: 256
//                consecutive panel rows; level l >= 1: the winners of eight groups of the level before) and leaves its winners'
//                original rows, with their row numbers, in its slot of a candidate buffer; the last launch is one workgroup and turns
//                the winners into the sub-panel's interchanges;
//   dtp_swap     those interchanges on ALL columns of the panel, resolved into one pass of loads and one of stores per column;
//   dtp_factor   the sub-panel without pivoting: every workgroup factors the w x w tile in LDS for itself and solves its 256 rows below.
// Nothing reads what another workgroup of the same launch writes.
#include "mpf_internal.h"
#include <limits.h>

constexpr int DV_IB = 32;    // sub-panel width (dpanel.hip's piece width)
constexpr int DV_T = 256;    // rows per workgroup

template <bool FUSED>
__device__ __forceinline__ double dv_mulsub(double x, double m, double u) {
    if (FUSED) return __builtin_fma(-m, u, x);
    const double t = m * u; // file is compiled with -ffp-contract=off: stays mul + sub
    return x - t;
}

// An LDS pointer the optimiser cannot see through: keeps it from hoisting every LDS read of the fully unrolled recurrences to the
// top of the loop nest (hundreds of VGPRs and spills; see dpanel.hip).
typedef __attribute__((address_space(3))) const double dv_lds_cdouble;
__device__ __forceinline__ dv_lds_cdouble *dv_opaque_lds(dv_lds_cdouble *p) {
    asm volatile("" : "+v"(p));
    return p;
}

// search key of an element: |a|'s bit pattern (monotone in |a|), 0 for a NaN
__device__ __forceinline__ unsigned long long dv_key(double a) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(a) & 0x7FFFFFFFFFFFFFFFull;
    return b > 0x7FF0000000000000ull ? 0ull : b;
}
// (k1, r1) beats (k0, r0): larger key, or the same key in an earlier row
__device__ __forceinline__ bool dv_beats(unsigned long long k1, int r1, unsigned long long k0, int r0) {
    return k1 > k0 || (k1 == k0 && r1 < r0);
}
// best (key, row) of the workgroup, in every thread; redk / redr: DV_T / 64 entries each, not reused by the caller before a barrier
__device__ __forceinline__ void dv_block_best(unsigned long long &key, int &row, unsigned long long *redk, int *redr) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)key, o), hi = (unsigned)__shfl_xor((int)(unsigned)(key >> 32), o);
        const unsigned long long k1 = ((unsigned long long)hi << 32) | lo;
        const int r1 = __shfl_xor(row, o);
        if (dv_beats(k1, r1, key, row)) { key = k1; row = r1; }
    }
    if ((threadIdx.x & 63) == 0) { redk[threadIdx.x >> 6] = key; redr[threadIdx.x >> 6] = row; }
    __syncthreads();
    key = redk[0]; row = redr[0];
#pragma unroll
    for (int i = 1; i < DV_T / 64; ++i)
        if (dv_beats(redk[i], redr[i], key, row)) { key = redk[i]; row = redr[i]; }
}

// Side buffers of one launch parity: cand[b] = {key, row} of workgroup b's candidate, crow[b][DV_IB] = that row's sub-panel entries,
// top[DV_IB] = the sub-panel entries of the row that is "row j" of the next step.
struct DvSide { ulonglong2 *cand; double *crow; double *top; };

// One column step.  jj = -1: no elimination, the launch only leaves the candidates and the top row of the sub-panel's first column.
template <bool FUSED>
__global__ __launch_bounds__(DV_T) void dpv_step_kernel(double *P, long long ld, int rows, int j0, int w, int jj, DvSide in, DvSide out,
                                                       int nblk, int *ipiv, int ipiv_offset, int *info, int info_base) {
    __shared__ double u[DV_IB], t[DV_IB];
    __shared__ unsigned long long redk[2][DV_T / 64];
    __shared__ int redr[2][DV_T / 64];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int j = j0 + jj;                                        // panel column (and row) of this step
    const long long r = (long long)j0 + (long long)b * DV_T + tid;   // this thread's row, the same for the whole sub-panel
    int p = -1;
    if (jj >= 0) {
        // ---- the winner over the workgroups' candidates: every workgroup finds the same one ----
        unsigned long long bk = 0;
        int br = INT_MAX;
        for (int i = tid; i < nblk; i += DV_T) {
            const ulonglong2 c = in.cand[i];
            if (dv_beats(c.x, (int)c.y, bk, br)) { bk = c.x; br = (int)c.y; }
        }
        dv_block_best(bk, br, redk[0], redr[0]);
        const bool valid = br >= j && br < rows;                  // always, for j < rows; keeps every access in range regardless
        p = valid ? br : j;
        if (tid < DV_IB) {
            t[tid] = in.top[tid];                                                             // old row j
            u[tid] = valid ? in.crow[(long long)((p - j0) / DV_T) * DV_IB + tid] : t[tid];    // old row p: the pivot row
        }
        __syncthreads();
        if (b == 0) {
            if (tid < w) P[j + (long long)(j0 + tid) * ld] = u[tid];       // the pivot row lands in row j (all sub-panel columns)
            if (tid == 0) {
                ipiv[j] = p + 1 + ipiv_offset;
                if (u[jj] == 0.0 && info) atomicMin(info, info_base + j + 1);
            }
        }
    }
    const int lo = jj < 0 ? 0 : jj;                               // first sub-panel column this step reads
    const bool live = r > j && r < rows;
    const bool moved = jj >= 0 && r == p;                         // this thread's row receives the old row j
    double x[DV_IB];
    if (live) {
#pragma unroll
        for (int c = 0; c < DV_IB; ++c) x[c] = moved ? t[c] : ((c >= lo && c < w) ? P[r + (long long)(j0 + c) * ld] : 0.0);
        if (jj >= 0) {
            double xj = 0.0;
#pragma unroll
            for (int c = 0; c < DV_IB; ++c) xj = c == jj ? x[c] : xj;
            const double m = xj / u[jj];
#pragma unroll
            for (int c = 0; c < DV_IB; ++c) {
                if (c == jj) x[c] = m;
                else if (c > jj && c < w) x[c] = dv_mulsub<FUSED>(x[c], m, u[c]);
            }
#pragma unroll
            for (int c = 0; c < DV_IB; ++c)
                if (c < w && (c >= jj || moved)) P[r + (long long)(j0 + c) * ld] = x[c];
        }
    }
    // ---- this workgroup's candidate for column j + 1, with its row; workgroup 0 also leaves row j + 1 itself ----
    const int jn = jj + 1;
    if (jn >= w) return;
    unsigned long long key = 0;
    int row = INT_MAX;
    if (live) {
        double xn = 0.0;
#pragma unroll
        for (int c = 0; c < DV_IB; ++c) xn = c == jn ? x[c] : xn;
        key = dv_key(xn);
        row = (int)r;
    }
    dv_block_best(key, row, redk[1], redr[1]);
    if (tid == 0) out.cand[b] = make_ulonglong2(key, (unsigned long long)(unsigned)row);
    if (live && (r == row || (b == 0 && r == (long long)j + 1))) {
        // the row's entries left of column jj were not loaded above (unless the row has just moved): they are this thread's own
#pragma unroll
        for (int c = 0; c < DV_IB; ++c)
            if (c < lo && c < w && !moved) x[c] = P[r + (long long)(j0 + c) * ld];
        if (r == row) {
#pragma unroll
            for (int c = 0; c < DV_IB; ++c) out.crow[(long long)b * DV_IB + c] = x[c];
        }
        if (b == 0 && r == (long long)j + 1) {
#pragma unroll
            for (int c = 0; c < DV_IB; ++c) out.top[c] = x[c];
        }
    }
}

// the sub-panel's w interchanges, in order, on the panel's columns outside the sub-panel: one thread per column
__global__ __launch_bounds__(DV_T) void dpv_swap_kernel(double *P, long long ld, int rows, int cols, int j0, int w, const int *ipiv,
                                                       int ipiv_offset) {
    int c = blockIdx.x * DV_T + threadIdx.x;
    if (c >= cols - w) return;
    if (c >= j0) c += w;
    double *a = P + (long long)c * ld;
    for (int jj = 0; jj < w; ++jj) {
        const int cur = j0 + jj, piv = ipiv[cur] - 1 - ipiv_offset;
        if (piv != cur && piv >= 0 && piv < rows) { const double v = a[cur]; a[cur] = a[piv]; a[piv] = v; }
    }
}

// U row-block: rows j0 .. j0+w-1 of the columns right of the sub-panel, x_i -= l_ij x_j for j < i ascending; one thread per column
template <bool FUSED>
__global__ __launch_bounds__(DV_T) void dpv_usolve_kernel(double *P, long long ld, int cols, int j0, int w) {
    __shared__ double L[DV_IB][DV_IB + 1];
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = tid + DV_T * i, rr = e & 31, cc = e >> 5;
        L[rr][cc] = (rr < w && cc < rr) ? P[(j0 + rr) + (long long)(j0 + cc) * ld] : 0.0;
    }
    __syncthreads();
    const long long c = (long long)j0 + w + (long long)blockIdx.x * DV_T + tid;
    if (c >= cols) return;
    double *pc = P + j0 + c * ld;
    double x[DV_IB];
#pragma unroll
    for (int i = 0; i < DV_IB; ++i) x[i] = i < w ? pc[i] : 0.0;
#pragma unroll
    for (int j = 0; j < DV_IB; ++j) {
        dv_lds_cdouble *lj = dv_opaque_lds((dv_lds_cdouble *)&L[0][j]);
#pragma unroll
        for (int i = j + 1; i < DV_IB; ++i)
            if (i < w) x[i] = dv_mulsub<FUSED>(x[i], lj[i * (DV_IB + 1)], x[j]);
    }
#pragma unroll
    for (int i = 0; i < DV_IB; ++i)
        if (i < w) pc[i] = x[i];
}

// rank-w update of the rows below the tile, DV_IB columns per workgroup (blockIdx.y) right of the sub-panel, one row per thread
template <bool FUSED>
__global__ __launch_bounds__(DV_T) void dpv_update_kernel(double *P, long long ld, int rows, int cols, int j0, int w) {
    __shared__ double Ut[DV_IB][DV_IB];   // Ut[j][cc], read as a broadcast
    const int tid = threadIdx.x;
    const int c0 = j0 + w + blockIdx.y * DV_IB;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = tid + DV_T * i, j = e & 31, cc = e >> 5;
        Ut[j][cc] = (j < w && c0 + cc < cols) ? P[(j0 + j) + (long long)(c0 + cc) * ld] : 0.0;
    }
    __syncthreads();
    const long long r = (long long)j0 + w + (long long)blockIdx.x * DV_T + tid;
    if (r >= rows) return;
    double x[DV_IB], mv[DV_IB];
#pragma unroll
    for (int j = 0; j < DV_IB; ++j) mv[j] = P[r + (long long)(j0 + (j < w ? j : w - 1)) * ld];
#pragma unroll
    for (int cc = 0; cc < DV_IB; ++cc) x[cc] = (c0 + cc < cols) ? P[r + (long long)(c0 + cc) * ld] : 0.0;
#pragma unroll
    for (int j = 0; j < DV_IB; ++j) {
        if (j < w) {
            dv_lds_cdouble *uj = dv_opaque_lds((dv_lds_cdouble *)&Ut[j][0]);
#pragma unroll
            for (int cc = 0; cc < DV_IB; ++cc) x[cc] = dv_mulsub<FUSED>(x[cc], mv[j], uj[cc]);
        }
    }
#pragma unroll
    for (int cc = 0; cc < DV_IB; ++cc)
        if (c0 + cc < cols) P[r + (long long)(c0 + cc) * ld] = x[cc];
}

// Scratch of a panel of `rows` rows in 8-byte words: two parities of {candidates (16 bytes each), their rows, the top row}
static int64_t dpiv_scratch_words(int rows) {
    const int64_t nblk = ((int64_t)rows + DV_T - 1) / DV_T;
    return 2 * (2 * nblk + nblk * DV_IB + DV_IB);
}

int dgetf2_piv_reserve(mpf_ctx *c, int rows) {
    MPF_HIP_TRY(c, c->dpiv.grow(dpiv_scratch_words(rows)));
    return 0;
}

int launch_dgetf2_piv(mpf_ctx *c, double *P, int64_t ld, int rows, int cols, int fused, int info_base, int ipiv_offset, int *d_ipiv) {
    if (rows < 1 || cols < 1) return 0;
    { const int e = dgetf2_piv_reserve(c, rows); if (e) return e; }
    int *info = &c->ws->info;
    const int64_t nblk0 = ((int64_t)rows + DV_T - 1) / DV_T;
    DvSide side[2];
    {   // (16-byte aligned: hipMalloc's base, then multiples of 16 bytes)
        unsigned long long *base = c->dpiv;
        for (int q = 0; q < 2; ++q) {
            side[q].cand = (ulonglong2 *)base;
            side[q].crow = (double *)(base + 2 * nblk0);
            side[q].top = side[q].crow + nblk0 * DV_IB;
            base += 2 * nblk0 + nblk0 * DV_IB + DV_IB;
        }
    }
    const int kmax = rows < cols ? rows : cols;                   // columns that have a pivot
    for (int j0 = 0; j0 < kmax; j0 += DV_IB) {
        const int w = kmax - j0 < DV_IB ? kmax - j0 : DV_IB;
        const int nblk = (int)(((int64_t)rows - j0 + DV_T - 1) / DV_T);
        for (int jj = -1; jj < w; ++jj) {
            const DvSide &out = side[(jj + 1) & 1], &in = side[jj & 1];
            if (fused) dpv_step_kernel<true><<<nblk, DV_T, 0, c->stream>>>(P, ld, rows, j0, w, jj, in, out, nblk, d_ipiv, ipiv_offset, info, info_base);
            else dpv_step_kernel<false><<<nblk, DV_T, 0, c->stream>>>(P, ld, rows, j0, w, jj, in, out, nblk, d_ipiv, ipiv_offset, info, info_base);
        }
        if (cols > w)
            dpv_swap_kernel<<<(cols - w + DV_T - 1) / DV_T, DV_T, 0, c->stream>>>(P, ld, rows, cols, j0, w, d_ipiv, ipiv_offset);
        const int right = cols - j0 - w;
        if (right > 0) {
            const int gu = (right + DV_T - 1) / DV_T;
            if (fused) dpv_usolve_kernel<true><<<gu, DV_T, 0, c->stream>>>(P, ld, cols, j0, w);
            else dpv_usolve_kernel<false><<<gu, DV_T, 0, c->stream>>>(P, ld, cols, j0, w);
            const int64_t below = (int64_t)rows - j0 - w;
            if (below > 0) {
                dim3 grid((unsigned)((below + DV_T - 1) / DV_T), (unsigned)((right + DV_IB - 1) / DV_IB));
                if (fused) dpv_update_kernel<true><<<grid, DV_T, 0, c->stream>>>(P, ld, rows, cols, j0, w);
                else dpv_update_kernel<false><<<grid, DV_T, 0, c->stream>>>(P, ld, rows, cols, j0, w);
            }
        }
    }
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}

// ======================================================================================================================================
// Tournament pivoting: the rule is stated in include/mpf_c.h (mpf_dgetf2_tp).
// ======================================================================================================================================
constexpr int TP_FAN = DV_T / DV_IB;             // lists merged at a time: 8 lists of 32 rows fill a stack of 256
constexpr int TP_SLOT = DV_IB * DV_IB;           // doubles of a group's candidate slot: val[c * DV_IB + rank]

// A level's candidates: group g's winner of rank s has its sub-panel entries at val[g * TP_SLOT + c * DV_IB + s] and its panel row
// in idx[g * DV_IB + s] (-1: the group had fewer rows than that).
struct TpCand { double *val; int *idx; };

// select() on one stack per workgroup, one row per thread.  level0: thread t of group g holds panel row j0 + 256 g + t;
// otherwise rank t % 32 of list 8 g + t / 32 of `in` (gin lists).  Rows never move between threads: a thread keeps its row's
// CURRENT position in the stack (cp), which is what dgetf2's interchange changes and what breaks a tie.  last: the launch has ONE workgroup and its list is the
// tournament's: the winners become the interchanges ipiv[j0 .. j0+w-1]; otherwise the list goes to slot g of `out`.
__global__ __launch_bounds__(DV_T) void dtp_select_kernel(const double *P, long long ld, int rows, int j0, int w, int level0, TpCand in, int gin,
                                                         TpCand out, int last, int *ipiv, int ipiv_offset) {
    __shared__ double urow[2][DV_T / 64][DV_IB];             // per step parity and wave: the eliminated row of the wave's best position
    __shared__ unsigned long long redk[2][DV_T / 64];
    __shared__ int redr[2][DV_T / 64];
    __shared__ int win[DV_IB], wcnt[DV_T / 64];
    const int tid = threadIdx.x, g = blockIdx.x, wave = tid >> 6;
    const long long r0 = (long long)j0 + (long long)g * DV_T + tid;     // level 0: this position's panel row
    const int lst = g * TP_FAN + (tid >> 5), rk = tid & 31;              // level >= 1: this position's list and rank
    bool valid;
    if (level0) valid = r0 < rows;
    else valid = lst < gin && in.idx[(long long)lst * DV_IB + rk] >= 0;
    double x[DV_IB];
#pragma unroll
    for (int c = 0; c < DV_IB; ++c) {
        double v = 0.0;
        if (valid && c < w) v = level0 ? P[r0 + (long long)(j0 + c) * ld] : in.val[(long long)lst * TP_SLOT + c * DV_IB + rk];
        x[c] = v;
    }
    // position in the stack: the rows present, in thread order (level 0: the first m threads; above, lists may be short)
    const unsigned long long present = __ballot(valid);
    if ((tid & 63) == 0) wcnt[wave] = __popcll(present);
    const int m = __syncthreads_count(valid);
    const int n = m < w ? m : w;                                         // length of the list
    int cp = __popcll(present & ((1ull << (tid & 63)) - 1ull));
    for (int i = 0; i < wave; ++i) cp += wcnt[i];
    bool open = valid;                                                   // not chosen yet: cp >= s at step s
#pragma unroll
    for (int s = 0; s < DV_IB; ++s) {
        if (s < n) {                                                     // (uniform)
            const int par = s & 1;
            unsigned long long key = open ? dv_key(x[s]) : 0ull;
            const int mine = (cp << 8) | tid;                            // ordered by position (unique among open rows); carries the thread
            int pos = open ? mine : INT_MAX;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)key, o), hi = (unsigned)__shfl_xor((int)(unsigned)(key >> 32), o);
                const unsigned long long k1 = ((unsigned long long)hi << 32) | lo;
                const int p1 = __shfl_xor(pos, o);
                if (dv_beats(k1, p1, key, pos)) { key = k1; pos = p1; }
            }
            if ((tid & 63) == 0) { redk[par][wave] = key; redr[par][wave] = pos; }
            if (open && pos == mine) {                                   // the wave's best publishes its row: the winner's is among the four
#pragma unroll
                for (int c = s; c < DV_IB; ++c) urow[par][wave][c] = x[c];
            }
            __syncthreads();
            key = redk[par][0]; pos = redr[par][0];
#pragma unroll
            for (int i = 1; i < DV_T / 64; ++i)
                if (dv_beats(redk[par][i], redr[par][i], key, pos)) { key = redk[par][i]; pos = redr[par][i]; }
            // (s < n: a row is still open, so pos names one of this workgroup's threads)
            const int wt = pos & (DV_T - 1), wcp = pos >> 8;
            if (tid == 0) win[s] = wt;
            if (tid == wt) open = false;
            else if (open && cp == s) cp = wcp;                          // dgetf2's interchange: the row at position s goes where the pivot row was
            if (open) {
                dv_lds_cdouble *u = dv_opaque_lds((dv_lds_cdouble *)&urow[par][wt >> 6][0]);
                const double mlt = x[s] / u[s];
#pragma unroll
                for (int c = s + 1; c < DV_IB; ++c) x[c] = dv_mulsub<false>(x[c], mlt, u[c]);   // unfused whatever the panel's form is
            }
        }
    }
    __syncthreads();
    if (!last) {
        // the winners' ORIGINAL rows, re-read from the source
#pragma unroll
        for (int i = 0; i < TP_SLOT / DV_T; ++i) {
            const int e = tid + DV_T * i, s = e & 31, c = e >> 5;
            if (s < n && c < w) {
                const int p = win[s];
                const double v = level0 ? P[(long long)j0 + (long long)g * DV_T + p + (long long)(j0 + c) * ld]
                                        : in.val[(long long)(g * TP_FAN + (p >> 5)) * TP_SLOT + c * DV_IB + (p & 31)];
                out.val[(long long)g * TP_SLOT + c * DV_IB + s] = v;
            }
        }
        if (tid < DV_IB) {
            int row = -1;
            if (tid < n) {
                const int p = win[tid];
                row = level0 ? j0 + g * DV_T + p : in.idx[(long long)(g * TP_FAN + (p >> 5)) * DV_IB + (p & 31)];
            }
            out.idx[(long long)g * DV_IB + tid] = row;
        }
    } else if (tid < 64) {
        // winners q_0 .. q_{n-1} -> sequential interchanges: cur = the row at which original row q_lane stands now
        int cur = -1;
        if (tid < n) {
            const int p = win[tid];
            cur = level0 ? j0 + p : in.idx[(long long)(p >> 5) * DV_IB + (p & 31)];
        }
        for (int t = 0; t < n; ++t) {
            const int p = __shfl(cur, t);                                // where q_t stands: exchanged with row j0 + t
            if (tid > t && cur == j0 + t) cur = p;                       // the row that stood at j0 + t goes there
            if (tid == t) ipiv[j0 + t] = p + 1 + ipiv_offset;
        }
    }
}

// The sub-panel's w interchanges on ALL columns of the panel, one thread per column.  Wave 0 first resolves the sequential
// interchanges into what they leave behind -- at most 2 w rows, each receiving one original row -- so a column takes two memory
// round trips (all loads, then all stores) instead of w dependent ones.  Lanes 0 .. 31 stand for rows j0 .. j0+31, lanes 32 .. 63
// for the rows below the tile that an interchange reaches, in the order met.
__global__ __launch_bounds__(DV_T) void dtp_swap_kernel(double *P, long long ld, int rows, int cols, int j0, int w, const int *ipiv,
                                                       int ipiv_offset) {
    __shared__ int mpos[2 * DV_IB], msrc[2 * DV_IB];          // row mpos[i] receives the row that stood at msrc[i]; mpos < 0: nothing
    const int tid = threadIdx.x;
    if (tid < 64) {
        int piv = -1;                                             // lane s < w: the row interchange s exchanges row j0 + s with
        if (tid < w) {
            piv = ipiv[j0 + tid] - 1 - ipiv_offset;
            if (piv < j0 + tid || piv >= rows) piv = j0 + tid;    // (never: keeps every access in range regardless)
        }
        int pos = tid < DV_IB ? j0 + tid : -1, src = pos, nout = 0;
        for (int s = 0; s < w; ++s) {
            const int p = __shfl(piv, s);
            int L;
            if (p < j0 + DV_IB) L = p - j0;
            else {
                const unsigned long long hit = __ballot(tid >= DV_IB && tid - DV_IB < nout && pos == p);
                if (hit) L = __ffsll((long long)hit) - 1;
                else {
                    L = DV_IB + nout++;
                    if (tid == L) { pos = p; src = p; }
                }
            }
            const int a = __shfl(src, s), b = __shfl(src, L);
            if (tid == s) src = b;
            if (tid == L) src = a;
        }
        const bool used = tid < DV_IB || tid - DV_IB < nout;      // (a narrow tail sub-panel reaches rows j0 + w .. j0 + 31 through lanes w .. 31)
        mpos[tid] = (used && src != pos) ? pos : -1;
        msrc[tid] = src;
    }
    __syncthreads();
    const int c = blockIdx.x * DV_T + tid;
    if (c >= cols) return;
    double *a = P + (long long)c * ld;
    double v[2 * DV_IB];
#pragma unroll
    for (int i = 0; i < 2 * DV_IB; ++i) v[i] = mpos[i] >= 0 ? a[msrc[i]] : 0.0;
#pragma unroll
    for (int i = 0; i < 2 * DV_IB; ++i)
        if (mpos[i] >= 0) a[mpos[i]] = v[i];
}

// The sub-panel without pivoting (contract C3's arithmetic: per element one update per k ascending, then the division by the
// diagonal).  Every workgroup factors the w x w tile in LDS for itself; workgroup b brings rows j0 + w + 256 b .. to A21 U11^-1,
// workgroup 0 also stores the tile and reports a zero diagonal entry.
template <bool FUSED>
__global__ __launch_bounds__(DV_T) void dtp_factor_kernel(double *P, long long ld, int rows, int j0, int w, int *info, int info_base) {
    __shared__ double T[DV_IB][DV_IB + 1];
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = tid + DV_T * i, rr = e & 31, cc = e >> 5;
        T[rr][cc] = (rr < w && cc < w) ? P[(j0 + rr) + (long long)(j0 + cc) * ld] : (rr == cc ? 1.0 : 0.0);
    }
    // right-looking, one barrier per step: step k writes only rows and columns > k and reads row k, column k (both final after
    // step k - 1); the multiplier a_ik / a_kk is formed by every thread that needs it and stored once, at the end
    for (int k = 0; k + 1 < w; ++k) {
        __syncthreads();
        const double d = T[k][k];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + DV_T * i, rr = e & 31, cc = e >> 5;
            if (rr > k && cc > k && rr < w && cc < w) {
                double l = T[rr][k] / d;
                asm volatile("" : "+v"(l));   // the fused form negates the QUOTIENT (not the dividend): a NaN keeps dgetf2_npv's sign
                T[rr][cc] = dv_mulsub<FUSED>(T[rr][cc], l, T[k][cc]);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = tid + DV_T * i, rr = e & 31, cc = e >> 5;
        if (rr > cc && rr < w) T[rr][cc] = T[rr][cc] / T[cc][cc];
    }
    __syncthreads();
    if (blockIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + DV_T * i, rr = e & 31, cc = e >> 5;
            if (rr < w && cc < w) P[(j0 + rr) + (long long)(j0 + cc) * ld] = T[rr][cc];
        }
        if (tid < w && T[tid][tid] == 0.0 && info) atomicMin(info, info_base + j0 + tid + 1);
    }
    const long long r = (long long)j0 + w + (long long)blockIdx.x * DV_T + tid;
    if (r >= rows) return;
    double x[DV_IB];
#pragma unroll
    for (int c = 0; c < DV_IB; ++c) x[c] = c < w ? P[r + (long long)(j0 + c) * ld] : 0.0;
#pragma unroll
    for (int k = 0; k < DV_IB; ++k) {
        if (k < w) {
            dv_lds_cdouble *uk = dv_opaque_lds((dv_lds_cdouble *)&T[k][0]);
            const double l = x[k] / uk[k];
            x[k] = l;
#pragma unroll
            for (int c = k + 1; c < DV_IB; ++c) x[c] = dv_mulsub<FUSED>(x[c], l, uk[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < DV_IB; ++c)
        if (c < w) P[r + (long long)(j0 + c) * ld] = x[c];
}

// groups of a level: 256 rows each at level 0, eight lists each above
static int64_t tp_groups0(int64_t rows) { return (rows + DV_T - 1) / DV_T; }
static int64_t tp_groups_up(int64_t g) { return (g + TP_FAN - 1) / TP_FAN; }
// a candidate buffer of g groups in doubles: the rows, then their numbers (32 ints = 16 doubles per group)
static int64_t tp_cand_words(int64_t g) { return g * (TP_SLOT + DV_IB / 2); }

int dgetf2_tp_reserve(mpf_ctx *c, int rows) {
    const int64_t g0 = tp_groups0(rows);
    MPF_HIP_TRY(c, c->dtp.grow(tp_cand_words(g0) + tp_cand_words(tp_groups_up(g0))));
    return 0;
}

int launch_dgetf2_tp(mpf_ctx *c, double *P, int64_t ld, int rows, int cols, int fused, int info_base, int ipiv_offset, int *d_ipiv) {
    if (rows < 1 || cols < 1) return 0;
    { const int e = dgetf2_tp_reserve(c, rows); if (e) return e; }
    int *info = &c->ws->info;
    // level 0 writes buffer 0 (one slot per group of the tallest sub-panel), level 1 buffer 1 (an eighth of that), level 2 buffer 0 again ...
    const int64_t g0max = tp_groups0(rows), g1max = tp_groups_up(g0max);
    TpCand buf[2];
    buf[0].val = c->dtp;
    buf[0].idx = (int *)(buf[0].val + g0max * TP_SLOT);
    buf[1].val = buf[0].val + tp_cand_words(g0max);
    buf[1].idx = (int *)(buf[1].val + g1max * TP_SLOT);
    const TpCand none{nullptr, nullptr};
    const int kmax = rows < cols ? rows : cols;                   // columns that have a pivot
    for (int j0 = 0; j0 < kmax; j0 += DV_IB) {
        const int w = kmax - j0 < DV_IB ? kmax - j0 : DV_IB;
        int g = (int)tp_groups0((int64_t)rows - j0);
        dtp_select_kernel<<<g, DV_T, 0, c->stream>>>(P, ld, rows, j0, w, 1, none, 0, buf[0], g == 1, d_ipiv, ipiv_offset);
        for (int q = 0; g > 1; q ^= 1) {
            const int gn = (int)tp_groups_up(g);
            dtp_select_kernel<<<gn, DV_T, 0, c->stream>>>(P, ld, rows, j0, w, 0, buf[q], g, buf[q ^ 1], gn == 1, d_ipiv, ipiv_offset);
            g = gn;
        }
        dtp_swap_kernel<<<(cols + DV_T - 1) / DV_T, DV_T, 0, c->stream>>>(P, ld, rows, cols, j0, w, d_ipiv, ipiv_offset);
        const int64_t below = (int64_t)rows - j0 - w;
        const unsigned gf = below > 0 ? (unsigned)((below + DV_T - 1) / DV_T) : 1u;
        if (fused) dtp_factor_kernel<true><<<gf, DV_T, 0, c->stream>>>(P, ld, rows, j0, w, info, info_base);
        else dtp_factor_kernel<false><<<gf, DV_T, 0, c->stream>>>(P, ld, rows, j0, w, info, info_base);
        const int right = cols - j0 - w;
        if (right > 0) {
            const int gu = (right + DV_T - 1) / DV_T;
            if (fused) dpv_usolve_kernel<true><<<gu, DV_T, 0, c->stream>>>(P, ld, cols, j0, w);
            else dpv_usolve_kernel<false><<<gu, DV_T, 0, c->stream>>>(P, ld, cols, j0, w);
            if (below > 0) {
                dim3 grid((unsigned)((below + DV_T - 1) / DV_T), (unsigned)((right + DV_IB - 1) / DV_IB));
                if (fused) dpv_update_kernel<true><<<grid, DV_T, 0, c->stream>>>(P, ld, rows, cols, j0, w);
                else dpv_update_kernel<false><<<grid, DV_T, 0, c->stream>>>(P, ld, rows, cols, j0, w);
            }
        }
    }
    MPF_HIP_TRY(c, hipGetLastError());
    return 0;
}
