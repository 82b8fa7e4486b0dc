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
