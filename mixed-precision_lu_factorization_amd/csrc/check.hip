// The reference's acceptance test on the device (benchmark.cpp:106-144: get_LU, L * U, reverse row_permute, element-wise
// compare to 1e-10) so that it scales to BASELINE sizes: the reference forms L * U with a CBLAS call on the host
// (benchmark.cpp:77-82), 7e13 flops at N = 32768.  Here R = P^T A - L U is formed with the library's own fp64 MFMA GEMM
// (undoing the pivots on A instead of applying them to L U compares the same element pairs) and reduced to
// max |R| (the reference's criterion) and ||R||_F / ||A||_F.
#include "mpf_internal.h"
#include <cmath>

__global__ __launch_bounds__(256) void split_lu_kernel(const double *__restrict__ LU, long long ldlu, double *__restrict__ Lm,
                                                      double *__restrict__ Um, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= n) return;
    const double v = LU[i + j * ldlu];
    Lm[i + j * n] = i > j ? v : (i == j ? 1.0 : 0.0);   // benchmark.cpp:59-75 get_LU
    Um[i + j * n] = i <= j ? v : 0.0;
}

// per-block partials: [0] max |r| (NaN counts as +inf), [1] sum r^2, [2] sum a^2
__global__ __launch_bounds__(256) void check_reduce_kernel(const double *__restrict__ R, const double *__restrict__ A, long long lda,
                                                          long long n, double *__restrict__ part) {
    __shared__ double sm[3][4];
    double mx = 0, s2 = 0, a2 = 0;
    const long long total = n * n;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const long long i = t % n, j = t / n;
        const double r = R[t], a = A[i + j * lda];
        const double d = r != r ? INFINITY : fabs(r);
        mx = d > mx ? d : mx;
        s2 += r * r;
        a2 += a * a;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double m2 = __shfl_xor(mx, o);
        mx = m2 > mx ? m2 : mx;
        s2 += __shfl_xor(s2, o);
        a2 += __shfl_xor(a2, o);
    }
    if ((threadIdx.x & 63) == 0) { sm[0][threadIdx.x >> 6] = mx; sm[1][threadIdx.x >> 6] = s2; sm[2][threadIdx.x >> 6] = a2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double m = sm[0][0];
        for (int i = 1; i < 4; ++i) m = sm[0][i] > m ? sm[0][i] : m;
        part[3 * blockIdx.x + 0] = m;
        part[3 * blockIdx.x + 1] = (sm[1][0] + sm[1][1]) + (sm[1][2] + sm[1][3]);
        part[3 * blockIdx.x + 2] = (sm[2][0] + sm[2][1]) + (sm[2][2] + sm[2][3]);
    }
}

extern "C" int mpf_check_plu_dev(mpf_ctx *c, const double *d_A, int64_t lda, const double *d_LU, int64_t ldlu, const int32_t *d_ipiv,
                                 int64_t N, double *max_abs_err, double *fro_rel_err) {
    if (!c || !d_A || !d_LU || !d_ipiv) return -1;
    if (N <= 0 || lda < N || ldlu < N) { c->err = "check_plu: bad N / leading dimension"; return -1; }
    MPF_HIP_TRY(c, hipSetDevice(c->device));
    Buf<double> R, Lm, Um, part;
    const int nred = 1024;
    int rc = 0;
    if (R.grow(N * N) != hipSuccess || Lm.grow(N * N) != hipSuccess || Um.grow(N * N) != hipSuccess || part.grow(3 * nred) != hipSuccess) {
        c->err = "check_plu: out of device memory (needs 3 N^2 doubles of scratch)";
        return -2;
    }
    if (hipMemcpy2DAsync(R, (size_t)N * 8, d_A, (size_t)lda * 8, (size_t)N * 8, (size_t)N, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) return -2;
    // P^T A: the swaps in forward order on every column (the inverse of benchmark.cpp:84-95's reverse pass over L U)
    rc = launch_laswp_seq(c, R, N, N, 0, (int)N, d_ipiv, N);
    if (rc) return rc;
    dim3 g((unsigned)((N + 255) / 256), (unsigned)N);
    split_lu_kernel<<<g, 256, 0, c->stream>>>(d_LU, ldlu, Lm, Um, N);
    rc = launch_dgemm_minus(c, N, N, (int)N, Lm, N, Um, N, R, N);   // R -= L U (benchmark.cpp:77-82 on the MFMA GEMM)
    if (rc) return rc;
    check_reduce_kernel<<<nred, 256, 0, c->stream>>>(R, d_A, lda, N, part);
    std::vector<double> h(3 * nred);
    if (hipMemcpyAsync(h.data(), part, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) { c->err = "check_plu: device error"; return -2; }
    double mx = 0, s2 = 0, a2 = 0;
    for (int i = 0; i < nred; ++i) { mx = h[3 * i] > mx ? h[3 * i] : mx; s2 += h[3 * i + 1]; a2 += h[3 * i + 2]; }
    if (max_abs_err) *max_abs_err = mx;
    if (fro_rel_err) *fro_rel_err = a2 > 0 ? std::sqrt(s2 / a2) : std::sqrt(s2);
    return 0;
}

// host-buffer form for the harness (benchmark.cpp:228-233): uploads A, the factors and the pivots, checks on the device
extern "C" int mpf_check_plu_host(const double *A, const double *LU, const int32_t *ipiv, int64_t N, double *max_abs_err,
                                  double *fro_rel_err) {
    if (!A || !LU || !ipiv || N <= 0) return -1;
    mpf_ctx *c = nullptr;
    int rc = mpf_create(&c, 0);
    if (rc) return rc;
    {
        Buf<double> dA, dLU;
        Buf<int32_t> dP;
        const size_t bytes = (size_t)N * (size_t)N * sizeof(double);
        if (dA.grow(N * N) != hipSuccess || dLU.grow(N * N) != hipSuccess || dP.grow(N) != hipSuccess) rc = -2;
        if (!rc && (hipMemcpy(dA, A, bytes, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dLU, LU, bytes, hipMemcpyHostToDevice) != hipSuccess ||
                    hipMemcpy(dP, ipiv, (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess)) rc = -2;
        if (!rc) rc = mpf_check_plu_dev(c, dA, N, dLU, N, dP, N, max_abs_err, fro_rel_err);
    }   // (the buffers go before the context)
    mpf_destroy(c);
    return rc;
}
