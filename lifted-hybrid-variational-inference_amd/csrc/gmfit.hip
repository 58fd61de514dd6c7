// gmfit.hip -- batched EM fit of scalar Gaussian mixtures to the rows of x [R][n] (sampling_utils.fit_scalar_gm_from_samples),
// gfx950.
//   gm_fit_kernel<KT>   one workgroup of LHVI_GMFIT_BLOCK threads per row; centring, the Lloyd iterations of the start and
//                       the EM loop are phases of the one launch, the stop decision is taken by lane 0 and read by the
//                       whole workgroup from LDS.  KT: the compile-time bound of the component loops (K <= KT).
// The arithmetic is csrc/gmfit.hpp's, shared with the host twin at the end of this file.
//
// Per pass a thread keeps its 3 KT + 1 partial sums in registers.  They are added over the wave on the DPP path, lane 0 of
// every wave stores its totals to LDS, and after a barrier thread 0 adds the waves in index order: no atomics, the same bits
// in every run and at every position of the row in the launch.  The workgroup size is a compile-time constant because the
// order of the sums, and with it the last bits of a fit, depends on it (docs/kernels_gmfit.md has both sizes measured).
#include "common.hpp"
#include "gmfit.hpp"

#ifndef LHVI_GMFIT_BLOCK
#define LHVI_GMFIT_BLOCK 256
#endif

namespace lhvi {
namespace gmfit {

constexpr int GM_BLOCK = LHVI_GMFIT_BLOCK;
constexpr int GM_WAVES = GM_BLOCK / WAVE;
constexpr int PART_STRIDE = 3 * MAX_K + 1;
static_assert(GM_BLOCK % WAVE == 0 && GM_BLOCK >= WAVE && GM_BLOCK <= 1024, "whole wavefronts, at most 1024 threads");

struct DevCtx {
    int lane, lanes;
    bool aligned;           // the row starts on a 16-byte boundary: a pair is one load
    double* part;           // LDS [GM_WAVES][PART_STRIDE]
    __device__ __forceinline__ void load2(const double* x, int64_t p, double& a, double& b) const {
        if (aligned) {
            const double2 v = ld2(x, p);
            a = v.x, b = v.y;
        } else {
            a = x[2 * p], b = x[2 * p + 1];
        }
    }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    template <int M>
    __device__ __forceinline__ void reduce(double (&acc)[M]) const {
        static_assert(M <= PART_STRIDE, "the LDS rows hold 3 MAX_K + 1 sums");
        const int wave = lane / WAVE;
#pragma unroll
        for (int j = 0; j < M; ++j) {
            const double t = dpp_wave_reduce(acc[j], SumOp());
            if (lane % WAVE == 0) part[wave * PART_STRIDE + j] = t;
        }
        __syncthreads();
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < M; ++j) {
                double t = part[j];
                for (int wv = 1; wv < GM_WAVES; ++wv) t += part[wv * PART_STRIDE + j];
                acc[j] = t;
            }
        }
    }
};

template <int KT>
__global__ void __launch_bounds__(GM_BLOCK) gm_fit_kernel(Args a, const double* __restrict__ x, const double* __restrict__ init,
                                                          double* w, double* mu, double* var, double* lower_bound,
                                                          int32_t* n_iter, int32_t* flags) {
    __shared__ double part[GM_WAVES * PART_STRIDE];
    __shared__ double sh[SH_DOUBLES];
    const int64_t r = blockIdx.x;
    const double* xr = x + r * a.n;
    const DevCtx ctx{(int)threadIdx.x, GM_BLOCK, (reinterpret_cast<uintptr_t>(xr) & 15) == 0, part};
    fit_row<KT>(a, xr, init ? init + r * 3 * a.K : nullptr, ctx, sh, w + r * a.K, mu + r * a.K, var + r * a.K, lower_bound + r,
                n_iter + r, flags + r);
}

static int fit_check(int32_t R, int64_t n, int32_t K, const double* x, double reg_covar, int32_t max_iter, int32_t kmeans_its,
                     double* w, double* mu, double* var, double* lower_bound, int32_t* n_iter, int32_t* flags) {
    if (R < 1 || K < 1 || K > LHVI_GMFIT_MAX_K || n < K || max_iter < 1 || kmeans_its < 0 || !(reg_covar >= 0.0)) return LHVI_E_ARG;
    if (!x || !w || !mu || !var || !lower_bound || !n_iter || !flags) return LHVI_E_ARG;
    return LHVI_OK;
}

static Args make_args(int64_t n, int32_t K, double reg_covar, double tol, int32_t max_iter, int32_t kmeans_its) {
    Args a{};
    a.n = n, a.K = K, a.max_iter = max_iter, a.kmeans_its = kmeans_its, a.reg_covar = reg_covar, a.tol = tol;
    for (int k = 0; k < K; ++k) a.q[k] = normal_quantile((k + 0.5) / K);
    return a;
}

}  // namespace gmfit
}  // namespace lhvi

using namespace lhvi;
using namespace lhvi::gmfit;

extern "C" {

int lhvi_gm_fit(int32_t R, int64_t n, int32_t K, const double* x, const double* init, double reg_covar, double tol,
                int32_t max_iter, int32_t kmeans_its, double* w, double* mu, double* var, double* lower_bound, int32_t* n_iter,
                int32_t* flags, void* stream) {
    const int rc = fit_check(R, n, K, x, reg_covar, max_iter, kmeans_its, w, mu, var, lower_bound, n_iter, flags);
    if (rc) return rc;
    const Args a = make_args(n, K, reg_covar, tol, max_iter, kmeans_its);
    hipStream_t st = as_stream(stream);
#define LHVI_GM_LAUNCH(KT) \
    hipLaunchKernelGGL(gm_fit_kernel<KT>, dim3((unsigned)R), dim3(GM_BLOCK), 0, st, a, x, init, w, mu, var, lower_bound, n_iter, flags)
    if (K == 1) LHVI_GM_LAUNCH(1);
    else if (K == 2) LHVI_GM_LAUNCH(2);
    else if (K == 3) LHVI_GM_LAUNCH(3);
    else if (K == 4) LHVI_GM_LAUNCH(4);
    else if (K == 5) LHVI_GM_LAUNCH(5);
    else if (K <= 8) LHVI_GM_LAUNCH(8);
    else LHVI_GM_LAUNCH(16);
#undef LHVI_GM_LAUNCH
    return check_launch();
}

int lhvi_gm_fit_host(int32_t R, int64_t n, int32_t K, const double* x, const double* init, double reg_covar, double tol,
                     int32_t max_iter, int32_t kmeans_its, double* w, double* mu, double* var, double* lower_bound,
                     int32_t* n_iter, int32_t* flags) {
    const int rc = fit_check(R, n, K, x, reg_covar, max_iter, kmeans_its, w, mu, var, lower_bound, n_iter, flags);
    if (rc) return rc;
    const Args a = make_args(n, K, reg_covar, tol, max_iter, kmeans_its);
    double sh[SH_DOUBLES];
    for (int64_t r = 0; r < R; ++r)
        fit_row<MAX_K>(a, x + r * n, init ? init + r * 3 * K : nullptr, HostCtx(), sh, w + r * K, mu + r * K, var + r * K,
                       lower_bound + r, n_iter + r, flags + r);
    return LHVI_OK;
}

}  // extern "C"
