// gmfit.hpp -- EM fit of a K-component scalar Gaussian mixture to one row of samples (sampling_utils.fit_scalar_gm_from_samples:
// scikit-learn's GaussianMixture(n_components=K, covariance_type='diag') on one column), written once for the device
// (csrc/gmfit.hip: one workgroup per row) and the host (lhvi_gm_fit_host: one "lane").  docs/kernels_gmfit.md.
//
// A row is read in PAIRS: lane l of L takes the pairs l, l + L, ... and within a pair the even element first, so which lane
// adds which sample in which order depends on (n, L) alone -- not on the alignment of the row, which only decides whether a
// pair is one 16-byte load or two 8-byte ones.  Ctx::reduce adds the lanes' partial sums in a fixed order.  Contraction is
// off for the whole file: a * b + c is rounded twice on both sides, so the host twin differs from the device only by the
// order of its sums and by the library's exp / log.
//
// Ctx: lane, lanes; load2(x, p, a, b): elements 2p, 2p + 1; reduce(acc): the lanes' totals of every acc[j] in lane 0, after
// a barrier; sync(): barrier.  Every barrier is reached by all lanes: the branches around them are on values read from `sh`
// after a barrier, or on launch arguments.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>
#include "../../include/lhvi.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LHVI_HD __host__ __device__ __forceinline__
#else
#define LHVI_HD inline
#endif

#pragma clang fp contract(off)

namespace lhvi {
namespace gmfit {

constexpr int MAX_K = LHVI_GMFIT_MAX_K;
constexpr double LOG_2PI = 1.8378770664093453;
constexpr double NEG_INF = -__builtin_huge_val();
// the parameters every lane reads, written by lane 0 between two barriers: per component a = log w - (log 2 pi + log var) / 2,
// mu (the Lloyd centre before the fit), 1 / var, w, var; then the row's mean and the stop word
enum { SH_A = 0, SH_MU = MAX_K, SH_IV = 2 * MAX_K, SH_W = 3 * MAX_K, SH_VAR = 4 * MAX_K, SH_MEAN = 5 * MAX_K, SH_STOP, SH_DOUBLES };
enum { FLAG_CONVERGED = 1, FLAG_NONFINITE = 2 };

struct Args {
    int64_t n;
    int32_t K, max_iter, kmeans_its;
    double reg_covar, tol;
    double q[MAX_K];        // Phi^-1((k + 1/2) / K): the start centres in units of the row's standard deviation
};

struct HostCtx {
    int lane = 0, lanes = 1;
    void load2(const double* x, int64_t p, double& a, double& b) const { a = x[2 * p], b = x[2 * p + 1]; }
    template <int M>
    void reduce(double (&)[M]) const {}
    void sync() const {}
};

// f(x[i]) for the lane's samples; the next pair is loaded before the current one is used
template <class Ctx, class F>
LHVI_HD void for_each(const double* x, int64_t n, const Ctx& ctx, F&& f) {
    const int64_t np = n >> 1;
    int64_t p = ctx.lane;
    double a0 = 0.0, b0 = 0.0;
    if (p < np) ctx.load2(x, p, a0, b0);
    while (p < np) {
        const int64_t q = p + ctx.lanes;
        double a1 = 0.0, b1 = 0.0;
        if (q < np) ctx.load2(x, q, a1, b1);
        f(a0);
        f(b0);
        a0 = a1, b0 = b1, p = q;
    }
    if ((n & 1) && np % ctx.lanes == ctx.lane) f(x[n - 1]);
}

// _estimate_gaussian_parameters / _estimate_gaussian_covariances_diag / _m_step of scikit-learn 1.7 from the sums nk, s1, s2
// of r_k, r_k y, r_k y^2 (acc[k], acc[KT + k], acc[2 KT + k]), and what the E-step reads
template <int KT>
LHVI_HD void m_step(const Args& a, const double* acc, double* sh) {
    double wsum = 0.0;
#pragma unroll
    for (int k = 0; k < KT; ++k)            // (constant indices: acc stays in registers)
        if (k < a.K) {
            const double nk = acc[k] + 10.0 * DBL_EPSILON, mu = acc[KT + k] / nk;
            sh[SH_MU + k] = mu;
            sh[SH_VAR + k] = acc[2 * KT + k] / nk - mu * mu + a.reg_covar;
            sh[SH_W + k] = nk / (double)a.n;
            wsum += sh[SH_W + k];
        }
    for (int k = 0; k < a.K; ++k) sh[SH_W + k] /= wsum;
}

LHVI_HD void e_step_consts(const Args& a, double* sh) {
    for (int k = 0; k < a.K; ++k) {
        sh[SH_A + k] = log(sh[SH_W + k]) - 0.5 * (LOG_2PI + log(sh[SH_VAR + k]));
        sh[SH_IV + k] = 1.0 / sh[SH_VAR + k];
    }
}

// the fit of one row x[0 .. n): KT >= K is the compile-time bound of the component loops; sh: SH_DOUBLES doubles shared by
// the lanes.  Lane 0 writes w, mu, var [K], lower_bound, n_iter, flags.
template <int KT, class Ctx>
LHVI_HD void fit_row(const Args& a, const double* x, const double* init, const Ctx& ctx, double* sh, double* w, double* mu,
                     double* var, double* lower_bound, int32_t* n_iter, int32_t* flags) {
    const int K = a.K;
    const int64_t n = a.n;
    double acc[3 * KT + 1];
    auto clear = [&]() {
#pragma unroll
        for (int j = 0; j < 3 * KT + 1; ++j) acc[j] = 0.0;
    };
    // ---- centring: the mean, and whether every sample is finite
    clear();
    for_each(x, n, ctx, [&](double v) {
        acc[0] += v;
        acc[1] += fabs(v) <= DBL_MAX ? 0.0 : 1.0;
    });
    ctx.reduce(acc);
    if (ctx.lane == 0) {
        const bool bad = acc[1] > 0.0;
        sh[SH_MEAN] = acc[0] / (double)n;
        sh[SH_STOP] = bad ? 1.0 : 0.0;
        if (bad) {
            for (int k = 0; k < K; ++k) w[k] = mu[k] = var[k] = __builtin_nan("");
            *lower_bound = __builtin_nan("");
            *n_iter = 0;
            *flags = FLAG_NONFINITE;
        }
    }
    ctx.sync();
    if (sh[SH_STOP] != 0.0) return;
    const double mean = sh[SH_MEAN];                    // (lane 0 writes SH_STOP again only after the barrier of a later reduce)

    if (init) {                 // weights_init / means_init / precisions_init of scikit-learn: taken as they are
        if (ctx.lane == 0) {
            for (int k = 0; k < K; ++k) {
                sh[SH_W + k] = init[k];
                sh[SH_MU + k] = init[K + k] - mean;
                sh[SH_VAR + k] = init[2 * K + k];
            }
            e_step_consts(a, sh);
        }
        ctx.sync();
    } else {
        // ---- the deterministic start: centres at the quantiles of N(0, sd^2), Lloyd iterations, one M-step from the labels
        clear();
        for_each(x, n, ctx, [&](double v) {
            const double y = v - mean;
            acc[0] += y * y;
        });
        ctx.reduce(acc);
        if (ctx.lane == 0) {
            const double sd = sqrt(acc[0] / (double)n);
            for (int k = 0; k < K; ++k) sh[SH_MU + k] = sd * a.q[k];
        }
        ctx.sync();
        for (int t = 0; t <= a.kmeans_its; ++t) {
            double c[KT];
#pragma unroll
            for (int k = 0; k < KT; ++k) c[k] = k < K ? sh[SH_MU + k] : 0.0;
            clear();
            for_each(x, n, ctx, [&](double v) {
                const double y = v - mean;
                int best = 0;
                double dbest = fabs(y - c[0]);
#pragma unroll
                for (int k = 1; k < KT; ++k)
                    if (k < K) {
                        const double d = fabs(y - c[k]);
                        if (d < dbest) dbest = d, best = k;         // ties to the lowest component
                    }
#pragma unroll
                for (int k = 0; k < KT; ++k)
                    if (k < K) {
                        const bool s = k == best;
                        acc[k] += s ? 1.0 : 0.0;
                        acc[KT + k] += s ? y : 0.0;
                        acc[2 * KT + k] += s ? y * y : 0.0;
                    }
            });
            ctx.reduce(acc);
            if (ctx.lane == 0) {
                if (t < a.kmeans_its) {
#pragma unroll
                    for (int k = 0; k < KT; ++k)
                        if (k < K && acc[k] > 0.0) sh[SH_MU + k] = acc[KT + k] / acc[k];        // an empty cluster keeps its centre
                } else {
                    m_step<KT>(a, acc, sh);
                    e_step_consts(a, sh);
                }
            }
            ctx.sync();
        }
    }

    // ---- EM
    double prev = NEG_INF;      // lane 0
    int it = 0;
    for (;;) {
        double ca[KT], cm[KT], ci[KT];
#pragma unroll
        for (int k = 0; k < KT; ++k) {
            ca[k] = k < K ? sh[SH_A + k] : 0.0;
            cm[k] = k < K ? sh[SH_MU + k] : 0.0;
            ci[k] = k < K ? sh[SH_IV + k] : 0.0;
        }
        clear();
        for_each(x, n, ctx, [&](double v) {
            const double y = v - mean;
            double lp[KT];
            double m = NEG_INF;
#pragma unroll
            for (int k = 0; k < KT; ++k)
                if (k < K) {
                    const double d = y - cm[k];
                    lp[k] = ca[k] - 0.5 * (d * d) * ci[k];
                    m = fmax(m, lp[k]);
                }
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < KT; ++k)
                if (k < K) {
                    lp[k] = exp(lp[k] - m);
                    s += lp[k];
                }
            acc[3 * KT] += m + log(s);
            const double inv = 1.0 / s, yy = y * y;
#pragma unroll
            for (int k = 0; k < KT; ++k)
                if (k < K) {
                    const double r = lp[k] * inv;
                    acc[k] += r;
                    acc[KT + k] += r * y;
                    acc[2 * KT + k] += r * yy;
                }
        });
        ctx.reduce(acc);
        if (ctx.lane == 0) {
            const double lb = acc[3 * KT] / (double)n, change = lb - prev;
            prev = lb;
            m_step<KT>(a, acc, sh);
            e_step_consts(a, sh);
            ++it;
            const bool conv = fabs(change) < a.tol, stop = conv || it >= a.max_iter;
            sh[SH_STOP] = stop ? 1.0 : 0.0;
            if (stop) {
                for (int k = 0; k < K; ++k) w[k] = sh[SH_W + k], mu[k] = sh[SH_MU + k] + mean, var[k] = sh[SH_VAR + k];
                *lower_bound = lb;
                *n_iter = it;
                *flags = conv ? FLAG_CONVERGED : 0;
            }
        }
        ctx.sync();
        if (sh[SH_STOP] != 0.0) break;
    }
}

// Phi^-1(p), 0 < p < 1, by bisection on erfc: host only, K values per call
inline double normal_quantile(double p) {
    double lo = -40.0, hi = 40.0;
    for (int i = 0; i < 200 && lo < hi; ++i) {
        const double z = 0.5 * (lo + hi);
        if (z <= lo || z >= hi) break;
        if (0.5 * erfc(-z * 0.70710678118654752440) < p) lo = z; else hi = z;
    }
    return 0.5 * (lo + hi);
}

}  // namespace gmfit
}  // namespace lhvi
