// exact.hip -- exact hybrid-Gaussian baseline by enumeration of the discrete states (gibbs/hybrid_gaussian_mrf.py), gfx950.
//   exact_config_kernel   one configuration per group of `lanes` lanes of a one-wavefront workgroup, everything in LDS
//                         (csrc/exact.hpp: assembly in factor order, Cholesky, L^-1, mean, diag(J^-1), optionally J^-1)
//   exact_partial_kernel / exact_final_kernel    log Z: max pass, then a sum in a fixed order (the same bits on every run)
//   exact_marginal_kernel every discrete variable's marginal, one workgroup per (variable, state)
//   exact_mix_prepare_kernel / exact_mixture_kernel    the M-component mixture of a continuous variable: log density and its
//                         first two derivatives at x[v, :]
//   exact_polish_kernel   safeguarded Newton on the log density from given starts, clipped to the domain (marginal MAP)
#include "common.hpp"
#include "exact.hpp"
#include "hg_launch.hpp"

namespace lhvi {
namespace exact {

constexpr int RB = 256;            // workgroup of the reductions
constexpr int PARTS = 1024;        // partial results of the two-stage reductions
constexpr int MIX_PTS = 4;         // query points of one mixture workgroup

using hg::DevCtx;

__global__ void __launch_bounds__(WAVE) exact_config_kernel(lhvi_exact_t m, int64_t begin, int64_t count, int lanes, double* logp,
                                                            double* means, double* vars, double* covs, unsigned long long* bad) {
    extern __shared__ double lds[];
    const int gpb = WAVE / lanes, grp = threadIdx.x / lanes;
    const int64_t idx = (int64_t)blockIdx.x * gpb + grp;
    const bool valid = idx < count;
    const int64_t cfg = begin + (valid ? idx : count - 1);      // a padding group repeats the last configuration, stores nothing
    const int ws = (ws_doubles(m.Nc, m.Nd) + 1) & ~1;
    DevCtx ctx{(int)threadIdx.x % lanes, lanes};
    const int rc = config(m, cfg, lds + grp * ws, ctx, valid ? logp + cfg : nullptr, valid ? means + cfg * m.Nc : nullptr,
                          valid ? vars + cfg * m.Nc : nullptr, valid && covs ? covs + cfg * m.Nc * m.Nc : nullptr);
    if (rc && valid && ctx.lane == 0) atomicMin(bad, (unsigned long long)cfg);
}

// ---- fixed-order reductions ----------------------------------------------------------------------------------------------
template <class Op>
__device__ __forceinline__ double block_tree(double v, double* sh, Op op) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = RB / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = op(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// stage 1: part[b] = max (SUM = false) or sum of exp(logp - *shift) (SUM = true) over the b-th contiguous slice
template <bool SUM>
__global__ void __launch_bounds__(RB) exact_partial_kernel(int64_t M, const double* __restrict__ logp, const double* shift,
                                                           double* part) {
    __shared__ double sh[RB];
    const int64_t per = (M + gridDim.x - 1) / gridDim.x, lo = per * blockIdx.x, hi = lo + per < M ? lo + per : M;
    const double sft = SUM ? *shift : 0.0;
    double acc = SUM ? 0.0 : -__builtin_huge_val();
    for (int64_t i = lo + threadIdx.x; i < hi; i += RB) acc = SUM ? acc + exp(logp[i] - sft) : fmax(acc, logp[i]);
    const double r = SUM ? block_tree(acc, sh, SumOp()) : block_tree(acc, sh, MaxOp());
    if (threadIdx.x == 0) part[blockIdx.x] = r;
}

// stage 2 (one workgroup): out[0] = max of the parts (SUM = false) or shift + log(sum of the parts) (SUM = true)
template <bool SUM>
__global__ void __launch_bounds__(RB) exact_final_kernel(int n, const double* __restrict__ part, const double* shift, double* out) {
    __shared__ double sh[RB];
    double acc = SUM ? 0.0 : -__builtin_huge_val();
    for (int i = threadIdx.x; i < n; i += RB) acc = SUM ? acc + part[i] : fmax(acc, part[i]);
    const double r = SUM ? block_tree(acc, sh, SumOp()) : block_tree(acc, sh, MaxOp());
    if (threadIdx.x == 0) out[0] = SUM ? *shift + log(r) : r;
}

__global__ void __launch_bounds__(RB) exact_table_kernel(int64_t M, const double* __restrict__ logp, const double* logZ,
                                                         double* table) {
    const int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x;
    if (i < M) table[i] = exp(logp[i] - *logZ);
}

// workgroup b = the b-th (variable, state) pair: the sum of the table over the other axes
__global__ void __launch_bounds__(RB) exact_marginal_kernel(lhvi_exact_t m, const double* __restrict__ table, double* marg) {
    __shared__ double sh[RB];
    int d = 0, s = blockIdx.x;
    while (s >= m.dstates[d]) s -= m.dstates[d++];
    const int64_t st = m.dstride[d], n = m.M / m.dstates[d];
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += RB) acc += table[(i / st) * st * m.dstates[d] + s * st + i % st];
    const double r = block_tree(acc, sh, SumOp());
    if (threadIdx.x == 0) marg[blockIdx.x] = r;
}

// ---- mixtures --------------------------------------------------------------------------------------------------------------
// mix [Nc][M][3] = (log w_k - 1/2 log(2 pi var_kj), mean_kj, 1 / var_kj); a component of weight 0 gets -inf
__global__ void __launch_bounds__(RB) exact_mix_prepare_kernel(int Nc, int64_t M, const double* __restrict__ table,
                                                               const double* __restrict__ means, const double* __restrict__ vars,
                                                               double* mix) {
    const int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x;
    if (i >= M * Nc) return;
    const int64_t k = i / Nc;
    const int j = (int)(i % Nc);
    const double w = table[k], iv = 1.0 / vars[i];
    double* o = mix + ((int64_t)j * M + k) * 3;
    o[0] = w > 0.0 ? log(w) + (-0.5 * 1.8378770664093453 + 0.5 * log(iv)) : -__builtin_huge_val();
    o[1] = means[i];
    o[2] = iv;
}

// running log-sum-exp with first and second derivative sums: f = sum e^t, (mx, s0, s1, s2) = (max t, sum e^(t - mx),
// sum e^(t - mx) a, sum e^(t - mx) (a^2 - 1/var)) with a = d t / d x
struct Acc {
    double mx, s0, s1, s2;
};
__device__ __forceinline__ Acc acc_merge(const Acc& p, const Acc& q) {
    if (q.mx == -__builtin_huge_val()) return p;
    if (p.mx == -__builtin_huge_val()) return q;
    const double mx = fmax(p.mx, q.mx), ep = exp(p.mx - mx), eq = exp(q.mx - mx);
    return Acc{mx, p.s0 * ep + q.s0 * eq, p.s1 * ep + q.s1 * eq, p.s2 * ep + q.s2 * eq};
}

// the mixture of variable j at x, by the whole workgroup (fixed order: thread-strided components, then a tree);
// res = (log f, (log f)', (log f)'')
__device__ __forceinline__ void mix_eval(const double* __restrict__ mj, int64_t M, double x, Acc* sh, double res[3]) {
    Acc a{-__builtin_huge_val(), 0.0, 0.0, 0.0};
    for (int64_t k = threadIdx.x; k < M; k += RB) {
        const double c0 = mj[3 * k], d = mj[3 * k + 1] - x, iv = mj[3 * k + 2];
        const double g = d * iv, t = c0 - 0.5 * d * g;
        if (t == -__builtin_huge_val()) continue;
        if (t > a.mx) {
            const double r = exp(a.mx - t);
            a = Acc{t, a.s0 * r, a.s1 * r, a.s2 * r};
        }
        const double e = exp(t - a.mx);
        a.s0 += e;
        a.s1 += e * g;
        a.s2 += e * (g * g - iv);
    }
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int s = RB / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = acc_merge(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    a = sh[0];
    __syncthreads();
    const double g = a.s1 / a.s0;
    res[0] = a.mx + log(a.s0);
    res[1] = g;
    res[2] = a.s2 / a.s0 - g * g;
}

// x [Nc][npts], out [Nc][npts][3]; workgroup (tile of MIX_PTS points, variable)
__global__ void __launch_bounds__(RB) exact_mixture_kernel(int64_t M, const double* __restrict__ mix, int npts,
                                                           const double* __restrict__ x, double* out) {
    __shared__ Acc sh[RB];
    const int j = blockIdx.y;
    const double* mj = mix + (int64_t)j * M * 3;
    for (int p = blockIdx.x * MIX_PTS; p < npts && p < (int)(blockIdx.x + 1) * MIX_PTS; ++p) {
        double res[3];
        mix_eval(mj, M, x[(int64_t)j * npts + p], sh, res);
        if (threadIdx.x < 3) out[((int64_t)j * npts + p) * 3 + threadIdx.x] = res[threadIdx.x];
    }
}

// Newton on log f from x [Nc][S], each start by one workgroup: step -g/h where h < 0 (else a gradient step scaled by the
// smallest component variance), clipped to [lo, hi], halved while it lowers log f; stops when the step is below
// 1e-14 max(1, |x|).  x: in / out; out_logf [Nc][S]: log f at the result.
__global__ void __launch_bounds__(RB) exact_polish_kernel(int64_t M, const double* __restrict__ mix, int S, double* x,
                                                          const double* __restrict__ lo, const double* __restrict__ hi,
                                                          const double* __restrict__ vmin, int max_iter, double* out_logf) {
    __shared__ Acc sh[RB];
    const int j = blockIdx.y, s = blockIdx.x;
    const double* mj = mix + (int64_t)j * M * 3;
    const double a = lo[j], b = hi[j];
    double cur = fmin(fmax(x[(int64_t)j * S + s], a), b), res[3];
    mix_eval(mj, M, cur, sh, res);
    double f = res[0], g = res[1], h = res[2];
    for (int it = 0; it < max_iter; ++it) {
        double step = h < 0.0 ? -g / h : g * vmin[j];
        bool moved = false;
        for (int half = 0; half < 40; ++half) {
            const double cand = fmin(fmax(cur + step, a), b);
            if (cand == cur) break;
            mix_eval(mj, M, cand, sh, res);
            if (res[0] >= f) {
                moved = fabs(cand - cur) > 1e-14 * fmax(1.0, fabs(cur));
                cur = cand, f = res[0], g = res[1], h = res[2];
                break;
            }
            step *= 0.5;
        }
        if (!moved) break;
    }
    if (threadIdx.x == 0) {
        x[(int64_t)j * S + s] = cur;
        out_logf[(int64_t)j * S + s] = f;
    }
}

static int model_check(const lhvi_exact_t* m) {
    if (!m || m->Nd < 0 || m->Nc < 0 || m->M < 1 || m->n_quad < 0 || m->n_tab < 0) return LHVI_E_ARG;
    if (m->Nd && (!m->dstates || !m->dstride)) return LHVI_E_ARG;
    if (m->n_quad && (!m->quad_ptr || !m->quad_desc || !m->quad_par)) return LHVI_E_ARG;
    if (m->n_tab && (!m->tab_ptr || !m->tab_desc || !m->tab_par)) return LHVI_E_ARG;
    if (m->Nc > LHVI_EXACT_MAX_NC) return LHVI_E_UNSUPPORTED;
    return LHVI_OK;
}

}  // namespace exact
}  // namespace lhvi

using namespace lhvi;
using namespace lhvi::exact;

extern "C" {

size_t lhvi_exact_lds_bytes(int32_t Nc, int32_t Nd, int32_t lanes) {
    if (Nc < 0 || Nd < 0 || !hg::lanes_ok(lanes)) return 0;
    return hg::wave_lds_bytes(lanes, ws_doubles(Nc, Nd));
}

int lhvi_exact_configs(const lhvi_exact_t* m, int64_t cfg_begin, int64_t cfg_count, int32_t lanes, double* logp, double* means,
                       double* vars, double* covs, uint64_t* bad, void* stream) {
    int rc = model_check(m);
    if (rc) return rc;
    if (cfg_begin < 0 || cfg_count < 0 || cfg_begin + cfg_count > m->M || !logp || !means || !vars || !bad) return LHVI_E_ARG;
    if (!hg::lanes_ok(lanes)) return LHVI_E_ARG;
    hg::WaveShape sh;
    rc = hg::wave_shape(cfg_count, lanes, ws_doubles(m->Nc, m->Nd), sh);
    if (rc || !cfg_count) return rc;
    hipLaunchKernelGGL(exact_config_kernel, dim3((unsigned)sh.blocks), dim3(WAVE), sh.lds, as_stream(stream), *m, cfg_begin, cfg_count,
                       (int)lanes, logp, means, vars, covs, reinterpret_cast<unsigned long long*>(bad));
    return check_launch();
}

int lhvi_exact_normalize(int64_t M, const double* logp, double* table, double* logZ, double* ws, void* stream) {
    if (M < 1 || !logp || !table || !logZ || !ws) return LHVI_E_ARG;
    const int parts = (int)(M < (int64_t)PARTS * RB ? (M + RB - 1) / RB : PARTS);
    hipStream_t st = as_stream(stream);
    double *part = ws, *mx = ws + PARTS;
    hipLaunchKernelGGL(exact_partial_kernel<false>, dim3(parts), dim3(RB), 0, st, M, logp, (const double*)nullptr, part);
    hipLaunchKernelGGL(exact_final_kernel<false>, dim3(1), dim3(RB), 0, st, parts, part, (const double*)nullptr, mx);
    hipLaunchKernelGGL(exact_partial_kernel<true>, dim3(parts), dim3(RB), 0, st, M, logp, (const double*)mx, part);
    hipLaunchKernelGGL(exact_final_kernel<true>, dim3(1), dim3(RB), 0, st, parts, part, (const double*)mx, logZ);
    hipLaunchKernelGGL(exact_table_kernel, dim3(grid_for(M, RB)), dim3(RB), 0, st, M, logp, (const double*)logZ, table);
    return check_launch();
}

int lhvi_exact_marginals(const lhvi_exact_t* m, int32_t n_states, const double* table, double* marg, void* stream) {
    const int rc = model_check(m);
    if (rc) return rc;
    if (n_states < 0) return LHVI_E_ARG;
    if (n_states == 0) return LHVI_OK;
    if (!table || !marg) return LHVI_E_ARG;
    hipLaunchKernelGGL(exact_marginal_kernel, dim3(n_states), dim3(RB), 0, as_stream(stream), *m, table, marg);
    return check_launch();
}

int lhvi_exact_mix_prepare(int32_t Nc, int64_t M, const double* table, const double* means, const double* vars, double* mix,
                           void* stream) {
    if (Nc < 1 || M < 1 || !table || !means || !vars || !mix) return LHVI_E_ARG;
    hipLaunchKernelGGL(exact_mix_prepare_kernel, dim3(grid_for(M * Nc, RB)), dim3(RB), 0, as_stream(stream), (int)Nc, M, table,
                       means, vars, mix);
    return check_launch();
}

int lhvi_exact_mixture(int32_t Nc, int64_t M, const double* mix, int32_t npts, const double* x, double* out, void* stream) {
    if (Nc < 1 || Nc > 65535 || M < 1 || npts < 0 || !mix || !x || !out) return LHVI_E_ARG;
    if (npts == 0) return LHVI_OK;
    hipLaunchKernelGGL(exact_mixture_kernel, dim3((npts + MIX_PTS - 1) / MIX_PTS, Nc), dim3(RB), 0, as_stream(stream), M, mix,
                       (int)npts, x, out);
    return check_launch();
}

int lhvi_exact_map_polish(int32_t Nc, int64_t M, const double* mix, int32_t S, double* x, const double* lo, const double* hi,
                          const double* vmin, int32_t max_iter, double* out_logf, void* stream) {
    if (Nc < 1 || Nc > 65535 || M < 1 || S < 1 || max_iter < 0 || !mix || !x || !lo || !hi || !vmin || !out_logf) return LHVI_E_ARG;
    hipLaunchKernelGGL(exact_polish_kernel, dim3(S, Nc), dim3(RB), 0, as_stream(stream), M, mix, (int)S, x, lo, hi, vmin,
                       (int)max_iter, out_logf);
    return check_launch();
}

int lhvi_exact_config_host(const lhvi_exact_t* m, int64_t cfg, double* logp, double* mean, double* var, double* cov) {
    const int rc = model_check(m);
    if (rc) return rc;
    if (cfg < 0 || cfg >= m->M) return LHVI_E_ARG;
    double* W = new double[ws_doubles(m->Nc, m->Nd) + 2];
    const int bad = config(*m, cfg, W, HostCtx(), logp, mean, var, cov);
    delete[] W;
    return bad ? LHVI_E_NOT_PD : LHVI_OK;
}

}  // extern "C"
