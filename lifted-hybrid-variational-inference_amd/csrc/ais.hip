// ais.hip -- annealed importance sampling for log Z of a hybrid Gaussian MRF (docs/kernels_ais.md), gfx950.
//   ais_chain_kernel     steps [t_begin, t_end) of one annealing run per group of `lanes` lanes of a one-wavefront workgroup;
//                        the chain's workspace in LDS (csrc/ais.hpp: the Gibbs kernel's plus mu0), its state (x_d, log weight)
//                        in the caller's arrays between launches
//   ais_max_* / ais_sum_*    the reduction over the chains' log weights: a max pass, then sums in a fixed order (two stages, no
//                        floating-point atomics: the same bits on every run)
#include "common.hpp"
#include "ais.hpp"
#include "hg_launch.hpp"

namespace lhvi {
namespace ais {

constexpr int RB = 256;            // workgroup of the reductions
constexpr int PARTS = 1024;        // partial results of the two-stage reductions
constexpr int SUMS = 6;            // sums of the second pass

using hg::DevCtx;
using hg::lds_disc_doubles;

__global__ void __launch_bounds__(WAVE) ais_chain_kernel(lhvi_gibbs_t g, int64_t chains, int T, const double* __restrict__ betas,
                                                         int t_begin, int t_end, int lanes, double tau0,
                                                         const double* __restrict__ mu0, int32_t* x_d, double* logw,
                                                         const double* z, const double* u, unsigned long long* bad) {
    extern __shared__ double lds[];
    const int Nc = g.ex.Nc, Nd = g.ex.Nd;
    const int gpb = WAVE / lanes, grp = threadIdx.x / lanes;
    const int64_t idx = (int64_t)blockIdx.x * gpb + grp;
    const bool valid = idx < chains;
    const int64_t chain = valid ? idx : chains - 1;             // a padding group repeats the last chain, stores nothing
    const int dd = lds_disc_doubles(g);
    const int ws = (ws_doubles(Nc, Nd, dd) + 1) & ~1;
    DevCtx ctx{(int)threadIdx.x % lanes, lanes};
    // a padding group has a scratch row of its own (rows are allocated for a multiple of 64 chains)
    const gibbs::Workspace w = gibbs::layout(g, lds + grp * ws, g.table_scratch ? g.table_scratch + idx * g.table_doubles : nullptr);
    double* m0 = base_mean(Nc, Nd, dd, lds + grp * ws);
    for (int n = ctx.lane; n < Nd; n += lanes) w.dig[n] = x_d[chain * Nd + n];
    for (int r = ctx.lane; r < Nc; r += lanes) m0[r] = mu0[r];
    ctx.sync();
    gibbs::Draws dr{g.seed, z, u, chains, chain, Nc, Nd, g.disc_block_its};
    dr.tag_normal = TAG_NORMAL;
    dr.tag_uniform = TAG_UNIFORM;
    const Base base{tau0, m0};
    double lw = logw[chain];
    bool dead = !valid;
    for (int t = t_begin; t < t_end; ++t) {
        const bool was_dead = dead;
        const int rc = step(g, t, T, betas, base, dr, w, ctx, dead, lw);
        if (rc && !was_dead && ctx.lane == 0)
            atomicMin(bad, ((unsigned long long)chain << 32) | (unsigned long long)(unsigned)t);
    }
    if (valid) {
        for (int n = ctx.lane; n < Nd; n += lanes) x_d[chain * Nd + n] = w.dig[n];
        if (ctx.lane == 0) logw[chain] = lw;
    }
}

// ---- fixed-order reductions over the log weights ------------------------------------------------------------------------------
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

// pass 1, stage 1: part[b] = max over the b-th contiguous slice
__global__ void __launch_bounds__(RB) ais_max_partial_kernel(int64_t C, const double* __restrict__ lw, double* part) {
    __shared__ double sh[RB];
    const int64_t per = (C + gridDim.x - 1) / gridDim.x, lo = per * blockIdx.x, hi = lo + per < C ? lo + per : C;
    double acc = -__builtin_huge_val();
    for (int64_t i = lo + threadIdx.x; i < hi; i += RB) acc = fmax(acc, lw[i]);
    const double r = block_tree(acc, sh, MaxOp());
    if (threadIdx.x == 0) part[blockIdx.x] = r;
}

// pass 1, stage 2 (one workgroup)
__global__ void __launch_bounds__(RB) ais_max_final_kernel(int n, const double* __restrict__ part, double* mx) {
    __shared__ double sh[RB];
    double acc = -__builtin_huge_val();
    for (int i = threadIdx.x; i < n; i += RB) acc = fmax(acc, part[i]);
    const double r = block_tree(acc, sh, MaxOp());
    if (threadIdx.x == 0) mx[0] = r;
}

// the six terms of a chain with d = lw - max: exp(d), exp(2 d), lw, lw^2, d, d^2
__device__ __forceinline__ void terms(double lw, double mx, double (&v)[SUMS]) {
    const double d = lw - mx;
    v[0] = exp(d); v[1] = exp(2.0 * d); v[2] = lw; v[3] = lw * lw; v[4] = d; v[5] = d * d;
}

// pass 2, stage 1: part[k][b] = the k-th sum over the b-th contiguous slice
__global__ void __launch_bounds__(RB) ais_sum_partial_kernel(int64_t C, const double* __restrict__ lw, const double* mx, double* part) {
    __shared__ double sh[RB];
    const int64_t per = (C + gridDim.x - 1) / gridDim.x, lo = per * blockIdx.x, hi = lo + per < C ? lo + per : C;
    const double m = *mx;
    double acc[SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, v[SUMS];
    for (int64_t i = lo + threadIdx.x; i < hi; i += RB) {
        terms(lw[i], m, v);
        for (int k = 0; k < SUMS; ++k) acc[k] += v[k];
    }
    for (int k = 0; k < SUMS; ++k) {
        const double r = block_tree(acc[k], sh, SumOp());
        if (threadIdx.x == 0) part[k * PARTS + blockIdx.x] = r;
    }
}

// pass 2, stage 2 (one workgroup): out [LHVI_AIS_REDUCE_OUT]
__global__ void __launch_bounds__(RB) ais_sum_final_kernel(int n, const double* __restrict__ part, const double* mx, double* out) {
    __shared__ double sh[RB];
    double s[SUMS];
    for (int k = 0; k < SUMS; ++k) {
        double acc = 0.0;
        for (int i = threadIdx.x; i < n; i += RB) acc += part[k * PARTS + i];
        s[k] = block_tree(acc, sh, SumOp());
    }
    if (threadIdx.x == 0) {
        const double m = *mx;
        out[0] = m + log(s[0]);
        out[1] = 2.0 * m + log(s[1]);
        out[2] = s[2];
        out[3] = s[3];
        out[4] = m;
        out[5] = s[0];
        out[6] = s[1];
        out[7] = s[4];
        out[8] = s[5];
    }
}

static int run_check(const lhvi_gibbs_t* m, int32_t T, const double* betas, int32_t t_begin, int32_t t_end, double tau0,
                     const double* mu0, const int32_t* x_d, const double* logw) {
    if (T < 1 || !betas || t_begin < 0 || t_end < t_begin || t_end > T || !logw) return LHVI_E_ARG;
    if (!(tau0 > 0.0) || (m->ex.Nc && !mu0) || (m->ex.Nd && !x_d)) return LHVI_E_ARG;
    return LHVI_OK;
}

}  // namespace ais
}  // namespace lhvi

using namespace lhvi;
using namespace lhvi::ais;

extern "C" {

size_t lhvi_ais_lds_bytes(int32_t Nc, int32_t Nd, int32_t table_doubles, int32_t lanes) {
    if (Nc < 0 || Nd < 0 || table_doubles < 0 || !hg::lanes_ok(lanes)) return 0;
    return hg::wave_lds_bytes(lanes, ais::ws_doubles(Nc, Nd, table_doubles));
}

int lhvi_ais_run(const lhvi_gibbs_t* m, int64_t chains, int32_t T, const double* betas, int32_t t_begin, int32_t t_end,
                 int32_t lanes, double tau0, const double* mu0, int32_t* x_d, double* logw, const double* z, const double* u,
                 uint64_t* bad, void* stream) {
    int rc = hg::gibbs_check(m, hg::ITS);            // a run reads neither num_burnin nor num_samples
    if (rc) return rc;
    if (chains < 0 || chains > 0xffffffffLL || !bad) return LHVI_E_ARG;
    rc = run_check(m, T, betas, t_begin, t_end, tau0, mu0, x_d, logw);
    if (rc) return rc;
    if (!hg::lanes_ok(lanes)) return LHVI_E_ARG;
    const int64_t work = t_end == t_begin ? 0 : chains;
    hg::WaveShape sh;
    rc = hg::wave_shape(work, lanes, ais::ws_doubles(m->ex.Nc, m->ex.Nd, lds_disc_doubles(*m)), sh);
    if (rc || !work) return rc;
    hipLaunchKernelGGL(ais_chain_kernel, dim3((unsigned)sh.blocks), dim3(WAVE), sh.lds, as_stream(stream), *m, chains, (int)T, betas,
                       (int)t_begin, (int)t_end, (int)lanes, tau0, mu0, x_d, logw, z, u,
                       reinterpret_cast<unsigned long long*>(bad));
    return check_launch();
}

int lhvi_ais_reduce(int64_t chains, const double* logw, double* out, double* ws, void* stream) {
    if (chains < 1 || !logw || !out || !ws) return LHVI_E_ARG;
    const int parts = (int)(chains < (int64_t)PARTS * RB ? (chains + RB - 1) / RB : PARTS);
    hipStream_t st = as_stream(stream);
    double *part = ws, *mx = ws + SUMS * PARTS;
    hipLaunchKernelGGL(ais_max_partial_kernel, dim3(parts), dim3(RB), 0, st, chains, logw, part);
    hipLaunchKernelGGL(ais_max_final_kernel, dim3(1), dim3(RB), 0, st, parts, (const double*)part, mx);
    hipLaunchKernelGGL(ais_sum_partial_kernel, dim3(parts), dim3(RB), 0, st, chains, logw, (const double*)mx, part);
    hipLaunchKernelGGL(ais_sum_final_kernel, dim3(1), dim3(RB), 0, st, parts, (const double*)part, (const double*)mx, out);
    return check_launch();
}

int lhvi_ais_chain_host(const lhvi_gibbs_t* m, int64_t chain, int32_t T, const double* betas, int32_t t_begin, int32_t t_end,
                        double tau0, const double* mu0, int32_t* x_d, double* logw, const double* z, const double* u) {
    int rc = hg::gibbs_check(m, hg::ITS);
    if (rc) return rc;
    rc = run_check(m, T, betas, t_begin, t_end, tau0, mu0, x_d, logw);
    if (rc) return rc;
    const int Nc = m->ex.Nc, Nd = m->ex.Nd;
    if (chain < 0 || chain > 0xffffffffLL) return LHVI_E_ARG;
    const bool injected = z || u;
    if (injected && ((Nc && !z) || (Nd && m->disc_block_its && !u))) return LHVI_E_ARG;     // both streams, or neither
    hg::HostWork hw(*m);
    const lhvi_gibbs_t& g = hw.g;
    double* W = hw.alloc(ais::ws_doubles(Nc, Nd, hw.dd) + 2);
    const gibbs::Workspace w = gibbs::layout(g, W, nullptr);
    double* m0 = base_mean(Nc, Nd, hw.dd, W);
    hw.digits_in(w, x_d);
    for (int r = 0; r < Nc; ++r) m0[r] = mu0[r];
    // injected draws are this chain's rows (z [T][Nc], u [T][its][Nd]); the Philox stream is that of chain `chain`
    gibbs::Draws dr{g.seed, z, u, 1, 0, Nc, Nd, g.disc_block_its};
    if (!injected) dr.chain = chain;
    dr.tag_normal = TAG_NORMAL;
    dr.tag_uniform = TAG_UNIFORM;
    const Base base{tau0, m0};
    double lw = *logw;
    bool dead = false;
    for (int t = t_begin; t < t_end; ++t) step(g, t, T, betas, base, dr, w, exact::HostCtx(), dead, lw);
    hw.digits_out(w, x_d);
    *logw = lw;
    return dead ? LHVI_E_NOT_PD : LHVI_OK;
}

}  // extern "C"
