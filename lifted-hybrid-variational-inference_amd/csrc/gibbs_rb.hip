// gibbs_rb.hip -- Rao-Blackwellised marginals of the block Gibbs sampler (docs/kernels_gibbs_rb.md), gfx950.
//   exact_config_at_kernel   the conditional Gaussian of one row of explicit discrete digits per group of `lanes` lanes of a
//                            one-wavefront workgroup: exact_config_kernel (csrc/exact.hip) with the row in the place of the
//                            digit decode, the same workspace in LDS, the same code after it (exact::config_at)
//   gibbs_rb_disc_kernel     kept samples [s_begin, s_end) of one chain per group of lanes: the reduced tables at the sample's
//                            x_c, every variable's conditional probabilities at the sample's other digits, added to the chain's
//                            row in sample order; the workspace and the place of the reduced tables of gibbs_chain_kernel
#include "common.hpp"
#include "gibbs_rb.hpp"
#include "hg_launch.hpp"

namespace lhvi {
namespace gibbs_rb {

using hg::DevCtx;
using hg::lds_disc_doubles;
using hg::lanes_ok;

__global__ void __launch_bounds__(WAVE) exact_config_at_kernel(lhvi_exact_t m, int64_t S, const int32_t* __restrict__ x_d, int lanes,
                                                               double* logp, double* means, double* vars,
                                                               unsigned long long* bad) {
    extern __shared__ double lds[];
    const int gpb = WAVE / lanes, grp = threadIdx.x / lanes;
    const int64_t idx = (int64_t)blockIdx.x * gpb + grp;
    const bool valid = idx < S;
    const int64_t row = valid ? idx : S - 1;                    // a padding group repeats the last row, stores nothing
    const int ws = (exact::ws_doubles(m.Nc, m.Nd) + 1) & ~1;
    DevCtx ctx{(int)threadIdx.x % lanes, lanes};
    const int rc = config_at(m, x_d + row * m.Nd, lds + grp * ws, ctx, valid && logp ? logp + row : nullptr,
                             valid ? means + row * m.Nc : nullptr, valid ? vars + row * m.Nc : nullptr);
    if (rc && valid && ctx.lane == 0) atomicMin(bad, (unsigned long long)row);
}

__global__ void __launch_bounds__(WAVE) gibbs_rb_disc_kernel(lhvi_gibbs_t g, int64_t chains, int s_begin, int s_end, int lanes,
                                                             const int32_t* __restrict__ disc, const double* __restrict__ cont,
                                                             double* prob_sum) {
    extern __shared__ double lds[];
    const int Nc = g.ex.Nc, Nd = g.ex.Nd;
    const int gpb = WAVE / lanes, grp = threadIdx.x / lanes;
    const int64_t idx = (int64_t)blockIdx.x * gpb + grp;
    const bool valid = idx < chains;
    const int64_t chain = valid ? idx : chains - 1;             // a padding group repeats the last chain, stores nothing
    const int ws = (gibbs::ws_doubles(Nc, Nd, lds_disc_doubles(g)) + 1) & ~1;
    DevCtx ctx{(int)threadIdx.x % lanes, lanes};
    // a padding group has a scratch row of its own (rows are allocated for a multiple of 64 chains)
    const gibbs::Workspace w = gibbs::layout(g, lds + grp * ws, g.table_scratch ? g.table_scratch + idx * g.table_doubles : nullptr);
    const int n_states = Nd ? g.dstate_off[Nd] : 0;
    disc_probs(g, s_begin, s_end, disc + chain * g.num_samples * Nd, cont + chain * g.num_samples * Nc, w, ctx,
               valid ? prob_sum + chain * n_states : nullptr);
}

}  // namespace gibbs_rb
}  // namespace lhvi

using namespace lhvi;
using namespace lhvi::gibbs_rb;

extern "C" {

int lhvi_exact_configs_at(const lhvi_exact_t* m, int64_t S, const int32_t* x_d, int32_t lanes, double* logp, double* means,
                          double* vars, uint64_t* bad, void* stream) {
    int rc = hg::exact_check(m);
    if (rc) return rc;
    if (S < 0 || !means || !vars || !bad || (m->Nd && S && !x_d) || !lanes_ok(lanes)) return LHVI_E_ARG;
    hg::WaveShape sh;
    rc = hg::wave_shape(S, lanes, exact::ws_doubles(m->Nc, m->Nd), sh);
    if (rc || !S) return rc;
    hipLaunchKernelGGL(exact_config_at_kernel, dim3((unsigned)sh.blocks), dim3(WAVE), sh.lds, as_stream(stream), *m, S, x_d, (int)lanes,
                       logp, means, vars, reinterpret_cast<unsigned long long*>(bad));
    return check_launch();
}

int lhvi_exact_config_at_host(const lhvi_exact_t* m, const int32_t* x_d_row, double* logp, double* mean, double* var) {
    const int rc = hg::exact_check(m);
    if (rc) return rc;
    if (m->Nd && !x_d_row) return LHVI_E_ARG;
    for (int n = 0; n < m->Nd; ++n)
        if (x_d_row[n] < 0 || x_d_row[n] >= m->dstates[n]) return LHVI_E_ARG;
    double* W = new double[exact::ws_doubles(m->Nc, m->Nd) + 2];
    const int bad = config_at(*m, x_d_row, W, exact::HostCtx(), logp, mean, var);
    delete[] W;
    return bad ? LHVI_E_NOT_PD : LHVI_OK;
}

int lhvi_gibbs_rb_disc(const lhvi_gibbs_t* m, int64_t chains, int32_t s_begin, int32_t s_end, int32_t lanes, const int32_t* disc,
                       const double* cont, double* prob_sum, void* stream) {
    int rc = hg::gibbs_check(m, hg::SAMPLES);        // what lhvi_gibbs_run asks of the fields this reads
    if (rc) return rc;
    if (chains < 0 || chains > 0xffffffffLL || s_begin < 0 || s_end < s_begin || s_end > m->num_samples || !lanes_ok(lanes))
        return LHVI_E_ARG;
    const int Nc = m->ex.Nc, Nd = m->ex.Nd;
    const int64_t work = s_end == s_begin || Nd == 0 ? 0 : chains;
    hg::WaveShape sh;
    rc = hg::wave_shape(work, lanes, gibbs::ws_doubles(Nc, Nd, lds_disc_doubles(*m)), sh);
    if (rc || !work) return rc;
    if (!disc || !prob_sum || (Nc && !cont)) return LHVI_E_ARG;
    hipLaunchKernelGGL(gibbs_rb_disc_kernel, dim3((unsigned)sh.blocks), dim3(WAVE), sh.lds, as_stream(stream), *m, chains, (int)s_begin,
                       (int)s_end, (int)lanes, disc, cont, prob_sum);
    return check_launch();
}

int lhvi_gibbs_rb_disc_host(const lhvi_gibbs_t* m, int32_t s_begin, int32_t s_end, const int32_t* disc, const double* cont,
                            double* prob_sum) {
    const int rc = hg::gibbs_check(m, hg::SAMPLES);
    if (rc) return rc;
    const int Nc = m->ex.Nc, Nd = m->ex.Nd;
    if (s_begin < 0 || s_end < s_begin || s_end > m->num_samples) return LHVI_E_ARG;
    if (s_end == s_begin || Nd == 0) return LHVI_OK;
    if (!disc || !prob_sum || (Nc && !cont)) return LHVI_E_ARG;
    for (int s = s_begin; s < s_end; ++s)
        for (int n = 0; n < Nd; ++n)
            if (disc[(int64_t)s * Nd + n] < 0 || disc[(int64_t)s * Nd + n] >= m->ex.dstates[n]) return LHVI_E_ARG;
    hg::HostWork hw(*m);
    disc_probs(hw.g, s_begin, s_end, disc, cont, gibbs::layout(hw.g, hw.alloc(gibbs::ws_doubles(Nc, Nd, hw.dd) + 2), nullptr),
               exact::HostCtx(), prob_sum);
    return LHVI_OK;
}

}  // extern "C"
