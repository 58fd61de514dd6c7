// gibbs_rb.hpp -- Rao-Blackwellised marginals of the block Gibbs sampler, written once for the device (csrc/gibbs_rb.hip: a group
// of lanes per row of digits / per chain) and the host (lhvi_exact_config_at_host, lhvi_gibbs_rb_disc_host: one "lane").  Same
// style as exact.hpp and gibbs.hpp, whose code this calls: exact::config_at is the conditional Gaussian of a row of digits, and
// gibbs::reduced_tables / gibbs::cond_lprobs are the sampler's own step 2 and log probabilities.  Every value is produced by ONE
// lane with a serial loop in a fixed order; all control flow around a ctx.sync() depends on the model and the range of samples
// alone.
#pragma once
#include "gibbs.hpp"

namespace lhvi {
namespace gibbs_rb {

// The conditional Gaussian of the row of digits x_d [Nd]: the lanes copy the digits into the workspace where exact::config
// decodes them, then run its code.  Returns 1 when J is not positive definite, the same value in every lane.
template <class Ctx>
LHVI_HD int config_at(const lhvi_exact_t& m, const int32_t* x_d, double* W, const Ctx& ctx, double* logp, double* mean,
                      double* var) {
    int32_t* dig = exact::digits(m.Nc, W);
    for (int d = ctx.lane; d < m.Nd; d += ctx.lanes) dig[d] = x_d[d];
    return exact::config_at(m, W, ctx, logp, mean, var, static_cast<double*>(nullptr));
}

// The kept samples [s_begin, s_end) of one chain (disc [num_samples][Nd], cont [num_samples][Nc]: the chain's rows):
// prob_sum [sum dstates] += p(x_n = k | x_d,-n, x_c) of every variable n at every sample, in sample order, state k by the lane
// that owns it.  prob_sum null (a padding group): the same work and barriers, nothing stored.  w: the sampler's workspace, of
// which x_c, lprobs, the reduced tables and the digits are used.
template <class Ctx>
LHVI_HD void disc_probs(const lhvi_gibbs_t& g, int s_begin, int s_end, const int32_t* disc, const double* cont,
                        const gibbs::Workspace& w, const Ctx& ctx, double* prob_sum) {
    const lhvi_exact_t& m = g.ex;
    const int Nc = m.Nc, Nd = m.Nd;
    for (int s = s_begin; s < s_end; ++s) {
        for (int r = ctx.lane; r < Nc; r += ctx.lanes) w.xc[r] = cont[(int64_t)s * Nc + r];
        for (int n = ctx.lane; n < Nd; n += ctx.lanes) w.dig[n] = disc[(int64_t)s * Nd + n];
        ctx.sync();
        gibbs::reduced_tables(g, w.xc, w.tab, ctx);
        ctx.sync();
        for (int n = 0; n < Nd; ++n) {
            const int d = m.dstates[n];
            gibbs::cond_lprobs(g, n, w.dig, w.tab, w.lprobs, ctx);
            ctx.sync();
            // the sampler's softmax (gibbs::iteration step 3): max and sum by every lane with the same bits
            double mx = -__builtin_huge_val(), sum = 0.0;
            for (int j = 0; j < d; ++j)
                if (w.lprobs[j] > mx) mx = w.lprobs[j];
            for (int j = 0; j < d; ++j) sum += exp(w.lprobs[j] - mx);
            const double scale = mx + log(sum);
            if (prob_sum)
                for (int j = ctx.lane; j < d; j += ctx.lanes) prob_sum[g.dstate_off[n] + j] += exp(w.lprobs[j] - scale);
            ctx.sync();                              // lprobs is the next variable's, x_c and the digits the next sample's
        }
    }
}

}  // namespace gibbs_rb
}  // namespace lhvi
