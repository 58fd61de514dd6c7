// ais.hpp -- one step of an annealed importance sampling chain (Neal 2001) for log Z of a hybrid Gaussian MRF, collapsed over
// x_c (docs/kernels_ais.md), written once for the device (csrc/ais.hip: a group of lanes per chain) and the host
// (lhvi_ais_chain_host: one "lane").  Same style as gibbs.hpp: loops over the rows a lane owns, ctx.sync() between phases, every
// value produced by ONE lane with a serial loop in a fixed order, so a chain's log weight and x_d depend neither on the number
// of lanes, nor on the chains of the launch, nor on the split of the steps over launches.  All control flow around a ctx.sync()
// depends on the model and the schedule alone.
//
// Path: f_beta = p~^beta f0^(1 - beta) with the base f0(x_d, x_c) = exp(-tau0 / 2 |x_c - mu0|^2), x_d uniform.  Given x_d
//   J_beta = beta J + (1 - beta) tau0 I,  b_beta = beta b + (1 - beta) tau0 mu0,  c_beta = beta c - (1 - beta) tau0 / 2 |mu0|^2
// and the collapsed mass is
//   log m_beta(x_d) = beta tables + c_beta + Nc / 2 log 2 pi - 1/2 log det J_beta + 1/2 |L_beta^-1 b_beta|^2.
// Step t adds log m_{beta_t+1}(x_d) - log m_{beta_t}(x_d) to the log weight, then (unless it is the last) makes one block
// Gibbs transition at beta_t+1 from the factor just computed.
//
// Workspace of a chain (doubles): that of gibbs.hpp (lprobs, the reduced tables when they live in LDS, the digits), then mu0 [Nc].
#pragma once
#include "gibbs.hpp"

namespace lhvi {
namespace ais {

// the fourth Philox counter word: "AISZ" normals, "AISU" uniforms; counter (chain, step, draw index, tag)
constexpr uint32_t TAG_NORMAL = 0x4149535au, TAG_UNIFORM = 0x41495355u;

struct Base {
    double tau0;
    const double* mu0;      // [Nc]
};

LHVI_HD int ws_doubles(int Nc, int Nd, int disc_doubles) { return gibbs::ws_doubles(Nc, Nd, disc_doubles) + Nc; }
// mu0 of the workspace W
LHVI_HD double* base_mean(int Nc, int Nd, int disc_doubles, double* W) { return W + gibbs::ws_doubles(Nc, Nd, disc_doubles); }

// temper: the joint A, b, c of exact::assemble become those of f_beta, a lane scaling the rows it owns:
// A_beta = beta A - (1 - beta) tau0 / 2 I (so that form_J gives J_beta), b_beta, c_beta.  beta = 1 leaves every value as it is
// (a product with 1, a sum with 0).  The caller syncs before (assemble's rows are complete) and after.
template <class Ctx>
LHVI_HD void temper(int Nc, double beta, const Base& base, double* mat, double* b, const Ctx& ctx, double& c) {
    const int ld = exact::ld_of(Nc);
    const double g = (1.0 - beta) * base.tau0;
    for (int r = ctx.lane; r < Nc; r += ctx.lanes) {
        for (int j = 0; j < Nc; ++j) mat[r * ld + j] *= beta;
        mat[r * ld + r] -= 0.5 * g;
        b[r] = beta * b[r] + g * base.mu0[r];
    }
    double mm = 0.0;
    for (int i = 0; i < Nc; ++i) mm += base.mu0[i] * base.mu0[i];
    c = beta * c - 0.5 * g * mm;
}

// collapsed_mass: log m_beta of the digits in w.dig; leaves L_beta (w.mat, w.ldiag, w.dinv) and y = L_beta^-1 b_beta (w.y) for
// the transition.  Returns 1 when J_beta is not positive definite, the same value in every lane; logm has the same bits in
// every lane.
template <class Ctx>
LHVI_HD int collapsed_mass(const lhvi_gibbs_t& g, double beta, const Base& base, const gibbs::Workspace& w, const Ctx& ctx,
                           double& logm) {
    const lhvi_exact_t& m = g.ex;
    const int Nc = m.Nc;
    double c = 0.0, logdet = 0.0, yy = 0.0;
    int bad = 0;
    const double ts = exact::table_sum(m, w.dig);
    if (Nc) {
        exact::assemble(m, w.dig, w.mat, w.b, ctx, c);
        ctx.sync();
        temper(Nc, beta, base, w.mat, w.b, ctx, c);
        ctx.sync();
        exact::form_J(Nc, w.mat, ctx);
        bad = exact::cholesky(Nc, w.mat, w.ldiag, w.dinv, ctx, logdet);
        gibbs::forward_solve(Nc, w, ctx);
        for (int i = 0; i < Nc; ++i) yy += w.y[i] * w.y[i];
    }
    double t = (double)Nc / 2 * 1.8378770664093453 + 0.5 * -logdet + 0.5 * yy;
    t += c;
    logm = beta * ts + t;
    return bad;
}

// transition: one block Gibbs iteration at beta from the factor collapsed_mass left: x_c = L^-T (y + z), the reduced tables at
// x_c, then disc_block_its sweeps of gibbs::iteration's categorical rule on beta * lprobs (the base's share of the exponent does
// not depend on x_d).  At beta = 1 the operations are gibbs::iteration's.
template <class Ctx>
LHVI_HD void transition(const lhvi_gibbs_t& g, int t, double beta, const gibbs::Draws& dr, const gibbs::Workspace& w,
                        const Ctx& ctx, bool dead) {
    const lhvi_exact_t& m = g.ex;
    const int Nc = m.Nc, Nd = m.Nd;
    if (Nc) gibbs::back_solve(Nc, t, dr, w, ctx);
    gibbs::reduced_tables(g, w.xc, w.tab, ctx);
    ctx.sync();
    for (int sweep = 0; sweep < g.disc_block_its; ++sweep)
        for (int n = 0; n < Nd; ++n) {
            const int d = m.dstates[n];
            gibbs::cond_lprobs(g, n, w.dig, w.tab, w.lprobs, ctx);
            ctx.sync();
            double mx = -__builtin_huge_val(), sum = 0.0;
            for (int j = 0; j < d; ++j)
                if (beta * w.lprobs[j] > mx) mx = beta * w.lprobs[j];
            for (int j = 0; j < d; ++j) sum += exp(beta * w.lprobs[j] - mx);
            const double scale = mx + log(sum), u = dr.uniform(t, sweep * Nd + n);
            double cum = 0.0;
            int pick = d - 1;
            for (int j = 0; j < d; ++j) {
                cum += exp(beta * w.lprobs[j] - scale);
                if (u <= cum) { pick = j; break; }
            }
            if (ctx.lane == 0 && !dead) w.dig[n] = pick;  // no lane reads the digits between the two barriers
            ctx.sync();
        }
}

// Step t of T of a chain whose x_d is in w.dig.  dead: the chain met a J_beta that is not positive definite; it keeps its x_d
// and its log weight from then on.  Returns 1 when one of this step's two factorisations fails (and sets dead), the same value
// in every lane.
template <class Ctx>
LHVI_HD int step(const lhvi_gibbs_t& g, int t, int T, const double* betas, const Base& base, const gibbs::Draws& dr,
                 const gibbs::Workspace& w, const Ctx& ctx, bool& dead, double& logw) {
    double lm0, lm1;
    int bad = collapsed_mass(g, betas[t], base, w, ctx, lm0);
    bad |= collapsed_mass(g, betas[t + 1], base, w, ctx, lm1);
    dead = dead || bad;
    if (!dead) logw += lm1 - lm0;
    if (t + 1 < T) transition(g, t, betas[t + 1], dr, w, ctx, dead);
    return bad;
}

}  // namespace ais
}  // namespace lhvi
