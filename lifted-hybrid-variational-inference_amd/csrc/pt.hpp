// pt.hpp -- parallel tempering (replica exchange) for the block Gibbs sampler of a hybrid Gaussian MRF (docs/kernels_pt.md),
// written once for the device (csrc/pt.hip: a group of lanes per replica, a ladder per workgroup or part of one) and the host
// (lhvi_pt_ladder_host: one "lane", the replicas in order).  Same style as gibbs.hpp / ais.hpp: loops over the rows a lane owns,
// every value produced by ONE lane with a serial loop in a fixed order, so a ladder's samples, accumulators and swap counters
// depend neither on the number of lanes, nor on how ladders are packed into workgroups, nor on the ladders of the launch, nor
// on the split of the iterations over launches.  All control flow around a ctx.sync() depends on the model and the schedule
// alone: an unpaired replica and a dead ladder do the work of a live pair and drop the result.
//
// A ladder is R replicas at betas[0] <= ... <= betas[R - 1] = 1 on the path of ais.hpp; replica r always sits at betas[r] and
// swaps exchange the digits.  Iteration `it` of a replica is
//   1. factor():           ais::collapsed_mass at its own beta (leaves L_beta and y), its pivot flag posted to the ladder's slots
//      (barrier)           ladder_bad(): a failed pivot anywhere kills the whole ladder
//      ais::transition     one block Gibbs iteration at beta
//   2. record()            replica R - 1, from iteration num_burnin on: the stores and sums of gibbs::iteration's step 4
//   3. when (it + 1) % swap_every == 0, swap round s = it / swap_every, pairs (r, r + 1) with r = s mod 2, s mod 2 + 2, ...:
//      swap_masses():      log m of its own digits at its own beta and at its partner's, posted to the slots
//      (barrier)           ladder_bad()
//      log_ratio(), accept(), exchange() by the lanes of the pair's lower replica, the counters by its lane 0
//      (barrier)
// The callers (pt_ladder_kernel, lhvi_pt_ladder_host) make this sequence from the pieces below; between two writes of a slot and
// between a write and its reads lies at least one barrier of the whole workgroup.
//
// Workspace of a ladder (doubles): R chain workspaces of ais.hpp, each rounded up to an even count, then the slots:
// lm [R][2] (own beta, partner's beta), then R int32 pivot flags.
#pragma once
#include "ais.hpp"

namespace lhvi {
namespace pt {

// the fourth Philox counter word: "PTNZ" normals, "PTUF" sweep uniforms (counter (ladder * R + r, iteration, draw index, tag)),
// "PTSW" the swap uniform of a pair (counter (ladder, iteration, lower replica, tag), its first uniform)
constexpr uint32_t TAG_NORMAL = 0x50544e5au, TAG_UNIFORM = 0x50545546u, TAG_SWAP = 0x50545357u;

LHVI_HD int chain_doubles(int Nc, int Nd, int disc_doubles) { return (ais::ws_doubles(Nc, Nd, disc_doubles) + 1) & ~1; }
LHVI_HD int slot_doubles(int R) { return (2 * R + (R + 1) / 2 + 1) & ~1; }
LHVI_HD int ws_doubles(int Nc, int Nd, int disc_doubles, int R) { return R * chain_doubles(Nc, Nd, disc_doubles) + slot_doubles(R); }

struct Slots {
    double* lm;         // [R][2]: log m of replica r's digits at betas[r], at its partner's beta
    int32_t* bad;       // [R]: the replica's last factorisations met a pivot <= 0
};
// the slots of the ladder whose workspace begins at W
LHVI_HD Slots slots(int Nc, int Nd, int disc_doubles, int R, double* W) {
    double* s = W + R * chain_doubles(Nc, Nd, disc_doubles);
    return Slots{s, reinterpret_cast<int32_t*>(s + 2 * R)};
}

// the swap uniform of pair `pair` (its lower replica) at iteration it: injected (usw [iters][ladders][max(R - 1, 1)]) or Philox
struct SwapDraws {
    uint64_t seed;
    const double* usw;
    int64_t ladders, ladder;
    int width;
    LHVI_HD double uniform(int it, int pair) const {
        if (usw) return usw[((int64_t)it * ladders + ladder) * width + pair];
        double u0, u1;
        gibbs::uniform2(seed, (uint32_t)ladder, (uint32_t)it, (uint32_t)pair, TAG_SWAP, u0, u1);
        return u0;
    }
};

// the lower replica of r's pair in swap round s, or -1 when r has no partner in this round
LHVI_HD int pair_of(int R, int s, int r) {
    const int par = s & 1;
    if (r < par) return -1;
    const int lo = r - ((r - par) & 1);
    return lo + 1 < R ? lo : -1;
}

// 1. the factor of the transition: L_beta and y of the replica's digits in its workspace, its pivot flag in the slots.  The caller
// syncs, then reads ladder_bad().
template <class Ctx>
LHVI_HD void factor(const lhvi_gibbs_t& g, double beta, const ais::Base& base, const gibbs::Workspace& w, const Ctx& ctx,
                    const Slots& sl, int r) {
    double lm;
    const int bad = ais::collapsed_mass(g, beta, base, w, ctx, lm);
    if (ctx.lane == 0) sl.bad[r] = bad;
}

// a pivot failed in some replica of the ladder: the same value in every lane of the ladder
LHVI_HD int ladder_bad(const Slots& sl, int R) {
    int bad = 0;
    for (int r = 0; r < R; ++r) bad |= sl.bad[r];
    return bad;
}

// 2. kept sample s of the beta = 1 replica and the ladder's accumulators: the stores and sums of step 4 of gibbs::iteration, each by
// the lane that owns it, operation for operation (the product of a second moment is rounded before it is added).  The caller
// has synced after the last write of the digits and of x_c.
template <class Ctx>
LHVI_HD void record(const lhvi_gibbs_t& g, int s, const gibbs::Workspace& w, const Ctx& ctx, const gibbs::Out& o) {
    const int Nc = g.ex.Nc, Nd = g.ex.Nd;
    for (int n = ctx.lane; n < Nd; n += ctx.lanes) {
        if (o.disc) o.disc[(int64_t)s * Nd + n] = w.dig[n];
        if (o.counts) o.counts[g.dstate_off[n] + w.dig[n]] += 1;
    }
    for (int r = ctx.lane; r < Nc; r += ctx.lanes) {
        const double x = w.xc[r];
        if (o.cont) o.cont[(int64_t)s * Nc + r] = x;
        if (o.sum1) o.sum1[r] += x;
        if (o.sum2)
            for (int q = 0; q <= r; ++q) {
#pragma clang fp contract(off)
                const double xx = x * w.xc[q];
                o.sum2[r * (r + 1) / 2 + q] += xx;
            }
    }
}

// 3. the swap-phase masses of replica r: log m of its digits at its own beta and at beta_partner (its own beta again when it has
// no partner: the same barriers, the result is dropped), posted with the pivot flag.  The caller syncs, then reads the slots.
template <class Ctx>
LHVI_HD void swap_masses(const lhvi_gibbs_t& g, double beta, double beta_partner, const ais::Base& base, const gibbs::Workspace& w,
                         const Ctx& ctx, const Slots& sl, int r) {
    double own, other;
    int bad = ais::collapsed_mass(g, beta, base, w, ctx, own);
    bad |= ais::collapsed_mass(g, beta_partner, base, w, ctx, other);
    if (ctx.lane == 0) {
        sl.lm[2 * r] = own;
        sl.lm[2 * r + 1] = other;
        sl.bad[r] = bad;
    }
}

// log acceptance ratio of the pair (lo, lo + 1):
// log m_{b_lo}(d_lo+1) + log m_{b_lo+1}(d_lo) - log m_{b_lo}(d_lo) - log m_{b_lo+1}(d_lo+1), summed in this order
LHVI_HD double log_ratio(const Slots& sl, int lo) {
    double la = sl.lm[2 * (lo + 1) + 1] + sl.lm[2 * lo + 1];
    la -= sl.lm[2 * lo];
    la -= sl.lm[2 * (lo + 1)];
    return la;
}

LHVI_HD bool accept(double la, double u) { return log(1.0 - u) <= la; }

// the digits of two replicas change places, digit n by the lane that owns it.  The caller syncs after.
template <class Ctx>
LHVI_HD void exchange(int Nd, int32_t* a, int32_t* b, const Ctx& ctx) {
    for (int n = ctx.lane; n < Nd; n += ctx.lanes) {
        const int32_t t = a[n];
        a[n] = b[n];
        b[n] = t;
    }
}

// the pair decision of swap round s at iteration it by the lanes of replica r, when r is the lower replica of a pair: the ratio
// from the slots, the pair's uniform, the exchange with replica r + 1 (whose digits lie `stride` int32 further), the counters
// (swap_try / swap_acc: this ladder's rows [R - 1]) by lane 0 with plain read-modify-write.  No barrier inside.
template <class Ctx>
LHVI_HD void decide(int Nd, int R, int it, int s, int r, const Slots& sl, const SwapDraws& sd, int32_t* dig, int64_t stride,
                    const Ctx& ctx, int32_t* swap_try, int32_t* swap_acc) {
    if (pair_of(R, s, r) != r) return;
    const bool acc = accept(log_ratio(sl, r), sd.uniform(it, r));
    if (acc) exchange(Nd, dig, dig + stride, ctx);
    if (ctx.lane == 0) {
        if (swap_try) swap_try[r] += 1;
        if (swap_acc && acc) swap_acc[r] += 1;
    }
}

}  // namespace pt
}  // namespace lhvi
