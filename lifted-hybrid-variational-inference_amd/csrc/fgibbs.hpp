// fgibbs.hpp -- single-site Gibbs on a ground flat graph: the update of one hidden variable of one chain, written once for the
// device (csrc/fgibbs.hip: one lane per (variable, chain), or a wavefront per (hub variable, chain)) and the host
// (lhvi_fgibbs_chain_host: one "lane", the sequential order).  Same style as gibbs.hpp: the lanes of a ctx share every sum over
// the variable's factors (ctx.sum: identity for one lane, the DPP wave reduction for 64) and the scalar logic -- slice level,
// shrinkage, inverse-CDF pick -- runs uniformly on all of them, on the same bits.
//
// A ctx also hands out the three structs (ctx.G(), ctx.P(), ctx.S()) and the interpreter's evaluation stack (ctx.stack()): the
// device reads the structs from the kernel's argument block where a field is used (the technique of pt.hip) instead of holding
// some fifty pointers in scalar registers through the loops, and keeps the stack in a column of LDS; the host passes pointers.
//
// State: x [V][C] / idx [V][C], chain fastest (the lanes of a wavefront of the lane kernel are consecutive chains of one variable:
// one coalesced read per factor argument, factor kind and parameters wave-uniform).
#pragma once
#include "gibbs.hpp"
#include "potential.hpp"

namespace lhvi {
namespace fgibbs {

// the fourth Philox counter word: "FGSU" sweep uniforms, "FGXI" the initial state
constexpr uint32_t TAG_SWEEP = 0x46475355u, TAG_INIT = 0x46475849u;
constexpr int MAX_STATES = LHVI_FGIBBS_MAX_STATES;
constexpr int MAX_SHRINK = 510;                 // draw pair p < 256 rides in the top byte of the first counter word
constexpr int64_t MAX_CHAINS = (int64_t)1 << 24;

struct HostCtx {
    const lhvi_graph_t* g;
    const lhvi_pots_t* pots;
    const lhvi_fgibbs_t* s;
    int64_t chains, c;
    double* xs;
    int32_t* is;
    int lane = 0, lanes = 1;
    int64_t C() const { return chains; }
    double* x() const { return xs; }
    int32_t* idx() const { return is; }
    void sync() const {}
    double sum(double v) const { return v; }
    const lhvi_graph_t& G() const { return *g; }
    const lhvi_pots_t& P() const { return *pots; }
    const lhvi_fgibbs_t& S() const { return *s; }
    MlnRegStack stack() const { return MlnRegStack(); }
};

// the state of variable v in the ctx's chain ctx.c of ctx.C() chains
template <class Ctx>
LHVI_POT_HD double& X(const Ctx& ctx, int v) { return ctx.x()[(int64_t)v * ctx.C() + ctx.c]; }
template <class Ctx>
LHVI_POT_HD int32_t& I(const Ctx& ctx, int v) { return ctx.idx()[(int64_t)v * ctx.C() + ctx.c]; }

// uniform `draw` of (chain, iteration, variable): injected, or half of Philox block (chain | pair << 24, it, v, tag)
template <class Ctx>
LHVI_POT_HD double uniform(const Ctx& ctx, int it, int v, int draw) {
    const lhvi_fgibbs_t& s = ctx.S();
    const int V = ctx.G().V;
    if (s.u) return s.u[(((int64_t)it * ctx.C() + ctx.c) * V + v) * (1 + s.max_shrink) + draw];
    double u0, u1;
    gibbs::uniform2(s.seed, (uint32_t)ctx.c | ((uint32_t)(draw >> 1) << 24), (uint32_t)it, (uint32_t)v, TAG_SWEEP, u0, u1);
    return (draw & 1) ? u1 : u0;
}

// g_v(t): the sum of log phi over v's var_edge row with x_v = t (state index ti), this lane's entries in row order, then over lanes
template <bool INTERP, class Ctx>
LHVI_POT_HD double cond_logp(const Ctx& ctx, int v, double t, int ti) {
    double acc = 0.0;
    const int end = ctx.G().var_ptr[v + 1];
    for (int k = ctx.G().var_ptr[v] + ctx.lane; k < end; k += ctx.lanes) {
        const int f = ctx.G().edge_fac[ctx.G().var_edge[k]];
        const int base = ctx.G().fac_ptr[f], arity = ctx.G().fac_ptr[f + 1] - base;
        double xs[LHVI_MAX_ARITY];
        int ix[LHVI_MAX_ARITY];
#pragma unroll
        for (int a = 0; a < LHVI_MAX_ARITY; ++a) {
            xs[a] = 0.0;
            ix[a] = 0;
            if (a < arity) {
                const int w = ctx.G().edge_var[base + a];
                xs[a] = w == v ? t : X(ctx, w);
                ix[a] = w == v ? ti : I(ctx, w);
            }
        }
        const int pot = ctx.G().fac_pot[f], kind = ctx.P().kind[pot];
        const double* __restrict__ par = ctx.P().param + ctx.P().off[pot];
        bool is_log = true;
        double val;
        if (kind == LHVI_POT_HYBRID_QUADRATIC) {
            // pot_eval's value with the continuous arguments read at xs[Nd + i]: a pointer into the middle of xs would keep the
            // array out of registers
            const int Nd = (int)par[0], Nc = (int)par[1];
            int cfg = 0, ncfg = 1;
            for (int i = 0; i < Nd; ++i) { cfg = cfg * (int)par[2 + i] + (int)xs[i]; ncfg *= (int)par[2 + i]; }
            val = quad_form_at(par + 2 + Nd + cfg * Nc * Nc, par + 2 + Nd + ncfg * Nc * Nc + cfg * Nc,
                               par[2 + Nd + ncfg * Nc * Nc + ncfg * Nc + cfg], Nc, xs, Nd);
        } else {
            auto st = ctx.stack();
            val = pot_eval_on<INTERP>(kind, par, xs, ix, is_log, st);
        }
        acc += is_log ? val : log(val);          // phi == 0: -inf
    }
    return ctx.sum(acc);
}

// the kept sample of (v, chain) at iteration `it`: by the lane that owns the pair, in iteration order
template <class Ctx>
LHVI_POT_HD void accumulate(const Ctx& ctx, int it, int v, bool cont) {
    const lhvi_fgibbs_t& s = ctx.S();
    const int k = it - s.num_burnin;
    if (k < 0 || k % s.thin != 0 || k / s.thin >= s.num_samples) return;
    const int64_t at = (int64_t)v * ctx.C() + ctx.c;
    const double xv = ctx.x()[at];
    if (cont) {
        if (s.sum1) s.sum1[at] += xv;
        if (s.sum2) {
            // the product is rounded before it is added: the sum of the stored samples' squares, term by term
#pragma clang fp contract(off)
            const double xx = xv * xv;
            s.sum2[at] += xx;
        }
    } else if (s.counts && s.cnt_off[v] >= 0) {
        s.counts[(int64_t)(s.cnt_off[v] + ctx.idx()[at]) * ctx.C() + ctx.c] += 1;
    }
    if (s.samples && s.keep_row[v] >= 0)
        s.samples[(int64_t)s.keep_row[v] * (ctx.C() * s.num_samples) + ctx.c * s.num_samples + k / s.thin] = xv;
}

// counters of a chain: several variables of one colour add to them in one launch, so the device adds atomically (integers: any
// order gives the same total)
LHVI_POT_HD void count(int32_t* p, int64_t c, int n) {
    if (!p) return;
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p + c, n);
#else
    p[c] += n;
#endif
}
LHVI_POT_HD void count(int64_t* p, int64_t c, int n) {
    if (!p) return;
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(reinterpret_cast<unsigned long long*>(p + c), (unsigned long long)n);
#else
    p[c] += n;
#endif
}

// One update of hidden variable v in the ctx's chain at iteration `it`.  lp: MAX_STATES doubles at stride `stride` that the ctx's lanes
// share (and no other ctx touches).  Every lane computes the same decisions; lane 0 stores.
template <bool INTERP, class Ctx>
LHVI_POT_HD void update(const Ctx& ctx, int it, int v, double* lp, int stride) {
    const int d = ctx.G().var_dom[v];
    const bool cont = ctx.G().dom_cont[d] != 0;
    if (cont) {
        // Neal's slice sampler, shrinkage from the whole domain interval
        const double x0 = X(ctx, v);
        const double y = cond_logp<INTERP>(ctx, v, x0, 0) + log(1.0 - uniform(ctx, it, v, 0));
        double L = ctx.G().dom_lo[d], R = ctx.G().dom_hi[d], xn = x0;
        int k = 1;
        bool got = false;
        for (; k <= ctx.S().max_shrink; ++k) {
            double x1;
            {
#pragma clang fp contract(off)
                const double step = uniform(ctx, it, v, k) * (R - L);
                x1 = L + step;
            }
            if (cond_logp<INTERP>(ctx, v, x1, 0) >= y) { xn = x1; got = true; break; }
            if (x1 < x0) L = x1; else R = x1;
        }
        if (ctx.lane == 0) {
            if (got) X(ctx, v) = xn;
            else count(ctx.S().capped, ctx.c, 1);
            count(ctx.S().evals, ctx.c, k + (got ? 1 : 0));
        }
    } else {
        const int p0 = ctx.G().dom_ptr[d], S = ctx.G().dom_ptr[d + 1] - p0;
        if (S > MAX_STATES) return;         // (lp holds MAX_STATES masses; the Python caller raises before any launch)
        double mx = -__builtin_huge_val();
        for (int j = 0; j < S; ++j) {
            const double val = cond_logp<INTERP>(ctx, v, ctx.G().dom_val[p0 + j], j);
            if (ctx.lane == 0) lp[j * stride] = val;
            if (val > mx) mx = val;
        }
        ctx.sync();
        if (mx == -__builtin_huge_val()) {
            if (ctx.lane == 0) count(ctx.S().stuck, ctx.c, 1);
        } else {
            const int pick = gibbs::softmax_pick(lp, stride, S, uniform(ctx, it, v, 0));
            if (ctx.lane == 0) {
                X(ctx, v) = ctx.G().dom_val[p0 + pick];
                I(ctx, v) = pick;
            }
        }
        if (ctx.lane == 0) count(ctx.S().evals, ctx.c, S);
        ctx.sync();                     // lp is free for the ctx's next variable
    }
    if (ctx.lane == 0) accumulate(ctx, it, v, cont);
}

// the initial state of variable v in chain c of C
LHVI_POT_HD void init_var(const lhvi_graph_t& g, const lhvi_fgibbs_t& s, int64_t C, int64_t c, double* x, int32_t* idx, int v) {
    const int d = g.var_dom[v];
    const bool cont = g.dom_cont[d] != 0;
    const int p0 = g.dom_ptr[d], S = g.dom_ptr[d + 1] - p0;
    const double val = g.var_value[v];
    double out = val;
    int st = 0;
    if (val != val) {
        if (s.init_x) {
            out = s.init_x[c * g.V + v];
        } else {
            double u0, u1;
            gibbs::uniform2(s.seed, (uint32_t)c, 0u, (uint32_t)v, TAG_INIT, u0, u1);
            if (cont) {
#pragma clang fp contract(off)
                const double step = u0 * (g.dom_hi[d] - g.dom_lo[d]);
                out = g.dom_lo[d] + step;
            } else {
                const int k = (int)(u0 * (double)S);
                out = g.dom_val[p0 + (k < S - 1 ? k : S - 1)];
            }
        }
    }
    if (!cont)
        for (int j = S - 1; j >= 0; --j)
            if (g.dom_val[p0 + j] == out) st = j;
    x[(int64_t)v * C + c] = out;
    idx[(int64_t)v * C + c] = st;
}

}  // namespace fgibbs
}  // namespace lhvi
