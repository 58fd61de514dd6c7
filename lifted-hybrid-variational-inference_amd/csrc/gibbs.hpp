// gibbs.hpp -- one outer iteration of a block Gibbs chain in a hybrid Gaussian MRF (gibbs/hybrid_gaussian_mrf.py::
// block_gibbs_sample :216-263 and the sweep of gibbs/disc_mrf_sampler.pyx), written once for the device (csrc/gibbs.hip: a group
// of lanes per chain) and the host (lhvi_gibbs_chain_host: one "lane").  Same style as exact.hpp: loops over the rows a lane
// owns, ctx.sync() between phases, every value produced by ONE lane with a serial loop in a fixed order, so a chain's samples
// do not depend on the number of lanes.  All control flow around a ctx.sync() depends on the model alone, never on a chain's
// state: the chains of a wavefront reach every barrier together.
//
// Workspace of a chain (doubles): mat [Nc][ld], b [Nc], y [Nc], xc [Nc], ldiag [Nc], dinv [Nc] (the layout of exact.hpp with
// x_c in the place of mu), lprobs [max_states], the conditional tables [table_doubles] when they live in LDS, then Nd int32
// digits (x_d).
#pragma once
#include "exact.hpp"

namespace lhvi {
namespace gibbs {

// the fourth Philox counter word: "GBNZ" normals, "GBUF" uniforms, "GBXI" the initial state
constexpr uint32_t TAG_NORMAL = 0x47424e5au, TAG_UNIFORM = 0x47425546u, TAG_INIT = 0x47425849u;

// ---- Philox4x32-10 (the round of mws.hip / pbp.hip) -------------------------------------------------------------------------------
LHVI_HD void philox4(uint32_t (&c)[4], uint64_t seed) {
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}
// two uniforms in [0, 1) (53 bits each) of counter (a, b, draw, tag)
LHVI_HD void uniform2(uint64_t seed, uint32_t a, uint32_t b, uint32_t draw, uint32_t tag, double& u0, double& u1) {
    uint32_t c[4] = {a, b, draw, tag};
    philox4(c, seed);
    const uint64_t r0 = ((uint64_t)c[0] << 32) | c[1], r1 = ((uint64_t)c[2] << 32) | c[3];
    u0 = (double)(r0 >> 11) * (1.0 / 9007199254740992.0);
    u1 = (double)(r1 >> 11) * (1.0 / 9007199254740992.0);
}

// The draws of one chain: injected (z [iters][chains][Nc], u [iters][chains][its][Nd], rows by absolute iteration) or the
// Philox stream of counter (chain, iteration, draw index, tag).  A draw depends on its counter and the seed alone.
struct Draws {
    uint64_t seed;
    const double *z, *u;
    int64_t chains, chain;
    int Nc, Nd, its;
    uint32_t tag_normal = TAG_NORMAL, tag_uniform = TAG_UNIFORM;   // the annealed sampler (csrc/ais.hpp) draws under tags of its own
    // z_r of iteration it: Box-Muller on the pair (r & ~1, r | 1) of counter draw r / 2
    LHVI_HD double normal(int it, int r) const {
        if (z) return z[((int64_t)it * chains + chain) * Nc + r];
        double u0, u1;
        uniform2(seed, (uint32_t)chain, (uint32_t)it, (uint32_t)(r >> 1), tag_normal, u0, u1);
        const double rad = sqrt(-2.0 * log(1.0 - u0)), ang = 6.283185307179586 * u1;
        return (r & 1) ? rad * sin(ang) : rad * cos(ang);
    }
    // the uniform of draw idx = sweep * Nd + variable of iteration it
    LHVI_HD double uniform(int it, int idx) const {
        if (u) return u[((int64_t)it * chains + chain) * ((int64_t)its * Nd) + idx];
        double u0, u1;
        uniform2(seed, (uint32_t)chain, (uint32_t)it, (uint32_t)(idx >> 1), tag_uniform, u0, u1);
        return (idx & 1) ? u1 : u0;
    }
};

LHVI_HD int gauss_doubles(int Nc) { return Nc * exact::ld_of(Nc) + 5 * Nc; }
// disc_doubles: max_states + the conditional tables kept in the workspace
LHVI_HD int ws_doubles(int Nc, int Nd, int disc_doubles) { return gauss_doubles(Nc) + disc_doubles + (Nd + 1) / 2; }

struct Workspace {
    double *mat, *b, *y, *xc, *ldiag, *dinv, *lprobs, *tab;
    int32_t* dig;
};
// tab_global: the chain's conditional-table row in global memory, or null (tables in the workspace)
LHVI_HD Workspace layout(const lhvi_gibbs_t& g, double* W, double* tab_global) {
    const int Nc = g.ex.Nc;
    Workspace w;
    w.mat = W;
    w.b = W + Nc * exact::ld_of(Nc);
    w.y = w.b + Nc;
    w.xc = w.y + Nc;
    w.ldiag = w.xc + Nc;
    w.dinv = w.ldiag + Nc;
    w.lprobs = w.dinv + Nc;
    double* end = w.lprobs + g.max_states;
    w.tab = tab_global ? tab_global : end;
    if (!tab_global) end += g.table_doubles;
    w.dig = reinterpret_cast<int32_t*>(end);
    return w;
}

// the outputs of one chain (each may be null): rows of this chain
struct Out {
    int32_t* disc;      // [num_samples][Nd]
    double* cont;       // [num_samples][Nc]
    int32_t* counts;    // [sum dstates]
    double *sum1, *sum2;
};

// local index of a descriptor's discrete scope (pairs (variable, local stride) at p) with variable n at state j
LHVI_HD int64_t local_with(const int32_t* p, int nd, const int32_t* dig, int n, int j) {
    int64_t l = 0;
    for (int a = 0; a < nd; ++a) l += (int64_t)(p[2 * a] == n ? j : dig[p[2 * a]]) * p[2 * a + 1];
    return l;
}

// The two pieces of the discrete block that iteration() below shares with the Rao-Blackwellised marginals (csrc/gibbs_rb.hpp);
// their floating-point operations are iteration()'s own.
//
// reduced_tables: the reduced log table of every strictly hybrid factor at xc (Potential.py get_table_params_given_x_c):
// sum(A_k * x x^T) row-major, + b_k . x, + c_k, entry k by the lane that owns it.  The caller syncs after.
template <class Ctx>
LHVI_HD void reduced_tables(const lhvi_gibbs_t& g, const double* xc, double* tab, const Ctx& ctx) {
    const lhvi_exact_t& m = g.ex;
    for (int h = 0; h < g.n_hyb; ++h) {
        const int32_t* rec = m.quad_desc + m.quad_ptr[g.hyb_quad[h]];
        const int nd = rec[0], nc = rec[1], stride = nc * nc + nc + 1;
        const int32_t* sc = rec + 3 + 2 * nd;
        const int L = g.hyb_off[h + 1] - g.hyb_off[h];
        for (int k = ctx.lane; k < L; k += ctx.lanes) {
            const double* P = m.quad_par + rec[2] + (int64_t)k * stride;
            double s = 0.0, t = 0.0;
            for (int a = 0; a < nc; ++a)
                for (int j = 0; j < nc; ++j) s += P[a * nc + j] * (xc[sc[a]] * xc[sc[j]]);
            for (int a = 0; a < nc; ++a) t += P[nc * nc + a] * xc[sc[a]];
            tab[g.hyb_off[h] + k] = (s + t) + P[nc * nc + nc];
        }
    }
}

// cond_lprobs: lprobs[j] = log p~(x_n = j | the other digits, x_c) up to a constant: variable n's table factors, then its hybrid
// factors' reduced tables, in factor order, state j by the lane that owns it.  The caller syncs after.
template <class Ctx>
LHVI_HD void cond_lprobs(const lhvi_gibbs_t& g, int n, const int32_t* dig, const double* tab, double* lprobs, const Ctx& ctx) {
    const lhvi_exact_t& m = g.ex;
    const int d = m.dstates[n];
    for (int j = ctx.lane; j < d; j += ctx.lanes) {
        double v = 0.0;
        for (int e = g.vt_ptr[n]; e < g.vt_ptr[n + 1]; ++e) {
            const int32_t* rec = m.tab_desc + m.tab_ptr[g.vt_fac[e]];
            v += m.tab_par[rec[1] + local_with(rec + 2, rec[0], dig, n, j)];
        }
        for (int e = g.vh_ptr[n]; e < g.vh_ptr[n + 1]; ++e) {
            const int h = g.vh_fac[e];
            const int32_t* rec = m.quad_desc + m.quad_ptr[g.hyb_quad[h]];
            v += tab[g.hyb_off[h] + local_with(rec + 3, rec[0], dig, n, j)];
        }
        lprobs[j] = v;
    }
}

// The two triangular solves of the Gaussian block, shared with the annealed sampler (csrc/ais.hpp); their floating-point
// operations are iteration()'s own.
//
// forward_solve: y = L^-1 b, one column per step: row r subtracts L[r][j] y[j] for j = 0 .. r - 1 in this order.  Every y is
// final and visible to all lanes on return.
template <class Ctx>
LHVI_HD void forward_solve(int Nc, const Workspace& w, const Ctx& ctx) {
    const int ld = exact::ld_of(Nc);
    for (int r = ctx.lane; r < Nc; r += ctx.lanes) w.y[r] = w.b[r];
    for (int j = 0; j < Nc; ++j) {
        for (int r = ctx.lane; r < Nc; r += ctx.lanes)
            if (r == j) w.y[j] *= w.dinv[j];
        ctx.sync();
        for (int r = ctx.lane; r < Nc; r += ctx.lanes)
            if (r > j) w.y[r] -= w.mat[r * ld + j] * w.y[j];
    }
}

// back_solve: x_c = L^-T (y + z) with z the normals of iteration `it`: row r subtracts L[i][r] x[i] for i = Nc - 1 .. r + 1 in
// this order.  Every x_c is final and visible to all lanes on return.
template <class Ctx>
LHVI_HD void back_solve(int Nc, int it, const Draws& dr, const Workspace& w, const Ctx& ctx) {
    const int ld = exact::ld_of(Nc);
    for (int r = ctx.lane; r < Nc; r += ctx.lanes) w.xc[r] = w.y[r] + dr.normal(it, r);
    for (int i = Nc - 1; i >= 0; --i) {
        for (int r = ctx.lane; r < Nc; r += ctx.lanes)
            if (r == i) w.xc[i] *= w.dinv[i];
        ctx.sync();
        for (int r = ctx.lane; r < Nc; r += ctx.lanes)
            if (r < i) w.xc[r] -= w.mat[i * ld + r] * w.xc[i];
    }
}

// The draw of a discrete conditional from its log masses lp[j * stride], j < d (disc_mrf_sampler.pyx :43-70): the softmax
// exp(v - (m + log sum)), then the first state with u <= cumulative sum; the last state catches rounding.  Shared with the
// single-site sampler on flat graphs (csrc/fgibbs.hpp), whose lanes keep a column of LDS each (stride = the workgroup).
LHVI_HD int softmax_pick(const double* lp, int stride, int d, double u) {
    double mx = -__builtin_huge_val(), sum = 0.0;
    for (int j = 0; j < d; ++j)
        if (lp[j * stride] > mx) mx = lp[j * stride];
    for (int j = 0; j < d; ++j) sum += exp(lp[j * stride] - mx);
    const double scale = mx + log(sum);
    double cum = 0.0;
    int pick = d - 1;
    for (int j = 0; j < d; ++j) {
        cum += exp(lp[j * stride] - scale);
        if (u <= cum) { pick = j; break; }
    }
    return pick;
}

// One outer iteration `it` of a chain whose x_d is in w.dig.  dead: the chain met a J that is not positive definite; it keeps
// its x_d from then on and stores nothing.  Returns 1 when this iteration's J is not positive definite (and sets dead), the
// same value in every lane.
template <class Ctx>
LHVI_HD int iteration(const lhvi_gibbs_t& g, int it, const Draws& dr, const Workspace& w, const Ctx& ctx, bool& dead,
                      const Out& o) {
    const lhvi_exact_t& m = g.ex;
    const int Nc = m.Nc, Nd = m.Nd;
    int bad = 0;
    if (Nc) {
        // 1. x_c | x_d (:217-233): J = L L^T, y = L^-1 b, x_c = L^-T (y + z) = mu + L^-T z
        double c, logdet;
        exact::assemble(m, w.dig, w.mat, w.b, ctx, c);
        ctx.sync();
        exact::form_J(Nc, w.mat, ctx);
        bad = exact::cholesky(Nc, w.mat, w.ldiag, w.dinv, ctx, logdet);
        dead = dead || bad;
        forward_solve(Nc, w, ctx);
        back_solve(Nc, it, dr, w, ctx);
    }
    // 2. the reduced tables at x_c, once per outer iteration
    reduced_tables(g, w.xc, w.tab, ctx);
    ctx.sync();
    // 3. x_d | x_c: disc_block_its sweeps over the variables in order (disc_mrf_sampler.pyx gibbs_sample_one)
    for (int sweep = 0; sweep < g.disc_block_its; ++sweep)
        for (int n = 0; n < Nd; ++n) {
            const int d = m.dstates[n];
            cond_lprobs(g, n, w.dig, w.tab, w.lprobs, ctx);
            ctx.sync();
            // softmax (:43-58) and the first state with u <= cumulative sum (:62-70), by every lane with the same bits; the
            // last state catches rounding
            const int pick = softmax_pick(w.lprobs, 1, d, dr.uniform(it, sweep * Nd + n));
            if (ctx.lane == 0 && !dead) w.dig[n] = pick;  // no lane reads the digits between the two barriers
            ctx.sync();
        }
    // 4. the kept sample (x_d after the sweeps, x_c; :260-263) and the chain's accumulators, each by the lane that owns it
    const int s = it - g.num_burnin;
    if (s >= 0 && !dead) {
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
                    // the product is rounded before it is added: the sum is that of the stored samples' products, term by
                    // term (a fused multiply-add would differ from it by a rounding that cancellation in a cross moment
                    // magnifies)
#pragma clang fp contract(off)
                    const double xx = x * w.xc[q];
                    o.sum2[r * (r + 1) / 2 + q] += xx;
                }
        }
    }
    return bad;
}

}  // namespace gibbs
}  // namespace lhvi
