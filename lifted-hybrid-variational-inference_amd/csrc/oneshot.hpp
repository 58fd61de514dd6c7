// oneshot.hpp -- what OneShot (osi/OneShot.py: a mixture belief fitted to the Bethe free energy) adds to the arithmetic of npvi.hpp,
// written once for the device (csrc/oneshot.hip) and the host (lhvi_oneshot_*_host: one "lane").  docs/kernels_oneshot.md has the
// formulas.  The factor term is npvi.hpp's factor_item with BFE = true; the gather is gather_finish<true>.
//
// var_item: the term kappa_v E_b[log b_v] of one hidden variable, kappa_v = c_v (1 - deg_v) (mixture_beliefs.py:441-502).  A lane owns
// NM mixture components (device: one; host: all).  Continuous: the K * T nodes a_kt = sqrt(2 Var_k) x_t + Mu_k; each lane evaluates
// its components' densities at the node, the group's total (Ctx::sum_m) is b_v(a), omega = w_k gh_w[t] log b_v is a constant, and the
// lane adds omega N_m / b_v into d / d w_m, omega r_m (a - Mu_m) / Var_m into d / d Mu_m, omega r_m ((a - Mu_m)^2 / Var_m - 1) / 2 into
// d / d lVar_m, r_m = w_m N_m / b_v.  Discrete: the nodes are the states, omega_s = b_v(s) log b_v(s); d / d Pi_m(s) = omega_s w_m / b_v(s)
// is written as it is (gather_finish<true> chains it through the row's softmax).
//
// Ctx: NM; m(i) the i-th component of the lane; sum_m(v) the group's total.
#pragma once
#include "npvi.hpp"

namespace lhvi {
namespace oneshot {

using npvi::MAX_K;
using npvi::VarInfo;

struct HostVarCtx {
    static constexpr int NM = MAX_K;
    int m(int i) const { return i; }
    double sum_m(double v) const { return v; }
};

// pv_c [V][K][2] (d / d Mu, d / d lVar), pv_d [V][K][Dmax] (d / d Pi), pvw [V][K + 1] (d aux / d w_m of the variable, then its
// objective): all of them times kappa_v; zeros for an observed row and where kappa_v == 0 (nothing is evaluated there)
template <class Ctx>
LHVI_HD void var_item(const lhvi_graph_t& g, const lhvi_vi_t& p, const double* __restrict__ var_coef, int v, Ctx& ctx,
                      double* __restrict__ pv_c, double* __restrict__ pv_d, double* __restrict__ pvw) {
    constexpr int NM = Ctx::NM;
    const int K = p.K, Dmax = p.Dmax;
    const double kap = var_coef[v];
    const VarInfo vi = npvi::var_info(g, v);
    if (!vi.hidden || kap == 0.0) {
        for (int i = 0; i < NM; ++i) {
            const int m = ctx.m(i);
            if (m >= K) continue;
            const int64_t row = (int64_t)v * K + m;
            pv_c[2 * row] = 0.0; pv_c[2 * row + 1] = 0.0;
            for (int t = 0; t < Dmax; ++t) pv_d[row * Dmax + t] = 0.0;
            pvw[(int64_t)v * (K + 1) + m] = 0.0;
            if (m == 0) pvw[(int64_t)v * (K + 1) + K] = 0.0;
        }
        return;
    }
    double gw[NM], wm[NM];
    double obj = 0.0;
#pragma unroll
    for (int i = 0; i < NM; ++i) {
        const int m = ctx.m(i);
        gw[i] = 0.0;
        wm[i] = m < K ? p.w[m] : 0.0;
    }
    if (vi.cont) {
        double mu[NM], var[NM], gmu[NM], glv[NM];
#pragma unroll
        for (int i = 0; i < NM; ++i) {
            const int m = ctx.m(i);
            const double* e = p.eta_c + ((int64_t)v * K + (m < K ? m : 0)) * 2;
            mu[i] = e[0]; var[i] = e[1];
            gmu[i] = 0.0; glv[i] = 0.0;
        }
        for (int k = 0; k < K; ++k) {
            const double* ek = p.eta_c + ((int64_t)v * K + k) * 2;
            const double sd = sqrt(2.0 * ek[1]), mk = ek[0], wk = p.w[k];
            for (int t = 0; t < p.T; ++t) {
                const double a = sd * p.gh_x[t] + mk;
                double n[NM], mine = 0.0;
#pragma unroll
                for (int i = 0; i < NM; ++i) {
                    n[i] = ctx.m(i) < K ? npvi::gauss_pdf(a, mu[i], var[i]) : 0.0;
                    mine += wm[i] * n[i];
                }
                const double b = ctx.sum_m(mine);
                const double omega = (wk * p.gh_w[t]) * log(b);
                obj += omega;
                const double rb = omega / b;
#pragma unroll
                for (int i = 0; i < NM; ++i) {
                    if (ctx.m(i) >= K) continue;
                    const double r = rb * n[i], rw = r * wm[i], d = a - mu[i];
                    gw[i] += r;
                    gmu[i] += rw * d / var[i];
                    glv[i] += rw * (0.5 * (d * d / var[i] - 1.0));
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NM; ++i) {
            const int m = ctx.m(i);
            if (m >= K) continue;
            const int64_t row = (int64_t)v * K + m;
            pv_c[2 * row] = kap * gmu[i]; pv_c[2 * row + 1] = kap * glv[i];
        }
    } else {
        for (int s = 0; s < vi.n; ++s) {
            double pi[NM], mine = 0.0;
#pragma unroll
            for (int i = 0; i < NM; ++i) {
                const int m = ctx.m(i);
                pi[i] = m < K ? p.eta_d[((int64_t)v * K + m) * Dmax + s] : 0.0;
                mine += wm[i] * pi[i];
            }
            const double b = ctx.sum_m(mine);
            const double omega = b * log(b);
            obj += omega;
            const double rb = omega / b;
#pragma unroll
            for (int i = 0; i < NM; ++i) {
                const int m = ctx.m(i);
                if (m >= K) continue;
                gw[i] += rb * pi[i];
                pv_d[((int64_t)v * K + m) * Dmax + s] = kap * (rb * wm[i]);
            }
        }
        for (int i = 0; i < NM; ++i) {
            const int m = ctx.m(i);
            if (m >= K) continue;
            for (int s = vi.n; s < Dmax; ++s) pv_d[((int64_t)v * K + m) * Dmax + s] = 0.0;
        }
    }
#pragma unroll
    for (int i = 0; i < NM; ++i) {
        const int m = ctx.m(i);
        if (m >= K) continue;
        pvw[(int64_t)v * (K + 1) + m] = kap * gw[i];
        if (m == 0) pvw[(int64_t)v * (K + 1) + K] = kap * obj;
    }
}

// g_tau and obj from the totals of the factors' and the variables' columns (totF, totV [K + 1]: d aux / d w_m, then the objective)
LHVI_HD void finish_weights(int K, const double* totF, const double* totV, const double* w, double* obj, double* g_tau) {
    double gw[MAX_K], dot = 0.0;
    for (int k = 0; k < K; ++k) {
        gw[k] = totF[k] + totV[k];
        dot += w[k] * gw[k];
    }
    for (int k = 0; k < K; ++k) g_tau[k] = w[k] * (gw[k] - dot);
    obj[0] = totF[K] + totV[K];
}

}  // namespace oneshot
}  // namespace lhvi
