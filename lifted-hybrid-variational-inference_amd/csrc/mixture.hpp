// mixture.hpp -- conditional queries on a fitted mixture belief q(x) = sum_k w_k prod_i q_ik(x_i) (osi/mixture_beliefs.py
// :505-746, osi/utils.py:66-98), written once for the device (csrc/mixture.hip) and the host (lhvi_mix_*_host: one "lane").
// Conditioning on x_o re-weights the K components: w' = softmax(log w + sum_{i in o} log q_ik(x_i)).
//
// Every sum is formed by ONE thread with a serial loop in a fixed order, so a value depends on its own inputs alone: not on
// the number of evidence rows in the call, not on the row's position, not on the number of lanes.  Contraction is off for
// the whole file: a * b + c is rounded twice on both sides, which is what makes the component sums of the device and of
// the host twin the same bits.
#pragma once
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
namespace mix {

constexpr int TILE = LHVI_MIX_TILE;     // observed variables of one stage-1 partial sum
constexpr int ROWS = LHVI_MIX_ROWS;     // evidence rows that share one pass over a tile's records
constexpr double NEG_INF = -__builtin_huge_val();

LHVI_HD int tiles_of(int n_obs) { return (n_obs + TILE - 1) / TILE; }

// records of row v, component k (lhvi_mix_prepare): rec = (c, mu, 1 / var), lpi = log pi, logw (by the items with v == 0)
LHVI_HD void prepare_one(int K, int Dmax, int normaliser, const double* w, const double* eta_c, const double* eta_d,
                         const int32_t* nstates, int v, int k, double* logw, double* rec, double* lpi) {
    const int64_t i = (int64_t)v * K + k;
    if (v == 0) logw[k] = log(w[k]);
    double c = 0.0, mu = 0.0, iv = 0.0;
    const int ns = nstates[v];
    if (ns == 0 && eta_c) {
        const double var = eta_c[2 * i + 1];
        mu = eta_c[2 * i];
        iv = 1.0 / var;
        // 'gaussian': -1/2 log 2 pi + 1/2 log(1 / var) (osi/mixture_beliefs.py:538); 'vi': -log(2.506628274631 var), the
        // density VarInference.norm_pdf evaluates (it divides by the variance)
        c = normaliser == LHVI_MIX_VI ? -log(2.506628274631 * var) : -0.5 * 1.8378770664093453 + 0.5 * log(iv);
    }
    rec[3 * i] = c;
    rec[3 * i + 1] = mu;
    rec[3 * i + 2] = iv;
    if (lpi)
        for (int s = 0; s < Dmax; ++s) lpi[i * Dmax + s] = ns > 0 && s < ns ? log(eta_d[i * Dmax + s]) : NEG_INF;
}

// log q_vk(x) of a continuous row: c - 1/2 (x - mu)^2 / var in the reference's order, -0.5 * (x - mu) ** 2 * var_inv
LHVI_HD double cont_term(const double* r, double x) {
    const double d = x - r[1];
    return r[0] + -0.5 * (d * d) * r[2];
}

// stage 1 of lhvi_mix_condition: out[j] = the sum, in index order, of log q_ok(X[m0 + j][o]) over the observed variables o of
// tile t, for component k and the R evidence rows m0 .. m0 + R - 1 (rows >= M: nothing).  NaN = not observed in that row.  A
// discrete value that is no state of its row gives NaN (the caller validates), a row without parameters adds nothing.
template <int R>
LHVI_HD void tile_partial(const lhvi_mix_t& b, int n_obs, const int32_t* obs_rows, const double* X, int64_t M, int64_t m0, int t,
                          int k, double* out) {
    double acc[R];
    for (int j = 0; j < R; ++j) acc[j] = 0.0;
    const int lo = t * TILE, hi = lo + TILE < n_obs ? lo + TILE : n_obs;
    for (int o = lo; o < hi; ++o) {
        const int v = obs_rows[o];
        if ((unsigned)v >= (unsigned)b.V) continue;             // no row of the belief: adds nothing (the caller validates)
        const int ns = b.nstates[v];
        const int64_t i = (int64_t)v * b.K + k;
        if (ns == 0) {
            const double r[3] = {b.rec[3 * i], b.rec[3 * i + 1], b.rec[3 * i + 2]};
            for (int j = 0; j < R; ++j) {
                if (m0 + j >= M) break;
                const double x = X[(m0 + j) * n_obs + o];
                if (x == x) acc[j] += cont_term(r, x);
            }
        } else if (ns > 0 && b.lpi) {
            const double* lp = b.lpi + i * b.Dmax;
            for (int j = 0; j < R; ++j) {
                if (m0 + j >= M) break;
                const double x = X[(m0 + j) * n_obs + o];
                if (x == x) {
                    const int s = x >= 0.0 && x < (double)ns ? (int)x : -1;
                    acc[j] += s >= 0 ? lp[s] : __builtin_nan("");
                }
            }
        }
    }
    for (int j = 0; j < R; ++j) out[j] = acc[j];
}

// stage 2, one evidence row: comp[k] = the tiles' partial sums in tile order, logp = logsumexp_k(log w + comp),
// condw[k] = exp(log w + comp - logp).  part: [tiles][K] of this row.  comp, logp, condw may each be null.
LHVI_HD void finish_row(const lhvi_mix_t& b, int tiles, const double* part, double* comp, double* logp, double* condw) {
    const int K = b.K;
    double mx = NEG_INF;
    for (int k = 0; k < K; ++k) {
        double c = 0.0;
        for (int t = 0; t < tiles; ++t) c += part[(int64_t)t * K + k];
        if (comp) comp[k] = c;
        mx = fmax(mx, b.logw[k] + c);       // (fmax drops a NaN operand: a NaN component shows in comp and condw)
    }
    double s = 0.0;
    for (int k = 0; k < K; ++k) {
        double c = 0.0;
        for (int t = 0; t < tiles; ++t) c += part[(int64_t)t * K + k];
        s += exp(b.logw[k] + c - mx);
    }
    const double lp = mx == NEG_INF ? NEG_INF : mx + log(s);
    if (logp) *logp = lp;
    if (condw)
        for (int k = 0; k < K; ++k) {
            double c = 0.0;
            for (int t = 0; t < tiles; ++t) c += part[(int64_t)t * K + k];
            condw[k] = exp(b.logw[k] + c - lp);
        }
}

// log of sum_k cw[k] N(x; mu_k, var_k) of continuous row v, with its first and second derivative in x: one pass in component
// order with a running maximum (components of weight 0 are skipped)
LHVI_HD void gm_eval(const lhvi_mix_t& b, int v, const double* cw, double x, double res[3]) {
    const double* r = b.rec + (int64_t)v * b.K * 3;
    double mx = NEG_INF, s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int k = 0; k < b.K; ++k) {
        const double wk = cw[k];
        if (!(wk > 0.0)) continue;
        const double d = r[3 * k + 1] - x, iv = r[3 * k + 2];
        const double g = d * iv, t = r[3 * k] + -0.5 * (d * d) * iv;
        if (t == NEG_INF) continue;
        if (t > mx) {
            const double sc = exp(mx - t);
            s0 *= sc, s1 *= sc, s2 *= sc;
            mx = t;
        }
        const double e = wk * exp(t - mx);
        s0 += e;
        s1 += e * g;
        s2 += e * (g * g - iv);
    }
    const double g = s1 / s0;
    res[0] = mx == NEG_INF ? NEG_INF : mx + log(s0);
    res[1] = g;
    res[2] = s2 / s0 - g * g;
}

LHVI_HD double clip(double x, double lo, double hi) { return fmin(fmax(x, lo), hi); }

// safeguarded Newton on the log density from x0 (clipped to [lo, hi]): step -g / h where h < 0, else g * vmin (vmin: the
// smallest component variance); the step is clipped to the bounds and halved while it lowers the density; stops when it
// moves x by less than 1e-14 max(1, |x|).  The iteration of exact_polish_kernel (docs/kernels_exact.md).
LHVI_HD void gm_newton(const lhvi_mix_t& b, int v, const double* cw, double x0, double lo, double hi, double vmin, int max_iter,
                       double* xout, double* fout) {
    double cur = clip(x0, lo, hi), res[3];
    gm_eval(b, v, cw, cur, res);
    double f = res[0], g = res[1], h = res[2];
    for (int it = 0; it < max_iter; ++it) {
        double step = h < 0.0 ? -g / h : g * vmin;
        bool moved = false;
        for (int half = 0; half < 40; ++half) {
            const double cand = clip(cur + step, lo, hi);
            if (cand == cur) break;
            gm_eval(b, v, cw, cand, res);
            if (res[0] >= f) {
                moved = fabs(cand - cur) > 1e-14 * fmax(1.0, fabs(cur));
                cur = cand, f = res[0], g = res[1], h = res[2];
                break;
            }
            step *= 0.5;
        }
        if (!moved) break;
    }
    *xout = cur;
    *fout = f;
}

// a lane's candidate for item (evidence row, query row): the best of the starts (continuous row: component means k = lane,
// lane + lanes, ...) or states (discrete row: s = lane, lane + lanes, ...) it owns.  key = the start / state index; a
// larger f wins, equal f the lower key, so that the merged answer does not depend on the number of lanes.
struct Cand {
    double f, x;
    int key;
};
LHVI_HD bool better(const Cand& a, const Cand& b) {           // a before b
    if (b.key < 0) return a.key >= 0;
    if (a.key < 0) return false;
    return a.f > b.f || (a.f == b.f && a.key < b.key);
}

LHVI_HD Cand lane_candidate(const lhvi_mix_t& b, int v, const double* cw, double lo, double hi, int max_iter, int lane, int lanes) {
    Cand best{NEG_INF, __builtin_nan(""), -1};
    const int ns = (unsigned)v < (unsigned)b.V ? b.nstates[v] : -1, K = b.K;
    if (ns == 0) {
        const double* r = b.rec + (int64_t)v * K * 3;
        double ivmax = 0.0;
        for (int k = 0; k < K; ++k) ivmax = fmax(ivmax, r[3 * k + 2]);
        const double vmin = 1.0 / ivmax;
        for (int k = lane; k < K; k += lanes) {
            if (!(cw[k] > 0.0)) continue;                      // a component of conditional weight 0 is no start
            Cand c{0.0, 0.0, k};
            gm_newton(b, v, cw, r[3 * k + 1], lo, hi, vmin, max_iter, &c.x, &c.f);
            if (better(c, best)) best = c;
        }
    } else if (ns > 0 && b.pi) {
        const double* pi = b.pi + (int64_t)v * K * b.Dmax;
        for (int s = lane; s < ns; s += lanes) {
            double p = 0.0;
            for (int k = 0; k < K; ++k) p += cw[k] * pi[(int64_t)k * b.Dmax + s];
            const Cand c{p, (double)s, s};
            if (better(c, best)) best = c;
        }
    }
    return best;
}

// the value row m observes for a query: the first non-NaN among the query's positions in the observed list, else NaN
LHVI_HD double observed_value(const int32_t* qobs_ptr, const int32_t* qobs_idx, int q, const double* Xm) {
    if (!qobs_ptr) return __builtin_nan("");
    for (int i = qobs_ptr[q]; i < qobs_ptr[q + 1]; ++i) {
        const double x = Xm[qobs_idx[i]];
        if (x == x) return x;
    }
    return __builtin_nan("");
}

// log sum_k cw[k] q_vk(x): a continuous row at the value x, a discrete row at the state index x (no state: NaN)
LHVI_HD double log_belief_point(const lhvi_mix_t& b, int v, const double* cw, double x) {
    const int ns = (unsigned)v < (unsigned)b.V ? b.nstates[v] : -1;
    if (ns == 0) {
        double res[3];
        gm_eval(b, v, cw, x, res);
        return res[0];
    }
    if (ns < 0 || !b.pi || !(x >= 0.0 && x < (double)ns)) return __builtin_nan("");
    const double* pi = b.pi + (int64_t)v * b.K * b.Dmax + (int)x;
    double p = 0.0;
    for (int k = 0; k < b.K; ++k) p += cw[k] * pi[(int64_t)k * b.Dmax];
    return log(p);
}

// ---- joint MAP: joint_map_from_belief_params (osi/mixture_beliefs.py:771-867) with get_multivar_gm_mode(init_xs=[xc])
// (osi/utils.py:101-161), one start per group of lanes ----------------------------------------------------------------------
// Coordinate ascent on the joint log density: projected gradient ascent with Polyak averaging in the continuous block, then
// one sweep over the discrete variables, each set to the first state of largest joint density.  The reference's decisions
// are kept one by one (docs/kernels_mixture.md lists them).  Every sum over the continuous variables is formed in ONE fixed
// order whatever the number of lanes: JM_CH chunk sums (chunk c: n = c, c + JM_CH, ... ascending), then the chunks in index
// order.  Chunk c, and with it x[n] of its variables, belongs to lane c mod lanes; component k to lane k mod lanes.  Every
// decision is taken by every lane from the same shared values, so all lanes reach every ctx.sync().
constexpr int JM_CH = 64;

struct JointArgs {
    int Nc, Nd;
    const int32_t *crows, *drows;       // [Nc] / [Nd] rows of the belief
    const double *lo, *hi;              // [Nc] bounds
    const double* logw;                 // [K] log weights of the mixture
    int coord_its, grad_its;
    double gamma, grad_lr, tol;
};

struct HostLanes {
    int lane = 0, lanes = 1;
    void sync() const {}
};

LHVI_HD int joint_ws_doubles(int K, int Nc, int Nd, int Dmax) { return 4 * Nc + (6 + JM_CH) * K + JM_CH + Dmax + (Nd + 1) / 2 + 1; }

struct JointWs {
    double *x, *xin, *xent, *xout, *consts, *tk, *ek, *gw, *xdclp, *tmplw, *redk, *red1, *objs;
    int32_t* xd;
};
LHVI_HD JointWs joint_carve(double* W, int K, int Nc, int Dmax) {
    JointWs w;
    w.x = W, w.xin = w.x + Nc, w.xent = w.xin + Nc, w.xout = w.xent + Nc, w.consts = w.xout + Nc, w.tk = w.consts + K;
    w.ek = w.tk + K, w.gw = w.ek + K, w.xdclp = w.gw + K, w.tmplw = w.xdclp + K, w.redk = w.tmplw + K;
    w.red1 = w.redk + JM_CH * K, w.objs = w.red1 + JM_CH;
    w.xd = reinterpret_cast<int32_t*>(w.objs + Dmax);
    return w;
}

template <class Ctx>
LHVI_HD double chunk_sum(const double* red, int stride, const Ctx&) {
    double s = 0.0;
    for (int c = 0; c < JM_CH; ++c) s += red[(int64_t)c * stride];
    return s;
}

// one call of get_multivar_gm_mode from w.x under the log weights w.tmplw: on return w.x is its best point, the value its
// objective there; `moved`: some bit of x differs from the entry point
template <class Ctx>
LHVI_HD double joint_ascent(const lhvi_mix_t& b, const JointArgs& a, const JointWs& w, const Ctx& ctx, bool& moved) {
    const int K = b.K, Nc = a.Nc;
    double best = NEG_INF, prev = NEG_INF, step = a.grad_lr;
    for (int c = ctx.lane; c < JM_CH; c += ctx.lanes)
        for (int n = c; n < Nc; n += JM_CH) w.xent[n] = w.xin[n] = w.x[n];
    for (int it = 0; it < a.grad_its; ++it) {
        for (int c = ctx.lane; c < JM_CH; c += ctx.lanes)
            for (int k = 0; k < K; ++k) {
                double p = 0.0;
                for (int n = c; n < Nc; n += JM_CH) {
                    const double* r = b.rec + ((int64_t)a.crows[n] * K + k) * 3;
                    const double d = w.x[n] - r[1];
                    p += d * d * r[2];
                }
                w.redk[c * K + k] = p;
            }
        ctx.sync();
        for (int k = ctx.lane; k < K; k += ctx.lanes) w.tk[k] = w.tmplw[k] + (w.consts[k] - 0.5 * chunk_sum(w.redk + k, K, ctx));
        ctx.sync();
        double mx = NEG_INF;
        for (int k = 0; k < K; ++k) mx = fmax(mx, w.tk[k]);
        for (int k = ctx.lane; k < K; k += ctx.lanes) w.ek[k] = exp(w.tk[k] - mx);
        ctx.sync();
        double s = 0.0;
        for (int k = 0; k < K; ++k) s += w.ek[k];
        const double obj = log(s) + mx;
        for (int k = ctx.lane; k < K; k += ctx.lanes) w.gw[k] = exp(w.tk[k] - obj);
        ctx.sync();
        const bool better_now = obj > best, back = obj <= prev;
        if (better_now) best = obj;
        if (back) step *= 0.5;            // after a step that did not improve: back to the best point, half the step; the
        for (int c = ctx.lane; c < JM_CH; c += ctx.lanes) {       // weights gw stay those of the rejected point
            double q = 0.0;
            for (int n = c; n < Nc; n += JM_CH) {
                if (better_now) w.xin[n] = w.x[n];
                const double xn = back ? w.xin[n] : w.x[n];
                double dx = 0.0;
                for (int k = 0; k < K; ++k) {
                    const double* r = b.rec + ((int64_t)a.crows[n] * K + k) * 3;
                    dx += w.gw[k] * ((r[1] - xn) * r[2]);
                }
                q += dx * dx;
                w.x[n] = a.gamma * xn + (1.0 - a.gamma) * clip(xn + dx * step, a.lo[n], a.hi[n]);
            }
            w.red1[c] = q;
        }
        ctx.sync();
        const double nrm = sqrt(chunk_sum(w.red1, 1, ctx));
        const bool stop = nrm < a.tol || fabs((obj - prev) / prev) < a.tol;      // prev = -inf: NaN, hence false
        ctx.sync();
        if (stop) break;
        prev = obj;
    }
    for (int c = ctx.lane; c < JM_CH; c += ctx.lanes) {
        double flag = 0.0;
        for (int n = c; n < Nc; n += JM_CH) {
            w.x[n] = w.xin[n];
            if (__builtin_bit_cast(uint64_t, w.x[n]) != __builtin_bit_cast(uint64_t, w.xent[n])) flag = 1.0;
        }
        w.red1[c] = flag;
    }
    ctx.sync();
    moved = chunk_sum(w.red1, 1, ctx) != 0.0;
    ctx.sync();
    return best;
}

// one start: x0 [Nc] (not clipped), xd0 [Nd]; outputs xc [Nc] (the continuous point of the best coordinate iteration), xd [Nd]
// (the LAST sweep's: the reference's best_xd aliases xd, :848) and the best objective
template <class Ctx>
LHVI_HD void joint_start(const lhvi_mix_t& b, const JointArgs& a, const double* x0, const int32_t* xd0, double* W, const Ctx& ctx,
                         double* xc_out, int32_t* xd_out, double* obj_out) {
    const int K = b.K, Nc = a.Nc, Nd = a.Nd;
    const JointWs w = joint_carve(W, K, Nc, b.Dmax);
    for (int c = ctx.lane; c < JM_CH; c += ctx.lanes) {
        for (int n = c; n < Nc; n += JM_CH) w.x[n] = w.xout[n] = x0[n];
        for (int k = 0; k < K; ++k) {
            double p = 0.0;
            for (int n = c; n < Nc; n += JM_CH) p += b.rec[((int64_t)a.crows[n] * K + k) * 3];
            w.redk[c * K + k] = p;
        }
    }
    for (int n = ctx.lane; n < Nd; n += ctx.lanes) w.xd[n] = xd0[n];
    ctx.sync();
    for (int k = ctx.lane; k < K; k += ctx.lanes) {
        w.consts[k] = chunk_sum(w.redk + k, K, ctx);
        double p = 0.0;
        for (int n = 0; n < Nd; ++n) p += b.lpi[((int64_t)a.drows[n] * K + k) * b.Dmax + w.xd[n]];
        w.xdclp[k] = p;
    }
    ctx.sync();
    double best_obj = NEG_INF, obj = NEG_INF;
    for (int it = 0; it < a.coord_its; ++it) {
        bool changed = false;
        if (Nc) {
            for (int k = ctx.lane; k < K; k += ctx.lanes) w.tmplw[k] = Nd ? a.logw[k] + w.xdclp[k] : a.logw[k];
            ctx.sync();
            obj = joint_ascent(b, a, w, ctx, changed);
        }
        if (Nd) {
            if (Nc) {
                for (int c = ctx.lane; c < JM_CH; c += ctx.lanes)
                    for (int k = 0; k < K; ++k) {
                        double p = 0.0;
                        for (int n = c; n < Nc; n += JM_CH) p += cont_term(b.rec + ((int64_t)a.crows[n] * K + k) * 3, w.x[n]);
                        w.redk[c * K + k] = p;
                    }
                ctx.sync();
            }
            for (int k = ctx.lane; k < K; k += ctx.lanes) w.tmplw[k] = Nc ? a.logw[k] + chunk_sum(w.redk + k, K, ctx) : a.logw[k];
            ctx.sync();
            for (int n = 0; n < Nd; ++n) {
                const int row = a.drows[n], ns = b.nstates[row], cur = w.xd[n];
                const double* lp = b.lpi + (int64_t)row * K * b.Dmax;
                for (int k = ctx.lane; k < K; k += ctx.lanes) w.xdclp[k] -= lp[(int64_t)k * b.Dmax + cur];
                ctx.sync();
                for (int s = ctx.lane; s < ns; s += ctx.lanes) {
                    double mx = NEG_INF;
                    for (int k = 0; k < K; ++k) mx = fmax(mx, w.tmplw[k] + (w.xdclp[k] + lp[(int64_t)k * b.Dmax + s]));
                    double e = 0.0;
                    for (int k = 0; k < K; ++k) e += exp(w.tmplw[k] + (w.xdclp[k] + lp[(int64_t)k * b.Dmax + s]) - mx);
                    w.objs[s] = log(e) + mx;
                }
                ctx.sync();
                int pick = 0;
                for (int s = 1; s < ns; ++s)
                    if (w.objs[s] > w.objs[pick]) pick = s;
                obj = w.objs[pick];
                changed = changed || pick != cur;
                for (int k = ctx.lane; k < K; k += ctx.lanes) w.xdclp[k] += lp[(int64_t)k * b.Dmax + pick];
                if (ctx.lane == 0) w.xd[n] = pick;
                ctx.sync();
            }
        }
        if (obj > best_obj) {
            best_obj = obj;
            for (int c = ctx.lane; c < JM_CH; c += ctx.lanes)
                for (int n = c; n < Nc; n += JM_CH) w.xout[n] = w.x[n];
        }
        if (!changed) break;        // the remaining iterations would repeat this one: neither xd nor a bit of xc moved
    }
    ctx.sync();
    for (int c = ctx.lane; c < JM_CH; c += ctx.lanes)
        for (int n = c; n < Nc; n += JM_CH) xc_out[n] = w.xout[n];
    for (int n = ctx.lane; n < Nd; n += ctx.lanes) xd_out[n] = w.xd[n];
    if (ctx.lane == 0) *obj_out = best_obj;
}

}  // namespace mix
}  // namespace lhvi
