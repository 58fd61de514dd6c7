// npvi.hpp -- the arithmetic of nonparametric variational inference (osi/NPVI.py, osi/mixture_beliefs.py), written once for the
// device (csrc/npvi.hip) and the host (lhvi_npvi_*_host: one "lane").  docs/kernels_npvi.md has the formulas.
//
// factor_item: one factor.  A lane owns NM mixture components (device: one, the lanes of a group are the components; host: all of
// them).  Per grid k the group fills the node positions and coefficients of every axis slot (x, c: shared by the group), each lane
// the values q of its own components at those nodes, so that a grid node costs K * arity multiplications and no exponential.  At a
// node the lanes' terms w_m prod_i q_im are added over the group (Ctx::sum_m) into the belief b; each lane then adds
// omega w_m prod_{j != i} q_jm / b into its own accumulator z of the node's slot on every hidden axis i.  After the grid the
// continuous axes' accumulators are folded into d/d mu and d/d log var (the nodes move with k); the discrete ones keep adding
// over the K grids (their nodes are the states) and are d/d pi as they stand.
//
// Ctx: NM; gl, gn (lane of the group, lanes of the group: who fills which slot of x / c); m(i) the i-th component of the lane;
// x(s), c(s) group tables; q(i, s), z(i, s) lane tables; sum_m(v) the group's total; sync() group barrier; point(), point_idx(),
// stack(): where the lane keeps the node it evaluates the potential at and the formula interpreter's stack (device: LDS, so that
// the evaluators' dynamic indexing costs no scratch memory).
#pragma once
#include "potential.hpp"

#define LHVI_HD __host__ __device__ __forceinline__

namespace lhvi {
namespace npvi {

constexpr int MAX_K = LHVI_NPVI_MAX_K;
constexpr int MAXA = LHVI_MAX_ARITY;
constexpr int SLOTS = LHVI_NPVI_MAX_SLOTS;
constexpr double INV_SQRT_2PI = 0.3989422804014327;
constexpr double HALF_LOG_2PI = 0.9189385332046727;

LHVI_HD double gauss_pdf(double x, double mu, double var) {
    const double iv = 1.0 / var, d = x - mu;
    return INV_SQRT_2PI * sqrt(iv) * exp(-0.5 * (d * d) * iv);
}

template <bool INTERP, class Stack>
LHVI_HD double neg_log_phi(int kind, const double* __restrict__ par, const double* x, const int* idx, Stack& st) {
    bool is_log;
    const double v = pot_eval_on<INTERP>(kind, par, x, idx, is_log, st);
    return is_log ? -v : -log(v);
}

struct HostCtx {
    static constexpr int NM = MAX_K;
    int gl = 0, gn = 1;
    double xt[SLOTS], ct[SLOTS], qt[MAX_K][SLOTS], zt[MAX_K][SLOTS];
    double px[MAXA];
    int pi[MAXA];
    MlnRegStack st;
    double* point() { return px; }
    int* point_idx() { return pi; }
    MlnRegStack& stack() { return st; }
    int m(int i) const { return i; }
    double& x(int s) { return xt[s]; }
    double& c(int s) { return ct[s]; }
    double& q(int i, int s) { return qt[i][s]; }
    double& z(int i, int s) { return zt[i][s]; }
    double sum_m(double v) const { return v; }
    void sync() const {}
};

// A per-lane predicate that lives across the loops below is kept by the compiler as a 64-bit lane mask in a scalar register pair; a
// dozen of them (hidden / continuous / present, per argument, and their conjunctions) overflow the scalar file and are spilled.
// The kinds of the arguments are therefore kept as small integers in vector registers and compared where they are used: opaque()
// hides the value from the optimiser so that the comparison is not hoisted out of the loop again.
LHVI_HD int opaque(int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(v));
#endif
    return v;
}
// the same for a pointer that is needed again only after the loops (the output arrays): parked in a vector register pair
template <class T>
LHVI_HD T* opaque_ptr(T* q) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(q));
#endif
    return q;
}
#define NPVI_IN(a) (opaque(ty[a]) != 0)
#define NPVI_HID(a) (opaque(ty[a]) >= 2)
#define NPVI_CONT(a) (opaque(ty[a]) == 3)

// pe_c [E][K][2], pe_d [E][K][Dmax], pf [F][K + 1] (d aux / d w_m of the factor, then its objective)
// MA, SCAP: the arity and the slots this build serves (a longer factor is reported through its objective); INTERP: formulas without a
// conditional-quadratic block are interpreted (lhvi_pots_t.interpreted != 0); BFE: the expectant is -log phi + log b (OneShot's Bethe
// free energy, csrc/oneshot.hip) instead of -log phi
template <int MA, bool INTERP, int SCAP, bool BFE = false, class Ctx>
LHVI_HD void factor_item(const lhvi_graph_t& g, const lhvi_pots_t& pots, const lhvi_vi_t& p, const double* __restrict__ fac_count,
                         int f, Ctx& ctx, double* pe_c, double* pe_d, double* pf) {
    constexpr int NM = Ctx::NM;
    const int K = p.K;
    pe_c = opaque_ptr(pe_c), pe_d = opaque_ptr(pe_d), pf = opaque_ptr(pf);
    const int base = g.fac_ptr[f], arity = g.fac_ptr[f + 1] - base;
    int vars[MA], len[MA], off[MA], fix[MA], dom[MA];
    int ty[MA];             // 0 no such argument, 1 observed, 2 hidden discrete, 3 hidden continuous (read through NPVI_*: see opaque)
    int S = 0, G = 1;
#pragma unroll
    for (int a = 0; a < MA; ++a) {
        const bool in = a < arity;
        const int32_t* r = p.edge_axis + 4 * (int64_t)(base + (in ? a : 0));
        vars[a] = in ? r[0] : 0;
        const int word = in ? r[1] : 1;
        len[a] = word & 0xffff;
        fix[a] = in ? r[2] : 0;
        dom[a] = in ? r[3] : 0;
        const bool hidden = in && ((word >> 16) & 1);
        ty[a] = !in ? 0 : !hidden ? 1 : ((word >> 17) & 1) ? 3 : 2;
        if (!hidden) len[a] = 1;
        off[a] = S;
        if (in) { S += len[a]; G *= len[a]; }
    }
    const double cf = fac_count ? fac_count[f] : 1.0;
    if (arity > MA || S > SCAP) {                 // (uniform over the group) not served: the objective says so
        for (int i = 0; i < NM; ++i) {
            const int m = ctx.m(i);
            if (m < K) pf[(int64_t)f * (K + 1) + m] = 0.0;
            if (m == 0) pf[(int64_t)f * (K + 1) + K] = NAN;
        }
#pragma unroll
        for (int a = 0; a < MA; ++a)
            for (int i = 0; i < NM; ++i) {
                const int m = ctx.m(i);
                if (m >= K || !NPVI_HID(a)) continue;
                const int64_t row = (int64_t)(base + a) * K + m;
                if (NPVI_CONT(a)) { pe_c[2 * row] = 0.0; pe_c[2 * row + 1] = 0.0; }
                else _Pragma("unroll 1") for (int t = 0; t < len[a]; ++t) pe_d[row * p.Dmax + t] = 0.0;
            }
        return;
    }
    const int pot = g.fac_pot[f];
    const int kind = pots.kind[pot];
    const double* __restrict__ par = pots.param + pots.off[pot];

    double gmu[NM][MA], glv[NM][MA], gw[NM];
    double obj = 0.0;
#pragma unroll
    for (int i = 0; i < NM; ++i) {
        gw[i] = 0.0;
#pragma unroll
        for (int a = 0; a < MA; ++a) { gmu[i][a] = 0.0; glv[i][a] = 0.0; }
        _Pragma("unroll 1") for (int s = 0; s < S; ++s) ctx.z(i, s) = 0.0;
    }
    double* x = ctx.point();
    int* idx = ctx.point_idx();
    for (int k = 0; k < K; ++k) {
        // ---- the group's tables: node positions and coefficients of grid k
        for (int s = ctx.gl; s < S; s += ctx.gn) {
            int v = 0, o = 0, d = 0; bool h = false, c = false;
#pragma unroll
            for (int b = 0; b < MA; ++b) if (NPVI_IN(b) && s >= off[b]) { v = vars[b]; o = off[b]; d = dom[b]; h = NPVI_HID(b); c = NPVI_CONT(b); }
            const int t = s - o;
            double xv, cv;
            if (h && c) {
                const double* e = p.eta_c + ((int64_t)v * K + k) * 2;
                xv = sqrt(2.0 * e[1]) * p.gh_x[t] + e[0];
                cv = p.gh_w[t];
            } else if (h) {
                xv = g.dom_val[d + t];
                cv = p.eta_d[((int64_t)v * K + k) * p.Dmax + t];
            } else {
                xv = g.var_value[v];
                cv = 1.0;
            }
            ctx.x(s) = xv; ctx.c(s) = cv;
        }
        ctx.sync();
        // ---- the lane's tables: its components at those nodes
#pragma unroll
        for (int i = 0; i < NM; ++i) {
            const int m = ctx.m(i);
            if (m >= K) continue;
            _Pragma("unroll 1") for (int s = 0; s < S; ++s) {
                int v = 0, o = 0; bool h = false, c = false;
#pragma unroll
                for (int b = 0; b < MA; ++b) if (NPVI_IN(b) && s >= off[b]) { v = vars[b]; o = off[b]; h = NPVI_HID(b); c = NPVI_CONT(b); }
                double qv = 1.0;
                if (h && c) {
                    const double* e = p.eta_c + ((int64_t)v * K + m) * 2;
                    qv = gauss_pdf(ctx.x(s), e[0], e[1]);
                    ctx.z(i, s) = 0.0;
                } else if (h) {
                    qv = p.eta_d[((int64_t)v * K + m) * p.Dmax + (s - o)];
                }
                ctx.q(i, s) = qv;
            }
        }
        // ---- the grid
        const double wk = p.w[k];
        _Pragma("unroll 1") for (int node = 0; node < G; ++node) {
            int it[MA];
            double coef = 1.0;
            int r = node;
#pragma unroll
            for (int a = MA - 1; a >= 0; --a) {
                it[a] = 0;
                if (NPVI_IN(a)) { const int n = opaque(len[a]); it[a] = r % n; r /= n; }
            }
#pragma unroll
            for (int a = 0; a < MA; ++a) {
                if (!NPVI_IN(a)) continue;
                x[a] = ctx.x(off[a] + it[a]);
                coef *= ctx.c(off[a] + it[a]);
                idx[a] = NPVI_HID(a) ? (NPVI_CONT(a) ? 0 : it[a]) : fix[a];
            }
            double F = neg_log_phi<INTERP>(kind, par, x, idx, ctx.stack());
            double omega = (wk * coef) * F;
            if constexpr (!BFE) obj += omega;
            double pm[NM], loo[NM][MA];
            double mine = 0.0;
#pragma unroll
            for (int i = 0; i < NM; ++i) {
                pm[i] = 0.0;
                const int m = ctx.m(i);
                if (m >= K) continue;
                double qa[MA], pre = 1.0, suf = 1.0;
#pragma unroll
                for (int a = 0; a < MA; ++a) {
                    qa[a] = NPVI_HID(a) ? ctx.q(i, off[a] + it[a]) : 1.0;
                    loo[i][a] = pre;
                    pre *= qa[a];
                }
#pragma unroll
                for (int a = MA - 1; a >= 0; --a) { loo[i][a] *= suf; suf *= qa[a]; }
                pm[i] = pre;
                mine += p.w[m] * pre;
            }
            const double b = ctx.sum_m(mine);
            if constexpr (BFE) {            // every lane has b now: the expectant takes log b in
                F += log(b);
                omega = (wk * coef) * F;
                obj += omega;
            }
            const double rb = omega / b;
#pragma unroll
            for (int i = 0; i < NM; ++i) {
                const int m = ctx.m(i);
                if (m >= K) continue;
                gw[i] += rb * pm[i];
                const double rw = rb * p.w[m];
#pragma unroll
                for (int a = 0; a < MA; ++a) if (NPVI_HID(a)) ctx.z(i, off[a] + it[a]) += rw * loo[i][a];
            }
        }
        // ---- continuous axes: the accumulators of this grid into d / d mu, d / d log var
#pragma unroll
        for (int i = 0; i < NM; ++i) {
            const int m = ctx.m(i);
            if (m >= K) continue;
#pragma unroll
            for (int a = 0; a < MA; ++a) {
                if (!(NPVI_HID(a) && NPVI_CONT(a))) continue;
                const double* e = p.eta_c + ((int64_t)vars[a] * K + m) * 2;
                const double mu = e[0], var = e[1];
                _Pragma("unroll 1") for (int t = 0; t < len[a]; ++t) {
                    const int s = off[a] + t;
                    const double zq = ctx.z(i, s) * ctx.q(i, s), d = ctx.x(s) - mu;
                    gmu[i][a] += zq * d / var;
                    glv[i][a] += zq * (0.5 * (d * d / var - 1.0));
                }
            }
        }
        ctx.sync();             // the next grid overwrites the group's tables
    }
    // ---- a variable that fills several positions: everything on its first one (the gather reads one row per (factor, variable))
#pragma unroll
    for (int a = 1; a < MA; ++a) {
        if (!NPVI_HID(a)) continue;
        int first = a;
#pragma unroll
        for (int b = MA - 1; b >= 0; --b) if (b < a && NPVI_HID(b) && vars[b] == vars[a]) first = b;
        if (first == a) continue;
#pragma unroll
        for (int i = 0; i < NM; ++i) {
            if (ctx.m(i) >= K) continue;
#pragma unroll
            for (int b = 0; b < MA; ++b)
                if (b == first) {
                    gmu[i][b] += gmu[i][a]; glv[i][b] += glv[i][a];
                    if (!NPVI_CONT(a)) _Pragma("unroll 1") for (int t = 0; t < len[a]; ++t) { ctx.z(i, off[b] + t) += ctx.z(i, off[a] + t); ctx.z(i, off[a] + t) = 0.0; }
                }
            gmu[i][a] = 0.0; glv[i][a] = 0.0;
        }
    }
#pragma unroll
    for (int i = 0; i < NM; ++i) {
        const int m = ctx.m(i);
        if (m >= K) continue;
        pf[(int64_t)f * (K + 1) + m] = cf * gw[i];
        if (m == 0) pf[(int64_t)f * (K + 1) + K] = cf * obj;
#pragma unroll
        for (int a = 0; a < MA; ++a) {
            if (!NPVI_HID(a)) continue;
            const int64_t row = (int64_t)(base + a) * K + m;
            if (NPVI_CONT(a)) { pe_c[2 * row] = cf * gmu[i][a]; pe_c[2 * row + 1] = cf * glv[i][a]; }
            else _Pragma("unroll 1") for (int t = 0; t < len[a]; ++t) pe_d[row * p.Dmax + t] = cf * ctx.z(i, off[a] + t);
        }
    }
}

#undef NPVI_IN
#undef NPVI_HID
#undef NPVI_CONT

// ---- entropy bound ------------------------------------------------------------------------------------------------------------
struct VarInfo { bool hidden, cont; int n; };
LHVI_HD VarInfo var_info(const lhvi_graph_t& g, int v) {
    const int d = g.var_dom[v];
    const double val = g.var_value[v];
    return VarInfo{val != val, g.dom_cont[d] != 0, g.dom_ptr[d + 1] - g.dom_ptr[d]};
}

// l_v(k, j): the log of the integral of q_vk q_vj (mixture_beliefs.py:911-930)
LHVI_HD double ent_pair(const lhvi_vi_t& p, int v, const VarInfo& vi, int k, int j) {
    if (vi.cont) {
        const double* ek = p.eta_c + ((int64_t)v * p.K + k) * 2;
        const double* ej = p.eta_c + ((int64_t)v * p.K + j) * 2;
        const double s = ek[1] + ej[1], d = ek[0] - ej[0];
        return -HALF_LOG_2PI - 0.5 * log(s) - 0.5 * (d * d / s);
    }
    const double* pk = p.eta_d + ((int64_t)v * p.K + k) * p.Dmax;
    const double* pj = p.eta_d + ((int64_t)v * p.K + j) * p.Dmax;
    double dot = 0.0;
    for (int t = 0; t < vi.n; ++t) dot += pk[t] * pj[t];
    return log(dot);
}

// row k of the K x K part: lse_k = logsumexp_j(L[k][j] + log w_j), U[k][j] = w_k exp(L[k][j]) / sum_j' exp(L[k][j']) w_j'
// (so that S[k][j] = U[k][j] w_j is w_k softmax_j, and d neg_ent / d w_j = lse_j + sum_k U[k][j]).  Lt: the lower triangle, row-major.
LHVI_HD int tri(int k, int j) { return k >= j ? k * (k + 1) / 2 + j : j * (j + 1) / 2 + k; }
LHVI_HD double ent_row(int K, const double* Lt, const double* w, int k, double* U) {
    double mx = -__builtin_huge_val();
    for (int j = 0; j < K; ++j) { const double a = Lt[tri(k, j)] + log(w[j]); mx = a > mx ? a : mx; }
    double den = 0.0;
    for (int j = 0; j < K; ++j) { const double e = exp(Lt[tri(k, j)] - mx); U[k * K + j] = e; den += e * w[j]; }
    // (exp(L - mx) w_j = exp(L + log w_j - mx))
    for (int j = 0; j < K; ++j) U[k * K + j] = w[k] * U[k * K + j] / den;
    return mx + log(den);
}

// g_tau and obj from the factors' totals (sum_f pf[f][.]: tot [K + 1]), the rows' lse and U; SS = S + S^T for the gather
LHVI_HD void finish_weights(int K, const double* tot, const double* w, const double* lse, const double* U, double* SS, double* obj,
                            double* g_tau) {
    double gw[MAX_K], dot = 0.0, ne = 0.0;
    for (int k = 0; k < K; ++k) {
        double col = 0.0;
        for (int i = 0; i < K; ++i) col += U[i * K + k];
        gw[k] = tot[k] + (lse[k] + col);
        dot += w[k] * gw[k];
        ne += w[k] * lse[k];
    }
    for (int k = 0; k < K; ++k) g_tau[k] = w[k] * (gw[k] - dot);
    for (int k = 0; k < K; ++k)
        for (int j = 0; j < K; ++j) SS[k * K + j] = U[k * K + j] * w[j] + U[j * K + k] * w[k];
    obj[0] = tot[K] + ne;
}

// the gradient rows of (v, m) from the sums over the variable's edges: c0, c1 (continuous) or the raw d / d pi already in
// g_rho[v][m][:] (discrete); adds the entropy term through SS and chains a discrete row through its softmax.
// BFE: SS is instead the variable term's rows (oneshot.hpp's var_item), [V][K][2] followed by [V][K][Dmax], added as they stand
template <bool BFE = false>
LHVI_HD void gather_finish(const lhvi_graph_t& g, const lhvi_vi_t& p, const double* __restrict__ var_count, const double* __restrict__ SS,
                           int v, int m, const VarInfo& vi, double c0, double c1, double* __restrict__ g_c, double* __restrict__ g_rho) {
    const int K = p.K;
    const int64_t row = (int64_t)v * K + m;
    const double cv = var_count ? var_count[v] : 1.0;
    if (!vi.hidden) {
        g_c[2 * row] = 0.0; g_c[2 * row + 1] = 0.0;
        for (int t = 0; t < p.Dmax; ++t) g_rho[row * p.Dmax + t] = 0.0;
        return;
    }
    if constexpr (BFE) {
        const double* __restrict__ pv_d = SS + (int64_t)g.V * K * 2;
        if (vi.cont) {
            g_c[2 * row] = c0 + SS[2 * row];
            g_c[2 * row + 1] = c1 + SS[2 * row + 1];
            for (int t = 0; t < p.Dmax; ++t) g_rho[row * p.Dmax + t] = 0.0;
            return;
        }
        g_c[2 * row] = 0.0; g_c[2 * row + 1] = 0.0;
        const double* pk = p.eta_d + row * p.Dmax;
        double* gr = g_rho + row * p.Dmax;
        double dot = 0.0;
        for (int t = 0; t < vi.n; ++t) { gr[t] += pv_d[row * p.Dmax + t]; dot += pk[t] * gr[t]; }
        for (int t = 0; t < vi.n; ++t) gr[t] = pk[t] * (gr[t] - dot);
        for (int t = vi.n; t < p.Dmax; ++t) gr[t] = 0.0;
        return;
    }
    if (vi.cont) {
        const double* ek = p.eta_c + row * 2;
        double em = 0.0, ev = 0.0;
        for (int j = 0; j < K; ++j) {
            const double* ej = p.eta_c + ((int64_t)v * K + j) * 2;
            const double s = ek[1] + ej[1], d = ek[0] - ej[0], co = SS[m * K + j] * cv;
            em += co * (-d / s);
            ev += co * (-0.5 / s + 0.5 * (d * d) / (s * s));
        }
        g_c[2 * row] = c0 + em;
        g_c[2 * row + 1] = c1 + ev * ek[1];
        for (int t = 0; t < p.Dmax; ++t) g_rho[row * p.Dmax + t] = 0.0;
        return;
    }
    g_c[2 * row] = 0.0; g_c[2 * row + 1] = 0.0;
    const double* pk = p.eta_d + row * p.Dmax;
    double* gr = g_rho + row * p.Dmax;
    for (int j = 0; j < K; ++j) {
        const double* pj = p.eta_d + ((int64_t)v * K + j) * p.Dmax;
        double dot = 0.0;
        for (int t = 0; t < vi.n; ++t) dot += pk[t] * pj[t];
        const double co = SS[m * K + j] * cv / dot;
        for (int t = 0; t < vi.n; ++t) gr[t] += co * pj[t];
    }
    double dot = 0.0;
    for (int t = 0; t < vi.n; ++t) dot += pk[t] * gr[t];
    for (int t = 0; t < vi.n; ++t) gr[t] = pk[t] * (gr[t] - dot);
    for (int t = vi.n; t < p.Dmax; ++t) gr[t] = 0.0;
}

// ---- update -------------------------------------------------------------------------------------------------------------------
struct Step { double lr_t, b1, b2, eps; int fix_mix; };
LHVI_HD double tf_adam(double th, double& m, double& s, double gr, const Step& a) {
    m = a.b1 * m + (1.0 - a.b1) * gr;
    s = a.b2 * s + (1.0 - a.b2) * (gr * gr);
    return th - a.lr_t * m / (sqrt(s) + a.eps);
}
LHVI_HD double clip(double x, double lo, double hi) { return fmin(fmax(x, lo), hi); }

LHVI_HD void update_tau(int K, const lhvi_npvi_opt_t& o, const Step& a) {
    double mx = -__builtin_huge_val();
    for (int k = 0; k < K; ++k) {
        double t = tf_adam(o.tau[k], o.m_tau[k], o.s_tau[k], o.g_tau[k], a);
        if (a.fix_mix) t = 0.0;
        o.tau[k] = t;
        mx = t > mx ? t : mx;
    }
    double den = 0.0;
    for (int k = 0; k < K; ++k) den += exp(o.tau[k] - mx);
    for (int k = 0; k < K; ++k) o.w[k] = exp(o.tau[k] - mx) / den;
}

LHVI_HD void update_row(const lhvi_graph_t& g, int K, int Dmax, const lhvi_npvi_opt_t& o, const Step& a, int v, int m) {
    const VarInfo vi = var_info(g, v);
    if (!vi.hidden) return;
    const int64_t row = (int64_t)v * K + m;
    if (vi.cont) {
        double mu = tf_adam(o.theta_c[2 * row], o.m_c[2 * row], o.s_c[2 * row], o.g_c[2 * row], a);
        double lv = tf_adam(o.theta_c[2 * row + 1], o.m_c[2 * row + 1], o.s_c[2 * row + 1], o.g_c[2 * row + 1], a);
        mu = clip(mu, o.mu_lo[v], o.mu_hi[v]);
        lv = clip(lv, o.lvar_lo, o.lvar_hi);
        o.theta_c[2 * row] = mu; o.theta_c[2 * row + 1] = lv;
        o.eta_c[2 * row] = mu; o.eta_c[2 * row + 1] = exp(lv);
        return;
    }
    double* rho = o.rho + row * Dmax;
    double* pi = o.eta_d + row * Dmax;
    double mx = -__builtin_huge_val();
    for (int t = 0; t < vi.n; ++t) {
        const double r = tf_adam(rho[t], o.m_rho[row * Dmax + t], o.s_rho[row * Dmax + t], o.g_rho[row * Dmax + t], a);
        rho[t] = r;
        mx = r > mx ? r : mx;
    }
    double den = 0.0;
    for (int t = 0; t < vi.n; ++t) den += exp(rho[t] - mx);
    for (int t = 0; t < vi.n; ++t) pi[t] = exp(rho[t] - mx) / den;
}

}  // namespace npvi
}  // namespace lhvi
