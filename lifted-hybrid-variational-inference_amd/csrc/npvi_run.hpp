// npvi_run.hpp -- the host side that csrc/npvi.hip and csrc/oneshot.hip share: the workspace's common prefix and its carving, the
// argument checks, the host gather over a variable's edges, the Adam loop on the device and on the host, and the bodies of the
// eight entry points.  A solver describes its objective in a struct O:
//   O::VAR_COEF                 whether the objective reads the extra input var_coef (a null one is then refused)
//   O::Ws, O::carve(g, p, c)    the workspace: WsPrefix plus the solver's own tail, taken from the Carver in layout order
//   O::grad_device(g, pots, p, a, w, st)      enqueues one objective and gradient;  O::grad_host(g, pots, p, a, w): its host twin
#pragma once
#include "npvi_dev.hpp"

namespace lhvi {
namespace npvi {

// what one gradient reads and writes beside the graph and the belief; var_coef is OneShot's
struct GradArgs {
    const double *var_count, *fac_count, *var_coef;
    int32_t max_slots, max_arity;
    double *obj, *g_tau, *g_c, *g_rho;
};

// hands out 256-byte aligned pieces of a workspace in order; without a base it only counts
struct Carver {
    char* base;
    size_t off = 0;
    double* take(size_t bytes) {
        double* at = base ? reinterpret_cast<double*>(base + off) : nullptr;
        off += (bytes + 255) & ~(size_t)255;
        return at;
    }
};

// pe_c [E][K][2], pe_d [E][K][Dmax], pf [F][K + 1], partF [nbF][K + 1]; nbV blocks of variables for the solver's partV
struct WsPrefix { double *pe_c, *pe_d, *pf, *partF; int nbF, nbV; };
inline WsPrefix carve_prefix(const lhvi_graph_t* g, const lhvi_vi_t* p, Carver& c) {
    const size_t K = (size_t)p->K, D = (size_t)(p->Dmax < 1 ? 1 : p->Dmax), E = (size_t)(g->E < 1 ? 1 : g->E);
    const int nbF = (int)grid_for(g->F), nbV = (int)grid_for(g->V);
    double* pe_c = c.take(E * K * 2 * sizeof(double));
    double* pe_d = c.take(E * K * D * sizeof(double));
    double* pf = c.take((size_t)(g->F < 1 ? 1 : g->F) * (K + 1) * sizeof(double));
    double* partF = c.take((size_t)nbF * (K + 1) * sizeof(double));
    return WsPrefix{pe_c, pe_d, pf, partF, nbF, nbV};
}

template <class O>
inline size_t workspace_bytes(const lhvi_graph_t* g, const lhvi_vi_t* p) {
    if (!g || !p || p->K < 1 || p->K > LHVI_NPVI_MAX_K) return 0;
    Carver c{nullptr};
    O::carve(g, p, c);
    return c.off;
}

template <class O>
inline typename O::Ws carve(const lhvi_graph_t* g, const lhvi_vi_t* p, void* ws) {
    Carver c{static_cast<char*>(ws)};
    return O::carve(g, p, c);
}

template <class O>
inline int check_grad(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const GradArgs& a) {
    if (!g || !pots || !p || !a.obj || !a.g_tau || !a.g_c || !a.g_rho || (O::VAR_COEF && !a.var_coef)) return LHVI_E_ARG;
    if (p->K < 1 || p->K > LHVI_NPVI_MAX_K || p->T < 1 || p->Dmax < 1 || g->V < 1 || g->F < 0) return LHVI_E_ARG;
    if (!p->gh_x || !p->gh_w || !p->w || !p->eta_c || !p->eta_d || (g->E > 0 && !p->edge_axis) || p->obs_var) return LHVI_E_ARG;
    return LHVI_OK;
}

// the checks of a run; on success `a` is the gradient's arguments of every update but obj
template <class O>
inline int check_run(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const lhvi_npvi_opt_t* o, const double* var_coef,
                     int32_t iterations, GradArgs& a) {
    if (!o || iterations < 0) return LHVI_E_ARG;
    if (!o->tau || !o->theta_c || !o->rho || !o->m_tau || !o->s_tau || !o->m_c || !o->s_c || !o->m_rho || !o->s_rho || !o->g_tau ||
        !o->g_c || !o->g_rho || !o->obj || !o->w || !o->eta_c || !o->eta_d || !o->mu_lo || !o->mu_hi)
        return LHVI_E_ARG;
    a = GradArgs{o->var_count, o->fac_count, var_coef, o->max_slots, o->max_arity, o->obj, o->g_tau, o->g_c, o->g_rho};
    return check_grad<O>(g, pots, p, a);
}

inline Step make_step(const lhvi_npvi_opt_t* o, int it, int32_t fix_mix_its) {
    const double t = (double)(o->t + it + 1);
    return Step{o->lr * sqrt(1.0 - pow(o->b2, t)) / (1.0 - pow(o->b1, t)), o->b1, o->b2, o->eps, it < fix_mix_its ? 1 : 0};
}

// host twin of the gather kernels: a row's edges in var_ptr order.  SS as gather_finish<BFE> reads it
template <bool BFE>
inline void gather_host(const lhvi_graph_t& g, const lhvi_vi_t& p, const double* var_count, const double* SS, const double* pe_c,
                        const double* pe_d, double* g_c, double* g_rho) {
    const int K = p.K;
    for (int v = 0; v < g.V; ++v) {
        const VarInfo vi = var_info(g, v);
        for (int m = 0; m < K; ++m) {
            double c0 = 0.0, c1 = 0.0;
            const int64_t row = (int64_t)v * K + m;
            if (vi.hidden && vi.cont) {
                for (int j = g.var_ptr[v]; j < g.var_ptr[v + 1]; ++j) {
                    const int64_t e = (int64_t)g.var_edge[j] * K + m;
                    c0 += pe_c[2 * e]; c1 += pe_c[2 * e + 1];
                }
            } else if (vi.hidden) {
                for (int t = 0; t < vi.n; ++t) {
                    double s = 0.0;
                    for (int j = g.var_ptr[v]; j < g.var_ptr[v + 1]; ++j) s += pe_d[((int64_t)g.var_edge[j] * K + m) * p.Dmax + t];
                    g_rho[row * p.Dmax + t] = s;
                }
            }
            gather_finish<BFE>(g, p, var_count, SS, v, m, vi, c0, c1, g_c, g_rho);
        }
    }
}

// ---- the entry points' bodies ------------------------------------------------------------------------------------------------
template <class O>
inline int grad_entry(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const GradArgs& a, void* ws, size_t ws_bytes,
                      void* stream) {
    const int rc = check_grad<O>(g, pots, p, a);
    if (rc) return rc;
    if (!ws || ws_bytes < workspace_bytes<O>(g, p)) return LHVI_E_ARG;
    return O::grad_device(g, pots, p, a, carve<O>(g, p, ws), as_stream(stream));
}

template <class O>
inline int run_entry(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const lhvi_npvi_opt_t* o, const double* var_coef,
                     int32_t iterations, int32_t fix_mix_its, double* obj_log, void* ws, size_t ws_bytes, void* stream) {
    GradArgs a;
    int rc = check_run<O>(g, pots, p, o, var_coef, iterations, a);
    if (rc) return rc;
    if (!ws || ws_bytes < workspace_bytes<O>(g, p)) return LHVI_E_ARG;
    const typename O::Ws w = carve<O>(g, p, ws);
    hipStream_t st = as_stream(stream);
    for (int it = 0; it < iterations; ++it) {
        a.obj = obj_log ? obj_log + it : o->obj;
        rc = O::grad_device(g, pots, p, a, w, st);
        if (rc) return rc;
        hipLaunchKernelGGL(npvi_update_kernel, dim3(grid_for((int64_t)g->V * p->K)), dim3(BLOCK), 0, st, *g, p->K, p->Dmax, *o,
                           make_step(o, it, fix_mix_its));
    }
    return check_launch();
}

// the host twins allocate their own workspace; a failed malloc is an argument error like every other
template <class O, class Body>
inline int with_host_ws(const lhvi_graph_t* g, const lhvi_vi_t* p, Body body) {
    void* ws = malloc(workspace_bytes<O>(g, p));
    if (!ws) return LHVI_E_ARG;
    body(carve<O>(g, p, ws));
    free(ws);
    return LHVI_OK;
}

template <class O>
inline int grad_host_entry(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const GradArgs& a) {
    const int rc = check_grad<O>(g, pots, p, a);
    if (rc) return rc;
    return with_host_ws<O>(g, p, [&](const typename O::Ws& w) { O::grad_host(g, pots, p, a, w); });
}

template <class O>
inline int run_host_entry(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const lhvi_npvi_opt_t* o,
                          const double* var_coef, int32_t iterations, int32_t fix_mix_its, double* obj_log) {
    GradArgs a;
    const int rc = check_run<O>(g, pots, p, o, var_coef, iterations, a);
    if (rc) return rc;
    return with_host_ws<O>(g, p, [&](const typename O::Ws& w) {
        for (int it = 0; it < iterations; ++it) {
            a.obj = obj_log ? obj_log + it : o->obj;
            O::grad_host(g, pots, p, a, w);
            const Step s = make_step(o, it, fix_mix_its);
            update_tau(p->K, *o, s);
            for (int v = 0; v < g->V; ++v)
                for (int m = 0; m < p->K; ++m) update_row(*g, p->K, p->Dmax, *o, s, v, m);
        }
    });
}

}  // namespace npvi
}  // namespace lhvi
