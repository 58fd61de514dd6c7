// oneshot.hip -- OneShot (osi/OneShot.py): a K-component product mixture fitted to the Bethe free energy, on gfx950.  The parameters,
// their view, the factor grid, the reductions, the gather and the update are NPVI's (csrc/npvi_dev.hpp, csrc/npvi.hip); the
// arithmetic that is OneShot's own is csrc/oneshot.hpp's, shared with the host twins at the end of this file.  docs/kernels_oneshot.md.
//   npvi_factor_kernel<KP, SL, MA, INTERP, true>
//                               NPVI's factor kernel with the expectant -log phi + log b: log b joins F once the butterfly has given
//                               every lane b.  The same three builds per KP, picked by the same hints.
//   oneshot_var_kernel<KP>      the variable term kappa_v E_b[log b_v]: a group of KP lanes per variable, lane m = mixture component m.
//                               The group walks the K * T nodes of a continuous variable (the states of a discrete one), every lane
//                               evaluates its own component there, a __shfl_xor butterfly gives all of them b_v; a lane keeps its
//                               own accumulators in registers.  Writes the variable's gradient rows, its K partials of d / d w and
//                               its objective; zeros, with nothing evaluated, for observed rows and kappa_v == 0.  No LDS, no atomics.
//   npvi_colsum_kernel          stage one of the fixed-order sums over the factors and over the variables (K + 1 columns each)
//   oneshot_weights_kernel      one workgroup: stage two of both sums, g_tau through the softmax, obj
//   npvi_gather_kernel<true>, npvi_gather_hub_kernel<true>
//                               the edges' partials in rv.nb order plus the variable kernel's row, the softmax chain of a discrete row
//   npvi_update_kernel          as it is
#include "npvi_dev.hpp"
#include "oneshot.hpp"

namespace lhvi {
namespace oneshot {

using namespace lhvi::npvi;

template <int KP>
struct DevVarCtx {
    static constexpr int NM = 1;
    int gl;
    __device__ __forceinline__ int m(int) const { return gl; }
    __device__ __forceinline__ double sum_m(double v) const {
#pragma unroll
        for (int d = 1; d < KP; d <<= 1) v += __shfl_xor(v, d, 64);
        return v;
    }
};

template <int KP>
__global__ void __launch_bounds__(BLOCK) oneshot_var_kernel(lhvi_graph_t g, lhvi_vi_t p, const double* __restrict__ var_coef,
                                                            double* __restrict__ pv_c, double* __restrict__ pv_d,
                                                            double* __restrict__ pvw) {
    const int64_t v = (int64_t)blockIdx.x * (BLOCK / KP) + threadIdx.x / KP;
    if (v >= g.V) return;                            // (whole groups leave together)
    DevVarCtx<KP> ctx{(int)threadIdx.x % KP};
    var_item(g, p, var_coef, (int)v, ctx, pv_c, pv_d, pvw);
}

// one workgroup.  partF [nbF][K + 1], partV [nbV][K + 1]
__global__ void __launch_bounds__(BLOCK) oneshot_weights_kernel(lhvi_vi_t p, const double* __restrict__ partF, int nbF,
                                                                const double* __restrict__ partV, int nbV, double* __restrict__ obj,
                                                                double* __restrict__ g_tau) {
    __shared__ double sh[WAVES * (MAX_K + 1)];
    __shared__ double totF[MAX_K + 1], totV[MAX_K + 1];
    const int K = p.K;
    for (int col = 0; col <= K; ++col) {
        double t = 0.0;
        for (int b = threadIdx.x; b < nbF; b += BLOCK) t += partF[(int64_t)b * (K + 1) + col];
        block_col_put(sh, K + 1, col, t);
    }
    block_cols_flush(sh, K + 1, totF);
    __syncthreads();
    for (int col = 0; col <= K; ++col) {
        double t = 0.0;
        for (int b = threadIdx.x; b < nbV; b += BLOCK) t += partV[(int64_t)b * (K + 1) + col];
        block_col_put(sh, K + 1, col, t);
    }
    block_cols_flush(sh, K + 1, totV);
    __syncthreads();
    if (threadIdx.x == 0) finish_weights(K, totF, totV, p.w, obj, g_tau);
}

struct Layout { size_t pe_c, pe_d, pf, partF, pv, pvw, partV, total; int nbF, nbV; };
static Layout layout(const lhvi_graph_t* g, const lhvi_vi_t* p) {
    Layout l{};
    const size_t K = (size_t)p->K, D = (size_t)(p->Dmax < 1 ? 1 : p->Dmax), E = (size_t)(g->E < 1 ? 1 : g->E);
    const size_t V = (size_t)(g->V < 1 ? 1 : g->V);
    l.nbF = (int)grid_for(g->F), l.nbV = (int)grid_for(g->V);
    size_t o = 0;
    l.pe_c = o; o += align256(E * K * 2 * sizeof(double));
    l.pe_d = o; o += align256(E * K * D * sizeof(double));
    l.pf = o; o += align256((size_t)(g->F < 1 ? 1 : g->F) * (K + 1) * sizeof(double));
    l.partF = o; o += align256((size_t)l.nbF * (K + 1) * sizeof(double));
    l.pv = o; o += align256(V * K * (2 + D) * sizeof(double));         // [V][K][2], then [V][K][Dmax]
    l.pvw = o; o += align256(V * (K + 1) * sizeof(double));
    l.partV = o; o += align256((size_t)l.nbV * (K + 1) * sizeof(double));
    l.total = o;
    return l;
}

struct Ws { double *pe_c, *pe_d, *pf, *partF, *pv_c, *pv_d, *pvw, *partV; };
static Ws carve(const lhvi_graph_t* g, const lhvi_vi_t* p, const Layout& l, void* ws) {
    char* b = static_cast<char*>(ws);
    auto at = [b](size_t o) { return reinterpret_cast<double*>(b + o); };
    return Ws{at(l.pe_c), at(l.pe_d), at(l.pf), at(l.partF), at(l.pv), at(l.pv) + (size_t)g->V * p->K * 2, at(l.pvw), at(l.partV)};
}

static int grad_device(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const double* var_count,
                       const double* fac_count, const double* var_coef, int32_t max_slots, int32_t max_arity, double* obj,
                       double* g_tau, double* g_c, double* g_rho, void* ws, hipStream_t st) {
    const Layout l = layout(g, p);
    const Ws w = carve(g, p, l, ws);
    if (g->F > 0) {
        launch_factor_build<true>(g, pots, p, fac_count, max_slots, max_arity, w.pe_c, w.pe_d, w.pf, st);
        hipLaunchKernelGGL(npvi_colsum_kernel, dim3(l.nbF), dim3(BLOCK), 0, st, w.pf, (int64_t)g->F, p->K + 1, w.partF);
    }
#define LHVI_ONESHOT_VAR(KP) \
    hipLaunchKernelGGL(oneshot_var_kernel<KP>, dim3(grid_for(g->V, BLOCK / KP)), dim3(BLOCK), 0, st, *g, *p, var_coef, w.pv_c, w.pv_d, \
                       w.pvw)
    if (p->K == 1) LHVI_ONESHOT_VAR(1);
    else if (p->K == 2) LHVI_ONESHOT_VAR(2);
    else if (p->K <= 4) LHVI_ONESHOT_VAR(4);
    else LHVI_ONESHOT_VAR(16);
#undef LHVI_ONESHOT_VAR
    hipLaunchKernelGGL(npvi_colsum_kernel, dim3(l.nbV), dim3(BLOCK), 0, st, w.pvw, (int64_t)g->V, p->K + 1, w.partV);
    hipLaunchKernelGGL(oneshot_weights_kernel, dim3(1), dim3(BLOCK), 0, st, *p, w.partF, g->F > 0 ? l.nbF : 0, w.partV, l.nbV, obj, g_tau);
    hipLaunchKernelGGL(npvi_gather_kernel<true>, dim3(grid_for((int64_t)g->V * p->K)), dim3(BLOCK), 0, st, *g, *p, var_count, w.pv_c,
                       w.pe_c, w.pe_d, g_c, g_rho);
    if (g->n_hubs > 0)
        hipLaunchKernelGGL(npvi_gather_hub_kernel<true>, dim3(grid_for((int64_t)g->n_hubs * p->K * WAVE)), dim3(BLOCK), 0, st, *g, *p,
                           var_count, w.pv_c, w.pe_c, w.pe_d, g_c, g_rho);
    return check_launch();
}

// ---- host twin: the same npvi.hpp / oneshot.hpp code, sums in index order ------------------------------------------------------
static void grad_host(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const double* var_count,
                      const double* fac_count, const double* var_coef, double* obj, double* g_tau, double* g_c, double* g_rho,
                      void* ws) {
    const Layout l = layout(g, p);
    const Ws w = carve(g, p, l, ws);
    const int K = p->K;
    HostCtx ctx;
    HostVarCtx vctx;
    double totF[MAX_K + 1] = {0.0}, totV[MAX_K + 1] = {0.0};
    for (int f = 0; f < g->F; ++f) {
        factor_item<MAXA, true, SLOTS, true>(*g, *pots, *p, fac_count, f, ctx, w.pe_c, w.pe_d, w.pf);
        for (int c = 0; c <= K; ++c) totF[c] += w.pf[(int64_t)f * (K + 1) + c];
    }
    for (int v = 0; v < g->V; ++v) {
        var_item(*g, *p, var_coef, v, vctx, w.pv_c, w.pv_d, w.pvw);
        for (int c = 0; c <= K; ++c) totV[c] += w.pvw[(int64_t)v * (K + 1) + c];
    }
    finish_weights(K, totF, totV, p->w, obj, g_tau);
    for (int v = 0; v < g->V; ++v) {
        const VarInfo vi = var_info(*g, v);
        for (int m = 0; m < K; ++m) {
            double c0 = 0.0, c1 = 0.0;
            const int64_t row = (int64_t)v * K + m;
            if (vi.hidden && vi.cont) {
                for (int j = g->var_ptr[v]; j < g->var_ptr[v + 1]; ++j) {
                    const int64_t e = (int64_t)g->var_edge[j] * K + m;
                    c0 += w.pe_c[2 * e]; c1 += w.pe_c[2 * e + 1];
                }
            } else if (vi.hidden) {
                for (int t = 0; t < vi.n; ++t) {
                    double s = 0.0;
                    for (int j = g->var_ptr[v]; j < g->var_ptr[v + 1]; ++j) s += w.pe_d[((int64_t)g->var_edge[j] * K + m) * p->Dmax + t];
                    g_rho[row * p->Dmax + t] = s;
                }
            }
            gather_finish<true>(*g, *p, var_count, w.pv_c, v, m, vi, c0, c1, g_c, g_rho);
        }
    }
}

}  // namespace oneshot
}  // namespace lhvi

using namespace lhvi;
using namespace lhvi::oneshot;

extern "C" {

size_t lhvi_oneshot_workspace_bytes(const lhvi_graph_t* g, const lhvi_vi_t* p) {
    if (!g || !p || p->K < 1 || p->K > LHVI_NPVI_MAX_K) return 0;
    return layout(g, p).total;
}

int lhvi_oneshot_grad(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const double* var_count,
                      const double* fac_count, const double* var_coef, int32_t max_slots, int32_t max_arity, double* obj, double* g_tau,
                      double* g_c, double* g_rho, void* ws, size_t ws_bytes, void* stream) {
    const int rc = check_args(g, pots, p, obj, g_tau, g_c, g_rho);
    if (rc) return rc;
    if (!var_coef || !ws || ws_bytes < layout(g, p).total) return LHVI_E_ARG;
    return grad_device(g, pots, p, var_count, fac_count, var_coef, max_slots, max_arity, obj, g_tau, g_c, g_rho, ws, as_stream(stream));
}

int lhvi_oneshot_run(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const lhvi_npvi_opt_t* o,
                     const double* var_coef, int32_t iterations, int32_t fix_mix_its, double* obj_log, void* ws, size_t ws_bytes,
                     void* stream) {
    int rc = check_opt(o, iterations);
    if (rc) return rc;
    rc = check_args(g, pots, p, o->obj, o->g_tau, o->g_c, o->g_rho);
    if (rc) return rc;
    if (!var_coef || !ws || ws_bytes < layout(g, p).total) return LHVI_E_ARG;
    hipStream_t st = as_stream(stream);
    for (int it = 0; it < iterations; ++it) {
        rc = grad_device(g, pots, p, o->var_count, o->fac_count, var_coef, o->max_slots, o->max_arity, obj_log ? obj_log + it : o->obj,
                         o->g_tau, o->g_c, o->g_rho, ws, st);
        if (rc) return rc;
        hipLaunchKernelGGL(npvi_update_kernel, dim3(grid_for((int64_t)g->V * p->K)), dim3(BLOCK), 0, st, *g, p->K, p->Dmax, *o,
                           make_step(o, it, fix_mix_its));
    }
    return check_launch();
}

int lhvi_oneshot_grad_host(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const double* var_count,
                           const double* fac_count, const double* var_coef, double* obj, double* g_tau, double* g_c, double* g_rho) {
    const int rc = check_args(g, pots, p, obj, g_tau, g_c, g_rho);
    if (rc) return rc;
    if (!var_coef) return LHVI_E_ARG;
    void* ws = malloc(layout(g, p).total);
    if (!ws) return LHVI_E_ARG;
    grad_host(g, pots, p, var_count, fac_count, var_coef, obj, g_tau, g_c, g_rho, ws);
    free(ws);
    return LHVI_OK;
}

int lhvi_oneshot_run_host(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const lhvi_npvi_opt_t* o,
                          const double* var_coef, int32_t iterations, int32_t fix_mix_its, double* obj_log) {
    int rc = check_opt(o, iterations);
    if (rc) return rc;
    rc = check_args(g, pots, p, o->obj, o->g_tau, o->g_c, o->g_rho);
    if (rc) return rc;
    if (!var_coef) return LHVI_E_ARG;
    void* ws = malloc(layout(g, p).total);
    if (!ws) return LHVI_E_ARG;
    for (int it = 0; it < iterations; ++it) {
        grad_host(g, pots, p, o->var_count, o->fac_count, var_coef, obj_log ? obj_log + it : o->obj, o->g_tau, o->g_c, o->g_rho, ws);
        const Step a = make_step(o, it, fix_mix_its);
        update_tau(p->K, *o, a);
        for (int v = 0; v < g->V; ++v)
            for (int m = 0; m < p->K; ++m) update_row(*g, p->K, p->Dmax, *o, a, v, m);
    }
    free(ws);
    return LHVI_OK;
}

}  // extern "C"
