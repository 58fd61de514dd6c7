// npvi.hip -- nonparametric variational inference (osi/NPVI.py) on gfx950; the arithmetic is csrc/npvi.hpp's, shared with the host
// twins at the end of this file.  docs/kernels_npvi.md.  The factor and gather kernels, the block reduction and the argument checks
// live in csrc/npvi_dev.hpp, which csrc/oneshot.hip shares; the other kernels are defined here.
//   npvi_factor_kernel<KP, SL, MA, INTERP>
//                               a group of KP lanes per factor, lane m = mixture component m (KP = K rounded up to 1, 2, 4, 16): every
//                               lane walks the factor's K grids, the group adds the lanes' terms of the belief at each node with
//                               shuffles.  Tables in LDS: SL slots of node positions / coefficients per group, SL slots of component
//                               values and of accumulators per lane (SL = 8 or LHVI_NPVI_MAX_SLOTS), the node the potential is
//                               evaluated at and, in the INTERP build, the formula interpreter's stack.  Three builds per KP:
//                               <8 slots, arity 3>, <24, 3> without the interpreter, <24, LHVI_MAX_ARITY> with it; the caller's
//                               hints (max_slots, max_arity, lhvi_pots_t.interpreted) pick one.  Writes per-edge partials,
//                               per-factor d / d w partials and the factor's objective; no atomics.
//   npvi_colsum_kernel          stage one of the fixed-order sums over the factors (K + 1 columns)
//   npvi_entropy_kernel         stage one of L[k][j] = sum_v c_v l_v(k, j): a thread per variable, the lower triangle
//   npvi_weights_kernel         one workgroup: stage two of both sums, the logsumexp rows, S + S^T, g_tau, obj
//   npvi_gather_kernel          a thread per (variable, k): its edges' partials in rv.nb order, the entropy gradient through
//                               S + S^T, the softmax chain of a discrete row;  npvi_gather_hub_kernel: a wavefront per (hub, k)
//   npvi_update_kernel          TensorFlow's Adam on tau / rho / (mu, log var), clips, fix_mix reset, softmaxes, eta_c
#include "npvi_dev.hpp"

namespace lhvi {
namespace npvi {

__global__ void __launch_bounds__(BLOCK) npvi_colsum_kernel(const double* __restrict__ in, int64_t N, int C, double* __restrict__ part) {
    __shared__ double sh[WAVES * COLS_MAX];
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    for (int col = 0; col < C; ++col) block_col_put(sh, C, col, i < N ? in[i * C + col] : 0.0);
    block_cols_flush(sh, C, part + (int64_t)blockIdx.x * C);
}

__global__ void __launch_bounds__(BLOCK) npvi_entropy_kernel(lhvi_graph_t g, lhvi_vi_t p, const double* __restrict__ var_count,
                                                             double* __restrict__ part) {
    __shared__ double sh[WAVES * COLS_MAX];
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    const bool in = v < g.V;
    const VarInfo vi = in ? var_info(g, v) : VarInfo{false, false, 0};
    const double cv = (in && var_count) ? var_count[v] : 1.0;
    const int NP = p.K * (p.K + 1) / 2;
    int col = 0;
    for (int k = 0; k < p.K; ++k)
        for (int j = 0; j <= k; ++j, ++col) block_col_put(sh, NP, col, vi.hidden ? cv * ent_pair(p, v, vi, k, j) : 0.0);
    block_cols_flush(sh, NP, part + (int64_t)blockIdx.x * NP);
}

// one workgroup.  partF [nbF][K + 1], partV [nbV][NP]
__global__ void __launch_bounds__(BLOCK) npvi_weights_kernel(lhvi_vi_t p, const double* __restrict__ partF, int nbF,
                                                             const double* __restrict__ partV, int nbV, double* __restrict__ SS,
                                                             double* __restrict__ obj, double* __restrict__ g_tau) {
    __shared__ double sh[WAVES * COLS_MAX];
    __shared__ double tot[MAX_K + 1], Lt[NP_MAX], U[MAX_K * MAX_K], lse[MAX_K];
    const int K = p.K, NP = K * (K + 1) / 2;
    for (int col = 0; col <= K; ++col) {
        double t = 0.0;
        for (int b = threadIdx.x; b < nbF; b += BLOCK) t += partF[(int64_t)b * (K + 1) + col];
        block_col_put(sh, K + 1, col, t);
    }
    block_cols_flush(sh, K + 1, tot);
    __syncthreads();
    for (int col = 0; col < NP; ++col) {
        double t = 0.0;
        for (int b = threadIdx.x; b < nbV; b += BLOCK) t += partV[(int64_t)b * NP + col];
        block_col_put(sh, NP, col, t);
    }
    block_cols_flush(sh, NP, Lt);
    __syncthreads();
    if ((int)threadIdx.x < K) lse[threadIdx.x] = ent_row(K, Lt, p.w, threadIdx.x, U);
    __syncthreads();
    if (threadIdx.x == 0) finish_weights(K, tot, p.w, lse, U, SS, obj, g_tau);
}

__global__ void __launch_bounds__(BLOCK) npvi_update_kernel(lhvi_graph_t g, int K, int Dmax, lhvi_npvi_opt_t o, Step a) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i == 0) update_tau(K, o, a);
    if (i < (int64_t)g.V * K) update_row(g, K, Dmax, o, a, (int)(i / K), (int)(i % K));
}

struct Layout { size_t pe_c, pe_d, pf, partF, partV, SS, total; int nbF, nbV; };
static Layout layout(const lhvi_graph_t* g, const lhvi_vi_t* p) {
    Layout l{};
    const size_t K = (size_t)p->K, D = (size_t)(p->Dmax < 1 ? 1 : p->Dmax), E = (size_t)(g->E < 1 ? 1 : g->E);
    l.nbF = (int)grid_for(g->F), l.nbV = (int)grid_for(g->V);
    size_t o = 0;
    l.pe_c = o; o += align256(E * K * 2 * sizeof(double));
    l.pe_d = o; o += align256(E * K * D * sizeof(double));
    l.pf = o; o += align256((size_t)(g->F < 1 ? 1 : g->F) * (K + 1) * sizeof(double));
    l.partF = o; o += align256((size_t)l.nbF * (K + 1) * sizeof(double));
    l.partV = o; o += align256((size_t)l.nbV * (K * (K + 1) / 2) * sizeof(double));
    l.SS = o; o += align256(K * K * sizeof(double));
    l.total = o;
    return l;
}

static int grad_device(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const double* var_count,
                       const double* fac_count, int32_t max_slots, int32_t max_arity, double* obj, double* g_tau, double* g_c,
                       double* g_rho, void* ws, hipStream_t st) {
    const Layout l = layout(g, p);
    char* b = static_cast<char*>(ws);
    double* pe_c = reinterpret_cast<double*>(b + l.pe_c);
    double* pe_d = reinterpret_cast<double*>(b + l.pe_d);
    double* pf = reinterpret_cast<double*>(b + l.pf);
    double* partF = reinterpret_cast<double*>(b + l.partF);
    double* partV = reinterpret_cast<double*>(b + l.partV);
    double* SS = reinterpret_cast<double*>(b + l.SS);
    if (g->F > 0) {
        launch_factor_build<false>(g, pots, p, fac_count, max_slots, max_arity, pe_c, pe_d, pf, st);
        hipLaunchKernelGGL(npvi_colsum_kernel, dim3(l.nbF), dim3(BLOCK), 0, st, pf, (int64_t)g->F, p->K + 1, partF);
    }
    hipLaunchKernelGGL(npvi_entropy_kernel, dim3(l.nbV), dim3(BLOCK), 0, st, *g, *p, var_count, partV);
    hipLaunchKernelGGL(npvi_weights_kernel, dim3(1), dim3(BLOCK), 0, st, *p, partF, g->F > 0 ? l.nbF : 0, partV, l.nbV, SS, obj, g_tau);
    hipLaunchKernelGGL(npvi_gather_kernel<false>, dim3(grid_for((int64_t)g->V * p->K)), dim3(BLOCK), 0, st, *g, *p, var_count, SS, pe_c, pe_d,
                       g_c, g_rho);
    if (g->n_hubs > 0)
        hipLaunchKernelGGL(npvi_gather_hub_kernel<false>, dim3(grid_for((int64_t)g->n_hubs * p->K * WAVE)), dim3(BLOCK), 0, st, *g, *p,
                           var_count, SS, pe_c, pe_d, g_c, g_rho);
    return check_launch();
}

// ---- host twin: the same npvi.hpp code, sums in index order --------------------------------------------------------------------
static void grad_host(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const double* var_count,
                      const double* fac_count, double* obj, double* g_tau, double* g_c, double* g_rho, double* ws) {
    const Layout l = layout(g, p);
    char* b = reinterpret_cast<char*>(ws);
    double* pe_c = reinterpret_cast<double*>(b + l.pe_c);
    double* pe_d = reinterpret_cast<double*>(b + l.pe_d);
    double* pf = reinterpret_cast<double*>(b + l.pf);
    double* SS = reinterpret_cast<double*>(b + l.SS);
    const int K = p->K;
    HostCtx ctx;
    double tot[MAX_K + 1] = {0.0}, Lt[NP_MAX] = {0.0}, U[MAX_K * MAX_K], lse[MAX_K];
    for (int f = 0; f < g->F; ++f) {
        factor_item<MAXA, true, SLOTS>(*g, *pots, *p, fac_count, f, ctx, pe_c, pe_d, pf);
        for (int c = 0; c <= K; ++c) tot[c] += pf[(int64_t)f * (K + 1) + c];
    }
    for (int v = 0; v < g->V; ++v) {
        const VarInfo vi = var_info(*g, v);
        if (!vi.hidden) continue;
        const double cv = var_count ? var_count[v] : 1.0;
        int col = 0;
        for (int k = 0; k < K; ++k)
            for (int j = 0; j <= k; ++j, ++col) Lt[col] += cv * ent_pair(*p, v, vi, k, j);
    }
    for (int k = 0; k < K; ++k) lse[k] = ent_row(K, Lt, p->w, k, U);
    finish_weights(K, tot, p->w, lse, U, SS, obj, g_tau);
    for (int v = 0; v < g->V; ++v) {
        const VarInfo vi = var_info(*g, v);
        for (int m = 0; m < K; ++m) {
            double c0 = 0.0, c1 = 0.0;
            const int64_t row = (int64_t)v * K + m;
            if (vi.hidden && vi.cont) {
                for (int j = g->var_ptr[v]; j < g->var_ptr[v + 1]; ++j) {
                    const int64_t e = (int64_t)g->var_edge[j] * K + m;
                    c0 += pe_c[2 * e]; c1 += pe_c[2 * e + 1];
                }
            } else if (vi.hidden) {
                for (int t = 0; t < vi.n; ++t) {
                    double s = 0.0;
                    for (int j = g->var_ptr[v]; j < g->var_ptr[v + 1]; ++j) s += pe_d[((int64_t)g->var_edge[j] * K + m) * p->Dmax + t];
                    g_rho[row * p->Dmax + t] = s;
                }
            }
            gather_finish(*g, *p, var_count, SS, v, m, vi, c0, c1, g_c, g_rho);
        }
    }
}

}  // namespace npvi
}  // namespace lhvi

using namespace lhvi;
using namespace lhvi::npvi;

extern "C" {

size_t lhvi_npvi_workspace_bytes(const lhvi_graph_t* g, const lhvi_vi_t* p) {
    if (!g || !p || p->K < 1 || p->K > LHVI_NPVI_MAX_K) return 0;
    return layout(g, p).total;
}

int lhvi_npvi_grad(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const double* var_count,
                   const double* fac_count, int32_t max_slots, int32_t max_arity, double* obj, double* g_tau, double* g_c,
                   double* g_rho, void* ws, size_t ws_bytes, void* stream) {
    const int rc = check_args(g, pots, p, obj, g_tau, g_c, g_rho);
    if (rc) return rc;
    if (!ws || ws_bytes < layout(g, p).total) return LHVI_E_ARG;
    return grad_device(g, pots, p, var_count, fac_count, max_slots, max_arity, obj, g_tau, g_c, g_rho, ws, as_stream(stream));
}

int lhvi_npvi_run(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const lhvi_npvi_opt_t* o, int32_t iterations,
                  int32_t fix_mix_its, double* obj_log, void* ws, size_t ws_bytes, void* stream) {
    int rc = check_opt(o, iterations);
    if (rc) return rc;
    rc = check_args(g, pots, p, o->obj, o->g_tau, o->g_c, o->g_rho);
    if (rc) return rc;
    if (!ws || ws_bytes < layout(g, p).total) return LHVI_E_ARG;
    hipStream_t st = as_stream(stream);
    for (int it = 0; it < iterations; ++it) {
        rc = grad_device(g, pots, p, o->var_count, o->fac_count, o->max_slots, o->max_arity, obj_log ? obj_log + it : o->obj, o->g_tau,
                         o->g_c, o->g_rho, ws, st);
        if (rc) return rc;
        hipLaunchKernelGGL(npvi_update_kernel, dim3(grid_for((int64_t)g->V * p->K)), dim3(BLOCK), 0, st, *g, p->K, p->Dmax, *o,
                           make_step(o, it, fix_mix_its));
    }
    return check_launch();
}

int lhvi_npvi_grad_host(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const double* var_count,
                        const double* fac_count, double* obj, double* g_tau, double* g_c, double* g_rho) {
    const int rc = check_args(g, pots, p, obj, g_tau, g_c, g_rho);
    if (rc) return rc;
    double* ws = static_cast<double*>(malloc(layout(g, p).total));
    if (!ws) return LHVI_E_ARG;
    grad_host(g, pots, p, var_count, fac_count, obj, g_tau, g_c, g_rho, ws);
    free(ws);
    return LHVI_OK;
}

int lhvi_npvi_run_host(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const lhvi_npvi_opt_t* o,
                       int32_t iterations, int32_t fix_mix_its, double* obj_log) {
    int rc = check_opt(o, iterations);
    if (rc) return rc;
    rc = check_args(g, pots, p, o->obj, o->g_tau, o->g_c, o->g_rho);
    if (rc) return rc;
    double* ws = static_cast<double*>(malloc(layout(g, p).total));
    if (!ws) return LHVI_E_ARG;
    for (int it = 0; it < iterations; ++it) {
        grad_host(g, pots, p, o->var_count, o->fac_count, obj_log ? obj_log + it : o->obj, o->g_tau, o->g_c, o->g_rho, ws);
        const Step a = make_step(o, it, fix_mix_its);
        update_tau(p->K, *o, a);
        for (int v = 0; v < g->V; ++v)
            for (int m = 0; m < p->K; ++m) update_row(*g, p->K, p->Dmax, *o, a, v, m);
    }
    free(ws);
    return LHVI_OK;
}

}  // extern "C"
