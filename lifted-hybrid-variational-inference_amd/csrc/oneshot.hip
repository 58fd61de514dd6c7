// oneshot.hip -- OneShot (osi/OneShot.py): a K-component product mixture fitted to the Bethe free energy, on gfx950.  The parameters,
// their view, the factor grid, the reductions, the gather and the update are NPVI's (csrc/npvi_dev.hpp, csrc/npvi.hip), and so are
// the workspace prefix, the checks, the Adam loops and the entry points' bodies (csrc/npvi_run.hpp).  The arithmetic that is
// OneShot's own is csrc/oneshot.hpp's, shared with the host twin at the end of this file; `Oneshot` is the objective the driver
// runs.  docs/kernels_oneshot.md.
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
#include "npvi_run.hpp"
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

// the objective of csrc/npvi_run.hpp's driver: the Bethe free energy
struct Oneshot {
    static constexpr bool VAR_COEF = true;
    struct Ws : WsPrefix { double *pv_c, *pv_d, *pvw, *partV; };      // pv_c [V][K][2] and pv_d [V][K][Dmax] in one piece, pvw and partV [.][K + 1]
    static Ws carve(const lhvi_graph_t* g, const lhvi_vi_t* p, Carver& c) {
        const WsPrefix pre = carve_prefix(g, p, c);
        const size_t K = (size_t)p->K, D = (size_t)(p->Dmax < 1 ? 1 : p->Dmax), V = (size_t)(g->V < 1 ? 1 : g->V);
        double* pv = c.take(V * K * (2 + D) * sizeof(double));
        double* pvw = c.take(V * (K + 1) * sizeof(double));
        return Ws{pre, pv, pv ? pv + (size_t)g->V * p->K * 2 : nullptr, pvw, c.take((size_t)pre.nbV * (K + 1) * sizeof(double))};
    }

    static int grad_device(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const GradArgs& a, const Ws& w,
                           hipStream_t st) {
        if (g->F > 0) {
            launch_factor_build<true>(g, pots, p, a.fac_count, a.max_slots, a.max_arity, w.pe_c, w.pe_d, w.pf, st);
            hipLaunchKernelGGL(npvi_colsum_kernel, dim3(w.nbF), dim3(BLOCK), 0, st, w.pf, (int64_t)g->F, p->K + 1, w.partF);
        }
#define LHVI_ONESHOT_VAR(KP) \
    hipLaunchKernelGGL(oneshot_var_kernel<KP>, dim3(grid_for(g->V, BLOCK / KP)), dim3(BLOCK), 0, st, *g, *p, a.var_coef, w.pv_c, w.pv_d, \
                       w.pvw)
        if (p->K == 1) LHVI_ONESHOT_VAR(1);
        else if (p->K == 2) LHVI_ONESHOT_VAR(2);
        else if (p->K <= 4) LHVI_ONESHOT_VAR(4);
        else LHVI_ONESHOT_VAR(16);
#undef LHVI_ONESHOT_VAR
        hipLaunchKernelGGL(npvi_colsum_kernel, dim3(w.nbV), dim3(BLOCK), 0, st, w.pvw, (int64_t)g->V, p->K + 1, w.partV);
        hipLaunchKernelGGL(oneshot_weights_kernel, dim3(1), dim3(BLOCK), 0, st, *p, w.partF, g->F > 0 ? w.nbF : 0, w.partV, w.nbV, a.obj,
                           a.g_tau);
        hipLaunchKernelGGL(npvi_gather_kernel<true>, dim3(grid_for((int64_t)g->V * p->K)), dim3(BLOCK), 0, st, *g, *p, a.var_count, w.pv_c,
                           w.pe_c, w.pe_d, a.g_c, a.g_rho);
        if (g->n_hubs > 0)
            hipLaunchKernelGGL(npvi_gather_hub_kernel<true>, dim3(grid_for((int64_t)g->n_hubs * p->K * WAVE)), dim3(BLOCK), 0, st, *g, *p,
                               a.var_count, w.pv_c, w.pe_c, w.pe_d, a.g_c, a.g_rho);
        return check_launch();
    }

    // host twin: the same npvi.hpp / oneshot.hpp code, sums in index order
    static void grad_host(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const GradArgs& a, const Ws& w) {
        const int K = p->K;
        HostCtx ctx;
        HostVarCtx vctx;
        double totF[MAX_K + 1] = {0.0}, totV[MAX_K + 1] = {0.0};
        for (int f = 0; f < g->F; ++f) {
            factor_item<MAXA, true, SLOTS, true>(*g, *pots, *p, a.fac_count, f, ctx, w.pe_c, w.pe_d, w.pf);
            for (int c = 0; c <= K; ++c) totF[c] += w.pf[(int64_t)f * (K + 1) + c];
        }
        for (int v = 0; v < g->V; ++v) {
            var_item(*g, *p, a.var_coef, v, vctx, w.pv_c, w.pv_d, w.pvw);
            for (int c = 0; c <= K; ++c) totV[c] += w.pvw[(int64_t)v * (K + 1) + c];
        }
        finish_weights(K, totF, totV, p->w, a.obj, a.g_tau);
        gather_host<true>(*g, *p, a.var_count, w.pv_c, w.pe_c, w.pe_d, a.g_c, a.g_rho);
    }
};

}  // namespace oneshot
}  // namespace lhvi

using namespace lhvi::npvi;
using lhvi::oneshot::Oneshot;

extern "C" {

size_t lhvi_oneshot_workspace_bytes(const lhvi_graph_t* g, const lhvi_vi_t* p) { return workspace_bytes<Oneshot>(g, p); }

int lhvi_oneshot_grad(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const double* var_count,
                      const double* fac_count, const double* var_coef, int32_t max_slots, int32_t max_arity, double* obj, double* g_tau,
                      double* g_c, double* g_rho, void* ws, size_t ws_bytes, void* stream) {
    return grad_entry<Oneshot>(g, pots, p, GradArgs{var_count, fac_count, var_coef, max_slots, max_arity, obj, g_tau, g_c, g_rho}, ws,
                               ws_bytes, stream);
}

int lhvi_oneshot_run(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const lhvi_npvi_opt_t* o,
                     const double* var_coef, int32_t iterations, int32_t fix_mix_its, double* obj_log, void* ws, size_t ws_bytes,
                     void* stream) {
    return run_entry<Oneshot>(g, pots, p, o, var_coef, iterations, fix_mix_its, obj_log, ws, ws_bytes, stream);
}

int lhvi_oneshot_grad_host(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const double* var_count,
                           const double* fac_count, const double* var_coef, double* obj, double* g_tau, double* g_c, double* g_rho) {
    return grad_host_entry<Oneshot>(g, pots, p, GradArgs{var_count, fac_count, var_coef, 0, 0, obj, g_tau, g_c, g_rho});
}

int lhvi_oneshot_run_host(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const lhvi_npvi_opt_t* o,
                          const double* var_coef, int32_t iterations, int32_t fix_mix_its, double* obj_log) {
    return run_host_entry<Oneshot>(g, pots, p, o, var_coef, iterations, fix_mix_its, obj_log);
}

}  // extern "C"
