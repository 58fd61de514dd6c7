// npvi.hip -- nonparametric variational inference (osi/NPVI.py) on gfx950; the arithmetic is csrc/npvi.hpp's, shared with the host
// twin at the end of this file.  docs/kernels_npvi.md.  The factor and gather kernels and the block reduction live in
// csrc/npvi_dev.hpp; the workspace prefix, the checks, the host gather, the Adam loops and the entry points' bodies in
// csrc/npvi_run.hpp; csrc/oneshot.hip shares both.  Here: the other kernels and `Npvi`, the objective the driver runs.
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
#include "npvi_run.hpp"

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

// the objective of csrc/npvi_run.hpp's driver: the negative ELBO with the entropy bound
struct Npvi {
    static constexpr bool VAR_COEF = false;
    struct Ws : WsPrefix { double *partV, *SS; };       // partV [nbV][K (K + 1) / 2], SS [K][K]
    static Ws carve(const lhvi_graph_t* g, const lhvi_vi_t* p, Carver& c) {
        const WsPrefix pre = carve_prefix(g, p, c);
        const size_t K = (size_t)p->K;
        double* partV = c.take((size_t)pre.nbV * (K * (K + 1) / 2) * sizeof(double));
        return Ws{pre, partV, c.take(K * K * sizeof(double))};
    }

    static int grad_device(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const GradArgs& a, const Ws& w,
                           hipStream_t st) {
        if (g->F > 0) {
            launch_factor_build<false>(g, pots, p, a.fac_count, a.max_slots, a.max_arity, w.pe_c, w.pe_d, w.pf, st);
            hipLaunchKernelGGL(npvi_colsum_kernel, dim3(w.nbF), dim3(BLOCK), 0, st, w.pf, (int64_t)g->F, p->K + 1, w.partF);
        }
        hipLaunchKernelGGL(npvi_entropy_kernel, dim3(w.nbV), dim3(BLOCK), 0, st, *g, *p, a.var_count, w.partV);
        hipLaunchKernelGGL(npvi_weights_kernel, dim3(1), dim3(BLOCK), 0, st, *p, w.partF, g->F > 0 ? w.nbF : 0, w.partV, w.nbV, w.SS, a.obj,
                           a.g_tau);
        hipLaunchKernelGGL(npvi_gather_kernel<false>, dim3(grid_for((int64_t)g->V * p->K)), dim3(BLOCK), 0, st, *g, *p, a.var_count, w.SS,
                           w.pe_c, w.pe_d, a.g_c, a.g_rho);
        if (g->n_hubs > 0)
            hipLaunchKernelGGL(npvi_gather_hub_kernel<false>, dim3(grid_for((int64_t)g->n_hubs * p->K * WAVE)), dim3(BLOCK), 0, st, *g, *p,
                               a.var_count, w.SS, w.pe_c, w.pe_d, a.g_c, a.g_rho);
        return check_launch();
    }

    // host twin: the same npvi.hpp code, sums in index order
    static void grad_host(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const GradArgs& a, const Ws& w) {
        const int K = p->K;
        HostCtx ctx;
        double tot[MAX_K + 1] = {0.0}, Lt[NP_MAX] = {0.0}, U[MAX_K * MAX_K], lse[MAX_K];
        for (int f = 0; f < g->F; ++f) {
            factor_item<MAXA, true, SLOTS>(*g, *pots, *p, a.fac_count, f, ctx, w.pe_c, w.pe_d, w.pf);
            for (int c = 0; c <= K; ++c) tot[c] += w.pf[(int64_t)f * (K + 1) + c];
        }
        for (int v = 0; v < g->V; ++v) {
            const VarInfo vi = var_info(*g, v);
            if (!vi.hidden) continue;
            const double cv = a.var_count ? a.var_count[v] : 1.0;
            int col = 0;
            for (int k = 0; k < K; ++k)
                for (int j = 0; j <= k; ++j, ++col) Lt[col] += cv * ent_pair(*p, v, vi, k, j);
        }
        for (int k = 0; k < K; ++k) lse[k] = ent_row(K, Lt, p->w, k, U);
        finish_weights(K, tot, p->w, lse, U, w.SS, a.obj, a.g_tau);
        gather_host<false>(*g, *p, a.var_count, w.SS, w.pe_c, w.pe_d, a.g_c, a.g_rho);
    }
};

}  // namespace npvi
}  // namespace lhvi

using namespace lhvi::npvi;

extern "C" {

size_t lhvi_npvi_workspace_bytes(const lhvi_graph_t* g, const lhvi_vi_t* p) { return workspace_bytes<Npvi>(g, p); }

int lhvi_npvi_grad(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const double* var_count,
                   const double* fac_count, int32_t max_slots, int32_t max_arity, double* obj, double* g_tau, double* g_c,
                   double* g_rho, void* ws, size_t ws_bytes, void* stream) {
    return grad_entry<Npvi>(g, pots, p, GradArgs{var_count, fac_count, nullptr, max_slots, max_arity, obj, g_tau, g_c, g_rho}, ws, ws_bytes,
                            stream);
}

int lhvi_npvi_run(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const lhvi_npvi_opt_t* o, int32_t iterations,
                  int32_t fix_mix_its, double* obj_log, void* ws, size_t ws_bytes, void* stream) {
    return run_entry<Npvi>(g, pots, p, o, nullptr, iterations, fix_mix_its, obj_log, ws, ws_bytes, stream);
}

int lhvi_npvi_grad_host(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const double* var_count,
                        const double* fac_count, double* obj, double* g_tau, double* g_c, double* g_rho) {
    return grad_host_entry<Npvi>(g, pots, p, GradArgs{var_count, fac_count, nullptr, 0, 0, obj, g_tau, g_c, g_rho});
}

int lhvi_npvi_run_host(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const lhvi_npvi_opt_t* o,
                       int32_t iterations, int32_t fix_mix_its, double* obj_log) {
    return run_host_entry<Npvi>(g, pots, p, o, nullptr, iterations, fix_mix_its, obj_log);
}

}  // extern "C"
