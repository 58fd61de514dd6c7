// fgibbs.hip -- single-site Gibbs / slice sampling on a ground flat graph (csrc/fgibbs.hpp; docs/kernels_fgibbs.md), gfx950.
//   fgibbs_colour_kernel  one thread per (variable of the colour, chain), chain fastest: with a multiple of 64 chains a wavefront
//                         is ONE variable over 64 chains -- the walk over its factors, their kinds and parameters are uniform
//                         (scalar loads), the state reads coalesced; with fewer chains a wavefront spans several variables and
//                         diverges per variable, same results.  The log masses of a discrete update and the formula
//                         interpreter's stack: a column of LDS per thread.
//   fgibbs_hub_kernel     one wavefront per (hub variable, chain): lanes stride over the variable's row, a DPP wave sum per
//                         evaluation of g_v; level, shrinkage and pick run on every lane with the same bits.
//   fgibbs_init_kernel    the initial state.
// A launch per colour per iteration in stream order: the colours of an iteration depend on each other.
#include "common.hpp"
#include "fgibbs.hpp"

namespace lhvi {
namespace fgibbs {

constexpr int CB = 128;                 // colour kernel: two wavefronts, 16 + 12 doubles of LDS per thread
constexpr int IB = 256;

// the whole argument block of an update kernel: one struct at offset 0, read where a field is used (csrc/pt.hip::arg_block) so
// that the compiler does not hold the three structs' pointers in scalar registers through the loops
struct KArgs {
    lhvi_graph_t g;
    lhvi_pots_t pots;
    lhvi_fgibbs_t s;
    int64_t chains;
    double* x;
    int32_t* idx;
    int32_t it, first, count;
};
__device__ __forceinline__ const KArgs& kargs() {
    auto p = (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(const KArgs*)p;
}

// STRIDE: the threads of the workgroup (a thread's interpreter stack is a column of LDS); WAVE_WIDE: the 64 lanes share a variable
template <bool INTERP, int STRIDE, bool WAVE_WIDE>
struct DevCtx {
    int lane, lanes;
    double* stk;
    int64_t c;
    __device__ __forceinline__ int64_t C() const { return kargs().chains; }
    __device__ __forceinline__ double* x() const { return kargs().x; }
    __device__ __forceinline__ int32_t* idx() const { return kargs().idx; }
    __device__ __forceinline__ const lhvi_graph_t& G() const { return kargs().g; }
    __device__ __forceinline__ const lhvi_pots_t& P() const { return kargs().pots; }
    __device__ __forceinline__ const lhvi_fgibbs_t& S() const { return kargs().s; }
    __device__ __forceinline__ void sync() const { if (WAVE_WIDE) __syncthreads(); }
    __device__ __forceinline__ double sum(double v) const { return WAVE_WIDE ? dpp_wave_reduce(v, SumOp()) : v; }
    __device__ __forceinline__ auto stack() const {
        if constexpr (INTERP) return MlnLdsStack<STRIDE>{stk};
        else return MlnNoStack();
    }
};

template <bool INTERP>
__global__ void __launch_bounds__(CB) fgibbs_colour_kernel(KArgs) {
    __shared__ double lp[MAX_STATES * CB];
    __shared__ double stk[INTERP ? MLN_STACK * CB : 1];
    const int64_t chains = kargs().chains;
    const int64_t t = (int64_t)blockIdx.x * CB + threadIdx.x;
    if (t >= (int64_t)kargs().count * chains) return;
    const int v = kargs().s.col_var[kargs().first + (int)(t / chains)];
    if (kargs().g.var_ptr[v + 1] - kargs().g.var_ptr[v] > kargs().s.hub_degree) return;        // the hub kernel's
    update<INTERP>(DevCtx<INTERP, CB, false>{0, 1, stk + threadIdx.x, t % chains}, kargs().it, v, lp + threadIdx.x, CB);
}

template <bool INTERP>
__global__ void __launch_bounds__(WAVE) fgibbs_hub_kernel(KArgs) {
    __shared__ double lp[MAX_STATES];
    __shared__ double stk[INTERP ? MLN_STACK * WAVE : 1];
    const int64_t chains = kargs().chains, b = blockIdx.x;
    const int v = kargs().s.hub_var[kargs().first + (int)(b / chains)];
    update<INTERP>(DevCtx<INTERP, WAVE, true>{(int)threadIdx.x, WAVE, stk + threadIdx.x, b % chains}, kargs().it, v, lp, 1);
}

__global__ void __launch_bounds__(IB) fgibbs_init_kernel(lhvi_graph_t g, lhvi_fgibbs_t s, int64_t chains, double* x, int32_t* idx) {
    const int64_t t = (int64_t)blockIdx.x * IB + threadIdx.x;
    if (t >= (int64_t)g.V * chains) return;
    init_var(g, s, chains, t % chains, x, idx, (int)(t / chains));
}

static int check(const lhvi_graph_t* g, const lhvi_fgibbs_t* s, int64_t chains, const double* x, const int32_t* idx) {
    if (!g || !s || chains < 0 || g->V < 0) return LHVI_E_ARG;
    if (g->edge_count || g->var_mult || g->fac_mult) return LHVI_E_UNSUPPORTED;
    if (chains > MAX_CHAINS || s->max_shrink > MAX_SHRINK) return LHVI_E_UNSUPPORTED;
    if (s->n_colours < 0 || s->max_shrink < 0 || s->hub_degree < 0 || s->num_burnin < 0 || s->num_samples < 0 || s->thin < 1)
        return LHVI_E_ARG;
    if (g->V && chains && (!x || !idx)) return LHVI_E_ARG;
    if (s->n_colours && (!s->col_ptr || !s->col_var || !s->hub_ptr)) return LHVI_E_ARG;
    if ((s->counts && !s->cnt_off) || (s->samples && !s->keep_row)) return LHVI_E_ARG;
    return LHVI_OK;
}

}  // namespace fgibbs
}  // namespace lhvi

using namespace lhvi;
using namespace lhvi::fgibbs;

extern "C" {

int lhvi_fgibbs_init(const lhvi_graph_t* g, const lhvi_fgibbs_t* s, int64_t chains, double* x, int32_t* idx, void* stream) {
    const int rc = check(g, s, chains, x, idx);
    if (rc) return rc;
    if (chains == 0 || g->V == 0) return LHVI_OK;
    const int64_t blocks = ((int64_t)g->V * chains + IB - 1) / IB;
    if (blocks > 0x7fffffff) return LHVI_E_UNSUPPORTED;
    hipLaunchKernelGGL(fgibbs_init_kernel, dim3((unsigned)blocks), dim3(IB), 0, as_stream(stream), *g, *s, chains, x, idx);
    return check_launch();
}

int lhvi_fgibbs_run(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_fgibbs_t* s, int64_t chains, int32_t it_begin,
                    int32_t it_end, const int32_t* col_ptr_host, const int32_t* hub_ptr_host, double* x, int32_t* idx, void* stream) {
    const int rc = check(g, s, chains, x, idx);
    if (rc) return rc;
    if (!pots || it_begin < 0 || it_end < it_begin) return LHVI_E_ARG;
    if (s->n_colours && (!col_ptr_host || !hub_ptr_host)) return LHVI_E_ARG;
    if (chains == 0) return LHVI_OK;
    for (int c = 0; c < s->n_colours; ++c) {
        const int64_t n = col_ptr_host[c + 1] - col_ptr_host[c], h = hub_ptr_host[c + 1] - hub_ptr_host[c];
        if (n < 0 || h < 0 || h > n || (h && !s->hub_var)) return LHVI_E_ARG;
        if ((n * chains + CB - 1) / CB > 0x7fffffff || h * chains > 0x7fffffff) return LHVI_E_UNSUPPORTED;
    }
    const bool interp = pots->interpreted != 0;
    hipStream_t st = as_stream(stream);
    KArgs ka{*g, *pots, *s, chains, x, idx, 0, 0, 0};
    for (int it = it_begin; it < it_end; ++it)
        for (int c = 0; c < s->n_colours; ++c) {
            const int n = col_ptr_host[c + 1] - col_ptr_host[c], h = hub_ptr_host[c + 1] - hub_ptr_host[c];
            ka.it = it;
            if (n > h) {
                ka.first = col_ptr_host[c];
                ka.count = n;
                const dim3 grid((unsigned)(((int64_t)n * chains + CB - 1) / CB));
                if (interp) hipLaunchKernelGGL(fgibbs_colour_kernel<true>, grid, dim3(CB), 0, st, ka);
                else hipLaunchKernelGGL(fgibbs_colour_kernel<false>, grid, dim3(CB), 0, st, ka);
            }
            if (h) {
                ka.first = hub_ptr_host[c];
                ka.count = h;
                const dim3 grid((unsigned)((int64_t)h * chains));
                if (interp) hipLaunchKernelGGL(fgibbs_hub_kernel<true>, grid, dim3(WAVE), 0, st, ka);
                else hipLaunchKernelGGL(fgibbs_hub_kernel<false>, grid, dim3(WAVE), 0, st, ka);
            }
            const int lrc = check_launch();
            if (lrc) return lrc;
        }
    return LHVI_OK;
}

int lhvi_fgibbs_chain_host(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_fgibbs_t* s, int64_t chains, int64_t chain,
                           int32_t init, int32_t it_begin, int32_t it_end, double* x, int32_t* idx) {
    const int rc = check(g, s, chains, x, idx);
    if (rc) return rc;
    if (!pots || chain < 0 || chain >= chains || it_begin < 0 || it_end < it_begin) return LHVI_E_ARG;
    if (init)
        for (int v = 0; v < g->V; ++v) init_var(*g, *s, chains, chain, x, idx, v);
    double lp[MAX_STATES];
    const bool interp = pots->interpreted != 0;
    const HostCtx ctx{g, pots, s, chains, chain, x, idx};
    for (int it = it_begin; it < it_end; ++it)
        for (int k = 0; k < (s->n_colours ? s->col_ptr[s->n_colours] : 0); ++k) {
            if (interp) update<true>(ctx, it, s->col_var[k], lp, 1);
            else update<false>(ctx, it, s->col_var[k], lp, 1);
        }
    return LHVI_OK;
}

}  // extern "C"
