// npvi_dev.hpp -- the device side that csrc/npvi.hip and csrc/oneshot.hip share: the factor kernel (with its switch for the
// Bethe-free-energy expectant) and its launch, the fixed-order block reduction and the gather kernels (with their switch for what
// is added to the edges' sums).  npvi_colsum_kernel and npvi_update_kernel are defined in npvi.hip.  The host side the two share --
// workspace, checks, the Adam loops, the entry points' bodies -- is csrc/npvi_run.hpp.
#pragma once
#include "common.hpp"
#include "npvi.hpp"

namespace lhvi {
namespace npvi {

template <bool INTERP, int BLK> struct DevStack { using type = MlnLdsStack<BLK>; static constexpr int DOUBLES = MLN_STACK * BLK; };
template <int BLK> struct DevStack<false, BLK> { using type = MlnNoStack; static constexpr int DOUBLES = 1; };
constexpr int PT = MAXA + 1;        // doubles / ints per lane for the evaluation point (odd: neighbouring lanes on different banks)

template <int KP, int SL, int BLK, bool INTERP>
struct DevCtx {
    static constexpr int NM = 1;
    static constexpr int GROUPS = BLK / KP;
    int gl, gn;
    double* xt;     // [SL][GROUPS] + group
    double* ct;
    double* qt;     // [SL][BLK] + thread
    double* zt;
    double* px;     // [BLK][PT] + thread * PT
    int* pi;
    typename DevStack<INTERP, BLK>::type st;
    __device__ __forceinline__ double* point() { return px; }
    __device__ __forceinline__ int* point_idx() { return pi; }
    __device__ __forceinline__ typename DevStack<INTERP, BLK>::type& stack() { return st; }
    __device__ __forceinline__ int m(int) const { return gl; }
    __device__ __forceinline__ double& x(int s) { return xt[s * GROUPS]; }
    __device__ __forceinline__ double& c(int s) { return ct[s * GROUPS]; }
    __device__ __forceinline__ double& q(int, int s) { return qt[s * BLK]; }
    __device__ __forceinline__ double& z(int, int s) { return zt[s * BLK]; }
    __device__ __forceinline__ double sum_m(double v) const {
#pragma unroll
        for (int d = 1; d < KP; d <<= 1) v += __shfl_xor(v, d, 64);
        return v;
    }
    __device__ __forceinline__ void sync() const {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
};

template <int SL> struct FacBlock { static constexpr int value = SL <= 8 ? 128 : 64; };

// BFE: the expectant of OneShot's Bethe free energy (factor_item)
template <int KP, int SL, int MA, bool INTERP, bool BFE = false>
__global__ void __launch_bounds__(FacBlock<SL>::value) npvi_factor_kernel(lhvi_graph_t g, lhvi_pots_t pots, lhvi_vi_t p,
                                                                          const double* __restrict__ fac_count, double* __restrict__ pe_c,
                                                                          double* __restrict__ pe_d, double* __restrict__ pf) {
    constexpr int BLK = FacBlock<SL>::value;
    using Ctx = DevCtx<KP, SL, BLK, INTERP>;
    __shared__ double sh_x[SL * Ctx::GROUPS], sh_c[SL * Ctx::GROUPS], sh_q[SL * BLK], sh_z[SL * BLK], sh_px[PT * BLK];
    __shared__ double sh_st[DevStack<INTERP, BLK>::DOUBLES];
    __shared__ int sh_pi[PT * BLK];
    const int grp = threadIdx.x / KP;
    const int64_t f = (int64_t)blockIdx.x * Ctx::GROUPS + grp;
    if (f >= g.F) return;                            // (whole groups leave together)
    Ctx ctx{(int)threadIdx.x % KP, KP, sh_x + grp, sh_c + grp, sh_q + threadIdx.x, sh_z + threadIdx.x, sh_px + threadIdx.x * PT,
            sh_pi + threadIdx.x * PT, {}};
    if constexpr (INTERP) ctx.st.base = sh_st + threadIdx.x;
    factor_item<MA, INTERP, SL, BFE>(g, pots, p, fac_count, (int)f, ctx, pe_c, pe_d, pf);
}

constexpr int NP_MAX = MAX_K * (MAX_K + 1) / 2;
constexpr int COLS_MAX = NP_MAX > MAX_K + 1 ? NP_MAX : MAX_K + 1;
constexpr int WAVES = BLOCK / WAVE;

// the workgroup's total of column `col` of the threads' values -> sh[wave][col]; block_cols_flush then adds the waves in index order
__device__ __forceinline__ void block_col_put(double* sh, int C, int col, double v) {
    const double t = dpp_wave_reduce(v, SumOp());
    if (threadIdx.x % WAVE == 0) sh[(threadIdx.x / WAVE) * C + col] = t;
}
__device__ __forceinline__ void block_cols_flush(const double* sh, int C, double* __restrict__ out) {
    __syncthreads();
    for (int col = threadIdx.x; col < C; col += BLOCK) {
        double t = sh[col];
        for (int wv = 1; wv < WAVES; ++wv) t += sh[wv * C + col];
        out[col] = t;
    }
}

// npvi.hip
__global__ void __launch_bounds__(BLOCK) npvi_colsum_kernel(const double* __restrict__ in, int64_t N, int C, double* __restrict__ part);
__global__ void __launch_bounds__(BLOCK) npvi_update_kernel(lhvi_graph_t g, int K, int Dmax, lhvi_npvi_opt_t o, Step a);

// SS: S + S^T of the entropy bound; with BFE the variable term's rows (gather_finish)
template <bool BFE = false>
__global__ void __launch_bounds__(BLOCK) npvi_gather_kernel(lhvi_graph_t g, lhvi_vi_t p, const double* __restrict__ var_count,
                                                            const double* __restrict__ SS, const double* __restrict__ pe_c,
                                                            const double* __restrict__ pe_d, double* __restrict__ g_c,
                                                            double* __restrict__ g_rho) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= (int64_t)g.V * p.K) return;
    const int v = (int)(i / p.K), m = (int)(i % p.K);
    const int lo = g.var_ptr[v], hi = g.var_ptr[v + 1];
    if (g.n_hubs > 0 && hi - lo > LHVI_HUB_DEGREE) return;          // a wavefront's (npvi_gather_hub_kernel)
    const VarInfo vi = var_info(g, v);
    double c0 = 0.0, c1 = 0.0;
    if (vi.hidden && vi.cont) {
        for (int j = lo; j < hi; ++j) {
            const double2 t = ld2(pe_c, (int64_t)g.var_edge[j] * p.K + m);
            c0 += t.x; c1 += t.y;
        }
    } else if (vi.hidden) {
        for (int t = 0; t < vi.n; ++t) {
            double s = 0.0;
            for (int j = lo; j < hi; ++j) s += pe_d[((int64_t)g.var_edge[j] * p.K + m) * p.Dmax + t];
            g_rho[i * p.Dmax + t] = s;
        }
    }
    gather_finish<BFE>(g, p, var_count, SS, v, m, vi, c0, c1, g_c, g_rho);
}

template <bool BFE = false>
__global__ void __launch_bounds__(BLOCK) npvi_gather_hub_kernel(lhvi_graph_t g, lhvi_vi_t p, const double* __restrict__ var_count,
                                                                const double* __restrict__ SS, const double* __restrict__ pe_c,
                                                                const double* __restrict__ pe_d, double* __restrict__ g_c,
                                                                double* __restrict__ g_rho) {
    const int64_t item = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) / WAVE;
    const int lane = threadIdx.x % WAVE;
    if (item >= (int64_t)g.n_hubs * p.K) return;                    // (whole wavefronts)
    const int v = g.hub_vars[item / p.K], m = (int)(item % p.K);
    const int lo = g.var_ptr[v], hi = g.var_ptr[v + 1];
    const VarInfo vi = var_info(g, v);
    double c0 = 0.0, c1 = 0.0;
    if (vi.hidden && vi.cont) {
        for (int j = lo + lane; j < hi; j += WAVE) {
            const double2 t = ld2(pe_c, (int64_t)g.var_edge[j] * p.K + m);
            c0 += t.x; c1 += t.y;
        }
        c0 = dpp_wave_reduce(c0, SumOp());
        c1 = dpp_wave_reduce(c1, SumOp());
    } else if (vi.hidden) {
        for (int t = 0; t < vi.n; ++t) {
            double s = 0.0;
            for (int j = lo + lane; j < hi; j += WAVE) s += pe_d[((int64_t)g.var_edge[j] * p.K + m) * p.Dmax + t];
            s = dpp_wave_reduce(s, SumOp());
            if (lane == 0) g_rho[((int64_t)v * p.K + m) * p.Dmax + t] = s;
        }
    }
    if (lane == 0) gather_finish<BFE>(g, p, var_count, SS, v, m, vi, c0, c1, g_c, g_rho);
}

template <int SL, int MA, bool INTERP, bool BFE = false>
inline void launch_factors(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const double* fac_count, double* pe_c,
                           double* pe_d, double* pf, hipStream_t st) {
    constexpr int BLK = FacBlock<SL>::value;
#define LHVI_NPVI_LAUNCH(KP) \
    hipLaunchKernelGGL((npvi_factor_kernel<KP, SL, MA, INTERP, BFE>), dim3(grid_for(g->F, BLK / KP)), dim3(BLK), 0, st, *g, *pots, *p, \
                       fac_count, pe_c, pe_d, pf)
    if (p->K == 1) LHVI_NPVI_LAUNCH(1);
    else if (p->K == 2) LHVI_NPVI_LAUNCH(2);
    else if (p->K <= 4) LHVI_NPVI_LAUNCH(4);
    else LHVI_NPVI_LAUNCH(16);
#undef LHVI_NPVI_LAUNCH
}

// the factor build the caller's hints select
template <bool BFE>
inline void launch_factor_build(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const double* fac_count,
                                int32_t max_slots, int32_t max_arity, double* pe_c, double* pe_d, double* pf, hipStream_t st) {
    const bool lean = pots->interpreted == 0 && max_arity > 0 && max_arity <= 3;
    if (lean && max_slots > 0 && max_slots <= 8) launch_factors<8, 3, false, BFE>(g, pots, p, fac_count, pe_c, pe_d, pf, st);
    else if (lean) launch_factors<SLOTS, 3, false, BFE>(g, pots, p, fac_count, pe_c, pe_d, pf, st);
    else launch_factors<SLOTS, MAXA, true, BFE>(g, pots, p, fac_count, pe_c, pe_d, pf, st);
}

}  // namespace npvi
}  // namespace lhvi
