// hg_energy.hip -- joint log potentials of assignments of a hybrid Gaussian MRF and the first-index arg-max over them (the
// joint MAP of the exact and Gibbs baselines: osi/hybrid_mln_experiment.py:267-279), gfx950.  docs/kernels_hg_energy.md.
//   hg_energy_kernel        one lane per assignment, one wavefront per workgroup.  The workgroup's 64 x Nc block of x_c is staged
//                           with coalesced loads into LDS at the odd row stride Nc | 1 (a lane's row starts on a bank of its own);
//                           the descriptor words are wave-uniform, only the parameter offset (the local configuration) and the
//                           row differ per lane.  The arithmetic is csrc/hg_energy.hpp's, shared with the host twin.
//   argmax_partial_kernel / argmax_final_kernel    (value, index) of the largest non-NaN entry, the smallest index on ties: a
//                           comparison reduction, so the answer is the definition's whatever the slices and the tree.
#include "common.hpp"
#include "hg_energy.hpp"

namespace lhvi {
namespace hg {

constexpr int RB = 256;            // workgroup of the arg-max
constexpr int PARTS = 1024;        // partial results of its first stage

struct Row {                       // the continuous point of an assignment: its row in LDS (device) or of x_c (host)
    const double* row;
    LHVI_HD double operator()(int v) const { return row[v]; }
};

// IMPLICIT: assignment s has the digits of configuration cfg_begin + s; else those of x_d [S][Nd]
template <bool IMPLICIT>
__global__ void __launch_bounds__(WAVE) hg_energy_kernel(lhvi_exact_t m, int64_t S, int64_t cfg_begin,
                                                         const int32_t* __restrict__ x_d, const double* __restrict__ x_c,
                                                         double* __restrict__ out) {
    extern __shared__ double lds[];
    const int Nc = m.Nc, ld = exact::ld_of(Nc);
    const int64_t s0 = (int64_t)blockIdx.x * WAVE;
    const int rows = S - s0 < WAVE ? (int)(S - s0) : WAVE;      // >= 1: the grid is ceil(S / 64)
    const int n = rows * Nc;                                    // the block's part of x_c is contiguous: n doubles from s0 * Nc
    for (int i = threadIdx.x; i < n; i += WAVE) {
        const int r = i / Nc;
        lds[r * ld + (i - r * Nc)] = x_c[s0 * Nc + i];
    }
    __syncthreads();
    if ((int)threadIdx.x >= rows) return;                       // a lane past S reads no row and stores nothing
    const int64_t s = s0 + threadIdx.x;
    const Row x{lds + threadIdx.x * ld};
    out[s] = IMPLICIT ? energy(m, CfgDigits{m.dstride, m.dstates, cfg_begin + s}, x)
                      : energy(m, RowDigits{x_d + s * m.Nd}, x);
}

__device__ __forceinline__ Best block_best(Best b, double* shv, int64_t* shi) {
    shv[threadIdx.x] = b.v, shi[threadIdx.x] = b.i;
    __syncthreads();
    for (int s = RB / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            b = best_merge(b, Best{shv[threadIdx.x + s], shi[threadIdx.x + s]});      // b is the thread's own slot
            shv[threadIdx.x] = b.v, shi[threadIdx.x] = b.i;
        }
        __syncthreads();
    }
    return Best{shv[0], shi[0]};
}

// stage 1: (pv, pi)[b] = the best of the b-th contiguous slice (index -1: the slice holds no number)
__global__ void __launch_bounds__(RB) argmax_partial_kernel(int64_t n, const double* __restrict__ v, double* __restrict__ pv,
                                                            int64_t* __restrict__ pi) {
    __shared__ double shv[RB];
    __shared__ int64_t shi[RB];
    const int64_t per = (n + gridDim.x - 1) / gridDim.x, lo = per * blockIdx.x, hi = lo + per < n ? lo + per : n;
    Best b = best_none();
    for (int64_t i = lo + threadIdx.x; i < hi; i += RB) best_take(b, v[i], i);
    b = block_best(b, shv, shi);
    if (threadIdx.x == 0) pv[blockIdx.x] = b.v, pi[blockIdx.x] = b.i;
}

// stage 2 (one workgroup)
__global__ void __launch_bounds__(RB) argmax_final_kernel(int parts, const double* __restrict__ pv, const int64_t* __restrict__ pi,
                                                          int64_t* __restrict__ index, double* __restrict__ value) {
    __shared__ double shv[RB];
    __shared__ int64_t shi[RB];
    Best b = best_none();
    for (int i = threadIdx.x; i < parts; i += RB) b = best_merge(b, Best{pv[i], pi[i]});
    b = block_best(b, shv, shi);
    if (threadIdx.x == 0) {
        index[0] = b.i;
        value[0] = b.i < 0 ? __builtin_nan("") : b.v;
    }
}

static int energy_check(const lhvi_exact_t* m, int64_t S, int64_t cfg_begin, const int32_t* x_d, const double* x_c,
                        const double* out) {
    if (!m || S < 0 || m->Nd < 0 || m->Nc < 0 || m->n_quad < 0 || m->n_tab < 0) return LHVI_E_ARG;
    if (m->Nc > LHVI_EXACT_MAX_NC) return LHVI_E_UNSUPPORTED;
    if (S == 0) return LHVI_OK;
    if (!out || (m->Nc && !x_c)) return LHVI_E_ARG;
    if (!x_d && (cfg_begin < 0 || (m->Nd && (!m->dstates || !m->dstride)))) return LHVI_E_ARG;
    if (m->n_quad && (!m->quad_ptr || !m->quad_desc || !m->quad_par)) return LHVI_E_ARG;
    if (m->n_tab && (!m->tab_ptr || !m->tab_desc || !m->tab_par)) return LHVI_E_ARG;
    return LHVI_OK;
}

}  // namespace hg
}  // namespace lhvi

using namespace lhvi;
using namespace lhvi::hg;

extern "C" {

int lhvi_hg_energy(const lhvi_exact_t* m, int64_t S, int64_t cfg_begin, const int32_t* x_d, const double* x_c, double* out,
                   void* stream) {
    const int rc = energy_check(m, S, cfg_begin, x_d, x_c, out);
    if (rc || S == 0) return rc;
    const int64_t blocks = (S + WAVE - 1) / WAVE;
    if (blocks > 0x7fffffff) return LHVI_E_UNSUPPORTED;
    const size_t lds = (size_t)WAVE * exact::ld_of(m->Nc) * sizeof(double);
    if (x_d)
        hipLaunchKernelGGL(hg_energy_kernel<false>, dim3((unsigned)blocks), dim3(WAVE), lds, as_stream(stream), *m, S, cfg_begin, x_d,
                           x_c, out);
    else
        hipLaunchKernelGGL(hg_energy_kernel<true>, dim3((unsigned)blocks), dim3(WAVE), lds, as_stream(stream), *m, S, cfg_begin, x_d,
                           x_c, out);
    return check_launch();
}

int lhvi_hg_energy_host(const lhvi_exact_t* m, int64_t S, int64_t cfg_begin, const int32_t* x_d, const double* x_c, double* out) {
    const int rc = energy_check(m, S, cfg_begin, x_d, x_c, out);
    if (rc) return rc;
    for (int64_t s = 0; s < S; ++s) {
        const Row x{m->Nc ? x_c + s * m->Nc : nullptr};
        out[s] = x_d ? energy(*m, RowDigits{x_d + s * m->Nd}, x) : energy(*m, CfgDigits{m->dstride, m->dstates, cfg_begin + s}, x);
    }
    return LHVI_OK;
}

size_t lhvi_argmax_first_ws_bytes(int64_t n) {
    (void)n;
    return (size_t)PARTS * (sizeof(double) + sizeof(int64_t));
}

int lhvi_argmax_first(int64_t n, const double* v, int64_t* index, double* value, void* ws, void* stream) {
    if (n < 0 || (n && !v) || !index || !value || !ws) return LHVI_E_ARG;
    const int parts = (int)(n < (int64_t)PARTS * RB ? (n + RB - 1) / RB : PARTS);
    double* pv = static_cast<double*>(ws);
    int64_t* pi = reinterpret_cast<int64_t*>(pv + PARTS);
    hipStream_t st = as_stream(stream);
    if (parts) hipLaunchKernelGGL(argmax_partial_kernel, dim3(parts), dim3(RB), 0, st, n, v, pv, pi);
    hipLaunchKernelGGL(argmax_final_kernel, dim3(1), dim3(RB), 0, st, parts, (const double*)pv, (const int64_t*)pi, index, value);
    return check_launch();
}

int lhvi_argmax_first_host(int64_t n, const double* v, int64_t* index, double* value) {
    if (n < 0 || (n && !v) || !index || !value) return LHVI_E_ARG;
    Best b = best_none();
    for (int64_t i = 0; i < n; ++i) best_take(b, v[i], i);
    index[0] = b.i;
    value[0] = b.i < 0 ? __builtin_nan("") : b.v;
    return LHVI_OK;
}

}  // extern "C"
