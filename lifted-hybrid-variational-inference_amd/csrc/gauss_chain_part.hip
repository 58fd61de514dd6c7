// gauss_chain_part.hip -- the block-tridiagonal Gaussian systems of gauss_chain.hip solved in S segments along time: one level of
// nested dissection, for the single long chain that one workgroup walks too slowly.  Arithmetic, partition and workspace layout:
// csrc/gauss_chain.hpp; docs/kernels_gauss_chain.md.  Three launches on the caller's stream:
//   gc_part_stage1_kernel<P>   one 256-thread workgroup per (system, interior): chain_solve on the interior, its two spikes, its
//                              blocks of G and g (buffers as gc_solve_kernel<P>: LDS below P = 64, else the interior's own tiles)
//   gc_part_assemble_kernel    one workgroup per (system, separator): D~, O~, h~ of the reduced chain, then gc_solve_kernel<P>
//                              through lhvi_gauss_chain_solve on the B reduced chains, covariances kept
//   gc_part_correct_kernel<P>  one workgroup per (system, interior): the correction of its blocks, the separator after it, and
//                              for interior 0 the system's logdet and bad pivot
// No atomics and no waiting between workgroups; every result element has one owner.
#include "common.hpp"
#include "gauss_chain.hpp"

namespace lhvi {
namespace gchain {

constexpr int PART_GT = 256;

struct PartCtx {
    int lane, lanes;
    __device__ __forceinline__ void sync() const { __syncthreads(); }
};

// the buffers of chain_solve in `mem` (LDS or heap); below P = 64 all of them, else the tile and the vectors
template <int P>
LHVI_GE_HD constexpr int part_mem_doubles() {
    using S = Shape<P>;
    return S::TILE_A + 2 * S::E + 3 * P + (S::BUFS_IN_LDS ? 5 * S::BUF : 0);
}

template <int P>
LHVI_GE_HD Bufs part_bufs(double* mem, const PartArgs& g, int64_t b, int64_t p) {
    using S = Shape<P>;
    Bufs w;
    double* q = mem;
    w.a = q, q += S::TILE_A;
    w.ldiag = q, q += S::E;
    w.xdiag = q, q += S::E;
    w.yv = q, q += P;
    w.rv = q, q += P;
    w.mv = q, q += P;
    w.Sm = w.a;
    if (S::BUFS_IN_LDS) {
        w.Wm = q, w.Cm = q + S::BUF, w.Gm = q + 2 * S::BUF, w.Hm = q + 3 * S::BUF, w.Sg = q + 4 * S::BUF;
    } else {
        part_workspace_bufs<P>(g, b, p, w);
    }
    return w;
}

// the two tiles of T that part_correct needs
template <int P>
LHVI_GE_HD Bufs part_correct_bufs(double* mem, const PartArgs& g, int64_t b, int64_t p) {
    using S = Shape<P>;
    Bufs w = Bufs();
    if (S::BUFS_IN_LDS) {
        w.Wm = mem, w.Cm = mem + S::BUF;
    } else {
        part_workspace_bufs<P>(g, b, p, w);
    }
    return w;
}

template <int P>
__global__ void __launch_bounds__(PART_GT) gc_part_stage1_kernel(PartArgs g) {
    __shared__ double sm[part_mem_doubles<P>()];
    const int64_t b = blockIdx.x / g.q.S, p = blockIdx.x % g.q.S;
    part_stage1<P>(g, b, p, part_bufs<P>(sm, g, b, p), PartCtx{(int)threadIdx.x, PART_GT});
}

__global__ void __launch_bounds__(PART_GT) gc_part_assemble_kernel(PartArgs g) {
    part_assemble(g, blockIdx.x / g.l.R, blockIdx.x % g.l.R, PartCtx{(int)threadIdx.x, PART_GT});
}

template <int P>
__global__ void __launch_bounds__(PART_GT) gc_part_correct_kernel(PartArgs g) {
    __shared__ double sm[Shape<P>::BUFS_IN_LDS ? 2 * Shape<P>::BUF : 1];
    const int64_t b = blockIdx.x / g.q.S, p = blockIdx.x % g.q.S;
    part_correct<P>(g, b, p, part_correct_bufs<P>(sm, g, b, p), PartCtx{(int)threadIdx.x, PART_GT});
}

template <int P>
static void part_host_stages(const PartArgs& g, int stage) {
    double* mem = new double[part_mem_doubles<P>()];
    for (int64_t b = 0; b < g.B; ++b)
        for (int64_t p = 0; p < g.q.S; ++p) {
            if (stage == 1) part_stage1<P>(g, b, p, part_bufs<P>(mem, g, b, p), gauss::HostCtx());
            if (stage == 2 && p < g.l.R) part_assemble(g, b, p, gauss::HostCtx());
            if (stage == 3) part_correct<P>(g, b, p, part_correct_bufs<P>(mem, g, b, p), gauss::HostCtx());
        }
    delete[] mem;
}

static int part_arg_check(int64_t B, int64_t M, int64_t n, int64_t S) {
    if (B < 0 || M < 0 || n < 1 || S < 1) return LHVI_E_ARG;
    if (n > MAX_BLOCK || B > 0x7fffffff) return LHVI_E_UNSUPPORTED;
    return LHVI_OK;
}

static PartArgs part_args(int64_t B, int64_t M, int64_t n, int64_t S, const double* D, const double* O, const double* h, double* ws,
                          double* mu, double* var, double* cov, double* cross, double* logdet, int32_t* bad) {
    PartArgs g;
    g.B = B, g.M = M, g.n = (int)n;
    g.q = partition_of(M, S);
    g.l = part_layout(B, M, (int)n, padded_edge((int)n), g.q.S);
    g.D = D, g.O = O, g.h = h, g.ws = ws, g.mu = mu, g.var = var, g.cov = cov, g.cross = cross, g.logdet = logdet, g.bad = bad;
    return g;
}

}  // namespace gchain
}  // namespace lhvi

using namespace lhvi;
using namespace lhvi::gchain;

#define LHVI_GC_PART_DISPATCH(P_, CALL)      \
    switch (P_) {                            \
        case 8: CALL(8); break;              \
        case 16: CALL(16); break;            \
        case 32: CALL(32); break;            \
        case 64: CALL(64); break;            \
        default: CALL(128); break;           \
    }

extern "C" {

int64_t lhvi_gauss_chain_segments(int64_t M, int64_t S, int64_t* first, int64_t* last) {
    if (M < 1 || S < 1) return 0;
    const Partition q = partition_of(M, S);
    for (int64_t p = 0; p < q.S; ++p) {
        if (first) first[p] = first_block(q, p);
        if (last) last[p] = last_block(q, p);
    }
    return q.S;
}

size_t lhvi_gauss_chain_part_ws_doubles(int64_t B, int64_t M, int64_t n, int64_t S) {
    if (part_arg_check(B, M, n, S) != LHVI_OK) return 0;
    const Partition q = partition_of(M, S);
    if (q.S == 1) return lhvi_gauss_chain_ws_doubles(B, M, n);
    return (size_t)part_layout(B, M, (int)n, padded_edge((int)n), q.S).total;
}

int lhvi_gauss_chain_part_solve(int64_t B, int64_t M, int64_t n, int64_t S, const double* D, const double* O, const double* h,
                                double* ws, double* mu, double* var, double* cov, double* cross, double* logdet, int32_t* bad,
                                void* stream) {
    int rc = part_arg_check(B, M, n, S);
    if (rc) return rc;
    if (B == 0 || M == 0) return LHVI_OK;
    if (partition_of(M, S).S == 1) return lhvi_gauss_chain_solve(B, M, n, D, O, h, ws, mu, var, cov, cross, logdet, bad, stream);
    if (!D || !O || !h || !ws || !mu || !var || !logdet || !bad) return LHVI_E_ARG;
    const PartArgs g = part_args(B, M, n, S, D, O, h, ws, mu, var, cov, cross, logdet, bad);
    if (B * g.q.S > 0x7fffffff) return LHVI_E_UNSUPPORTED;
    hipStream_t st = as_stream(stream);
    const dim3 interiors((unsigned)(B * g.q.S)), separators((unsigned)(B * g.l.R)), block(PART_GT);
    const int P = padded_edge((int)n);
#define LHVI_GC_STAGE1(P_) hipLaunchKernelGGL(gc_part_stage1_kernel<P_>, interiors, block, 0, st, g)
    LHVI_GC_PART_DISPATCH(P, LHVI_GC_STAGE1)
#undef LHVI_GC_STAGE1
    hipLaunchKernelGGL(gc_part_assemble_kernel, separators, block, 0, st, g);
    if ((rc = check_launch())) return rc;
    rc = lhvi_gauss_chain_solve(B, g.l.R, n, ws + g.l.Dr, ws + g.l.Or, ws + g.l.hr, ws + g.l.wsr, ws + g.l.mur, ws + g.l.varr,
                                ws + g.l.covr, ws + g.l.crossr, ws + g.l.logdetr, reinterpret_cast<int32_t*>(ws + g.l.badr), stream);
    if (rc) return rc;
#define LHVI_GC_CORRECT(P_) hipLaunchKernelGGL(gc_part_correct_kernel<P_>, interiors, block, 0, st, g)
    LHVI_GC_PART_DISPATCH(P, LHVI_GC_CORRECT)
#undef LHVI_GC_CORRECT
    return check_launch();
}

int lhvi_gauss_chain_part_host(int64_t B, int64_t M, int64_t n, int64_t S, const double* D, const double* O, const double* h,
                               double* ws, double* mu, double* var, double* cov, double* cross, double* logdet, int32_t* bad) {
    int rc = part_arg_check(B, M, n, S);
    if (rc) return rc;
    if (B == 0 || M == 0) return LHVI_OK;
    if (partition_of(M, S).S == 1) return lhvi_gauss_chain_host(B, M, n, D, O, h, ws, mu, var, cov, cross, logdet, bad);
    if (!D || !O || !h || !ws || !mu || !var || !logdet || !bad) return LHVI_E_ARG;
    const PartArgs g = part_args(B, M, n, S, D, O, h, ws, mu, var, cov, cross, logdet, bad);
    const int P = padded_edge((int)n);
#define LHVI_GC_HOST1(P_) part_host_stages<P_>(g, 1), part_host_stages<P_>(g, 2)
    LHVI_GC_PART_DISPATCH(P, LHVI_GC_HOST1)
#undef LHVI_GC_HOST1
    rc = lhvi_gauss_chain_host(B, g.l.R, n, ws + g.l.Dr, ws + g.l.Or, ws + g.l.hr, ws + g.l.wsr, ws + g.l.mur, ws + g.l.varr,
                               ws + g.l.covr, ws + g.l.crossr, ws + g.l.logdetr, reinterpret_cast<int32_t*>(ws + g.l.badr));
    if (rc != LHVI_OK && rc != LHVI_E_NOT_PD) return rc;
#define LHVI_GC_HOST3(P_) part_host_stages<P_>(g, 3)
    LHVI_GC_PART_DISPATCH(P, LHVI_GC_HOST3)
#undef LHVI_GC_HOST3
    for (int64_t b = 0; b < B; ++b)
        if (bad[2 * b] >= 0) return LHVI_E_NOT_PD;
    return LHVI_OK;
}

}  // extern "C"
