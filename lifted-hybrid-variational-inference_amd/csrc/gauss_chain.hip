// gauss_chain.hip -- exact marginals, log det J and neighbouring covariances of B block-tridiagonal Gaussian systems (the conditioned
// relational Kalman filters of Demo/RKF), gfx950.  Arithmetic and buffers: csrc/gauss_chain.hpp; docs/kernels_gauss_chain.md.
//   gc_solve_kernel<P>   one 256-thread workgroup per system walks the M blocks forward (Cholesky, W_t and C_t to the workspace)
//                        and backward (means, Sig_t, Sig[t, t+1]); P = the padded block edge
//     P = 8, 16, 32      every working buffer in LDS (row stride P + 1)
//     P = 64             the tile being factorised in LDS (gauss_exact's potrf_tile / trinv_tile), the other buffers in the
//                        system's workspace (five tiles of 33 KB: L2 resident)
//     P = 128            2 x 2 tiles of 64: the same, with S_t in the workspace too
// No atomics, one workgroup per system and a fixed order inside it: a system's bits depend on nothing else in the batch.
#include "common.hpp"
#include "gauss_chain.hpp"

namespace lhvi {
namespace gchain {

constexpr int GT = 256;

struct DevCtx {
    int lane, lanes;
    __device__ __forceinline__ void sync() const { __syncthreads(); }
};

template <int P>
__global__ void __launch_bounds__(GT) gc_solve_kernel(int64_t M, int n, const double* __restrict__ D, const double* __restrict__ O,
                                                      const double* __restrict__ h, double* ws, double* mu, double* var, double* cov,
                                                      double* cross, double* logdet, int32_t* bad) {
    using S = Shape<P>;
    constexpr int LDS_DOUBLES = S::TILE_A + 2 * S::E + 3 * P + (S::BUFS_IN_LDS ? 5 * S::BUF : 0);
    __shared__ double sm[LDS_DOUBLES];
    const System s = system_of(blockIdx.x, M, n, P, D, O, h, ws, mu, var, cov, cross, logdet, bad);
    Bufs w;
    double* p = sm;
    w.a = p, p += S::TILE_A;
    w.ldiag = p, p += S::E;
    w.xdiag = p, p += S::E;
    w.yv = p, p += P;
    w.rv = p, p += P;
    w.mv = p, p += P;
    w.Sm = w.a;
    if constexpr (S::BUFS_IN_LDS) {
        w.Wm = p, w.Cm = p + S::BUF, w.Gm = p + 2 * S::BUF, w.Hm = p + 3 * S::BUF, w.Sg = p + 4 * S::BUF;
    } else {
        workspace_bufs<P>(s, w);
    }
    chain_solve<P>(s, w, DevCtx{(int)threadIdx.x, GT});
}

template <int P>
static void host_system(const System& s) {
    using S = Shape<P>;
    double* mem = new double[S::TILE_A + 2 * S::E + 3 * P + (S::BUFS_IN_LDS ? 5 * S::BUF : 0)];
    Bufs w;
    double* p = mem;
    w.a = p, p += S::TILE_A;
    w.ldiag = p, p += S::E;
    w.xdiag = p, p += S::E;
    w.yv = p, p += P;
    w.rv = p, p += P;
    w.mv = p, p += P;
    w.Sm = w.a;
    if (S::BUFS_IN_LDS) {
        w.Wm = p, w.Cm = p + S::BUF, w.Gm = p + 2 * S::BUF, w.Hm = p + 3 * S::BUF, w.Sg = p + 4 * S::BUF;
    } else {
        workspace_bufs<P>(s, w);
    }
    chain_solve<P>(s, w, gauss::HostCtx());
    delete[] mem;
}

static int arg_check(int64_t B, int64_t M, int64_t n) {
    if (B < 0 || M < 0 || n < 1) return LHVI_E_ARG;
    if (n > MAX_BLOCK || B > 0x7fffffff) return LHVI_E_UNSUPPORTED;
    return LHVI_OK;
}

}  // namespace gchain
}  // namespace lhvi

using namespace lhvi;
using namespace lhvi::gchain;

extern "C" {

size_t lhvi_gauss_chain_ws_doubles(int64_t B, int64_t M, int64_t n) {
    if (arg_check(B, M, n) != LHVI_OK) return 0;
    return (size_t)(B * ws_per_system(M, padded_edge((int)n)));
}

int lhvi_gauss_chain_solve(int64_t B, int64_t M, int64_t n, const double* D, const double* O, const double* h, double* ws, double* mu,
                           double* var, double* cov, double* cross, double* logdet, int32_t* bad, void* stream) {
    const int rc = arg_check(B, M, n);
    if (rc) return rc;
    if (B == 0 || M == 0) return LHVI_OK;
    if (!D || !h || !ws || !mu || !var || !logdet || !bad || (M > 1 && !O)) return LHVI_E_ARG;
    hipStream_t st = as_stream(stream);
    const dim3 grid((unsigned)B), block(GT);
#define LHVI_GC_LAUNCH(P)                                                                                                       \
    hipLaunchKernelGGL(gc_solve_kernel<P>, grid, block, 0, st, M, (int)n, D, O, h, ws, mu, var, cov, cross, logdet, bad)
    switch (padded_edge((int)n)) {
        case 8: LHVI_GC_LAUNCH(8); break;
        case 16: LHVI_GC_LAUNCH(16); break;
        case 32: LHVI_GC_LAUNCH(32); break;
        case 64: LHVI_GC_LAUNCH(64); break;
        default: LHVI_GC_LAUNCH(128); break;
    }
#undef LHVI_GC_LAUNCH
    return check_launch();
}

int lhvi_gauss_chain_host(int64_t B, int64_t M, int64_t n, const double* D, const double* O, const double* h, double* ws, double* mu,
                          double* var, double* cov, double* cross, double* logdet, int32_t* bad) {
    const int rc = arg_check(B, M, n);
    if (rc) return rc;
    if (B == 0 || M == 0) return LHVI_OK;
    if (!D || !h || !ws || !mu || !var || !logdet || !bad || (M > 1 && !O)) return LHVI_E_ARG;
    const int P = padded_edge((int)n);
    int any_bad = 0;
    for (int64_t b = 0; b < B; ++b) {
        const System s = system_of(b, M, (int)n, P, D, O, h, ws, mu, var, cov, cross, logdet, bad);
        switch (P) {
            case 8: host_system<8>(s); break;
            case 16: host_system<16>(s); break;
            case 32: host_system<32>(s); break;
            case 64: host_system<64>(s); break;
            default: host_system<128>(s); break;
        }
        any_bad |= s.bad[0] >= 0;
    }
    return any_bad ? LHVI_E_NOT_PD : LHVI_OK;
}

}  // extern "C"
