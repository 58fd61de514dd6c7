// gmkl.hip -- batched KL(p || q) of scalar Gaussian mixtures (utils.kl_continuous_logpdf on mixture marginals), gfx950.
//   gm_kl_kernel   one wavefront (one workgroup of 64 threads) per row.  The method -- range, panels, the Gauss-Kronrod rule on
//                  every panel, depth-first bisection against the bound -- is csrc/gmkl.hpp's, shared with the host twin at the
//                  end of this file; this file supplies the lane mapping.  docs/kernels_gmkl.md.
//
// The lane mapping (DevCtx: 3 x 21 nodes on 64 lanes, the component list, the panel list and the stack in LDS, wave-uniform
// control flow) is csrc/gmkl_dev.hpp, shared with pbp_kl_kernel of csrc/pbp.hip; here its q side is the second mixture
// (MixtureQ).  20 024 bytes of LDS per wave, 8 waves per CU.  No atomics, no allocation, no private arrays, no scratch
// (tests/test_gmkl_kernel_resources.py).  The scalar register file is the scarce resource here (the exp / log polynomials and
// the rule's weights are scalar constants): what lives as long as the kernel -- the row's pointers and bounds, the range, the
// children of a bisection -- goes through LDS into vector registers instead.
#include "gmkl_dev.hpp"

namespace lhvi {
namespace gmkl {

__global__ void __launch_bounds__(WAVE) gm_kl_kernel(int32_t Kp, const double* __restrict__ wp, const double* __restrict__ mup,
                                                     const double* __restrict__ varp, int32_t Kq, const double* __restrict__ wq,
                                                     const double* __restrict__ muq, const double* __restrict__ varq,
                                                     const double* __restrict__ a, const double* __restrict__ b, double epsabs,
                                                     double epsrel, double* __restrict__ kl, double* __restrict__ abserr,
                                                     int32_t* __restrict__ status, int32_t* __restrict__ neval) {
    __shared__ Shared sh;
    const int64_t r = blockIdx.x;
    if (threadIdx.x == 0) {
        sh.in = Row{Kp, Kq, wp + r * Kp, mup + r * Kp, varp + r * Kp, wq + r * Kq, muq + r * Kq, varq + r * Kq, a[r], b[r], epsabs, epsrel};
        sh.kl = kl + r, sh.abserr = abserr ? abserr + r : nullptr;
        sh.status = status ? status + r : nullptr, sh.neval = neval ? neval + r : nullptr;
    }
    __syncthreads();
    Row in = sh.in;
    in.Kp = Kp, in.Kq = Kq;         // the loop bounds stay scalar
    const MixtureQ q;
    DevCtx<MixtureQ> ctx(sh, (int)threadIdx.x, q);
    kl_row(in, ctx, sh.kl, sh.abserr, sh.status, sh.neval);
}

static int kl_check_p(int32_t R, int32_t Kp, const double* wp, const double* mup, const double* varp, const double* a,
                      const double* b, double epsabs, double epsrel, const double* kl) {
    if (R < 1 || Kp < 1 || !(epsabs >= 0.0) || !(epsrel >= 0.0)) return LHVI_E_ARG;
    if (!wp || !mup || !varp || !a || !b || !kl) return LHVI_E_ARG;
    return LHVI_OK;
}

static int kl_check(int32_t R, int32_t Kp, const double* wp, const double* mup, const double* varp, int32_t Kq, const double* wq,
                    const double* muq, const double* varq, const double* a, const double* b, double epsabs, double epsrel,
                    const double* kl) {
    if (Kq < 1 || !wq || !muq || !varq) return LHVI_E_ARG;
    return kl_check_p(R, Kp, wp, mup, varp, a, b, epsabs, epsrel, kl);
}

}  // namespace gmkl
}  // namespace lhvi

using namespace lhvi;
using namespace lhvi::gmkl;

extern "C" {

size_t lhvi_gm_kl_ws_doubles(int32_t R) {
    (void)R;
    return 0;           // the panel list and the stack of a row are in LDS
}

int lhvi_gm_kl(int32_t R, int32_t Kp, const double* wp, const double* mup, const double* varp, int32_t Kq, const double* wq,
               const double* muq, const double* varq, const double* a, const double* b, double epsabs, double epsrel, double* ws,
               double* kl, double* abserr, int32_t* status, int32_t* neval, void* stream) {
    (void)ws;
    const int rc = kl_check(R, Kp, wp, mup, varp, Kq, wq, muq, varq, a, b, epsabs, epsrel, kl);
    if (rc) return rc;
    hipLaunchKernelGGL(gm_kl_kernel, dim3((unsigned)R), dim3(WAVE), 0, as_stream(stream), Kp, wp, mup, varp, Kq, wq, muq, varq, a,
                       b, epsabs, epsrel, kl, abserr, status, neval);
    return check_launch();
}

int lhvi_gm_kl_host(int32_t R, int32_t Kp, const double* wp, const double* mup, const double* varp, int32_t Kq, const double* wq,
                    const double* muq, const double* varq, const double* a, const double* b, double epsabs, double epsrel,
                    double* kl, double* abserr, int32_t* status, int32_t* neval) {
    const int rc = kl_check(R, Kp, wp, mup, varp, Kq, wq, muq, varq, a, b, epsabs, epsrel, kl);
    if (rc) return rc;
    HostCtx ctx;
    for (int64_t r = 0; r < R; ++r) {
        const Row in{Kp, Kq, wp + r * Kp, mup + r * Kp, varp + r * Kp, wq + r * Kq, muq + r * Kq, varq + r * Kq, a[r], b[r], epsabs, epsrel};
        kl_row(in, ctx, kl + r, abserr ? abserr + r : nullptr, status ? status + r : nullptr, neval ? neval + r : nullptr);
    }
    return LHVI_OK;
}

int lhvi_gm_kl_fn_host(int32_t R, int32_t Kp, const double* wp, const double* mup, const double* varp,
                       double (*logq)(double x, int64_t row, void* user), void* user, const double* a, const double* b,
                       double epsabs, double epsrel, double* kl, double* abserr, int32_t* status, int32_t* neval) {
    const int rc = kl_check_p(R, Kp, wp, mup, varp, a, b, epsabs, epsrel, kl);
    if (rc || !logq) return LHVI_E_ARG;
    HostCtxT<HostFnQ> ctx;
    ctx.q.logq = logq, ctx.q.user = user;
    for (int64_t r = 0; r < R; ++r) {
        const Row in{Kp, 0, wp + r * Kp, mup + r * Kp, varp + r * Kp, nullptr, nullptr, nullptr, a[r], b[r], epsabs, epsrel};
        ctx.q.row = r;
        kl_row(in, ctx, kl + r, abserr ? abserr + r : nullptr, status ? status + r : nullptr, neval ? neval + r : nullptr);
    }
    return LHVI_OK;
}

}  // extern "C"
