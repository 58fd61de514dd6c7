// gibbs.hip -- block Gibbs sampling in a hybrid Gaussian MRF (gibbs/hybrid_gaussian_mrf.py::block_gibbs_sample), gfx950.
//   gibbs_chain_kernel   iterations [it_begin, it_end) of one chain per group of `lanes` lanes of a one-wavefront workgroup;
//                        the chain's workspace in LDS (csrc/gibbs.hpp: J / L with exact.hpp's odd row stride, b, y, x_c, x_d,
//                        lprobs, the reduced tables when they fit), its state in the caller's x_d between launches
//   gibbs_init_kernel    the initial x_d from the Philox stream
#include "common.hpp"
#include "gibbs.hpp"
#include "hg_launch.hpp"

namespace lhvi {
namespace gibbs {

constexpr int IB = 256;

using hg::DevCtx;
using hg::lds_disc_doubles;

__global__ void __launch_bounds__(WAVE) gibbs_chain_kernel(lhvi_gibbs_t g, int64_t chains, int it_begin, int it_end, int lanes,
                                                           int32_t* x_d, const double* z, const double* u, int32_t* disc,
                                                           double* cont, int32_t* counts, double* sum1, double* sum2,
                                                           unsigned long long* bad) {
    extern __shared__ double lds[];
    const int Nc = g.ex.Nc, Nd = g.ex.Nd;
    const int gpb = WAVE / lanes, grp = threadIdx.x / lanes;
    const int64_t idx = (int64_t)blockIdx.x * gpb + grp;
    const bool valid = idx < chains;
    const int64_t chain = valid ? idx : chains - 1;             // a padding group repeats the last chain, stores nothing
    const int ws = (ws_doubles(Nc, Nd, lds_disc_doubles(g)) + 1) & ~1;
    DevCtx ctx{(int)threadIdx.x % lanes, lanes};
    // a padding group has a scratch row of its own (rows are allocated for a multiple of 64 chains)
    const Workspace w = layout(g, lds + grp * ws, g.table_scratch ? g.table_scratch + idx * g.table_doubles : nullptr);
    for (int n = ctx.lane; n < Nd; n += lanes) w.dig[n] = x_d[chain * Nd + n];
    ctx.sync();
    const Draws dr{g.seed, z, u, chains, chain, Nc, Nd, g.disc_block_its};
    const int n_states = Nd ? g.dstate_off[Nd] : 0;
    Out o{nullptr, nullptr, nullptr, nullptr, nullptr};
    if (valid) {
        o.disc = disc ? disc + chain * g.num_samples * Nd : nullptr;
        o.cont = cont ? cont + chain * g.num_samples * Nc : nullptr;
        o.counts = counts ? counts + chain * n_states : nullptr;
        o.sum1 = sum1 ? sum1 + chain * Nc : nullptr;
        o.sum2 = sum2 ? sum2 + chain * (Nc * (Nc + 1) / 2) : nullptr;
    }
    bool dead = !valid;
    for (int it = it_begin; it < it_end; ++it) {
        const bool was_dead = dead;
        const int rc = iteration(g, it, dr, w, ctx, dead, o);
        if (rc && !was_dead && ctx.lane == 0)
            atomicMin(bad, ((unsigned long long)chain << 32) | (unsigned long long)(unsigned)it);
    }
    if (valid)
        for (int n = ctx.lane; n < Nd; n += lanes) x_d[chain * Nd + n] = w.dig[n];
}

__global__ void __launch_bounds__(IB) gibbs_init_kernel(lhvi_gibbs_t g, int64_t chains, int32_t* x_d) {
    const int64_t i = (int64_t)blockIdx.x * IB + threadIdx.x;
    if (i >= chains * g.ex.Nd) return;
    const int64_t c = i / g.ex.Nd;
    const int n = (int)(i % g.ex.Nd), d = g.ex.dstates[n];
    double u0, u1;
    uniform2(g.seed, (uint32_t)c, (uint32_t)n, 0u, TAG_INIT, u0, u1);
    const int k = (int)(u0 * (double)d);
    x_d[i] = k < d - 1 ? k : d - 1;
}

}  // namespace gibbs
}  // namespace lhvi

using namespace lhvi;
using namespace lhvi::gibbs;

extern "C" {

size_t lhvi_gibbs_lds_bytes(int32_t Nc, int32_t Nd, int32_t table_doubles, int32_t lanes) {
    if (Nc < 0 || Nd < 0 || table_doubles < 0 || !hg::lanes_ok(lanes)) return 0;
    return hg::wave_lds_bytes(lanes, ws_doubles(Nc, Nd, table_doubles));
}

int lhvi_gibbs_init(const lhvi_gibbs_t* m, int64_t chains, int32_t* x_d, void* stream) {
    const int rc = hg::gibbs_check(m, hg::ALL_COUNTS);
    if (rc) return rc;
    if (chains < 0 || chains > 0xffffffffLL) return LHVI_E_ARG;
    if (chains == 0 || m->ex.Nd == 0) return LHVI_OK;
    if (!x_d) return LHVI_E_ARG;
    hipLaunchKernelGGL(gibbs_init_kernel, dim3(grid_for(chains * m->ex.Nd, IB)), dim3(IB), 0, as_stream(stream), *m, chains, x_d);
    return check_launch();
}

int lhvi_gibbs_run(const lhvi_gibbs_t* m, int64_t chains, int32_t it_begin, int32_t it_end, int32_t lanes, int32_t* x_d,
                   const double* z, const double* u, int32_t* disc, double* cont, int32_t* counts, double* sum1, double* sum2,
                   uint64_t* bad, void* stream) {
    int rc = hg::gibbs_check(m, hg::ALL_COUNTS);
    if (rc) return rc;
    if (chains < 0 || chains > 0xffffffffLL || it_begin < 0 || it_end < it_begin || !bad) return LHVI_E_ARG;
    if ((m->ex.Nd && !x_d) || !hg::lanes_ok(lanes)) return LHVI_E_ARG;
    const int64_t work = it_end == it_begin ? 0 : chains;
    hg::WaveShape sh;
    rc = hg::wave_shape(work, lanes, ws_doubles(m->ex.Nc, m->ex.Nd, lds_disc_doubles(*m)), sh);
    if (rc || !work) return rc;
    hipLaunchKernelGGL(gibbs_chain_kernel, dim3((unsigned)sh.blocks), dim3(WAVE), sh.lds, as_stream(stream), *m, chains, (int)it_begin,
                       (int)it_end, (int)lanes, x_d, z, u, disc, cont, counts, sum1, sum2,
                       reinterpret_cast<unsigned long long*>(bad));
    return check_launch();
}

int lhvi_gibbs_chain_host(const lhvi_gibbs_t* m, int32_t it_begin, int32_t it_end, int32_t* x_d, const double* z, const double* u,
                          int32_t* disc, double* cont, int32_t* counts, double* sum1, double* sum2) {
    const int rc = hg::gibbs_check(m, hg::ALL_COUNTS);
    if (rc) return rc;
    const int Nc = m->ex.Nc, Nd = m->ex.Nd;
    if (it_begin < 0 || it_end < it_begin || (Nd && !x_d) || (Nc && !z) || (Nd && m->disc_block_its && !u)) return LHVI_E_ARG;
    hg::HostWork hw(*m);
    const lhvi_gibbs_t& g = hw.g;
    const Workspace w = layout(g, hw.alloc(ws_doubles(Nc, Nd, hw.dd) + 2), nullptr);
    hw.digits_in(w, x_d);
    const Draws dr{g.seed, z, u, 1, 0, Nc, Nd, g.disc_block_its};
    const Out o{disc, cont, counts, sum1, sum2};
    bool dead = false;
    for (int it = it_begin; it < it_end; ++it) iteration(g, it, dr, w, exact::HostCtx(), dead, o);
    hw.digits_out(w, x_d);
    return dead ? LHVI_E_NOT_PD : LHVI_OK;
}

}  // extern "C"
