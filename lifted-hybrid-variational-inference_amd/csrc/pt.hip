// pt.hip -- parallel tempering for the block Gibbs sampler of a hybrid Gaussian MRF (docs/kernels_pt.md), gfx950.
//   pt_ladder_kernel     iterations [it_begin, it_end) of one ladder of R replicas per R * lanes threads: a group of `lanes` lanes
//                        per replica, the R chain workspaces (csrc/ais.hpp) and the exchange slots (csrc/pt.hpp) in LDS, the
//                        ladder's state (x_d [R][Nd]) in the caller's array between launches.  A workgroup is R * lanes threads
//                        rounded up to whole wavefronts (at most 256); when R * lanes <= 32 it is one wavefront that holds
//                        64 / (R * lanes) ladders.  Every barrier is __syncthreads(): the groups of a ladder may sit in different
//                        wavefronts.
#include "common.hpp"
#include "pt.hpp"
#include "hg_launch.hpp"

namespace lhvi {
namespace pt {

constexpr int MAX_BLOCK = 256;
// the lane index of a padding group (the threads a workgroup has beyond its ladders, the ladders a grid has beyond `ladders`):
// it owns no row of any loop and is no lane 0, so it stores nothing; it reads the workspace of the workgroup's first replica
// and takes part in every barrier
constexpr int NO_LANE = 1 << 30;

using hg::DevCtx;
using hg::lds_disc_doubles;

struct Shape {
    int per_ladder, ladders_per_block, block;
};
// threads of a ladder, ladders of a workgroup, threads of a workgroup
__host__ __device__ inline Shape shape_of(int R, int lanes) {
    Shape s;
    s.per_ladder = R * lanes;
    s.ladders_per_block = s.per_ladder <= WAVE / 2 ? WAVE / s.per_ladder : 1;
    s.block = s.ladders_per_block > 1 ? WAVE : (s.per_ladder + WAVE - 1) / WAVE * WAVE;
    return s;
}

// Everything a launch passes beyond the model, as the kernel's SECOND argument (the model is the first, at offset 0 of the
// argument block).
struct Args {
    int64_t ladders;
    const double *betas, *mu0, *z, *u, *usw;
    int32_t *x_d, *disc, *counts, *swap_try, *swap_acc;
    double *cont, *sum1, *sum2;
    unsigned long long* bad;
    double tau0;
    int R, it_begin, it_end, swap_every, lanes;
};
// The model and the arguments are read from the argument block where they are used instead of being loaded once and held in
// scalar registers through the whole kernel, which are far too few for them (the asm keeps the compiler from hoisting the
// loads back to the top; the technique of pbp.hip's heavy_arg_reload).
template <class T>
__device__ __forceinline__ const T& arg_block(size_t offset) {
    auto p = (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(const T*)(p + offset);
}
// A value the compiler may no longer take as unchanged from one iteration to the next: what it derives from it (a comparison
// of a loop-invariant pointer with null, a mask of the lanes that are lane 0) is formed again where it is used instead of once
// before the loop, where each such mask would hold a scalar register pair through the whole loop.
template <class T>
__device__ __forceinline__ void per_lane(T& v) { asm volatile("" : "+v"(v)); }
template <class T>
__device__ __forceinline__ void per_wave(T& v) { asm volatile("" : "+s"(v)); }
constexpr size_t ARGS_OFFSET = (sizeof(lhvi_gibbs_t) + alignof(Args) - 1) / alignof(Args) * alignof(Args);
__device__ __forceinline__ const lhvi_gibbs_t& model() { return arg_block<lhvi_gibbs_t>(0); }
__device__ __forceinline__ const Args& args() { return arg_block<Args>(ARGS_OFFSET); }

__global__ void __launch_bounds__(MAX_BLOCK) pt_ladder_kernel(lhvi_gibbs_t, Args) {
    extern __shared__ double lds[];
    int Nc = model().ex.Nc, Nd = model().ex.Nd;
    int R = args().R, lanes = args().lanes;
    const Shape sh = shape_of(R, lanes);
    const int local = threadIdx.x / sh.per_ladder, within = threadIdx.x % sh.per_ladder;
    const int64_t idx = (int64_t)blockIdx.x * sh.ladders_per_block + local;
    const bool valid = local < sh.ladders_per_block && idx < args().ladders;
    // a padding group stands at the workgroup's first replica
    const int64_t ladder = valid ? idx : (int64_t)blockIdx.x * sh.ladders_per_block;
    const int slot = valid ? local : 0;
    int r = valid ? within / lanes : 0, live = valid;
    const int64_t chain = ladder * R + r;
    int lane = valid ? within % lanes : NO_LANE;
    DevCtx ctx{lane, lanes};
    const int dd = lds_disc_doubles(model());
    int cw = chain_doubles(Nc, Nd, dd);
    double* W = lds + (size_t)slot * ws_doubles(Nc, Nd, dd, R);
    gibbs::Workspace w;
    {
        const lhvi_gibbs_t& g = model();
        w = gibbs::layout(g, W + r * cw, g.table_scratch ? g.table_scratch + chain * g.table_doubles : nullptr);
    }
    const Slots sl = slots(Nc, Nd, dd, R, W);
    double* m0 = ais::base_mean(Nc, Nd, dd, W + r * cw);
    {
        const Args& a = args();
        for (int n = ctx.lane; n < Nd; n += lanes) w.dig[n] = a.x_d[chain * Nd + n];
        for (int i = ctx.lane; i < Nc; i += lanes) m0[i] = a.mu0[i];
    }
    ctx.sync();
    gibbs::Out o{nullptr, nullptr, nullptr, nullptr, nullptr};
    int32_t *tries = nullptr, *accs = nullptr;
    {
        const Args& a = args();
        const lhvi_gibbs_t& g = model();
        const int n_states = Nd ? g.dstate_off[Nd] : 0;
        if (valid && r == R - 1) {
            o.disc = a.disc ? a.disc + ladder * g.num_samples * Nd : nullptr;
            o.cont = a.cont ? a.cont + ladder * g.num_samples * Nc : nullptr;
            o.counts = a.counts ? a.counts + ladder * n_states : nullptr;
            o.sum1 = a.sum1 ? a.sum1 + ladder * Nc : nullptr;
            o.sum2 = a.sum2 ? a.sum2 + ladder * (Nc * (Nc + 1) / 2) : nullptr;
        }
        tries = a.swap_try ? a.swap_try + ladder * (R - 1) : nullptr;
        accs = a.swap_acc ? a.swap_acc + ladder * (R - 1) : nullptr;
    }
    double beta = args().betas[r];
    int dead = 0;                   // (an int in a vector register: as a bool it would be a lane mask held through every phase)
    for (int it = args().it_begin; it < args().it_end; ++it) {
        // (again before each phase: the masks of one phase do not live through the next)
        const auto refresh = [&] {
            per_wave(Nc); per_wave(Nd); per_wave(R); per_wave(lanes); per_wave(cw);
            per_lane(lane); per_lane(r); per_lane(live); per_lane(dead); per_lane(beta); per_lane(m0);
            per_lane(o.disc); per_lane(o.cont); per_lane(o.counts); per_lane(o.sum1); per_lane(o.sum2); per_lane(tries); per_lane(accs);
            per_lane(w.mat); per_lane(w.b); per_lane(w.y); per_lane(w.xc); per_lane(w.ldiag); per_lane(w.dinv); per_lane(w.lprobs);
            per_lane(w.tab); per_lane(w.dig);
            return DevCtx{lane, lanes};
        };
        DevCtx ctx = refresh();
        // 1. the transition; the first failed pivot of a ladder is reported once, by replica 0
        factor(model(), beta, ais::Base{args().tau0, m0}, w, ctx, sl, r);
        ctx.sync();
        int rc = ladder_bad(sl, R);
        if (rc && !dead && live && r == 0 && ctx.lane == 0)
            atomicMin(args().bad, ((unsigned long long)ladder << 32) | (unsigned long long)(unsigned)it);
        dead |= rc;
        ctx = refresh();
        gibbs::Draws dr{model().seed, args().z, args().u, args().ladders * R, chain, Nc, Nd, model().disc_block_its};
        dr.tag_normal = TAG_NORMAL;
        dr.tag_uniform = TAG_UNIFORM;
        ais::transition(model(), it, beta, dr, w, ctx, (dead | !live) != 0);
        // 2. the kept sample, before the swap
        ctx = refresh();
        const int s_kept = it - model().num_burnin;
        if (live && r == R - 1 && s_kept >= 0 && !dead) record(model(), s_kept, w, ctx, o);
        // 3. the swap round
        const int swap_every = args().swap_every;
        if (swap_every > 0 && (it + 1) % swap_every == 0) {
            const int s = it / swap_every, lo = pair_of(R, s, r);
            const double other = lo < 0 ? beta : args().betas[lo == r ? r + 1 : lo];
            swap_masses(model(), beta, other, ais::Base{args().tau0, m0}, w, ctx, sl, r);
            ctx.sync();
            ctx = refresh();
            rc = ladder_bad(sl, R);
            if (rc && !dead && live && r == 0 && ctx.lane == 0)
                atomicMin(args().bad, ((unsigned long long)ladder << 32) | (unsigned long long)(unsigned)it);
            dead |= rc;
            if (live && !dead) {
                const SwapDraws sd{model().seed, args().usw, args().ladders, ladder, R > 1 ? R - 1 : 1};
                decide(Nd, R, it, s, r, sl, sd, w.dig, 2 * (int64_t)cw, ctx, tries, accs);
            }
            ctx.sync();
        }
    }
    if (live) {
        int32_t* x_d = args().x_d;
        for (int n = lane; n < Nd; n += lanes) x_d[chain * Nd + n] = w.dig[n];
    }
}

static int run_check(const lhvi_gibbs_t* m, int32_t R, const double* betas, int32_t it_begin, int32_t it_end, int32_t swap_every,
                     double tau0, const double* mu0, const int32_t* x_d) {
    if (R < 1 || !betas || it_begin < 0 || it_end < it_begin || swap_every < 0) return LHVI_E_ARG;
    if (!(tau0 > 0.0) || (m->ex.Nc && !mu0) || (m->ex.Nd && !x_d)) return LHVI_E_ARG;
    return LHVI_OK;
}

}  // namespace pt
}  // namespace lhvi

using namespace lhvi;
using namespace lhvi::pt;

extern "C" {

size_t lhvi_pt_lds_bytes(int32_t Nc, int32_t Nd, int32_t table_doubles, int32_t R, int32_t lanes) {
    if (Nc < 0 || Nd < 0 || table_doubles < 0 || R < 1 || !hg::lanes_ok(lanes)) return 0;
    if ((int64_t)R * lanes > MAX_BLOCK) return 0;
    return (size_t)shape_of(R, lanes).ladders_per_block * (size_t)pt::ws_doubles(Nc, Nd, table_doubles, R) * sizeof(double);
}

int lhvi_pt_run(const lhvi_gibbs_t* m, int64_t ladders, int32_t R, const double* betas, int32_t it_begin, int32_t it_end,
                int32_t swap_every, int32_t lanes, double tau0, const double* mu0, int32_t* x_d, const double* z, const double* u,
                const double* usw, int32_t* disc, double* cont, int32_t* counts, double* sum1, double* sum2, int32_t* swap_try,
                int32_t* swap_acc, uint64_t* bad, void* stream) {
    int rc = hg::gibbs_check(m, hg::ALL_COUNTS);
    if (rc) return rc;
    rc = run_check(m, R, betas, it_begin, it_end, swap_every, tau0, mu0, x_d);
    if (rc) return rc;
    if (ladders < 0 || !bad || ladders * (int64_t)R > 0xffffffffLL || !hg::lanes_ok(lanes)) return LHVI_E_ARG;
    if ((int64_t)R * lanes > MAX_BLOCK) return LHVI_E_UNSUPPORTED;
    const size_t lds = lhvi_pt_lds_bytes(m->ex.Nc, m->ex.Nd, lds_disc_doubles(*m), R, lanes);
    if (lds > hg::LDS_LIMIT) return LHVI_E_UNSUPPORTED;
    if (ladders == 0 || it_end == it_begin) return LHVI_OK;
    const Shape sh = shape_of(R, lanes);
    const int64_t blocks = (ladders + sh.ladders_per_block - 1) / sh.ladders_per_block;
    if (blocks > 0x7fffffff) return LHVI_E_UNSUPPORTED;
    Args a;
    a.ladders = ladders; a.betas = betas; a.mu0 = mu0; a.z = z; a.u = u; a.usw = usw;
    a.x_d = x_d; a.disc = disc; a.counts = counts; a.swap_try = swap_try; a.swap_acc = swap_acc;
    a.cont = cont; a.sum1 = sum1; a.sum2 = sum2;
    a.bad = reinterpret_cast<unsigned long long*>(bad);
    a.tau0 = tau0;
    a.R = R; a.it_begin = it_begin; a.it_end = it_end; a.swap_every = swap_every; a.lanes = lanes;
    hipLaunchKernelGGL(pt_ladder_kernel, dim3((unsigned)blocks), dim3(sh.block), lds, as_stream(stream), *m, a);
    return check_launch();
}

int lhvi_pt_ladder_host(const lhvi_gibbs_t* m, int64_t ladder, int32_t R, const double* betas, int32_t it_begin, int32_t it_end,
                        int32_t swap_every, double tau0, const double* mu0, int32_t* x_d, const double* z, const double* u,
                        const double* usw, int32_t* disc, double* cont, int32_t* counts, double* sum1, double* sum2,
                        int32_t* swap_try, int32_t* swap_acc) {
    int rc = hg::gibbs_check(m, hg::ALL_COUNTS);
    if (rc) return rc;
    rc = run_check(m, R, betas, it_begin, it_end, swap_every, tau0, mu0, x_d);
    if (rc) return rc;
    const int Nc = m->ex.Nc, Nd = m->ex.Nd;
    if (ladder < 0 || ladder * (int64_t)R > 0xffffffffLL) return LHVI_E_ARG;
    const bool injected = z || u || usw;
    if (injected && ((Nc && !z) || (Nd && m->disc_block_its && !u) || (R > 1 && swap_every && !usw))) return LHVI_E_ARG;
    hg::HostWork hw(*m);
    const lhvi_gibbs_t& g = hw.g;
    const int dd = hw.dd, cw = chain_doubles(Nc, Nd, dd);
    double* W = hw.alloc(pt::ws_doubles(Nc, Nd, dd, R));
    const Slots sl = slots(Nc, Nd, dd, R, W);
    gibbs::Workspace* w = new gibbs::Workspace[R];
    gibbs::Draws* dr = new gibbs::Draws[R];
    ais::Base* base = new ais::Base[R];
    for (int r = 0; r < R; ++r) {
        w[r] = gibbs::layout(g, W + r * cw, nullptr);
        double* m0 = ais::base_mean(Nc, Nd, dd, W + r * cw);
        hw.digits_in(w[r], x_d + r * Nd);
        for (int i = 0; i < Nc; ++i) m0[i] = mu0[i];
        // injected draws are this ladder's rows (z [iters][R][Nc], u [iters][R][its][Nd], usw [iters][max(R - 1, 1)]); the Philox
        // stream is that of ladder `ladder`
        dr[r] = gibbs::Draws{g.seed, z, u, R, r, Nc, Nd, g.disc_block_its};
        if (!injected) dr[r].chain = ladder * R + r;
        dr[r].tag_normal = TAG_NORMAL;
        dr[r].tag_uniform = TAG_UNIFORM;
        base[r] = ais::Base{tau0, m0};
    }
    const SwapDraws sd{g.seed, usw, 1, injected ? 0 : ladder, R > 1 ? R - 1 : 1};
    const gibbs::Out o{disc, cont, counts, sum1, sum2};
    const exact::HostCtx ctx;
    bool dead = false;
    for (int it = it_begin; it < it_end; ++it) {
        for (int r = 0; r < R; ++r) factor(g, betas[r], base[r], w[r], ctx, sl, r);
        dead = dead || ladder_bad(sl, R);
        for (int r = 0; r < R; ++r) {
            // replica r's factor is in its own workspace: nothing of another replica is read
            ais::transition(g, it, betas[r], dr[r], w[r], ctx, dead);
        }
        if (it >= g.num_burnin && !dead) record(g, it - g.num_burnin, w[R - 1], ctx, o);
        if (swap_every > 0 && (it + 1) % swap_every == 0) {
            const int s = it / swap_every;
            for (int r = 0; r < R; ++r) {
                const int lo = pair_of(R, s, r);
                swap_masses(g, betas[r], lo < 0 ? betas[r] : betas[lo == r ? r + 1 : lo], base[r], w[r], ctx, sl, r);
            }
            dead = dead || ladder_bad(sl, R);
            if (!dead)
                for (int r = 0; r < R; ++r) decide(Nd, R, it, s, r, sl, sd, w[r].dig, 2 * (int64_t)cw, ctx, swap_try, swap_acc);
        }
    }
    for (int r = 0; r < R; ++r) hw.digits_out(w[r], x_d + r * Nd);
    delete[] base;
    delete[] dr;
    delete[] w;
    return dead ? LHVI_E_NOT_PD : LHVI_OK;
}

}  // extern "C"
