// gmkl_dev.hpp -- the lane mapping of csrc/gmkl.hpp::kl_row on gfx950: one wavefront per row, a lane per quadrature node.
// Shared by gm_kl_kernel (csrc/gmkl.hip: q a second mixture) and pbp_kl_kernel (csrc/pbp.hip: q the belief of a particle
// solver).  docs/kernels_gmkl.md, docs/kernels_pbkl.md.
//
// Lanes take the quadrature nodes, 3 x 21 of 64: lane l works on interval l / 21 of the step at node l % 21 (lane 63 repeats
// lane 42 and is never read).  Pass 1 takes three panels per step, a bisection its two children side by side (the third group
// repeats the right child).  Every lane runs the components past its own node and keeps the running log-sum-exp; the
// components are wave-uniform values read from LDS: resident for the whole row when they fit CHUNK slots, else prepared in
// chunks of CHUNK (a lane per component: the logarithm and the division) in front of every evaluation.  The 21 values of a
// group go through LDS and every lane of the group forms the rule's sums itself, in QUADPACK's order (gk21_from_values): no
// cross-lane arithmetic, so the order of every sum is the host twin's.  The panel list and the stack are in LDS too: 20 024
// bytes per wave, 8 waves per CU.
//
// Control flow is wave-uniform: every decision is taken on values all lanes read from the same LDS words and made a scalar
// before the branch (uniform()), so the barriers (one wave per workgroup: they order the LDS traffic for the compiler) are
// reached by all lanes.
//
// The q side is a policy Q of the context:
//   scan(ctx, in, sc)          this lane's share of the q side's validity: sets sc.anyq, may set sc.bad (reduced afterwards)
//   slots(in)                  the slots of the component list q wants for the whole row, behind p's Kp
//   load_resident(ctx, in)     a resident row: the lanes from Kp on fill those slots
//   eval(ctx, in, x, m, s)     log q(x) = m + log(s) at the lane's node; called by every lane (it may hold barriers)
// This header includes gmkl.hpp, which switches contraction off for the rest of the including file.
#pragma once
#include "common.hpp"
#include "gmkl.hpp"

namespace lhvi {
namespace gmkl {

constexpr int CHUNK = 64;
constexpr int GROUP = 21, GROUPS = 3;

struct Comp { double la, mu, nhiv; };
struct Shared {
    double pr[MAX_PANELS], pe[MAX_PANELS];
    double sa[MAX_DEPTH], sb[MAX_DEPTH], sr[MAX_DEPTH], se[MAX_DEPTH];
    int sd[MAX_DEPTH];
    Comp c[CHUNK];
    double fv[WAVE];
    double child[2][2];     // (result, estimate) of the two children of a bisection
    Row in;                 // the row's pointers, bounds and tolerances, and where its outputs go: written by lane 0 and read
    double *kl, *abserr;    // back by every lane, which keeps them in vector registers (they live as long as the kernel and
    int32_t *status, *neval;// would crowd the scalar file)
};
static_assert(sizeof(Shared) <= 20 * 1024, "8 waves per CU: 160 KiB / 8");

template <class Q>
struct DevCtx {
    Shared& sh;
    int lane, g, j;         // the lane's interval of the step and its node
    bool resident;
    const Q& q;

    __device__ __forceinline__ DevCtx(Shared& s, int l, const Q& qside)
        : sh(s), lane(l), g(l / GROUP < GROUPS ? l / GROUP : GROUPS - 1), j(l < GROUP * GROUPS ? l % GROUP : 0), resident(false),
          q(qside) {}
    __device__ __forceinline__ bool lane0() const { return lane == 0; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    __device__ __forceinline__ static bool uniform(bool c) { return __builtin_amdgcn_readfirstlane((int)c) != 0; }
    __device__ __forceinline__ static int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

    __device__ __forceinline__ void scan(const Row& in, Scan& sc) const {
        for (int k = lane; k < in.Kp; k += WAVE) scan_p(sc, in.wp[k], in.mup[k], in.varp[k]);
        q.scan(*this, in, sc);
        sc.lo = -dpp_wave_reduce(-sc.lo, MaxOp());
        sc.hi = dpp_wave_reduce(sc.hi, MaxOp());
        sc.sdmin = -dpp_wave_reduce(-sc.sdmin, MaxOp());
        sc.bad = __any(sc.bad), sc.anyp = __any(sc.anyp), sc.anyq = __any(sc.anyq);
        // (the reductions leave scalars; the range lives as long as the kernel: through LDS into vector registers, as the row)
        if (lane == 0) sh.fv[0] = sc.lo, sh.fv[1] = sc.hi, sh.fv[2] = sc.sdmin;
        sync();
        sc.lo = sh.fv[0], sc.hi = sh.fv[1], sc.sdmin = sh.fv[2];
    }
    __device__ __forceinline__ void load(int slot, const double* w, const double* mu, const double* var, int k) const {
        Comp c;
        comp_consts(w[k], var[k], c.la, c.nhiv);
        c.mu = mu[k];
        sh.c[slot] = c;
    }
    __device__ __forceinline__ void prepare(const Row& in) {
        resident = in.Kp + Q::slots(in) <= CHUNK;
        if (resident) {
            if (lane < in.Kp) load(lane, in.wp, in.mup, in.varp, lane);
            else q.load_resident(*this, in);
            sync();
        }
    }
    __device__ __forceinline__ void run(int first, int n, double x, double& m, double& s) const {
#pragma unroll 1               // (unrolled, the loop holds more constants in scalar registers than the file has: spills)
        for (int c = first; c < first + n; ++c) {
            const Comp k = sh.c[c];             // (weight 0: la = -inf adds exp(-inf) = 0 and leaves the maximum, as skipping does,
            lse_step(m, s, k.la, k.mu, k.nhiv, x);      //  without a branch per component in this loop)
        }
    }
    __device__ __forceinline__ void side(int K, const double* w, const double* mu, const double* var, int first, double x,
                                         double& m, double& s) const {
        m = LSE_START, s = 0.0;
        for (int k0 = 0; k0 < K; k0 += CHUNK) {             // (resident: K <= CHUNK, one round on what prepare() left)
            const int n = K - k0 < CHUNK ? K - k0 : CHUNK;
            if (!resident) {
                sync();
                if (lane < n) load(lane, w, mu, var, k0 + lane);
                sync();
            }
            run(resident ? first : 0, n, x, m, s);
        }
    }
    __device__ __forceinline__ double f(const Row& in, double x) const {
        double mp, sp, mq, sq;
        side(in.Kp, in.wp, in.mup, in.varp, 0, x, mp, sp);
        q.eval(*this, in, x, mq, sq);
        return integrand(mp, sp, mq, sq);
    }
    // the rule on the lane's interval [a, b]: every lane of a group returns the group's result
    __device__ __forceinline__ Gk21 rule(const Row& in, double a, double b) const {
        const double centr = 0.5 * (a + b), hlgth = 0.5 * (b - a);
        const double v = f(in, gk21_node(j, centr, hlgth));
        sync();
        sh.fv[lane] = v;
        sync();
        const double* fv = sh.fv + g * GROUP;
        return gk21_from_values([&](int n) { return fv[n]; }, hlgth);
    }
    __device__ __forceinline__ void pass1(const Row& in, const Plan& pl) const {
        for (int i0 = 0; i0 < pl.P; i0 += GROUPS) {
            const int i = i0 + g, ic = i < pl.P ? i : pl.P - 1;        // a group past the last panel repeats it
            const Gk21 r = rule(in, panel_edge(pl, ic), panel_edge(pl, ic + 1));
            if (j == 0 && lane < GROUP * GROUPS && i < pl.P) sh.pr[i] = r.result, sh.pe[i] = r.abserr;
        }
        sync();
    }
    __device__ __forceinline__ double pres(int i) const { return sh.pr[i]; }
    __device__ __forceinline__ double perr(int i) const { return sh.pe[i]; }
    __device__ __forceinline__ void bisect(const Row& in, double a, double mid, double b, Gk21& l, Gk21& r) const {
        const Gk21 t = rule(in, g == 0 ? a : mid, g == 0 ? mid : b);         // one call: every lane takes part in its barriers
        if (lane == 0 || lane == GROUP) sh.child[g][0] = t.result, sh.child[g][1] = t.abserr;
        sync();
        l.result = sh.child[0][0], l.abserr = sh.child[0][1];
        r.result = sh.child[1][0], r.abserr = sh.child[1][1];
    }
    __device__ __forceinline__ void push(int t, double a, double b, double res, double err, int depth) const {
        if (lane == 0) sh.sa[t] = a, sh.sb[t] = b, sh.sr[t] = res, sh.se[t] = err, sh.sd[t] = depth;
    }
    __device__ __forceinline__ void pop(int t, double& a, double& b, double& res, double& err, int& depth) const {
        a = sh.sa[t], b = sh.sb[t], res = sh.sr[t], err = sh.se[t], depth = sh.sd[t];
    }
};

// q is the row's second mixture: its components follow p's in the resident list, or are streamed through it after p's
struct MixtureQ {
    template <class C> __device__ __forceinline__ void scan(const C& ctx, const Row& in, Scan& sc) const {
        for (int k = ctx.lane; k < in.Kq; k += WAVE) scan_q(sc, in.wq[k], in.muq[k], in.varq[k]);
    }
    __device__ __forceinline__ static int slots(const Row& in) { return in.Kq; }
    template <class C> __device__ __forceinline__ void load_resident(const C& ctx, const Row& in) const {
        if (ctx.lane < in.Kp + in.Kq) ctx.load(ctx.lane, in.wq, in.muq, in.varq, ctx.lane - in.Kp);
    }
    template <class C> __device__ __forceinline__ void eval(const C& ctx, const Row& in, double x, double& m, double& s) const {
        ctx.side(in.Kq, in.wq, in.muq, in.varq, in.Kp, x, m, s);
    }
};

}  // namespace gmkl
}  // namespace lhvi
