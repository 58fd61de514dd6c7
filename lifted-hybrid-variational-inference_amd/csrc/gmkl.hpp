// gmkl.hpp -- KL(p || q) of two scalar Gaussian mixtures by panel-seeded adaptive Gauss-Kronrod quadrature (the reference's
// utils.kl_continuous_logpdf on mixture marginals), written once for the device (csrc/gmkl.hip: one wavefront per row, a lane
// per quadrature node) and the host (lhvi_gm_kl_host: the nodes one after another).  docs/kernels_gmkl.md has the method.
//
// Shared here: the component constants, the running log-sum-exp of a node, the integrand, the range and panel plan, the
// acceptance rule and the refinement loop (pass 2).  q need not be a mixture: the integrand takes log q(x) as (mq, sq) with
// log q = mq + log(sq), and a context whose q side is another log density (a caller's function on the host, a particle
// solver's belief in csrc/pbp.hip) passes (log q(x), 1).  A Ctx supplies what depends on where the nodes are evaluated:
//   scan(in, sc)                   the validity of the row and the range of p (order-independent: min / max / or)
//   prepare(in)                    once per row, before the first evaluation
//   pass1(in, pl)                  the rule on every panel; afterwards pres(i), perr(i) are readable
//   bisect(in, a, mid, b, l, r)    the rule on [a, mid] and [mid, b]
//   push(slot, ...) / pop(slot, ...) / sync()      the stack of pass 2: at most MAX_DEPTH entries
//   lane0()                        whether this caller writes the row's outputs
//   uniform(c)                     a condition or count every lane holds alike, as one value (the device branches on a scalar)
// Contraction is off for the whole file: a * b + c is rounded twice on both sides, so the host twin differs from the device
// only by the library's exp / log / sqrt.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>
#include "../../include/lhvi.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LHVI_HD __host__ __device__ __forceinline__
#else
#define LHVI_HD inline
#endif

#pragma clang fp contract(off)

#include "gk21.hpp"

namespace lhvi {
namespace gmkl {

constexpr int MAX_PANELS = LHVI_GMKL_MAX_PANELS;
constexpr int MAX_DEPTH = 40;           // bisections below a panel
constexpr int MAX_BISECT = 4096;        // bisections of one row: past it intervals are accepted as they are (status bit 0)
constexpr double Z_RANGE = 10.0;        // the range reaches Z standard deviations beyond p's outermost components
constexpr double C_PANEL = 8.0;         // a panel is at most C standard deviations of p's narrowest component wide
constexpr double LOG_2PI = 1.8378770664093453;
constexpr double NEG_INF = -__builtin_huge_val();
enum { ST_TOL = 1, ST_CAP = 2, ST_INVALID = 4 };

struct Row {
    int32_t Kp, Kq;
    const double *wp, *mup, *varp, *wq, *muq, *varq;
    double a, b, epsabs, epsrel;
};

// log N(x; mu, var) + log w = la + nhiv (x - mu)^2; a component of weight 0 has la = -inf and is skipped
LHVI_HD void comp_consts(double w, double var, double& la, double& nhiv) {
    la = w == 0.0 ? NEG_INF : log(w) - 0.5 * (LOG_2PI + log(var));
    nhiv = -0.5 / var;
}

LHVI_HD bool comp_bad(double w, double mu, double var) {
    return !(fabs(mu) <= DBL_MAX) || !(var > 0.0 && var <= DBL_MAX) || !(w >= 0.0 && w <= DBL_MAX);
}

struct Scan {
    double lo = __builtin_huge_val(), hi = NEG_INF, sdmin = __builtin_huge_val();
    bool bad = false, anyp = false, anyq = false;
};
LHVI_HD void scan_p(Scan& sc, double w, double mu, double var) {
    sc.bad = sc.bad || comp_bad(w, mu, var);
    if (w > 0.0) {
        const double sd = sqrt(var);
        sc.lo = fmin(sc.lo, mu - Z_RANGE * sd);
        sc.hi = fmax(sc.hi, mu + Z_RANGE * sd);
        sc.sdmin = fmin(sc.sdmin, sd);
        sc.anyp = true;
    }
}
LHVI_HD void scan_q(Scan& sc, double w, double mu, double var) {
    sc.bad = sc.bad || comp_bad(w, mu, var);
    sc.anyq = sc.anyq || w > 0.0;
}

// one component into the running (max m, sum s of exp(t - m)) of a node: one exponential and no branch.  m starts at
// LSE_START = -DBL_MAX, not -inf, so that t - m is never inf - inf: a first component gives exp(-inf) = 0 and s = 0 * 0 + 1,
// a component of weight 0 (t = -inf) adds exp(-inf) = 0 and leaves m
constexpr double LSE_START = -DBL_MAX;
LHVI_HD void lse_step(double& m, double& s, double la, double mu, double nhiv, double x) {
    const double d = x - mu, t = la + nhiv * (d * d);
    const double e = exp(-fabs(t - m));
    s = t > m ? s * e + 1.0 : s + e;
    m = fmax(m, t);
}

// f = p (log p - log q) from the two running sums; 0 where p underflows, +inf where only q does
LHVI_HD double integrand(double mp, double sp, double mq, double sq) {
    const double lp = mp + log(sp), lq = mq + log(sq);
    const double ep = exp(lp);
    return ep == 0.0 ? 0.0 : ep * (lp - lq);
}

struct Plan {
    double L, U, range, h;
    int P, status;          // P = 0: nothing to integrate
};
LHVI_HD Plan make_plan(double a, double b, const Scan& sc) {
    Plan pl;
    pl.L = fmax(a, sc.lo), pl.U = fmin(b, sc.hi);
    pl.range = pl.U - pl.L, pl.h = 0.0, pl.P = 0, pl.status = 0;
    if (!(pl.U > pl.L)) return pl;
    const double want = ceil(pl.range / (C_PANEL * sc.sdmin));
    if (want > (double)MAX_PANELS) pl.P = MAX_PANELS, pl.status = ST_CAP;
    else pl.P = want < 1.0 ? 1 : (int)want;
    pl.h = pl.range / (double)pl.P;
    return pl;
}
LHVI_HD double panel_edge(const Plan& pl, int i) { return i >= pl.P ? pl.U : pl.L + (double)i * pl.h; }

// (an estimate that is not finite meets nothing, not even an infinite bound: where pass 1 already sees an infinite integrand
// area0 and the bound are infinite too, and the interval is accepted by the guard with status bit 0, as docs/kernels_gmkl.md says)
LHVI_HD bool meets(double err, double bound, double width, double range) { return err <= bound * (width / range) && err <= DBL_MAX; }

template <class Ctx>
LHVI_HD void kl_row(const Row& in, Ctx& ctx, double* kl, double* abserr, int32_t* status, int32_t* neval) {
    auto write = [&](double v, double e, int st, int ne) {
        if (ctx.lane0()) {
            *kl = v;
            if (abserr) *abserr = e;
            if (status) *status = st;
            if (neval) *neval = ne;
        }
    };
    Scan sc;
    ctx.scan(in, sc);
    if (sc.bad || !sc.anyp || !sc.anyq || in.a != in.a || in.b != in.b) {
        write(__builtin_nan(""), __builtin_nan(""), ST_INVALID, 0);
        return;
    }
    Plan pl = make_plan(in.a, in.b, sc);
    pl.P = ctx.uniform(pl.P), pl.status = ctx.uniform(pl.status);
    if (pl.P == 0) {
        write(0.0, 0.0, 0, 0);
        return;
    }
    __builtin_assume(pl.P >= 1);            // (the device reads P through a scalar: its loops need no guard)
    ctx.prepare(in);
    // ---- pass 1: the rule on every panel, the bound from their sum
    ctx.pass1(in, pl);
    double area0 = 0.0;
    for (int i = 0; i < pl.P; ++i) area0 += ctx.pres(i);
    const double bound = fmax(in.epsabs, in.epsrel * fabs(area0));
    // ---- pass 2: panel by panel, left to right, depth first; the left child stays in hand, the right one waits on the stack
    double sum = 0.0, esum = 0.0;
    int st = pl.status, ne = 21 * pl.P, nbis = 0;
    for (int i = 0; i < pl.P; ++i) {
        double a = panel_edge(pl, i), b = panel_edge(pl, i + 1), res = ctx.pres(i), err = ctx.perr(i);
        int depth = 0, top = 0;
        for (;;) {
            const bool ok = ctx.uniform(meets(err, bound, b - a, pl.range));
            if (ok || ctx.uniform(depth >= MAX_DEPTH || nbis >= MAX_BISECT || !(fabs(err) <= DBL_MAX))) {
                if (!ok) st |= ST_TOL;
                sum += res, esum += err;
                if (top == 0) break;
                ctx.pop(--top, a, b, res, err, depth);
                continue;
            }
            const double mid = 0.5 * (a + b);
            Gk21 l, r;
            ctx.bisect(in, a, mid, b, l, r);
            ++nbis, ne += 42, ++depth;
            ctx.push(top++, mid, b, r.result, r.abserr, depth);
            ctx.sync();
            b = mid, res = l.result, err = l.abserr;
        }
    }
    write(sum, esum, st, ne);
}

// ---- the host: one node after another, the components straight from the arrays.  The q side is a policy Q, as on the
// device (csrc/gmkl_dev.hpp): scan(in, sc) marks the row's q side (anyq, bad), eval(in, x, m, s) leaves log q(x) = m + log(s)
LHVI_HD void host_side(int K, const double* w, const double* mu, const double* var, double x, double& m, double& s) {
    m = LSE_START, s = 0.0;
    for (int k = 0; k < K; ++k) {
        double la, nhiv;
        comp_consts(w[k], var[k], la, nhiv);
        if (la == NEG_INF) continue;
        lse_step(m, s, la, mu[k], nhiv, x);
    }
}

struct HostMixtureQ {           // q is the row's second mixture
    void scan(const Row& in, Scan& sc) const {
        for (int k = 0; k < in.Kq; ++k) scan_q(sc, in.wq[k], in.muq[k], in.varq[k]);
    }
    void eval(const Row& in, double x, double& m, double& s) const { host_side(in.Kq, in.wq, in.muq, in.varq, x, m, s); }
};

struct HostFnQ {                // q is any log density: the caller's function of the point and the row (lhvi_gm_kl_fn_host)
    double (*logq)(double x, int64_t row, void* user);
    void* user;
    int64_t row;
    void scan(const Row&, Scan& sc) const { sc.anyq = true; }
    void eval(const Row&, double x, double& m, double& s) const { m = logq(x, row, user), s = 1.0; }
};

template <class Q>
struct HostCtxT {
    double pr[MAX_PANELS], pe[MAX_PANELS];
    double sa[MAX_DEPTH], sb[MAX_DEPTH], sr[MAX_DEPTH], se[MAX_DEPTH];
    int sd[MAX_DEPTH];
    Q q;

    bool lane0() const { return true; }
    static bool uniform(bool c) { return c; }
    static int uniform(int v) { return v; }
    void scan(const Row& in, Scan& sc) const {
        for (int k = 0; k < in.Kp; ++k) scan_p(sc, in.wp[k], in.mup[k], in.varp[k]);
        q.scan(in, sc);
    }
    void prepare(const Row&) {}
    double f(const Row& in, double x) const {
        double mp, sp, mq, sq;
        host_side(in.Kp, in.wp, in.mup, in.varp, x, mp, sp);
        q.eval(in, x, mq, sq);
        return integrand(mp, sp, mq, sq);
    }
    Gk21 rule(const Row& in, double a, double b) const {
        const double centr = 0.5 * (a + b), hlgth = 0.5 * (b - a);
        double fv[21];
        for (int j = 0; j < 21; ++j) fv[j] = f(in, gk21_node(j, centr, hlgth));
        return gk21_from_values([&](int j) { return fv[j]; }, hlgth);
    }
    void pass1(const Row& in, const Plan& pl) {
        for (int i = 0; i < pl.P; ++i) {
            const Gk21 r = rule(in, panel_edge(pl, i), panel_edge(pl, i + 1));
            pr[i] = r.result, pe[i] = r.abserr;
        }
    }
    double pres(int i) const { return pr[i]; }
    double perr(int i) const { return pe[i]; }
    void bisect(const Row& in, double a, double mid, double b, Gk21& l, Gk21& r) const { l = rule(in, a, mid), r = rule(in, mid, b); }
    void push(int t, double a, double b, double res, double err, int depth) { sa[t] = a, sb[t] = b, sr[t] = res, se[t] = err, sd[t] = depth; }
    void pop(int t, double& a, double& b, double& res, double& err, int& depth) const { a = sa[t], b = sb[t], res = sr[t], err = se[t], depth = sd[t]; }
    void sync() const {}
};
using HostCtx = HostCtxT<HostMixtureQ>;

}  // namespace gmkl
}  // namespace lhvi
