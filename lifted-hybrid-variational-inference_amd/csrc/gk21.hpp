// gk21.hpp -- QUADPACK's 21-point Gauss-Kronrod rule (dqk21) with its error estimate, shared by the particle kernels
// (csrc/pbp.hip: pbp_quad_kernel, a thread per integral) and the mixture KL (csrc/gmkl.hpp: a lane per node).
//   gk21(f, a, b)              the rule with the integrand as a callable: one thread evaluates the 21 nodes in QUADPACK's order
//   gk21_node(j, c, h)         the point of node j (0 .. 20, ascending) on the interval of centre c and half length h
//   gk21_from_values(fv, h)    the rule from the 21 values fv(j) at the nodes in ascending order, half length h: the sums run
//                              in gk21's order (centre, the five Gauss pairs, the five Kronrod pairs), so the same values give
//                              the same result whoever evaluated them
// This header sets no floating-point pragma: the including file decides on contraction.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LHVI_GK_HD __host__ __device__ __forceinline__
#else
#define LHVI_GK_HD inline
#endif

namespace lhvi {

struct Gk21 { double result, abserr, resabs, resasc; bool overflow; };

// QUADPACK's tables: abscissae and Kronrod weights by magnitude, outermost first, index 10 the centre; the Gauss weights of
// the abscissae 1, 3, 5, 7, 9.  Every loop over them is unrolled, so they are literals in the code, not memory.
constexpr double GK21_XGK[11] = {0.995657163025808080735527280689003, 0.973906528517171720077964012084452,
                                 0.930157491355708226001207180059508, 0.865063366688984510732096688423493,
                                 0.780817726586416897063717578345042, 0.679409568299024406234327365114874,
                                 0.562757134668604683339000099272694, 0.433395394129247190799265943165784,
                                 0.294392862701460198131126603103866, 0.148874338981631210884826001129720, 0.0};
constexpr double GK21_WGK[11] = {0.011694638867371874278064396062192, 0.032558162307964727478818972459390,
                                 0.054755896574351996031381300244580, 0.075039674810919952767043140916190,
                                 0.093125454583697605535065465083366, 0.109387158802297641899210590325805,
                                 0.123491976262065851077958109585166, 0.134709217311473325928054001771707,
                                 0.142775938577060080797094273138717, 0.147739104901338491374841515972068,
                                 0.149445554002916905664936468389821};
constexpr double GK21_WG[5] = {0.066671344308688137593568809893332, 0.149451349150580593145776339657697,
                               0.219086362515982043995534934228163, 0.269266719309996355091226921569469,
                               0.295524224714752870173815619188769};
constexpr double GK21_EPMACH = 2.220446049250313e-16, GK21_UFLOW = 2.2250738585072014e-308;

#if defined(__HIPCC__) || defined(__CUDACC__)
template <typename F>
__device__ Gk21 gk21(F&& f, double a, double b) {
    constexpr const double (&xgk)[11] = GK21_XGK, (&wgk)[11] = GK21_WGK, (&wg)[5] = GK21_WG;
    const double epmach = GK21_EPMACH, uflow = GK21_UFLOW;
    const double centr = 0.5 * (a + b), hlgth = 0.5 * (b - a), dhlgth = fabs(hlgth);
    double fv1[10], fv2[10];
    const double fc = f(centr);
    double resg = 0.0, resk = wgk[10] * fc, resabs = fabs(resk);
    for (int j = 0; j < 5; ++j) {
        const int jtw = 2 * j + 1;
        const double absc = hlgth * xgk[jtw];
        const double f1 = f(centr - absc), f2 = f(centr + absc);
        fv1[jtw] = f1; fv2[jtw] = f2;
        resg += wg[j] * (f1 + f2);
        resk += wgk[jtw] * (f1 + f2);
        resabs += wgk[jtw] * (fabs(f1) + fabs(f2));
    }
    for (int j = 0; j < 5; ++j) {
        const int jtwm1 = 2 * j;
        const double absc = hlgth * xgk[jtwm1];
        const double f1 = f(centr - absc), f2 = f(centr + absc);
        fv1[jtwm1] = f1; fv2[jtwm1] = f2;
        resk += wgk[jtwm1] * (f1 + f2);
        resabs += wgk[jtwm1] * (fabs(f1) + fabs(f2));
    }
    const double reskh = resk * 0.5;
    double resasc = wgk[10] * fabs(fc - reskh);
    for (int j = 0; j < 10; ++j) resasc += wgk[j] * (fabs(fv1[j] - reskh) + fabs(fv2[j] - reskh));
    Gk21 r;
    r.result = resk * hlgth;
    r.resabs = resabs * dhlgth;
    r.resasc = resasc * dhlgth;
    r.abserr = fabs((resk - resg) * hlgth);
    if (r.resasc != 0.0 && r.abserr != 0.0) r.abserr = r.resasc * fmin(1.0, pow(200.0 * r.abserr / r.resasc, 1.5));
    if (r.resabs > uflow / (50.0 * epmach)) r.abserr = fmax((epmach * 50.0) * r.resabs, r.abserr);
    r.overflow = !(fabs(resk) < __builtin_huge_val());
    return r;
}
#endif

// the point of node j (0 .. 20, ascending; nodes j and 20 - j are a pair) on the interval of centre `centr` and half length
// `hlgth`, formed as gk21 forms it.  j is a run-time value (a lane's node): the abscissa is picked by selects, not loaded.
LHVI_GK_HD double gk21_node(int j, double centr, double hlgth) {
    const int m = j <= 10 ? j : 20 - j;
    double x = 0.0;
#pragma unroll
    for (int i = 0; i < 10; ++i) x = m == i ? GK21_XGK[i] : x;
    const double absc = hlgth * x;
    return j < 10 ? centr - absc : j > 10 ? centr + absc : centr;
}

template <typename FV>
LHVI_GK_HD Gk21 gk21_from_values(FV&& fv, double hlgth) {
    const double dhlgth = fabs(hlgth);
    const double fc = fv(10);
    double resg = 0.0, resk = GK21_WGK[10] * fc, resabs = fabs(resk);
#pragma unroll
    for (int j = 0; j < 5; ++j) {               // the Gauss pairs
        const int k = 2 * j + 1;
        const double f1 = fv(k), f2 = fv(20 - k);
        resg += GK21_WG[j] * (f1 + f2);
        resk += GK21_WGK[k] * (f1 + f2);
        resabs += GK21_WGK[k] * (fabs(f1) + fabs(f2));
    }
#pragma unroll
    for (int j = 0; j < 5; ++j) {               // the Kronrod pairs
        const int k = 2 * j;
        const double f1 = fv(k), f2 = fv(20 - k);
        resk += GK21_WGK[k] * (f1 + f2);
        resabs += GK21_WGK[k] * (fabs(f1) + fabs(f2));
    }
    const double reskh = resk * 0.5;
    double resasc = GK21_WGK[10] * fabs(fc - reskh);
#pragma unroll
    for (int k = 0; k < 10; ++k) resasc += GK21_WGK[k] * (fabs(fv(k) - reskh) + fabs(fv(20 - k) - reskh));
    Gk21 r;
    r.result = resk * hlgth;
    r.resabs = resabs * dhlgth;
    r.resasc = resasc * dhlgth;
    r.abserr = fabs((resk - resg) * hlgth);
    if (r.resasc != 0.0 && r.abserr != 0.0) {
        const double t = 200.0 * r.abserr / r.resasc;         // t^1.5 as t sqrt(t): the last bit of an ESTIMATE, without pow
        r.abserr = r.resasc * fmin(1.0, t * sqrt(t));
    }
    if (r.resabs > GK21_UFLOW / (50.0 * GK21_EPMACH)) r.abserr = fmax((GK21_EPMACH * 50.0) * r.resabs, r.abserr);
    r.overflow = !(fabs(resk) < __builtin_huge_val());
    return r;
}

}  // namespace lhvi
