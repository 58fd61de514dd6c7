// vi_map.hip -- the MAP query of the variational solvers (VarInference.map, VarInference.py:355-376) for every row in one launch.
//
// The reference answers map(rv) of a continuous variable with scipy.optimize.minimize(-belief, x0 = the component mean of largest
// belief) under its defaults: BFGS with a forward-difference gradient.  lhvi_vi_map_bfgs runs that call for a row per thread,
// decision for decision, as SciPy 1.15 spells it:
//   _minimize_bfgs                  (scipy/optimize/_optimize.py)   the outer loop, its exits and the inverse-Hessian update, 1 x 1
//   approx_derivative, '2-point'    (scipy/optimize/_numdiff.py)    absolute step sqrt(eps), dx = (x + h) - x
//   line_search_wolfe1 / DCSRCH     (scipy/optimize/_linesearch.py, _dcsrch.py: MINPACK-2 dcsrch / dcstep)
//   line_search_wolfe2              (scalar_search_wolfe2, _zoom, _cubicmin, _quadmin) when dcsrch fails
// The answer is not "the" maximum: scipy stops on its own tests (a finite-difference gradient under gtol at the start point, a line
// search that fails near a narrow component), and the caller's results are the reference's only if every such decision is the same.
// So the arithmetic is IEEE fp64 in the reference's operation order with contraction off, Python's min / max / NumPy's clip and sign
// keep their NaN behaviour, and _cubicmin / _quadmin give up where NumPy's errstate(divide / over / invalid = 'raise') would raise.
// Latency-bound scalar code; rows diverge by iteration count (accepted: the launch replaces a Python loop of minimize calls).
#include "common.hpp"
#include "scipy_opt.hpp"

namespace lhvi {
namespace vimap {

constexpr double SQRT_EPS = 1.4901161193847656e-08;    // sqrt(np.finfo(float).eps): BFGS's `eps`, also _eps_for_method('2-point')
constexpr int MAX_K = 128;                             // numpy's pairwise block (PW_BLOCKSIZE): one level of its summation

// one hidden continuous row: w [K], eta [K][2] (mu, var)
struct Row {
    const double* w;
    const double* eta;
    int K;
    bool gauss;     // lhvi_vi_t.quirks & LHVI_VI_GAUSSIAN_PDF: the components are normal densities (an NPVI fit)
};

// b[k] = w[k] * norm_pdf(x, eta[k]) (VarInference.py:26-30, 346-348): np.e ** (-u * u * 0.5 / var) / (2.506628274631 * var)
VM_HD double term(const Row& r, int k, double x) {
    const double mu = r.eta[2 * k], var = r.eta[2 * k + 1];
    const double u = x - mu;
    return r.w[k] * (pow_e_np(-u * u * 0.5 / var) / (2.506628274631 * (r.gauss ? sqrt(var) : var)));
}

// np.sum(b) (VarInference.py:353): sequential below 8 terms, else numpy's pairwise block -- eight running sums, combined as
// ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the remainder one by one (K <= 128: no recursion)
VM_HD double belief(const Row& r, double x) {
    const int K = r.K;
    if (K < 8) {
        double s = 0.0;
        for (int k = 0; k < K; ++k) s += term(r, k, x);
        return s;
    }
    double a[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = term(r, j, x);
    int i = 8;
    for (; i < K - K % 8; i += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] += term(r, i + j, x);
    }
    double s = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    for (; i < K; ++i) s += term(r, i, x);
    return s;
}

// NumPy scalar arithmetic under errstate(divide / over / invalid = 'raise') (_cubicmin, _quadmin): a NaN out of non-NaN operands
// (0 / 0, inf - inf, 0 * inf, sqrt of a negative) or an infinity out of finite ones (overflow, x / 0) raises
struct Checked {
    bool raised = false;
    VM_HD double chk(double r, double a, double b) {
        if ((r != r && a == a && b == b) || (!finite(r) && r == r && finite(a) && finite(b))) raised = true;
        return r;
    }
    VM_HD double add(double a, double b) { return chk(a + b, a, b); }
    VM_HD double sub(double a, double b) { return chk(a - b, a, b); }
    VM_HD double mul(double a, double b) { return chk(a * b, a, b); }
    VM_HD double div(double a, double b) { return chk(a / b, a, b); }
    VM_HD double sqrt_(double a) { return chk(sqrt(a), a, 0.0); }
    VM_HD double pow3(double a) {          // a ** 3 (libm pow): the cube carried in double-double, rounded once
        const double s = a * a, se = fma(a, a, -s);
        const double c = s * a, ce = fma(s, a, -c) + se * a;
        return chk(c + ce, a, 0.0);
    }
};

// ---- the objective and its forward difference -----------------------------------------------------------------------------
struct Objective {
    Row r;
    VM_HD double f(double x) const { return -belief(r, x); }
    // approx_derivative(f, x, '2-point', abs_step = sqrt(eps), f0 = f(x)): h falls back to the relative step where x + h == x
    VM_HD double grad(double x, double fx) const {
        double h = SQRT_EPS;
        if ((x + h) - x == 0.0) h = SQRT_EPS * (x >= 0.0 ? 1.0 : -1.0) * (fabs(x) != fabs(x) ? fabs(x) : py_max(1.0, fabs(x)));
        const double x1 = x + h;
        const double dx = x1 - x;
        return (f(x1) - fx) / dx;
    }
};

// phi(s) = f(xk + s pk), derphi(s) = grad(xk + s pk) . pk; the last gradient is kept (the line searches return it)
struct Line {
    const Objective* obj;
    double xk, pk;
    double last_g = 0.0;
    VM_HD double phi(double s) const { return obj->f(xk + s * pk); }
    VM_HD double derphi(double s) {
        const double x = xk + s * pk;
        last_g = obj->grad(x, obj->f(x));
        return last_g * pk;
    }
};

// line_search_wolfe1 runs MINPACK-2 dcsrch / dcstep (scipy/optimize/_dcsrch.py): Dcsrch in scipy_opt.hpp

// alpha1 = min(1, 1.01 * 2 * (phi0 - old_phi0) / derphi0), the step both line searches start from
VM_HD double first_step(double phi0, double old_phi0, double derphi0) {
    double a = 1.0;
    if (derphi0 != 0) {
        a = py_min(1.0, 1.01 * 2 * (phi0 - old_phi0) / derphi0);
        if (a < 0) a = 1.0;
    }
    return a;
}

// scalar_search_wolfe1: true with the step, phi there (phi1) and the gradient there (ln.last_g)
VM_HD bool wolfe1(Line& ln, double phi0, double old_phi0, double derphi0, double& stp_out, double& phi1_out) {
    double stp = first_step(phi0, old_phi0, derphi0);
    // START
    if (stp < AMIN || stp > AMAX || derphi0 >= 0) return false;
    Dcsrch d;
    d.finit = phi0;
    d.ginit = derphi0;
    d.gtest = C1 * d.ginit;
    d.width = AMAX - AMIN;
    d.width1 = d.width / 0.5;
    d.stx = 0.0; d.fx = d.finit; d.gx = d.ginit;
    d.sty = 0.0; d.fy = d.finit; d.gy = d.ginit;
    d.stmin = 0;
    d.stmax = stp + 4.0 * stp;
    // the START call returns FG: the first evaluation, then 99 more calls of _iterate
    double phi1 = ln.phi(stp), derphi1 = ln.derphi(stp);
    for (int i = 1; i < 100; ++i) {
        const Task task = d.iterate(stp, phi1, derphi1);
        if (!finite(stp)) return false;
        if (task == T_FG) {
            phi1 = ln.phi(stp);
            derphi1 = ln.derphi(stp);
        } else {
            if (task != T_CONV) return false;
            stp_out = stp;
            phi1_out = phi1;
            return true;
        }
    }
    return false;
}

// _cubicmin: the minimiser of the cubic through (a, fa, fpa), (b, fb), (c, fc), or nothing (NaN)
VM_HD double cubicmin(double a, double fa, double fpa, double b, double fb, double c, double fc) {
    Checked k;
    const double C = fpa;
    const double db = k.sub(b, a), dc = k.sub(c, a);
    const double dbdc = k.mul(db, dc);
    const double denom = k.mul(k.mul(dbdc, dbdc), k.sub(db, dc));
    const double d00 = k.mul(dc, dc), d01 = -k.mul(db, db), d10 = -k.pow3(dc), d11 = k.pow3(db);
    const double v0 = k.sub(k.sub(fb, fa), k.mul(C, db)), v1 = k.sub(k.sub(fc, fa), k.mul(C, dc));
    // np.dot of the 2 x 2 matrix with the vector: BLAS forms each row as fma(m0, v0, m1 * v1) (no error checks)
    double A = fma(d00, v0, d01 * v1), B = fma(d10, v0, d11 * v1);
    A = k.div(A, denom);
    B = k.div(B, denom);
    const double radical = k.sub(k.mul(B, B), k.mul(k.mul(3.0, A), C));
    const double xmin = k.add(a, k.div(k.add(-B, k.sqrt_(radical)), k.mul(3.0, A)));
    return (k.raised || !finite(xmin)) ? NAN : xmin;
}

// _quadmin: the minimiser of the parabola through (a, fa, fpa), (b, fb), or nothing (NaN)
VM_HD double quadmin(double a, double fa, double fpa, double b, double fb) {
    Checked k;
    const double D = fa, C = fpa;
    const double db = k.sub(b, a * 1.0);
    const double B = k.div(k.sub(k.sub(fb, D), k.mul(C, db)), k.mul(db, db));
    const double xmin = k.sub(a, k.div(C, k.mul(2.0, B)));
    return (k.raised || !finite(xmin)) ? NAN : xmin;
}

// _zoom: true with the step and phi there; the gradient there is ln.last_g
VM_HD bool zoom(Line& ln, double a_lo, double a_hi, double phi_lo, double phi_hi, double derphi_lo, double phi0, double derphi0,
                double& a_star, double& phi_star) {
    const double delta1 = 0.2, delta2 = 0.1;
    double phi_rec = phi0, a_rec = 0;
    for (int i = 0;; ) {
        const double dalpha = a_hi - a_lo;
        double a, b;
        if (dalpha < 0) { a = a_hi; b = a_lo; } else { a = a_lo; b = a_hi; }
        double a_j = NAN, cchk = 0;
        if (i > 0) {
            cchk = delta1 * dalpha;
            a_j = cubicmin(a_lo, phi_lo, derphi_lo, a_hi, phi_hi, a_rec, phi_rec);
        }
        if (i == 0 || a_j != a_j || a_j > b - cchk || a_j < a + cchk) {
            const double qchk = delta2 * dalpha;
            a_j = quadmin(a_lo, phi_lo, derphi_lo, a_hi, phi_hi);
            if (a_j != a_j || a_j > b - qchk || a_j < a + qchk) a_j = a_lo + 0.5 * dalpha;
        }
        const double phi_aj = ln.phi(a_j);
        if (phi_aj > phi0 + C1 * a_j * derphi0 || phi_aj >= phi_lo) {
            phi_rec = phi_hi; a_rec = a_hi;
            a_hi = a_j; phi_hi = phi_aj;
        } else {
            const double derphi_aj = ln.derphi(a_j);
            if (fabs(derphi_aj) <= -C2 * derphi0) {
                a_star = a_j;
                phi_star = phi_aj;
                return true;
            }
            if (derphi_aj * (a_hi - a_lo) >= 0) {
                phi_rec = phi_hi; a_rec = a_hi;
                a_hi = a_lo; phi_hi = phi_lo;
            } else {
                phi_rec = phi_lo; a_rec = a_lo;
            }
            a_lo = a_j; phi_lo = phi_aj; derphi_lo = derphi_aj;
        }
        if (++i > 10) return false;
    }
}

// scalar_search_wolfe2 (amax = 1e100, maxiter 10, no extra condition): true with the step and phi there; have_g: ln.last_g is the
// gradient at the step (false after the ten doublings: BFGS evaluates it itself)
VM_HD bool wolfe2(Line& ln, double phi0, double old_phi0, double derphi0, double& alpha_star, double& phi_star, bool& have_g) {
    double alpha0 = 0;
    double alpha1 = derphi0 != 0 ? py_min(1.0, 1.01 * 2 * (phi0 - old_phi0) / derphi0) : 1.0;
    if (alpha1 < 0) alpha1 = 1.0;
    alpha1 = py_min(alpha1, AMAX);
    double phi_a1 = ln.phi(alpha1), phi_a0 = phi0, derphi_a0 = derphi0;
    have_g = true;
    for (int i = 0; i < 10; ++i) {
        if (alpha1 == 0 || alpha0 > AMAX) return false;
        if (phi_a1 > phi0 + C1 * alpha1 * derphi0 || (phi_a1 >= phi_a0 && i > 0))
            return zoom(ln, alpha0, alpha1, phi_a0, phi_a1, derphi_a0, phi0, derphi0, alpha_star, phi_star);
        const double derphi_a1 = ln.derphi(alpha1);
        if (fabs(derphi_a1) <= -C2 * derphi0) {
            alpha_star = alpha1;
            phi_star = phi_a1;
            return true;
        }
        if (derphi_a1 >= 0) return zoom(ln, alpha1, alpha0, phi_a1, phi_a0, derphi_a1, phi0, derphi0, alpha_star, phi_star);
        const double alpha2 = py_min(2 * alpha1, AMAX);
        alpha0 = alpha1;
        alpha1 = alpha2;
        phi_a0 = phi_a1;
        phi_a1 = ln.phi(alpha1);
        derphi_a0 = derphi_a1;
    }
    alpha_star = alpha1;
    phi_star = phi_a1;
    have_g = false;
    return true;
}

struct Result {
    double x, fun;
    int nit, status;
};

// _minimize_bfgs in one dimension from x0 (gtol on |g|, norm = inf; xrtol = 0)
VM_HD Result bfgs(const Objective& obj, double x0, double gtol, int maxiter) {
    double xk = x0;
    double old_fval = obj.f(xk);
    double gfk = obj.grad(xk, old_fval);
    int k = 0;
    double Hk = 1.0;
    double old_old_fval = old_fval + sqrt(gfk * gfk) / 2;          // np.linalg.norm(gfk) / 2
    int warnflag = 0;
    double gnorm = fabs(gfk);
    while (gnorm > gtol && k < maxiter) {
        const double pk = -(Hk * gfk);
        Line ln{&obj, xk, pk};
        const double derphi0 = gfk * pk;
        double alpha_k, fnew;
        bool have_g = true;
        if (!wolfe1(ln, old_fval, old_old_fval, derphi0, alpha_k, fnew) &&
            !wolfe2(ln, old_fval, old_old_fval, derphi0, alpha_k, fnew, have_g)) {
            warnflag = 2;
            break;
        }
        old_old_fval = old_fval;
        old_fval = fnew;
        const double sk = alpha_k * pk;
        const double xkp1 = xk + sk;
        xk = xkp1;
        const double gfkp1 = have_g ? ln.last_g : obj.grad(xkp1, obj.f(xkp1));
        const double yk = gfkp1 - gfk;
        gfk = gfkp1;
        k += 1;
        gnorm = fabs(gfk);
        if (gnorm <= gtol) break;
        if (alpha_k * sqrt(pk * pk) <= 0.0 * (0.0 + sqrt(xk * xk))) break;
        if (!finite(old_fval)) {
            warnflag = 2;
            break;
        }
        const double rhok_inv = yk * sk;
        const double rhok = rhok_inv == 0. ? 1000.0 : 1. / rhok_inv;
        const double A1 = 1.0 - sk * yk * rhok;
        const double A2 = 1.0 - yk * sk * rhok;
        Hk = A1 * (Hk * A2) + rhok * sk * sk;
    }
    Result r{xk, old_fval, k, warnflag};
    if (warnflag != 2) {
        if (k >= maxiter) r.status = 1;
        else if (gnorm != gnorm || old_fval != old_fval || xk != xk) r.status = 3;
    }
    return r;
}

// map of one continuous row (VarInference.map, VI:355-376): x0 = the first component mean of largest belief, then BFGS
VM_HD Result map_continuous(const Row& row, double gtol, int maxiter) {
    double x0 = row.eta[0], b0 = belief(row, x0);
    for (int k = 1; k < row.K; ++k) {
        const double x = row.eta[2 * k], b = belief(row, x);
        if (b > b0) { x0 = x; b0 = b; }
    }
    return bfgs(Objective{row}, x0, gtol, maxiter);
}

}  // namespace vimap

// One thread per query row: continuous hidden rows run vimap::map_continuous; a discrete hidden row takes the first state of
// largest sum_k w_k eta_d[v, k, s] (np.argmax; its value goes to xout); observed rows (and indices outside [0, V)) give NaN,
// status -1.
__global__ void __launch_bounds__(BLOCK) vi_map_bfgs_kernel(lhvi_graph_t g, lhvi_vi_t p, int64_t nq, const int32_t* __restrict__ row_var,
                                                           double gtol, int32_t maxiter, double* __restrict__ xout,
                                                           double* __restrict__ fout, int32_t* __restrict__ nit,
                                                           int32_t* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const int v = row_var[i];
    double x = NAN, f = NAN;
    int it = 0, st = -1;
    if (v >= 0 && v < g.V && is_hidden(g.var_value[v])) {
        const int d = g.var_dom[v];
        if (g.dom_cont[d]) {
            const vimap::Row row{p.w, p.eta_c + (int64_t)v * p.K * 2, p.K, (p.quirks & LHVI_VI_GAUSSIAN_PDF) != 0};
            const vimap::Result r = vimap::map_continuous(row, gtol, maxiter);
            x = r.x; f = -r.fun; it = r.nit; st = r.status;
        } else {
            const int n = g.dom_ptr[d + 1] - g.dom_ptr[d];
            const double* e = p.eta_d + (int64_t)v * p.K * p.Dmax;
            int best = 0;
            double bb = 0.0;
            for (int s = 0; s < n && s < p.Dmax; ++s) {
                // b = w * eta_d[v, :, s], np.sum(b) in numpy's order
                double acc[8], sum = 0.0;
                if (p.K < 8) {
                    for (int k = 0; k < p.K; ++k) sum += p.w[k] * e[k * p.Dmax + s];
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] = p.w[j] * e[j * p.Dmax + s];
                    int k = 8;
                    for (; k < p.K - p.K % 8; k += 8) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) acc[j] += p.w[k + j] * e[(k + j) * p.Dmax + s];
                    }
                    sum = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
                    for (; k < p.K; ++k) sum += p.w[k] * e[k * p.Dmax + s];
                }
                if (s == 0 || (sum > bb && bb == bb) || (sum != sum && bb == bb)) { best = s; bb = sum; }   // np.argmax: first max, NaN wins
            }
            x = g.dom_val[g.dom_ptr[d] + best];
            f = bb; st = 0;
        }
    }
    xout[i] = x;
    if (fout) fout[i] = f;
    if (nit) nit[i] = it;
    if (status) status[i] = st;
}

}  // namespace lhvi

using namespace lhvi;

extern "C" {

int lhvi_vi_map_bfgs(const lhvi_graph_t* g, const lhvi_vi_t* p, int64_t nq, const int32_t* row_var, double gtol, int32_t maxiter,
                     double* xout, double* fout, int32_t* nit, int32_t* status, void* stream) {
    if (!g || !p || nq < 0 || maxiter < 0 || !(gtol >= 0.0)) return LHVI_E_ARG;
    if (p->K <= 0 || p->K > vimap::MAX_K || p->Dmax <= 0) return LHVI_E_UNSUPPORTED;
    if (nq == 0) return LHVI_OK;
    if (!row_var || !xout || !p->w || !p->eta_c || !p->eta_d || !g->var_value || !g->var_dom || !g->dom_cont || !g->dom_ptr ||
        !g->dom_val)
        return LHVI_E_ARG;
    hipLaunchKernelGGL(vi_map_bfgs_kernel, dim3(grid_for(nq)), dim3(BLOCK), 0, as_stream(stream), *g, *p, nq, row_var, gtol, maxiter,
                       xout, fout, nit, status);
    return check_launch();
}

}  // extern "C"
