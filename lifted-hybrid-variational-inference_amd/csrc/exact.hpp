// exact.hpp -- one discrete configuration of the exact hybrid-Gaussian baseline (gibbs/hybrid_gaussian_mrf.py::convert_to_bn),
// written once for the device (csrc/exact.hip: a group of lanes per configuration) and the host (lhvi_exact_config_host: one
// "lane").  The work is phrased as loops over the rows a lane owns (row = lane, lane + lanes, ...) separated by ctx.sync();
// every matrix element is produced by ONE lane with a serial loop in a fixed order, so the result does not depend on the
// number of lanes: the packed and the one-wavefront-per-configuration launches give the same bits.
//
// Workspace of a configuration (doubles): mat [Nc][ld], b [Nc], y [Nc], mu [Nc], ldiag [Nc], dinv [Nc], then Nd int32 digits.
//   mat: the joint A of the reference (get_joint_quadratic_params, factor order), then J = -(A + A^T) in the lower triangle,
//   its Cholesky factor L below the diagonal (diagonal in ldiag, reciprocal in dinv), and (L^-1)^T above the diagonal.
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/lhvi.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LHVI_HD __host__ __device__ __forceinline__
#else
#define LHVI_HD inline
#endif

namespace lhvi {
namespace exact {

LHVI_HD int ld_of(int Nc) { return Nc | 1; }                                   // odd row stride: rows fall on different LDS banks
LHVI_HD int ws_doubles(int Nc, int Nd) { return Nc * ld_of(Nc) + 5 * Nc + (Nd + 1) / 2; }

struct HostCtx {
    int lane = 0, lanes = 1;
    void sync() const {}
};

// local configuration index of a descriptor's discrete scope: pairs (variable, local stride) at p
LHVI_HD int64_t local_cfg(const int32_t* p, int nd, const int32_t* dig) {
    int64_t l = 0;
    for (int a = 0; a < nd; ++a) l += (int64_t)dig[p[2 * a]] * p[2 * a + 1];
    return l;
}

// The three steps of a configuration that the block Gibbs sampler (csrc/gibbs.hpp) enters with the discrete digits already in
// the workspace.  config() below calls them in this order; their floating-point operations are config()'s own.
//
// assemble: the joint quadratic A (mat, all of it), b and the constant c of the discrete state `dig`: every factor in factor
// order, a lane adds the rows it owns (utils.get_joint_quadratic_params)
template <class Ctx>
LHVI_HD void assemble(const lhvi_exact_t& m, const int32_t* dig, double* mat, double* b, const Ctx& ctx, double& c) {
    const int Nc = m.Nc, ld = ld_of(Nc);
    for (int r = ctx.lane; r < Nc; r += ctx.lanes) {
        for (int j = 0; j < Nc; ++j) mat[r * ld + j] = 0.0;
        b[r] = 0.0;
    }
    ctx.sync();
    c = 0.0;
    for (int f = 0; f < m.n_quad; ++f) {
        const int32_t* rec = m.quad_desc + m.quad_ptr[f];
        const int nd = rec[0], nc = rec[1];
        const double* P = m.quad_par + rec[2] + local_cfg(rec + 3, nd, dig) * (int64_t)(nc * nc + nc + 1);
        const int32_t* sc = rec + 3 + 2 * nd;
        for (int r = ctx.lane; r < Nc; r += ctx.lanes)
            for (int a = 0; a < nc; ++a)
                if (sc[a] == r) {
                    for (int j = 0; j < nc; ++j) mat[r * ld + sc[j]] += P[a * nc + j];
                    b[r] += P[nc * nc + a];
                }
        c += P[nc * nc + nc];
    }
}

// the log tables' sum at `dig`, in factor order
LHVI_HD double table_sum(const lhvi_exact_t& m, const int32_t* dig) {
    double ts = 0.0;
    for (int f = 0; f < m.n_tab; ++f) {
        const int32_t* rec = m.tab_desc + m.tab_ptr[f];
        ts += m.tab_par[rec[1] + local_cfg(rec + 2, rec[0], dig)];
    }
    return ts;
}

// form_J: J = -(A + A^T), lower triangle in place (= -2A for the symmetric A every potential class produces); the upper
// triangle is read here for the last time.  The caller syncs before (assemble's rows are complete) and this syncs after.
template <class Ctx>
LHVI_HD void form_J(int Nc, double* mat, const Ctx& ctx) {
    const int ld = ld_of(Nc);
    for (int r = ctx.lane; r < Nc; r += ctx.lanes)
        for (int j = 0; j <= r; ++j) mat[r * ld + j] = -(mat[r * ld + j] + mat[j * ld + r]);
    ctx.sync();
}

// cholesky: left-looking, one column per step: a lane forms its row's entry and (redundantly, same bits) the pivot.  L below
// the diagonal of mat, its diagonal in ldiag, the reciprocal in dinv.  Returns 1 on a pivot <= 0 or NaN (taken as 1), the same
// value in every lane.
template <class Ctx>
LHVI_HD int cholesky(int Nc, double* mat, double* ldiag, double* dinv, const Ctx& ctx, double& logdet) {
    const int ld = ld_of(Nc);
    int bad = 0;
    logdet = 0.0;
    for (int j = 0; j < Nc; ++j) {
        double d = mat[j * ld + j];
        for (int k = 0; k < j; ++k) d -= mat[j * ld + k] * mat[j * ld + k];
        if (!(d > 0.0)) { bad = 1; d = 1.0; }
        const double l = sqrt(d);
        logdet += log(d);
        for (int r = ctx.lane; r < Nc; r += ctx.lanes) {
            if (r == j) { ldiag[j] = l; dinv[j] = 1.0 / l; }
            if (r > j) {
                double s = mat[r * ld + j];
                for (int k = 0; k < j; ++k) s -= mat[r * ld + k] * mat[j * ld + k];
                mat[r * ld + j] = s / l;
            }
        }
        ctx.sync();
    }
    return bad;
}

// the digits of a configuration's workspace W
LHVI_HD int32_t* digits(int Nc, double* W) { return reinterpret_cast<int32_t*>(W + Nc * ld_of(Nc) + 5 * Nc); }

// The conditional Gaussian of the discrete state whose digits the lanes have just written to digits(Nc, W) (digit d by lane
// d % lanes; assemble's first barrier publishes them): config() below after its digit decode, and csrc/gibbs_rb.hip with a row of
// explicit digits.  Reads neither m.M nor m.dstride.  Outputs (each may be null): logp = log p~(x_d), mean [Nc],
// var [Nc] = diag(J^-1), cov [Nc][Nc] = J^-1.  Returns 1 when J is not positive definite (a pivot <= 0 or NaN), the same value
// in every lane.
template <class Ctx>
LHVI_HD int config_at(const lhvi_exact_t& m, double* W, const Ctx& ctx, double* logp, double* mean, double* var, double* cov) {
    const int Nc = m.Nc, ld = ld_of(Nc);
    double *mat = W, *b = W + Nc * ld, *y = b + Nc, *mu = y + Nc, *ldiag = mu + Nc, *dinv = ldiag + Nc;
    int32_t* dig = reinterpret_cast<int32_t*>(dinv + Nc);
    double c, logdet;
    assemble(m, dig, mat, b, ctx, c);
    const double ts = table_sum(m, dig);
    ctx.sync();
    form_J(Nc, mat, ctx);
    const int bad = cholesky(Nc, mat, ldiag, dinv, ctx, logdet);
    // X = L^-1, column q by the lane that owns row q, stored transposed above the diagonal: mat[q][i] = X[i][q], i > q
    for (int q = ctx.lane; q < Nc; q += ctx.lanes)
        for (int i = q + 1; i < Nc; ++i) {
            double s = mat[i * ld + q] * dinv[q];
            for (int k = q + 1; k < i; ++k) s += mat[i * ld + k] * mat[q * ld + k];
            mat[q * ld + i] = -s * dinv[i];
        }
    ctx.sync();
    // y = X b
    for (int r = ctx.lane; r < Nc; r += ctx.lanes) {
        double s = 0.0;
        for (int q = 0; q < r; ++q) s += mat[q * ld + r] * b[q];
        y[r] = s + dinv[r] * b[r];
    }
    ctx.sync();
    // mu = X^T y, var = squared column norms of X
    for (int r = ctx.lane; r < Nc; r += ctx.lanes) {
        double s = dinv[r] * y[r], v = dinv[r] * dinv[r];
        for (int i = r + 1; i < Nc; ++i) {
            const double x = mat[r * ld + i];
            s += x * y[i];
            v += x * x;
        }
        mu[r] = s;
        if (mean) mean[r] = s;
        if (var) var[r] = v;
        if (cov) {
            cov[(int64_t)r * Nc + r] = v;
            for (int q = 0; q < r; ++q) {            // Sig[r][q] = sum_{i >= r} X[i][r] X[i][q], q < r
                double t = dinv[r] * mat[q * ld + r];
                for (int i = r + 1; i < Nc; ++i) t += mat[r * ld + i] * mat[q * ld + i];
                cov[(int64_t)r * Nc + q] = t;
                cov[(int64_t)q * Nc + r] = t;
            }
        }
    }
    ctx.sync();
    // log p~(x_d) = tables + c + Nc/2 log 2pi - 1/2 log det J + 1/2 mu.b (hybrid_gaussian_mrf.py:57-65, same order of additions)
    double mub = 0.0;
    for (int i = 0; i < Nc; ++i) mub += mu[i] * b[i];
    double t = (double)Nc / 2 * 1.8378770664093453 + 0.5 * -logdet + 0.5 * mub;
    t += c;
    if (logp && ctx.lane == 0) *logp = ts + t;
    ctx.sync();                                      // the workspace may be reused by the caller's next configuration
    return bad;
}

// One configuration by its index: the digit decode, then config_at.
template <class Ctx>
LHVI_HD int config(const lhvi_exact_t& m, int64_t cfg, double* W, const Ctx& ctx, double* logp, double* mean, double* var,
                   double* cov) {
    const int Nc = m.Nc, Nd = m.Nd;
    // digits(Nc, W), spelled as config_at's own chain of offsets: the compiler then shares the address with it, and
    // exact_config_kernel keeps the registers it had before the split (scripts/kernel_resources.sh)
    double* dinv = W + Nc * ld_of(Nc) + Nc + Nc + Nc + Nc;
    int32_t* dig = reinterpret_cast<int32_t*>(dinv + Nc);
    for (int d = ctx.lane; d < Nd; d += ctx.lanes) dig[d] = (int32_t)((cfg / m.dstride[d]) % m.dstates[d]);
    return config_at(m, W, ctx, logp, mean, var, cov);
}

}  // namespace exact
}  // namespace lhvi
