// hg_energy.hpp -- the joint log potential of one assignment (x_d, x_c) of a hybrid Gaussian MRF (osi/utils.py::
// eval_joint_assignment_energy on the flat model lhvi_exact_t) and the first-index arg-max's comparison, written once for the
// device (csrc/hg_energy.hip: one lane per assignment) and the host twins.  Every sum runs in one fixed order:
//   quadratic descriptors in descriptor order, each (sum_a sum_j P[a][j] x_a x_j, row-major) + (sum_a b_a x_a) + c,
//   then the table descriptors in descriptor order.
// The discrete state and the continuous point come through two callables, dig(variable) and x(variable): the device reads the
// digits from the configuration index or from x_d in global memory and the point from its row in LDS; no per-lane array.
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/lhvi.h"
#include "exact.hpp"

namespace lhvi {
namespace hg {

// the digits of a configuration index (exact::config's formula)
struct CfgDigits {
    const int64_t* dstride;
    const int32_t* dstates;
    int64_t cfg;
    LHVI_HD int operator()(int d) const { return (int)((cfg / dstride[d]) % dstates[d]); }
};

// the digits of an explicit row of x_d
struct RowDigits {
    const int32_t* row;
    LHVI_HD int operator()(int d) const { return row[d]; }
};

template <class Dig>
LHVI_HD int64_t local_cfg(const int32_t* p, int nd, const Dig& dig) {
    int64_t l = 0;
    for (int a = 0; a < nd; ++a) l += (int64_t)dig(p[2 * a]) * p[2 * a + 1];
    return l;
}

template <class Dig, class X>
LHVI_HD double energy(const lhvi_exact_t& m, const Dig& dig, const X& x) {
    double e = 0.0;
    for (int f = 0; f < m.n_quad; ++f) {
        const int32_t* rec = m.quad_desc + m.quad_ptr[f];
        const int nd = rec[0], nc = rec[1];
        const double* P = m.quad_par + rec[2] + local_cfg(rec + 3, nd, dig) * (int64_t)(nc * nc + nc + 1);
        const int32_t* sc = rec + 3 + 2 * nd;
        double q = 0.0, lin = 0.0;
        for (int a = 0; a < nc; ++a) {
            const double xa = x(sc[a]);
            for (int j = 0; j < nc; ++j) q += P[a * nc + j] * xa * x(sc[j]);
        }
        for (int a = 0; a < nc; ++a) lin += P[nc * nc + a] * x(sc[a]);
        e += (q + lin) + P[nc * nc + nc];
    }
    for (int f = 0; f < m.n_tab; ++f) {
        const int32_t* rec = m.tab_desc + m.tab_ptr[f];
        e += m.tab_par[rec[1] + local_cfg(rec + 2, rec[0], dig)];
    }
    return e;
}

// ---- first-index arg-max --------------------------------------------------------------------------------------------------
// (value, index) of the best entry so far; index -1: none yet.  NaN never enters; ties (+0 == -0 included) keep the smaller
// index, so merging in any order and any grouping gives the definition's answer.
struct Best {
    double v;
    int64_t i;
};
LHVI_HD Best best_none() { return Best{0.0, -1}; }
LHVI_HD Best best_merge(const Best& p, const Best& q) {
    const bool take = q.i >= 0 && (p.i < 0 || q.v > p.v || (q.v == p.v && q.i < p.i));
    return Best{take ? q.v : p.v, take ? q.i : p.i};
}
LHVI_HD void best_take(Best& b, double v, int64_t i) {
    if (v == v) b = best_merge(b, Best{v, i});
}

}  // namespace hg
}  // namespace lhvi
