// gauss_exact.hpp -- tile routines of the dense fp64 Cholesky behind the exact Gaussian-MRF marginals, written once for the device
// (csrc/gauss_exact.hip) and the host twin (lhvi_gauss_exact_host).
//
// Storage.  A symmetric N x N matrix is padded to Np = T * NB (identity on the padding, so no kernel has a ragged edge) and only
// its lower block triangle is kept: tile (i, j), j <= i, starts at tile_off(i, j) doubles and is column-major, element (r, c) at
// c * NB + r.  The factor L overwrites J tile by tile; X = L^-1 lives in a second triangle of the same shape.
//
// Arithmetic.  Every element is one fused multiply-add chain in ascending k (mac / the loops of potrf_tile and trinv_tile), on the
// device as on the host, so the two differ only where the device's sqrt, division or log differ from the host's.
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/lhvi.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LHVI_GE_HD __host__ __device__ __forceinline__
#else
#define LHVI_GE_HD inline
#endif

namespace lhvi {
namespace gauss {

constexpr int NB = LHVI_GAUSS_EXACT_NB;      // tile edge
constexpr int TILE = NB * NB;
constexpr int LDT = NB + 1;                  // row stride of a diagonal tile while it is factorised (odd: rows on different LDS banks)

LHVI_GE_HD int64_t tiles_of(int64_t N) { return (N + NB - 1) / NB; }
LHVI_GE_HD int64_t tri_tiles(int64_t T) { return T * (T + 1) / 2; }
LHVI_GE_HD int64_t tile_index(int64_t i, int64_t j) { return i * (i + 1) / 2 + j; }
LHVI_GE_HD int64_t tile_off(int64_t i, int64_t j) { return tile_index(i, j) * TILE; }
// element (gi, gj), gi >= gj, of a packed triangle
LHVI_GE_HD int64_t elem_off(int64_t gi, int64_t gj) { return tile_off(gi / NB, gj / NB) + (gj % NB) * NB + gi % NB; }

// (i, j) of the t-th tile of the triangle
LHVI_GE_HD void tile_of_index(int64_t t, int64_t& i, int64_t& j) {
    i = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (i * (i + 1) / 2 > t) --i;
    while ((i + 1) * (i + 2) / 2 <= t) ++i;
    j = t - i * (i + 1) / 2;
}

// one step of an inner product: acc - a b (SUB) or acc + a b
template <bool SUB>
LHVI_GE_HD double mac(double acc, double a, double b) {
    return SUB ? fma(-a, b, acc) : fma(a, b, acc);
}

struct HostCtx {
    int lane = 0, lanes = 1;
    void sync() const {}
};

// Cholesky of one diagonal tile, left-looking, one column per step (the column loop of exact.hpp with fused multiply-adds): `a`
// is row-major with stride LDT, its lower triangle is read.  A lane forms the entries of the rows it owns and, redundantly (same
// bits), the pivot.  On return the lower triangle, diagonal included, holds L (ldiag [NB]: scratch).  A pivot <= 0 or NaN is
// taken as 1; returns the first such column or -1, the same value in every lane.
template <class Ctx>
LHVI_GE_HD int potrf_tile(double* a, double* ldiag, const Ctx& ctx) {
    int bad = -1;
    for (int j = 0; j < NB; ++j) {
        double d = a[j * LDT + j];
        for (int k = 0; k < j; ++k) d = fma(-a[j * LDT + k], a[j * LDT + k], d);
        if (!(d > 0.0)) {
            if (bad < 0) bad = j;
            d = 1.0;
        }
        const double l = sqrt(d);
        for (int r = ctx.lane; r < NB; r += ctx.lanes) {
            if (r == j) ldiag[j] = l;
            if (r > j) {
                double s = a[r * LDT + j];
                for (int k = 0; k < j; ++k) s = fma(-a[r * LDT + k], a[j * LDT + k], s);
                a[r * LDT + j] = s / l;
            }
        }
        ctx.sync();
    }
    for (int r = ctx.lane; r < NB; r += ctx.lanes) a[r * LDT + r] = ldiag[r];
    ctx.sync();
    return bad;
}

// X = L^-1 of a factorised diagonal tile: the lane that owns q forms column q by forward substitution,
// X_iq = -(sum_{k = q}^{i - 1} L_ik X_kq) / L_ii, and keeps it TRANSPOSED above the diagonal of `a` (a[q][i] = X_iq, i > q: the
// upper triangle is free), X_qq in xdiag [NB]
template <class Ctx>
LHVI_GE_HD void trinv_tile(double* a, double* xdiag, const Ctx& ctx) {
    for (int q = ctx.lane; q < NB; q += ctx.lanes) {
        const double xq = 1.0 / a[q * LDT + q];
        xdiag[q] = xq;
        for (int i = q + 1; i < NB; ++i) {
            double s = a[i * LDT + q] * xq;
            for (int k = q + 1; k < i; ++k) s = fma(a[i * LDT + k], a[q * LDT + k], s);
            a[q * LDT + i] = -s / a[i * LDT + i];
        }
    }
    ctx.sync();
}
// elements of the two results of a diagonal tile after potrf_tile and trinv_tile
LHVI_GE_HD double diag_L(const double* a, int r, int c) { return r >= c ? a[r * LDT + c] : 0.0; }
LHVI_GE_HD double diag_X(const double* a, const double* xdiag, int r, int c) {
    return r > c ? a[c * LDT + r] : (r == c ? xdiag[r] : 0.0);
}

// The tile product of the blocked algorithm on the host, element by element in the device kernel's order:
//   C = (SUB ? C : 0) -/+ A op(B), op(B) = B^T (TRANSB) or B; C may be A or B (the result is formed aside)
template <bool TRANSB, bool SUB>
inline void tile_gemm_host(double* C, const double* A, const double* B) {
    double out[TILE];
    for (int c = 0; c < NB; ++c)
        for (int r = 0; r < NB; ++r) {
            double acc = SUB ? C[c * NB + r] : 0.0;
            for (int k = 0; k < NB; ++k) acc = mac<SUB>(acc, A[k * NB + r], TRANSB ? B[k * NB + c] : B[c * NB + k]);
            out[c * NB + r] = acc;
        }
    for (int e = 0; e < TILE; ++e) C[e] = out[e];
}

// per-tile partial sums of the moments (X tile column-major): row r of X b_j, column c of X^T y_i, squared norm of column c
LHVI_GE_HD double tile_row_dot(const double* X, int r, const double* bj) {
    double s = 0.0;
    for (int c = 0; c < NB; ++c) s = fma(X[c * NB + r], bj[c], s);
    return s;
}
LHVI_GE_HD double tile_col_dot(const double* X, int c, const double* yi) {
    double s = 0.0;
    for (int r = 0; r < NB; ++r) s = fma(X[c * NB + r], yi[r], s);
    return s;
}
LHVI_GE_HD double tile_col_sq(const double* X, int c) {
    double s = 0.0;
    for (int r = 0; r < NB; ++r) s = fma(X[c * NB + r], X[c * NB + r], s);
    return s;
}

}  // namespace gauss
}  // namespace lhvi
