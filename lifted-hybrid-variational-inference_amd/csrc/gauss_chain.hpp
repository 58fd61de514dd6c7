// gauss_chain.hpp -- block-tridiagonal fp64 Cholesky with the covariance recursion, written once for the device
// (csrc/gauss_chain.hip) and the host twin (lhvi_gauss_chain_host).  docs/kernels_gauss_chain.md has the derivation.
//
// One system: M diagonal blocks D_t [n][n] (symmetric), M - 1 blocks O_t = J[block t, block t + 1] [n][n], h_t [n].  The edge n is
// padded to P = padded_edge(n) in the working buffers (identity on D, zeros on O and h: the padding adds log 1 = 0 and stays
// decoupled), never in the caller's arrays.
//
//   forward   S_0 = D_0;  L_t = chol(S_t);  W_t = L_t^-1;  y_t = W_t (h_t - C_{t-1} y_{t-1});  C_t = O_t^T W_t^T;
//             S_{t+1} = D_{t+1} - C_t C_t^T;  logdet = 2 sum_t sum_i log L_t[i][i]
//   backward  G_t = C_t W_t;  mu_t = W_t^T (y_t - C_t^T mu_{t+1});  H_t = G_t^T Sig_{t+1} = -Sig[t, t+1];
//             Sig_t = W_t^T W_t + H_t G_t
//
// Arithmetic.  Every element is one fused multiply-add chain in ascending k, formed by whichever lane owns the element; the work
// is split over ctx.lanes lanes and the phases are separated by ctx.sync(), so the device (256 lanes, buffers in LDS or in an
// L2-resident workspace) and the host (one lane, buffers on the heap) run the same code and differ only where sqrt, division or
// log do.  A pivot <= 0 or NaN is taken as 1 (gauss_exact.hpp); the first one of a system is recorded as (block, column).
#pragma once
#include "gauss_exact.hpp"

namespace lhvi {
namespace gchain {

using gauss::mac;

constexpr int MAX_BLOCK = LHVI_GAUSS_CHAIN_MAX_BLOCK;
constexpr int NB = gauss::NB;

// the instantiated padded edges: 8, 16, 32 (everything in LDS), 64 (one tile of gauss_exact), 128 (2 x 2 such tiles)
LHVI_GE_HD int padded_edge(int n) { return n <= 8 ? 8 : n <= 16 ? 16 : n <= 32 ? 32 : n <= 64 ? 64 : 128; }

template <int P>
struct Shape {
    static constexpr int E = P < NB ? P : NB;             // edge of the tile that potrf / trinv work on
    static constexpr int LDA = E + 1;                     // its row stride (odd, as gauss::LDT)
    static constexpr int LD = P <= NB ? P + 1 : P;        // row stride of the P x P working buffers
    static constexpr int BUF = P * LD;
    static constexpr int TILE_A = E * LDA;
    static constexpr bool BUFS_IN_LDS = P < NB;
};

// doubles of workspace per system: W_t and C_t [P][P], y_t [P] for the backward pass, then the working buffers that do not fit LDS
LHVI_GE_HD int64_t ws_per_system(int64_t M, int P) {
    const int64_t pp = (int64_t)P * P;
    const int64_t ld = P <= NB ? P + 1 : P, nbuf = P < NB ? 0 : (P == NB ? 5 : 6);
    return M * pp + (M > 1 ? M - 1 : 0) * pp + M * P + nbuf * P * ld;
}

struct Bufs {
    double *a, *ldiag, *xdiag;              // the tile being factorised [E][LDA] and its two diagonals [E]
    double *Sm;                             // S_t [P][LD], lower triangle (P <= 64: the tile itself)
    double *Wm, *Cm, *Gm, *Hm, *Sg;         // [P][LD]: W_t, C_t, G_t (forward: scratch), H_t (forward: scratch), Sig_{t+1} (forward: O_t)
    double *yv, *rv, *mv;                   // [P]: y_t, a right-hand side, mu_{t+1}
};

struct System {
    int64_t M;
    int n;
    const double *D, *O, *h;                // [M][n][n], [M-1][n][n], [M][n]
    double *Wst, *Cst, *yst;                // workspace: [M][P][P], [M-1][P][P], [M][P]
    double *mu, *var, *cov, *cross;         // [M][n], [M][n], [M][n][n] or null, [M-1][n][n] or null
    double* logdet;                         // [1]
    int32_t* bad;                           // [2]: (block, column) of the first bad pivot, or (-1, -1)
};

// gauss::potrf_tile / trinv_tile at edge E (E = 64: those routines themselves)
template <int E, class Ctx>
LHVI_GE_HD int potrf_edge(double* a, double* ldiag, const Ctx& ctx) {
    if constexpr (E == NB) {
        return gauss::potrf_tile(a, ldiag, ctx);
    } else {
        constexpr int LDA = E + 1;
        int bad = -1;
        for (int j = 0; j < E; ++j) {
            double d = a[j * LDA + j];
            for (int k = 0; k < j; ++k) d = fma(-a[j * LDA + k], a[j * LDA + k], d);
            if (!(d > 0.0)) {
                if (bad < 0) bad = j;
                d = 1.0;
            }
            const double l = sqrt(d);
            for (int r = ctx.lane; r < E; r += ctx.lanes) {
                if (r == j) ldiag[j] = l;
                if (r > j) {
                    double s = a[r * LDA + j];
                    for (int k = 0; k < j; ++k) s = fma(-a[r * LDA + k], a[j * LDA + k], s);
                    a[r * LDA + j] = s / l;
                }
            }
            ctx.sync();
        }
        for (int r = ctx.lane; r < E; r += ctx.lanes) a[r * LDA + r] = ldiag[r];
        ctx.sync();
        return bad;
    }
}

template <int E, class Ctx>
LHVI_GE_HD void trinv_edge(double* a, double* xdiag, const Ctx& ctx) {
    if constexpr (E == NB) {
        gauss::trinv_tile(a, xdiag, ctx);
    } else {
        constexpr int LDA = E + 1;
        for (int q = ctx.lane; q < E; q += ctx.lanes) {
            const double xq = 1.0 / a[q * LDA + q];
            xdiag[q] = xq;
            for (int i = q + 1; i < E; ++i) {
                double s = a[i * LDA + q] * xq;
                for (int k = q + 1; k < i; ++k) s = fma(a[i * LDA + k], a[q * LDA + k], s);
                a[q * LDA + i] = -s / a[i * LDA + i];
            }
        }
        ctx.sync();
    }
}

// element (r, c) of X = L^-1 after potrf_edge and trinv_edge (gauss::diag_X at stride LDA)
template <int LDA>
LHVI_GE_HD double tile_X(const double* a, const double* xdiag, int r, int c) {
    return r > c ? a[c * LDA + r] : (r == c ? xdiag[r] : 0.0);
}

// factor the tile in w.a, add its sum of log pivots to `logsum` (lane 0's copy is the one that counts), record a bad pivot
template <int P, class Ctx>
LHVI_GE_HD void factor_tile(const Bufs& w, const Ctx& ctx, int64_t t, int col0, double& logsum, int& bad_block, int& bad_col) {
    using S = Shape<P>;
    const int rc = potrf_edge<S::E>(w.a, w.ldiag, ctx);
    if (rc >= 0 && bad_block < 0) bad_block = (int)t, bad_col = col0 + rc;
    for (int c = ctx.lane; c < S::E; c += ctx.lanes) w.xdiag[c] = log(w.ldiag[c]);      // xdiag is free until trinv_edge
    ctx.sync();
    if (ctx.lane == 0)
        for (int c = 0; c < S::E; ++c) logsum += w.xdiag[c];
    ctx.sync();
    trinv_edge<S::E>(w.a, w.xdiag, ctx);
}

// W_t = chol(S_t)^-1 into w.Wm (a plain lower-triangular matrix, zeros above the diagonal).  P <= 64: S_t is the tile.  P = 128:
// the 2 x 2 blocked factorisation on tiles of 64: L00 = chol(S00), L10 = S10 W00^T, L11 = chol(S11 - L10 L10^T),
// W10 = -W11 (L10 W00); L10 passes through w.Gm and L10 W00 through w.Hm.
template <int P, class Ctx>
LHVI_GE_HD void factor_block(const Bufs& w, const Ctx& ctx, int64_t t, double& logsum, int& bad_block, int& bad_col) {
    using S = Shape<P>;
    constexpr int LD = S::LD, LDA = S::LDA;
    if constexpr (P <= NB) {
        factor_tile<P>(w, ctx, t, 0, logsum, bad_block, bad_col);
        for (int e = ctx.lane; e < P * P; e += ctx.lanes) {
            const int i = e / P, j = e % P;
            w.Wm[i * LD + j] = tile_X<LDA>(w.a, w.xdiag, i, j);
        }
        ctx.sync();
    } else {
        constexpr int H = NB;
        static_assert(P == 2 * H, "two tiles a side");
        for (int e = ctx.lane; e < H * H; e += ctx.lanes) {
            const int i = e / H, j = e % H;
            if (j <= i) w.a[i * LDA + j] = w.Sm[i * LD + j];
        }
        ctx.sync();
        factor_tile<P>(w, ctx, t, 0, logsum, bad_block, bad_col);
        for (int e = ctx.lane; e < H * H; e += ctx.lanes) {
            const int i = e / H, j = e % H;
            w.Wm[i * LD + j] = tile_X<LDA>(w.a, w.xdiag, i, j);
            w.Wm[i * LD + H + j] = 0.0;
        }
        ctx.sync();
        for (int e = ctx.lane; e < H * H; e += ctx.lanes) {         // L10
            const int i = e / H, j = e % H;
            double acc = 0.0;
            for (int k = 0; k <= j; ++k) acc = mac<false>(acc, w.Sm[(H + i) * LD + k], w.Wm[j * LD + k]);
            w.Gm[i * LD + j] = acc;
        }
        ctx.sync();
        for (int e = ctx.lane; e < H * H; e += ctx.lanes) {         // S11 - L10 L10^T, and L10 W00
            const int i = e / H, j = e % H;
            if (j <= i) {
                double acc = w.Sm[(H + i) * LD + H + j];
                for (int k = 0; k < H; ++k) acc = mac<true>(acc, w.Gm[i * LD + k], w.Gm[j * LD + k]);
                w.a[i * LDA + j] = acc;
            }
            double acc = 0.0;
            for (int k = j; k < H; ++k) acc = mac<false>(acc, w.Gm[i * LD + k], w.Wm[k * LD + j]);
            w.Hm[i * LD + j] = acc;
        }
        ctx.sync();
        factor_tile<P>(w, ctx, t, H, logsum, bad_block, bad_col);
        for (int e = ctx.lane; e < H * H; e += ctx.lanes) {
            const int i = e / H, j = e % H;
            w.Wm[(H + i) * LD + H + j] = tile_X<LDA>(w.a, w.xdiag, i, j);
            double acc = 0.0;                                       // W10 = -W11 (L10 W00)
            for (int k = 0; k <= i; ++k) acc = mac<true>(acc, tile_X<LDA>(w.a, w.xdiag, i, k), w.Hm[k * LD + j]);
            w.Wm[(H + i) * LD + j] = acc;
        }
        ctx.sync();
    }
}

template <int P, class Ctx>
LHVI_GE_HD void chain_solve(const System& s, const Bufs& w, const Ctx& ctx) {
    using S = Shape<P>;
    constexpr int LD = S::LD, PP = P * P;
    const int n = s.n;
    const int64_t M = s.M, nn = (int64_t)n * n;
    double logsum = 0.0;
    int bad_block = -1, bad_col = -1;

    // ---- forward ----
    for (int64_t t = 0; t < M; ++t) {
        const double *Dt = s.D + t * nn, *ht = s.h + t * n;
        const bool more = t + 1 < M;
        // S_t (lower triangle), O_t, the right-hand side h_t - C_{t-1} y_{t-1}
        for (int e = ctx.lane; e < PP; e += ctx.lanes) {
            const int i = e / P, j = e % P;
            if (j <= i) {
                double acc = i < n ? Dt[(int64_t)i * n + j] : (i == j ? 1.0 : 0.0);
                if (t > 0)
                    for (int k = 0; k < P; ++k) acc = mac<true>(acc, w.Cm[i * LD + k], w.Cm[j * LD + k]);
                w.Sm[i * LD + j] = acc;
            }
            if (more) w.Sg[i * LD + j] = i < n && j < n ? s.O[t * nn + (int64_t)i * n + j] : 0.0;
        }
        for (int k = ctx.lane; k < P; k += ctx.lanes) {
            double acc = k < n ? ht[k] : 0.0;
            if (t > 0)
                for (int j = 0; j < P; ++j) acc = mac<true>(acc, w.Cm[k * LD + j], w.yv[j]);
            w.rv[k] = acc;
        }
        ctx.sync();
        factor_block<P>(w, ctx, t, logsum, bad_block, bad_col);
        // y_t = W_t r, C_t = O_t^T W_t^T; W_t, C_t and y_t are kept for the backward pass
        double *Wt = s.Wst + t * PP, *Ct = s.Cst + t * PP;
        for (int i = ctx.lane; i < P; i += ctx.lanes) {
            double acc = 0.0;
            for (int k = 0; k <= i; ++k) acc = mac<false>(acc, w.Wm[i * LD + k], w.rv[k]);
            w.yv[i] = acc;
            s.yst[t * P + i] = acc;
        }
        for (int e = ctx.lane; e < PP; e += ctx.lanes) {
            const int i = e / P, j = e % P;
            Wt[e] = w.Wm[i * LD + j];
            if (more) {
                double acc = 0.0;
                for (int k = 0; k <= j; ++k) acc = mac<false>(acc, w.Sg[k * LD + i], w.Wm[j * LD + k]);
                w.Cm[i * LD + j] = acc;
                Ct[e] = acc;
            }
        }
        ctx.sync();
    }
    if (ctx.lane == 0) {
        *s.logdet = 2.0 * logsum;
        s.bad[0] = bad_block;
        s.bad[1] = bad_col;
    }

    // ---- backward ----
    for (int64_t t = M - 1; t >= 0; --t) {
        const bool more = t + 1 < M;
        const double *Wt = s.Wst + t * PP, *Ct = s.Cst + t * PP;
        for (int e = ctx.lane; e < PP; e += ctx.lanes) {
            const int i = e / P, j = e % P;
            w.Wm[i * LD + j] = Wt[e];
            if (more) w.Cm[i * LD + j] = Ct[e];
        }
        for (int k = ctx.lane; k < P; k += ctx.lanes) w.yv[k] = s.yst[t * P + k];
        ctx.sync();
        // G_t = C_t W_t, the right-hand side y_t - C_t^T mu_{t+1}
        for (int k = ctx.lane; k < P; k += ctx.lanes) {
            double acc = w.yv[k];
            if (more)
                for (int j = 0; j < P; ++j) acc = mac<true>(acc, w.Cm[j * LD + k], w.mv[j]);
            w.rv[k] = acc;
        }
        if (more)
            for (int e = ctx.lane; e < PP; e += ctx.lanes) {
                const int i = e / P, j = e % P;
                double acc = 0.0;
                for (int k = j; k < P; ++k) acc = mac<false>(acc, w.Cm[i * LD + k], w.Wm[k * LD + j]);
                w.Gm[i * LD + j] = acc;
            }
        ctx.sync();
        // mu_t = W_t^T r, H_t = G_t^T Sig_{t+1}
        for (int i = ctx.lane; i < P; i += ctx.lanes) {
            double acc = 0.0;
            for (int k = i; k < P; ++k) acc = mac<false>(acc, w.Wm[k * LD + i], w.rv[k]);
            w.mv[i] = acc;
            if (i < n) s.mu[t * n + i] = acc;
        }
        if (more)
            for (int e = ctx.lane; e < PP; e += ctx.lanes) {
                const int i = e / P, j = e % P;
                double acc = 0.0;
                for (int k = 0; k < P; ++k) acc = mac<false>(acc, w.Gm[k * LD + i], w.Sg[k * LD + j]);
                w.Hm[i * LD + j] = acc;
                if (s.cross && i < n && j < n) s.cross[t * nn + (int64_t)i * n + j] = -acc;
            }
        ctx.sync();
        // Sig_t = W_t^T W_t + H_t G_t: the lower triangle is formed, the upper one mirrors it
        for (int e = ctx.lane; e < PP; e += ctx.lanes) {
            const int i = e / P, j = e % P;
            if (j > i) continue;
            double acc = 0.0;
            for (int k = i; k < P; ++k) acc = mac<false>(acc, w.Wm[k * LD + i], w.Wm[k * LD + j]);
            if (more)
                for (int k = 0; k < P; ++k) acc = mac<false>(acc, w.Hm[i * LD + k], w.Gm[k * LD + j]);
            w.Sg[i * LD + j] = acc;
            w.Sg[j * LD + i] = acc;
            if (i < n) {
                if (i == j) s.var[t * n + i] = acc;
                if (s.cov) {
                    s.cov[t * nn + (int64_t)i * n + j] = acc;
                    s.cov[t * nn + (int64_t)j * n + i] = acc;
                }
            }
        }
        ctx.sync();
    }
}

// the pointers of system b
LHVI_GE_HD System system_of(int64_t b, int64_t M, int n, int P, const double* D, const double* O, const double* h, double* ws,
                            double* mu, double* var, double* cov, double* cross, double* logdet, int32_t* bad) {
    const int64_t nn = (int64_t)n * n, pp = (int64_t)P * P, mo = M > 1 ? M - 1 : 0;
    System s;
    s.M = M, s.n = n;
    s.D = D + b * M * nn, s.O = O ? O + b * mo * nn : nullptr, s.h = h + b * M * n;
    double* base = ws + b * ws_per_system(M, P);
    s.Wst = base, s.Cst = base + M * pp, s.yst = s.Cst + mo * pp;
    s.mu = mu + b * M * n, s.var = var + b * M * n;
    s.cov = cov ? cov + b * M * nn : nullptr, s.cross = cross ? cross + b * mo * nn : nullptr;
    s.logdet = logdet + b, s.bad = bad + 2 * b;
    return s;
}

// the working buffers that live in the workspace (after W_t, C_t, y_t of the system)
template <int P>
LHVI_GE_HD void workspace_bufs(const System& s, Bufs& w) {
    using S = Shape<P>;
    double* p = s.yst + s.M * P;
    w.Wm = p, w.Cm = p + S::BUF, w.Gm = p + 2 * S::BUF, w.Hm = p + 3 * S::BUF, w.Sg = p + 4 * S::BUF;
    if (P > NB) w.Sm = p + 5 * S::BUF;
}

}  // namespace gchain
}  // namespace lhvi
