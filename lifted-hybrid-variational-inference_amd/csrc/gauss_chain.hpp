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

// ---- the partitioned solve: one level of nested dissection along time (csrc/gauss_chain_part.hip) ---------------------------------
//
// S interiors separated by S - 1 single blocks.  Stage 1 (per interior I = blocks a .. b): chain_solve on the interior as a system
// of its own (z = J_I^-1 h_I, Sig0, logdet_p land in the caller's arrays and in the interior's record), then the spikes
// V = J_I^-1 E through the kept W_t, C_t; E has O_{a-1}^T in block row a (columns L) and O_b in block row b (columns R):
//   forward   Y_a = W_a E_a;  Y_{t+1} = W_{t+1} (E_{t+1} - C_t Y_t)        backward  V_t = W_t^T (Y_t - C_t^T V_{t+1})
// and G = E^T V (GLL, GLR, GRR), gL = sum_t VL_t^T h_t, gR likewise.  Stage 2: D~_p = D_s - GRR_p - GLL_{p+1}, O~_p = -GLR_{p+1},
// h~_p = h_s - gR_p - gL_{p+1}, solved by chain_solve with the covariances.  Stage 3 (per interior): with m = [mu_L; mu_R],
// Sbb the covariance of the two separators and T_t = [VL_t VR_t] Sbb:  mu_t = z_t - V_t m,  Sig[t, t] = Sig0 + T_t V_t^T,
// Sig[t, t + 1] = Sig0 + T_t V_{t+1}^T,  Sig[b, b + 1] = -T_b[:, R],  Sig[a - 1, a] = -T_a[:, L]^T.
// The padding of V is zero (identity on D, zeros on O), so stages 2 and 3 run over n, not P.

struct Partition {
    int64_t M, S, base, extra;              // S = the effective segment count; the first `extra` interiors hold base + 1 blocks
};

LHVI_GE_HD Partition partition_of(int64_t M, int64_t S) {
    Partition q;
    const int64_t half = (M + 1) / 2;
    q.M = M;
    q.S = S < half ? S : half;
    if (q.S < 1) q.S = 1;
    q.base = (M - (q.S - 1)) / q.S, q.extra = (M - (q.S - 1)) % q.S;
    return q;
}
LHVI_GE_HD int64_t first_block(const Partition& q, int64_t p) { return p * (q.base + 1) + (p < q.extra ? p : q.extra); }
LHVI_GE_HD int64_t last_block(const Partition& q, int64_t p) { return first_block(q, p) + q.base - (p < q.extra ? 0 : 1); }

// The workspace of a partitioned solve, in doubles.  Per system: W_t, C_t [M][P][P] (a slot per block), y_t [M][P], the spikes VL_t,
// VR_t [M][P][P], per interior the working buffers that do not fit LDS and a record (GLL, GLR, GRR [n][n], gL, gR [n], logdet,
// bad).  Then, each batch-contiguous as chain_solve takes them: the reduced chain's D~, O~, h~, its mu, var, cov, cross, logdet,
// bad and its own workspace.
struct PartLayout {
    int64_t per_system, yst, VL, VR, bufs, buf_doubles, rec, rec_doubles;
    int64_t R, R1;                          // blocks of the reduced chain, and its off-diagonal blocks
    int64_t Dr, Or, hr, mur, varr, covr, crossr, logdetr, badr, wsr, total;
};

LHVI_GE_HD PartLayout part_layout(int64_t B, int64_t M, int n, int P, int64_t S) {
    const int64_t pp = (int64_t)P * P, nn = (int64_t)n * n;
    const int64_t ld = P <= NB ? P + 1 : P, nbuf = P < NB ? 0 : (P == NB ? 5 : 6);
    PartLayout l;
    l.R = S - 1, l.R1 = S > 2 ? S - 2 : 0;
    l.yst = 2 * M * pp, l.VL = l.yst + M * P, l.VR = l.VL + M * pp, l.bufs = l.VR + M * pp;
    l.buf_doubles = nbuf * P * ld, l.rec_doubles = 3 * nn + 2 * n + 2;
    l.rec = l.bufs + S * l.buf_doubles;
    l.per_system = l.rec + S * l.rec_doubles;
    l.Dr = B * l.per_system, l.Or = l.Dr + B * l.R * nn, l.hr = l.Or + B * l.R1 * nn;
    l.mur = l.hr + B * l.R * n, l.varr = l.mur + B * l.R * n, l.covr = l.varr + B * l.R * n;
    l.crossr = l.covr + B * l.R * nn, l.logdetr = l.crossr + B * l.R1 * nn, l.badr = l.logdetr + B, l.wsr = l.badr + B;
    l.total = l.wsr + B * ws_per_system(l.R, P);
    return l;
}

struct PartArgs {
    int64_t B, M;
    int n;
    Partition q;
    PartLayout l;
    const double *D, *O, *h;
    double *ws, *mu, *var, *cov, *cross, *logdet;
    int32_t* bad;
};

LHVI_GE_HD double* part_record(const PartArgs& g, int64_t b, int64_t p) { return g.ws + b * g.l.per_system + g.l.rec + p * g.l.rec_doubles; }

// interior p of system b as a system of its own; its logdet and bad pivot go to the interior's record
template <int P>
LHVI_GE_HD System part_interior(const PartArgs& g, int64_t b, int64_t p) {
    const int64_t nn = (int64_t)g.n * g.n, pp = (int64_t)P * P, M = g.M, mo = M - 1, a = first_block(g.q, p);
    double *base = g.ws + b * g.l.per_system, *rec = part_record(g, b, p);
    System s;
    s.M = last_block(g.q, p) - a + 1, s.n = g.n;
    s.D = g.D + (b * M + a) * nn, s.O = g.O + (b * mo + a) * nn, s.h = g.h + (b * M + a) * g.n;
    s.Wst = base + a * pp, s.Cst = base + (M + a) * pp, s.yst = base + g.l.yst + a * P;
    s.mu = g.mu + (b * M + a) * g.n, s.var = g.var + (b * M + a) * g.n;
    s.cov = g.cov ? g.cov + (b * M + a) * nn : nullptr, s.cross = g.cross ? g.cross + (b * mo + a) * nn : nullptr;
    s.logdet = rec + 3 * nn + 2 * g.n, s.bad = reinterpret_cast<int32_t*>(rec + 3 * nn + 2 * g.n + 1);
    return s;
}

// the working buffers of interior p that live in the workspace (P >= 64)
template <int P>
LHVI_GE_HD void part_workspace_bufs(const PartArgs& g, int64_t b, int64_t p, Bufs& w) {
    using S = Shape<P>;
    double* q = g.ws + b * g.l.per_system + g.l.bufs + p * g.l.buf_doubles;
    w.Wm = q, w.Cm = q + S::BUF, w.Gm = q + 2 * S::BUF, w.Hm = q + 3 * S::BUF, w.Sg = q + 4 * S::BUF;
    if (P > NB) w.Sm = q + 5 * S::BUF;
}

// One spike of an interior after chain_solve: V = J_I^-1 E for E = OL^T in the first block row (LEFT) or OR in the last one, into
// Vst [m][P][P]; then its blocks of G and its share of g.  OL = O_{a-1}, OR = O_b [n][n], null where the interior has no such
// neighbour.  The forward pass of the right spike is zero before the last block.  w.Sg holds Y_t, then V_t, of the block before.
template <int P, bool LEFT, class Ctx>
LHVI_GE_HD void part_spike(const System& s, const Bufs& w, const Ctx& ctx, const double* OL, const double* OR, double* Vst, double* rec) {
    using S = Shape<P>;
    constexpr int LD = S::LD, PP = P * P;
    const int n = s.n;
    const int64_t m = s.M, nn = (int64_t)n * n;
    // ---- forward ----
    for (int64_t t = LEFT ? 0 : m - 1; t < m; ++t) {
        const bool head = !LEFT || t == 0;
        for (int e = ctx.lane; e < PP; e += ctx.lanes) {
            const int i = e / P, j = e % P;
            w.Wm[i * LD + j] = s.Wst[t * PP + e];
            if (!head) w.Cm[i * LD + j] = s.Cst[(t - 1) * PP + e];
            if (head) w.Hm[i * LD + j] = i < n && j < n ? (LEFT ? OL[(int64_t)j * n + i] : OR[(int64_t)i * n + j]) : 0.0;
        }
        ctx.sync();
        if (!head) {
            for (int e = ctx.lane; e < PP; e += ctx.lanes) {
                const int i = e / P, j = e % P;
                double acc = 0.0;
                for (int k = 0; k < P; ++k) acc = mac<true>(acc, w.Cm[i * LD + k], w.Sg[k * LD + j]);
                w.Hm[i * LD + j] = acc;
            }
            ctx.sync();
        }
        for (int e = ctx.lane; e < PP; e += ctx.lanes) {
            const int i = e / P, j = e % P;
            double acc = 0.0;
            for (int k = 0; k <= i; ++k) acc = mac<false>(acc, w.Wm[i * LD + k], w.Hm[k * LD + j]);
            w.Sg[i * LD + j] = acc;
            if (LEFT) Vst[t * PP + e] = acc;
        }
        ctx.sync();
    }
    // ---- backward: w.Wm holds W of the last block, w.Sg its Y ----
    for (int64_t t = m - 1; t >= 0; --t) {
        const bool tail = t == m - 1;
        if (!tail) {
            for (int e = ctx.lane; e < PP; e += ctx.lanes) {
                const int i = e / P, j = e % P;
                w.Wm[i * LD + j] = s.Wst[t * PP + e];
                w.Cm[i * LD + j] = s.Cst[t * PP + e];
            }
            ctx.sync();
        }
        for (int e = ctx.lane; e < PP; e += ctx.lanes) {
            const int i = e / P, j = e % P;
            double acc;
            if (tail) {
                acc = w.Sg[i * LD + j];
            } else {
                acc = LEFT ? Vst[t * PP + e] : 0.0;
                for (int k = 0; k < P; ++k) acc = mac<true>(acc, w.Cm[k * LD + i], w.Sg[k * LD + j]);
            }
            w.Gm[i * LD + j] = acc;
        }
        ctx.sync();
        for (int e = ctx.lane; e < PP; e += ctx.lanes) {
            const int i = e / P, j = e % P;
            double acc = 0.0;
            for (int k = i; k < P; ++k) acc = mac<false>(acc, w.Wm[k * LD + i], w.Gm[k * LD + j]);
            w.Sg[i * LD + j] = acc;
            Vst[t * PP + e] = acc;
        }
        ctx.sync();
        if (!LEFT && tail)                                          // GRR = O_b^T VR_b
            for (int e = ctx.lane; e < n * n; e += ctx.lanes) {
                const int i = e / n, j = e % n;
                double acc = 0.0;
                for (int k = 0; k < n; ++k) acc = mac<false>(acc, OR[(int64_t)k * n + i], w.Sg[k * LD + j]);
                rec[2 * nn + e] = acc;
            }
    }
    // ---- GLL = O_{a-1} VL_a or GLR = O_{a-1} VR_a (w.Sg holds V of the first block), and g = sum_t V_t^T h_t ----
    if (OL)
        for (int e = ctx.lane; e < n * n; e += ctx.lanes) {
            const int i = e / n, j = e % n;
            double acc = 0.0;
            for (int k = 0; k < n; ++k) acc = mac<false>(acc, OL[(int64_t)i * n + k], w.Sg[k * LD + j]);
            rec[(LEFT ? 0 : nn) + e] = acc;
        }
    for (int j = ctx.lane; j < n; j += ctx.lanes) {
        double acc = 0.0;
        for (int64_t t = 0; t < m; ++t)
            for (int i = 0; i < n; ++i) acc = mac<false>(acc, Vst[t * PP + i * P + j], s.h[t * n + i]);
        rec[3 * nn + (LEFT ? 0 : n) + j] = acc;
    }
    ctx.sync();
}

// stage 1 for interior p of system b
template <int P, class Ctx>
LHVI_GE_HD void part_stage1(const PartArgs& g, int64_t b, int64_t p, const Bufs& w, const Ctx& ctx) {
    const int64_t nn = (int64_t)g.n * g.n, pp = (int64_t)P * P, a = first_block(g.q, p);
    const System s = part_interior<P>(g, b, p);
    chain_solve<P>(s, w, ctx);
    double *base = g.ws + b * g.l.per_system, *rec = part_record(g, b, p);
    const double* OL = p > 0 ? s.O - nn : nullptr;
    const double* OR = p + 1 < g.q.S ? s.O + (s.M - 1) * nn : nullptr;
    if (OL) part_spike<P, true>(s, w, ctx, OL, OR, base + g.l.VL + a * pp, rec);
    if (OR) part_spike<P, false>(s, w, ctx, OL, OR, base + g.l.VR + a * pp, rec);
}

// stage 2's input: separator p of system b in the reduced chain
template <class Ctx>
LHVI_GE_HD void part_assemble(const PartArgs& g, int64_t b, int64_t p, const Ctx& ctx) {
    const int n = g.n;
    const int64_t nn = (int64_t)n * n, s = last_block(g.q, p) + 1;
    const double *lo = part_record(g, b, p), *hi = part_record(g, b, p + 1);
    const double *Ds = g.D + (b * g.M + s) * nn, *hs = g.h + (b * g.M + s) * n;
    double *Dr = g.ws + g.l.Dr + (b * g.l.R + p) * nn, *Or = g.ws + g.l.Or + (b * g.l.R1 + p) * nn;
    double* hr = g.ws + g.l.hr + (b * g.l.R + p) * n;
    for (int64_t e = ctx.lane; e < nn; e += ctx.lanes) {
        Dr[e] = (Ds[e] - lo[2 * nn + e]) - hi[e];
        if (p + 1 < g.l.R) Or[e] = -hi[nn + e];
    }
    for (int k = ctx.lane; k < n; k += ctx.lanes) hr[k] = (hs[k] - lo[3 * nn + n + k]) - hi[3 * nn + k];
}

// stage 3 for interior p of system b: the correction of its blocks, the copy of the separator after it, and (p = 0) the system's
// logdet and bad pivot.  w.Wm and w.Cm hold T_t = V_t Sbb, columns L and R.
template <int P, class Ctx>
LHVI_GE_HD void part_correct(const PartArgs& g, int64_t b, int64_t p, const Bufs& w, const Ctx& ctx) {
    using S = Shape<P>;
    constexpr int LD = S::LD, PP = P * P;
    const int n = g.n;
    const int64_t nn = (int64_t)n * n, M = g.M, mo = M - 1, R = g.l.R, R1 = g.l.R1;
    const int64_t a = first_block(g.q, p), z = last_block(g.q, p);
    const bool hasL = p > 0, hasR = p + 1 < g.q.S;
    const double* base = g.ws + b * g.l.per_system;
    const double *mL = g.ws + g.l.mur + (b * R + p - 1) * n, *mR = mL + n;
    const double *SLL = g.ws + g.l.covr + (b * R + p - 1) * nn, *SRR = SLL + nn;
    const double* SLR = g.ws + g.l.crossr + (b * R1 + p - 1) * nn;
    double *mu = g.mu + b * M * n, *var = g.var + b * M * n;
    double *cov = g.cov ? g.cov + b * M * nn : nullptr, *cross = g.cross ? g.cross + b * mo * nn : nullptr;
    for (int64_t t = a; t <= z; ++t) {
        const double *VL = base + g.l.VL + t * PP, *VR = base + g.l.VR + t * PP;
        for (int e = ctx.lane; e < n * n; e += ctx.lanes) {
            const int i = e / n, c = e % n;
            if (hasL) {
                double acc = 0.0;
                for (int k = 0; k < n; ++k) acc = mac<false>(acc, VL[i * P + k], SLL[(int64_t)k * n + c]);
                if (hasR)
                    for (int k = 0; k < n; ++k) acc = mac<false>(acc, VR[i * P + k], SLR[(int64_t)c * n + k]);
                w.Wm[i * LD + c] = acc;
            }
            if (hasR) {
                double acc = 0.0;
                if (hasL)
                    for (int k = 0; k < n; ++k) acc = mac<false>(acc, VL[i * P + k], SLR[(int64_t)k * n + c]);
                for (int k = 0; k < n; ++k) acc = mac<false>(acc, VR[i * P + k], SRR[(int64_t)k * n + c]);
                w.Cm[i * LD + c] = acc;
            }
        }
        for (int i = ctx.lane; i < n; i += ctx.lanes) {
            double acc = mu[t * n + i];
            if (hasL)
                for (int k = 0; k < n; ++k) acc = mac<true>(acc, VL[i * P + k], mL[k]);
            if (hasR)
                for (int k = 0; k < n; ++k) acc = mac<true>(acc, VR[i * P + k], mR[k]);
            mu[t * n + i] = acc;
        }
        ctx.sync();
        for (int e = ctx.lane; e < n * n; e += ctx.lanes) {
            const int i = e / n, j = e % n;
            if (j <= i && (cov || i == j)) {
                double acc = i == j ? var[t * n + i] : cov[t * nn + e];
                if (hasL)
                    for (int c = 0; c < n; ++c) acc = mac<false>(acc, w.Wm[i * LD + c], VL[j * P + c]);
                if (hasR)
                    for (int c = 0; c < n; ++c) acc = mac<false>(acc, w.Cm[i * LD + c], VR[j * P + c]);
                if (i == j) var[t * n + i] = acc;
                if (cov) cov[t * nn + e] = acc, cov[t * nn + (int64_t)j * n + i] = acc;
            }
            if (!cross) continue;
            if (t < z) {
                double acc = cross[t * nn + e];
                if (hasL)
                    for (int c = 0; c < n; ++c) acc = mac<false>(acc, w.Wm[i * LD + c], VL[PP + j * P + c]);
                if (hasR)
                    for (int c = 0; c < n; ++c) acc = mac<false>(acc, w.Cm[i * LD + c], VR[PP + j * P + c]);
                cross[t * nn + e] = acc;
            } else if (hasR) {
                cross[t * nn + e] = -w.Cm[i * LD + j];
            }
            if (t == a && hasL) cross[(t - 1) * nn + e] = -w.Wm[j * LD + i];
        }
        ctx.sync();
    }
    if (hasR) {
        const int64_t s = z + 1;
        for (int e = ctx.lane; e < n * n; e += ctx.lanes) {
            if (e < n) mu[s * n + e] = mR[e], var[s * n + e] = g.ws[g.l.varr + (b * R + p) * n + e];
            if (cov) cov[s * nn + e] = SRR[e];
        }
    }
    if (p == 0 && ctx.lane == 0) {
        double acc = 0.0;
        int bad_block = -1, bad_col = -1;
        for (int64_t k = 0; k < g.q.S; ++k) {
            const double* rec = part_record(g, b, k) + 3 * nn + 2 * n;
            const int32_t* bd = reinterpret_cast<const int32_t*>(rec + 1);
            acc += rec[0];
            if (bd[0] >= 0 && (bad_block < 0 || first_block(g.q, k) + bd[0] < bad_block))
                bad_block = (int)(first_block(g.q, k) + bd[0]), bad_col = bd[1];
        }
        const int32_t* bd = reinterpret_cast<const int32_t*>(g.ws + g.l.badr + b);
        if (bd[0] >= 0 && (bad_block < 0 || last_block(g.q, bd[0]) + 1 < bad_block))
            bad_block = (int)(last_block(g.q, bd[0]) + 1), bad_col = bd[1];
        g.logdet[b] = acc + g.ws[g.l.logdetr + b];
        g.bad[2 * b] = bad_block, g.bad[2 * b + 1] = bad_col;
    }
}

}  // namespace gchain
}  // namespace lhvi
