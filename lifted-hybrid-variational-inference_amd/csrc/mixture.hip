// mixture.hip -- conditional queries on a fitted mixture belief (osi/mixture_beliefs.py:505-746), gfx950.
//   mix_prepare_kernel    per (row, component): the record (c, mu, 1 / var) and log pi
//   mix_tile_kernel       stage 1 of the conditioning: a thread sums one tile of observed variables for one component and a
//                         group of LHVI_MIX_ROWS evidence rows, which share its pass over the records
//   mix_finish_kernel     stage 2: a thread per evidence row adds the tiles in order, then logsumexp and the conditional weights
//   mix_map_kernel        marginal MAP of every (evidence row, query): a group of lanes per item, the lanes take the starts
//   mix_belief_kernel     log belief at P points per (evidence row, query)
// The arithmetic is csrc/mixture.hpp's, shared with the host twins at the end of this file.
#include "common.hpp"
#include "mixture.hpp"

namespace lhvi {
namespace mix {

__global__ void __launch_bounds__(BLOCK) mix_prepare_kernel(int V, int K, int Dmax, int normaliser, const double* __restrict__ w,
                                                            const double* __restrict__ eta_c, const double* __restrict__ eta_d,
                                                            const int32_t* __restrict__ nstates, double* logw, double* rec,
                                                            double* lpi) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= (int64_t)V * K) return;
    prepare_one(K, Dmax, normaliser, w, eta_c, eta_d, nstates, (int)(i / K), (int)(i % K), logw, rec, lpi);
}

// grid (items / BLOCK, tiles); item = (row group, component), the component fastest: neighbouring threads read neighbouring
// records and the same X values.  part: [M][tiles][K]
__global__ void __launch_bounds__(BLOCK) mix_tile_kernel(lhvi_mix_t b, int64_t M, int n_obs, const int32_t* __restrict__ obs_rows,
                                                         const double* __restrict__ X, double* part) {
    const int64_t item = (int64_t)blockIdx.x * BLOCK + threadIdx.x, groups = (M + ROWS - 1) / ROWS;
    if (item >= groups * b.K) return;
    const int k = (int)(item % b.K), t = blockIdx.y, tiles = gridDim.y;
    const int64_t m0 = item / b.K * ROWS;
    double out[ROWS];
    tile_partial<ROWS>(b, n_obs, obs_rows, X, M, m0, t, k, out);
    for (int j = 0; j < ROWS; ++j)
        if (m0 + j < M) part[((m0 + j) * tiles + t) * b.K + k] = out[j];
}

__global__ void __launch_bounds__(BLOCK) mix_finish_kernel(lhvi_mix_t b, int64_t M, int tiles, const double* __restrict__ part,
                                                           double* comp, double* logp, double* condw) {
    const int64_t m = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (m >= M) return;
    finish_row(b, tiles, part + m * tiles * b.K, comp ? comp + m * b.K : nullptr, logp ? logp + m : nullptr,
               condw ? condw + m * b.K : nullptr);
}

// one wavefront per workgroup, WAVE / lanes items each; item = m * n_q + q.  Every lane forms its candidate, one barrier,
// lane 0 of the group merges the candidates: the barrier is outside every branch.
__global__ void __launch_bounds__(WAVE) mix_map_kernel(lhvi_mix_t b, int64_t M, const double* __restrict__ condw, int n_q,
                                                       const int32_t* __restrict__ query_rows, const double* __restrict__ lo,
                                                       const double* __restrict__ hi, int n_obs, const double* __restrict__ X,
                                                       const int32_t* __restrict__ qobs_ptr, const int32_t* __restrict__ qobs_idx,
                                                       int lanes, int max_iter, double* xout, double* fout) {
    __shared__ Cand sh[WAVE];
    const int ipb = WAVE / lanes, lane = (int)threadIdx.x % lanes, grp = (int)threadIdx.x / lanes;
    const int64_t item = (int64_t)blockIdx.x * ipb + grp;
    const bool valid = item < M * n_q;
    const int64_t m = valid ? item / n_q : 0;
    const int q = valid ? (int)(item % n_q) : 0;
    Cand c{NEG_INF, __builtin_nan(""), -1};
    double obs = __builtin_nan("");
    if (valid) {
        obs = observed_value(qobs_ptr, qobs_idx, q, X + m * n_obs);
        if (!(obs == obs)) c = lane_candidate(b, query_rows[q], condw + m * b.K, lo[q], hi[q], max_iter, lane, lanes);
    }
    sh[threadIdx.x] = c;
    __syncthreads();
    if (valid && lane == 0) {
        Cand best = sh[grp * lanes];
        for (int j = 1; j < lanes; ++j)
            if (better(sh[grp * lanes + j], best)) best = sh[grp * lanes + j];
        const bool seen = obs == obs;
        xout[item] = seen ? obs : best.x;
        fout[item] = seen || best.key < 0 ? __builtin_nan("") : best.f;
    }
}

__global__ void __launch_bounds__(BLOCK) mix_belief_kernel(lhvi_mix_t b, int64_t M, const double* __restrict__ condw, int n_q,
                                                           const int32_t* __restrict__ query_rows, int P,
                                                           const double* __restrict__ x, double* out) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= M * n_q * P) return;
    const int64_t m = i / ((int64_t)n_q * P);
    const int64_t qp = i % ((int64_t)n_q * P);
    out[i] = log_belief_point(b, query_rows[qp / P], condw + m * b.K, x[qp]);
}

struct WaveLanes {
    int lane, lanes;
    __device__ __forceinline__ void sync() const { __syncthreads(); }
};

// one workgroup of one wavefront per start; ws: joint_ws_doubles() doubles per start
__global__ void __launch_bounds__(WAVE) mix_joint_kernel(lhvi_mix_t b, JointArgs a, const double* __restrict__ x0,
                                                         const int32_t* __restrict__ xd0, double* ws, double* xc, int32_t* xd,
                                                         double* best_obj) {
    const int64_t s = blockIdx.x;
    const int per = (joint_ws_doubles(b.K, a.Nc, a.Nd, b.Dmax) + 1) & ~1;
    joint_start(b, a, x0 + s * a.Nc, xd0 + s * a.Nd, ws + s * per, WaveLanes{(int)threadIdx.x, WAVE}, xc + s * a.Nc, xd + s * a.Nd,
                best_obj + s);
}

static int belief_check(const lhvi_mix_t* b) {
    if (!b || b->V < 0 || b->K < 1 || b->Dmax < 1) return LHVI_E_ARG;
    if (b->K > LHVI_MIX_MAX_K) return LHVI_E_UNSUPPORTED;
    if (b->V && (!b->nstates || !b->logw || !b->rec)) return LHVI_E_ARG;
    return LHVI_OK;
}

static int prepare_check(int32_t V, int32_t K, int32_t Dmax, int32_t normaliser, const double* w, const int32_t* nstates,
                         double* logw, double* rec) {
    if (V < 0 || K < 1 || Dmax < 1 || (normaliser != LHVI_MIX_GAUSSIAN && normaliser != LHVI_MIX_VI)) return LHVI_E_ARG;
    if (K > LHVI_MIX_MAX_K) return LHVI_E_UNSUPPORTED;
    if (V && (!w || !nstates || !logw || !rec)) return LHVI_E_ARG;
    return LHVI_OK;
}

static int condition_check(const lhvi_mix_t* b, int64_t M, int32_t n_obs, const int32_t* obs_rows, const double* X, double* ws) {
    const int rc = belief_check(b);
    if (rc) return rc;
    if (M < 0 || n_obs < 0 || (n_obs && M && (!obs_rows || !X || !ws))) return LHVI_E_ARG;
    return LHVI_OK;
}

static int query_check(const lhvi_mix_t* b, int64_t M, const double* condw, int32_t n_q, const int32_t* query_rows) {
    const int rc = belief_check(b);
    if (rc) return rc;
    if (M < 0 || n_q < 0 || (M && n_q && (!condw || !query_rows))) return LHVI_E_ARG;
    return LHVI_OK;
}

}  // namespace mix
}  // namespace lhvi

using namespace lhvi;
using namespace lhvi::mix;

extern "C" {

size_t lhvi_mix_condition_ws_doubles(int64_t M, int32_t n_obs, int32_t K) {
    if (M < 0 || n_obs < 0 || K < 0) return 0;
    return (size_t)M * tiles_of(n_obs) * K;
}

int lhvi_mix_prepare(int32_t V, int32_t K, int32_t Dmax, int32_t normaliser, const double* w, const double* eta_c,
                     const double* eta_d, const int32_t* nstates, double* logw, double* rec, double* lpi, void* stream) {
    const int rc = prepare_check(V, K, Dmax, normaliser, w, nstates, logw, rec);
    if (rc) return rc;
    if (lpi && !eta_d) return LHVI_E_ARG;
    if (V == 0) return LHVI_OK;
    hipLaunchKernelGGL(mix_prepare_kernel, dim3(grid_for((int64_t)V * K)), dim3(BLOCK), 0, as_stream(stream), (int)V, (int)K,
                       (int)Dmax, (int)normaliser, w, eta_c, eta_d, nstates, logw, rec, lpi);
    return check_launch();
}

int lhvi_mix_condition(const lhvi_mix_t* b, int64_t M, int32_t n_obs, const int32_t* obs_rows, const double* X, double* ws,
                       double* comp, double* logp, double* condw, void* stream) {
    const int rc = condition_check(b, M, n_obs, obs_rows, X, ws);
    if (rc) return rc;
    if (M == 0) return LHVI_OK;
    const int tiles = tiles_of(n_obs);
    const int64_t items = (M + ROWS - 1) / ROWS * b->K;
    if (items > (int64_t)0x7fffffff * BLOCK || tiles > 65535) return LHVI_E_UNSUPPORTED;
    hipStream_t st = as_stream(stream);
    if (tiles)
        hipLaunchKernelGGL(mix_tile_kernel, dim3(grid_for(items), tiles), dim3(BLOCK), 0, st, *b, M, (int)n_obs, obs_rows, X, ws);
    hipLaunchKernelGGL(mix_finish_kernel, dim3(grid_for(M)), dim3(BLOCK), 0, st, *b, M, tiles, (const double*)ws, comp, logp,
                       condw);
    return check_launch();
}

int lhvi_mix_marginal_map(const lhvi_mix_t* b, int64_t M, const double* condw, int32_t n_q, const int32_t* query_rows,
                          const double* lo, const double* hi, int32_t n_obs, const double* X, const int32_t* qobs_ptr,
                          const int32_t* qobs_idx, int32_t lanes, int32_t max_iter, double* xout, double* fout, void* stream) {
    const int rc = query_check(b, M, condw, n_q, query_rows);
    if (rc) return rc;
    if (lanes < 1 || lanes > WAVE || (lanes & (lanes - 1)) || max_iter < 0 || n_obs < 0) return LHVI_E_ARG;
    if (M == 0 || n_q == 0) return LHVI_OK;
    if (!lo || !hi || !xout || !fout || (qobs_ptr && (!qobs_idx || (n_obs && !X)))) return LHVI_E_ARG;
    const int ipb = WAVE / lanes;
    const int64_t blocks = (M * n_q + ipb - 1) / ipb;
    if (blocks > 0x7fffffff) return LHVI_E_UNSUPPORTED;
    hipLaunchKernelGGL(mix_map_kernel, dim3((unsigned)blocks), dim3(WAVE), 0, as_stream(stream), *b, M, condw, (int)n_q, query_rows,
                       lo, hi, (int)n_obs, X, qobs_ptr, qobs_idx, (int)lanes, (int)max_iter, xout, fout);
    return check_launch();
}

int lhvi_mix_log_belief(const lhvi_mix_t* b, int64_t M, const double* condw, int32_t n_q, const int32_t* query_rows, int32_t P,
                        const double* x, double* out, void* stream) {
    const int rc = query_check(b, M, condw, n_q, query_rows);
    if (rc) return rc;
    if (P < 0) return LHVI_E_ARG;
    if (M == 0 || n_q == 0 || P == 0) return LHVI_OK;
    if (!x || !out) return LHVI_E_ARG;
    const int64_t n = M * n_q * P;
    if (n > (int64_t)0x7fffffff * BLOCK) return LHVI_E_UNSUPPORTED;
    hipLaunchKernelGGL(mix_belief_kernel, dim3(grid_for(n)), dim3(BLOCK), 0, as_stream(stream), *b, M, condw, (int)n_q, query_rows,
                       (int)P, x, out);
    return check_launch();
}

static int joint_check(const lhvi_mix_t* b, const double* logw, int32_t Nc, const int32_t* crows, const double* lo, const double* hi,
                       int32_t Nd, const int32_t* drows, int32_t S, const double* x0, const int32_t* xd0, int32_t coord_its,
                       int32_t grad_its, double* ws, double* xc, int32_t* xd, double* best_obj) {
    const int rc = belief_check(b);
    if (rc) return rc;
    if (Nc < 0 || Nd < 0 || S < 0 || coord_its < 0 || grad_its < 0) return LHVI_E_ARG;
    if (S == 0) return LHVI_OK;
    if (!logw || !ws || !best_obj || (Nc && (!crows || !lo || !hi || !x0 || !xc)) || (Nd && (!drows || !xd0 || !xd || !b->lpi)))
        return LHVI_E_ARG;
    return LHVI_OK;
}

size_t lhvi_mix_joint_map_ws_doubles(int32_t K, int32_t Nc, int32_t Nd, int32_t Dmax, int32_t S) {
    if (K < 0 || Nc < 0 || Nd < 0 || Dmax < 0 || S < 0) return 0;
    return (size_t)S * ((joint_ws_doubles(K, Nc, Nd, Dmax) + 1) & ~1);
}

int lhvi_mix_joint_map(const lhvi_mix_t* b, const double* logw, int32_t Nc, const int32_t* crows, const double* lo, const double* hi,
                       int32_t Nd, const int32_t* drows, int32_t S, const double* x0, const int32_t* xd0, int32_t coord_its,
                       double gamma, double grad_lr, int32_t grad_its, double tol, double* ws, double* xc, int32_t* xd,
                       double* best_obj, void* stream) {
    const int rc = joint_check(b, logw, Nc, crows, lo, hi, Nd, drows, S, x0, xd0, coord_its, grad_its, ws, xc, xd, best_obj);
    if (rc || S == 0) return rc;
    const JointArgs a{Nc, Nd, crows, drows, lo, hi, logw, coord_its, grad_its, gamma, grad_lr, tol};
    hipLaunchKernelGGL(mix_joint_kernel, dim3(S), dim3(WAVE), 0, as_stream(stream), *b, a, x0, xd0, ws, xc, xd, best_obj);
    return check_launch();
}

int lhvi_mix_joint_map_host(const lhvi_mix_t* b, const double* logw, int32_t Nc, const int32_t* crows, const double* lo,
                            const double* hi, int32_t Nd, const int32_t* drows, int32_t S, const double* x0, const int32_t* xd0,
                            int32_t coord_its, double gamma, double grad_lr, int32_t grad_its, double tol, double* ws, double* xc,
                            int32_t* xd, double* best_obj) {
    const int rc = joint_check(b, logw, Nc, crows, lo, hi, Nd, drows, S, x0, xd0, coord_its, grad_its, ws, xc, xd, best_obj);
    if (rc || S == 0) return rc;
    const JointArgs a{Nc, Nd, crows, drows, lo, hi, logw, coord_its, grad_its, gamma, grad_lr, tol};
    const int per = (joint_ws_doubles(b->K, Nc, Nd, b->Dmax) + 1) & ~1;
    for (int64_t s = 0; s < S; ++s)
        joint_start(*b, a, x0 + s * Nc, xd0 + s * Nd, ws + s * per, HostLanes(), xc + s * Nc, xd + s * Nd, best_obj + s);
    return LHVI_OK;
}

// ---- host twins: the same mixture.hpp code, one "lane" -------------------------------------------------------------------
int lhvi_mix_prepare_host(int32_t V, int32_t K, int32_t Dmax, int32_t normaliser, const double* w, const double* eta_c,
                          const double* eta_d, const int32_t* nstates, double* logw, double* rec, double* lpi) {
    const int rc = prepare_check(V, K, Dmax, normaliser, w, nstates, logw, rec);
    if (rc) return rc;
    if (lpi && !eta_d) return LHVI_E_ARG;
    for (int v = 0; v < V; ++v)
        for (int k = 0; k < K; ++k) prepare_one(K, Dmax, normaliser, w, eta_c, eta_d, nstates, v, k, logw, rec, lpi);
    return LHVI_OK;
}

int lhvi_mix_condition_host(const lhvi_mix_t* b, int64_t M, int32_t n_obs, const int32_t* obs_rows, const double* X, double* ws,
                            double* comp, double* logp, double* condw) {
    const int rc = condition_check(b, M, n_obs, obs_rows, X, ws);
    if (rc) return rc;
    const int tiles = tiles_of(n_obs), K = b->K;
    for (int64_t m0 = 0; m0 < M; m0 += ROWS)
        for (int t = 0; t < tiles; ++t)
            for (int k = 0; k < K; ++k) {
                double out[ROWS];
                tile_partial<ROWS>(*b, n_obs, obs_rows, X, M, m0, t, k, out);
                for (int j = 0; j < ROWS && m0 + j < M; ++j) ws[((m0 + j) * tiles + t) * K + k] = out[j];
            }
    for (int64_t m = 0; m < M; ++m)
        finish_row(*b, tiles, ws + m * tiles * K, comp ? comp + m * K : nullptr, logp ? logp + m : nullptr,
                   condw ? condw + m * K : nullptr);
    return LHVI_OK;
}

int lhvi_mix_marginal_map_host(const lhvi_mix_t* b, int64_t M, const double* condw, int32_t n_q, const int32_t* query_rows,
                               const double* lo, const double* hi, int32_t n_obs, const double* X, const int32_t* qobs_ptr,
                               const int32_t* qobs_idx, int32_t max_iter, double* xout, double* fout) {
    const int rc = query_check(b, M, condw, n_q, query_rows);
    if (rc) return rc;
    if (max_iter < 0 || n_obs < 0) return LHVI_E_ARG;
    if (M == 0 || n_q == 0) return LHVI_OK;
    if (!lo || !hi || !xout || !fout || (qobs_ptr && (!qobs_idx || (n_obs && !X)))) return LHVI_E_ARG;
    for (int64_t m = 0; m < M; ++m)
        for (int q = 0; q < n_q; ++q) {
            const int64_t item = m * n_q + q;
            const double obs = observed_value(qobs_ptr, qobs_idx, q, X + m * n_obs);
            if (obs == obs) {
                xout[item] = obs;
                fout[item] = __builtin_nan("");
                continue;
            }
            const Cand c = lane_candidate(*b, query_rows[q], condw + m * b->K, lo[q], hi[q], max_iter, 0, 1);
            xout[item] = c.x;
            fout[item] = c.key < 0 ? __builtin_nan("") : c.f;
        }
    return LHVI_OK;
}

int lhvi_mix_log_belief_host(const lhvi_mix_t* b, int64_t M, const double* condw, int32_t n_q, const int32_t* query_rows,
                             int32_t P, const double* x, double* out) {
    const int rc = query_check(b, M, condw, n_q, query_rows);
    if (rc) return rc;
    if (P < 0) return LHVI_E_ARG;
    if (M == 0 || n_q == 0 || P == 0) return LHVI_OK;
    if (!x || !out) return LHVI_E_ARG;
    for (int64_t m = 0; m < M; ++m)
        for (int64_t qp = 0; qp < (int64_t)n_q * P; ++qp)
            out[m * n_q * P + qp] = log_belief_point(*b, query_rows[qp / P], condw + m * b->K, x[qp]);
    return LHVI_OK;
}

}  // extern "C"
