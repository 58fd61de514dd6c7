// gauss_exact.hip -- exact marginals of a Gaussian MRF by a dense blocked fp64 Cholesky (osi/utils.py
// get_gaussian_mean_params_from_quadratic_params), gfx950.  Storage and tile routines: csrc/gauss_exact.hpp.
//   ge_assemble_kernel   J = -(A + A^T) and b from the sorted contributions of the conditioned factors: one thread per entry,
//                        a serial sum in the host's order (no floating-point atomics)
//   ge_pack_kernel       the same J from a dense A
//   ge_potrf_kernel      step k, diagonal tile: L_kk and L_kk^-1 in LDS, one wavefront
//   ge_trsm_kernel       step k, panel: L_ik = A_ik L_kk^-T, one workgroup per tile below the diagonal
//   ge_syrk_kernel       step k, trailing update A_ij -= L_ik L_jk^T, one workgroup per lower-triangle tile (the flops)
//   ge_xrow_kernel / ge_xupd_kernel    X = L^-1 by blocked forward substitution: X_kj = L_kk^-1 W_kj, then W_ij -= L_ik X_kj
//   ge_moments*_kernel, ge_reduce_*    y = X b, mu = X^T y, var = squared column norms of X: per-tile partial sums, then sums
//                        over the tiles of a block row / column in ascending order
//   ge_cov_kernel        Sig[a][b] = sum_i X[i][a] X[i][b] for chosen columns
// The three products share tile_gemm: 64 x 64 output tile, 256 threads, a 4 x 4 register block each, the k panel staged
// through LDS 32 columns at a time (row stride 66 doubles), plain fp64 vector FMAs.
#include "common.hpp"
#include "gauss_exact.hpp"

namespace lhvi {
namespace gauss {

constexpr int KC = 32;             // k columns staged at a time
constexpr int LDS_LD = NB + 2;     // padded row stride of the staged panels (even: 16-byte aligned rows)
constexpr int GT = 256;            // threads of a product workgroup

struct DevCtx {
    int lane, lanes;
    __device__ __forceinline__ void sync() const { __syncthreads(); }
};

// C = (SUB ? C : 0) -/+ A op(B) on column-major tiles; C may alias A or B (it is written after the last panel is consumed)
template <bool TRANSB, bool SUB>
__device__ __forceinline__ void tile_gemm(double* __restrict__ sm, double* C, const double* A, const double* B) {
    double* As = sm;
    double* Bs = sm + KC * LDS_LD;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    double acc[4][4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        if (SUB) {
            const double4 c4 = *reinterpret_cast<const double4*>(C + (ty * 4 + v) * NB + tx * 4);
            acc[v][0] = c4.x, acc[v][1] = c4.y, acc[v][2] = c4.z, acc[v][3] = c4.w;
        } else {
            acc[v][0] = acc[v][1] = acc[v][2] = acc[v][3] = 0.0;
        }
    }
    for (int k0 = 0; k0 < NB; k0 += KC) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int idx = t * 4 + p * (GT * 4), kk = idx / NB, r = idx % NB;
            const double4 a4 = *reinterpret_cast<const double4*>(A + k0 * NB + idx);
            *reinterpret_cast<double2*>(As + kk * LDS_LD + r) = make_double2(a4.x, a4.y);
            *reinterpret_cast<double2*>(As + kk * LDS_LD + r + 2) = make_double2(a4.z, a4.w);
            if (TRANSB) {
                const double4 b4 = *reinterpret_cast<const double4*>(B + k0 * NB + idx);
                *reinterpret_cast<double2*>(Bs + kk * LDS_LD + r) = make_double2(b4.x, b4.y);
                *reinterpret_cast<double2*>(Bs + kk * LDS_LD + r + 2) = make_double2(b4.z, b4.w);
            } else {
                const int q = t + p * GT, c = q >> 3, kq = q & 7;
                const double4 b4 = *reinterpret_cast<const double4*>(B + c * NB + k0 + kq * 4);
                Bs[(kq * 4 + 0) * LDS_LD + c] = b4.x;
                Bs[(kq * 4 + 1) * LDS_LD + c] = b4.y;
                Bs[(kq * 4 + 2) * LDS_LD + c] = b4.z;
                Bs[(kq * 4 + 3) * LDS_LD + c] = b4.w;
            }
        }
        __syncthreads();
#pragma unroll 8
        for (int kk = 0; kk < KC; ++kk) {
            const double2 a01 = *reinterpret_cast<const double2*>(As + kk * LDS_LD + tx * 4);
            const double2 a23 = *reinterpret_cast<const double2*>(As + kk * LDS_LD + tx * 4 + 2);
            const double2 b01 = *reinterpret_cast<const double2*>(Bs + kk * LDS_LD + ty * 4);
            const double2 b23 = *reinterpret_cast<const double2*>(Bs + kk * LDS_LD + ty * 4 + 2);
            const double a[4] = {a01.x, a01.y, a23.x, a23.y}, b[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
            for (int v = 0; v < 4; ++v)
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[v][u] = mac<SUB>(acc[v][u], a[u], b[v]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int v = 0; v < 4; ++v)
        *reinterpret_cast<double4*>(C + (ty * 4 + v) * NB + tx * 4) = make_double4(acc[v][0], acc[v][1], acc[v][2], acc[v][3]);
}

#define LHVI_GE_PANELS __shared__ __attribute__((aligned(16))) double sm[2 * KC * LDS_LD]

__global__ void __launch_bounds__(GT) ge_trsm_kernel(double* Lt, const double* Xt, int64_t k) {
    LHVI_GE_PANELS;
    const int64_t i = k + 1 + blockIdx.x;
    double* T = Lt + tile_off(i, k);
    tile_gemm<true, false>(sm, T, T, Xt + tile_off(k, k));
}

__global__ void __launch_bounds__(GT) ge_syrk_kernel(double* Lt, int64_t k) {
    LHVI_GE_PANELS;
    int64_t a, b;
    tile_of_index(blockIdx.x, a, b);
    const int64_t i = k + 1 + a, j = k + 1 + b;
    tile_gemm<true, true>(sm, Lt + tile_off(i, j), Lt + tile_off(i, k), Lt + tile_off(j, k));
}

__global__ void __launch_bounds__(GT) ge_xrow_kernel(double* Xt, int64_t k) {
    LHVI_GE_PANELS;
    double* T = Xt + tile_off(k, blockIdx.x);
    tile_gemm<false, false>(sm, T, Xt + tile_off(k, k), T);
}

__global__ void __launch_bounds__(GT) ge_xupd_kernel(const double* Lt, double* Xt, int64_t k) {
    LHVI_GE_PANELS;
    const int64_t i = k + 1 + blockIdx.x, j = blockIdx.y;
    tile_gemm<false, true>(sm, Xt + tile_off(i, j), Lt + tile_off(i, k), Xt + tile_off(k, j));
}

// diagonal tile of step k (one wavefront, a lane per row): factor, inverse, log-determinant share, first bad pivot
__global__ void __launch_bounds__(WAVE) ge_potrf_kernel(double* Lt, double* Xt, int64_t k, double* tlog, int* bad) {
    __shared__ double a[NB * LDT], xdiag[NB], ldiag[NB];
    double* Lg = Lt + tile_off(k, k);
    double* Xg = Xt + tile_off(k, k);
    const int l = threadIdx.x;
    for (int c = 0; c < NB; ++c) a[l * LDT + c] = Lg[c * NB + l];
    __syncthreads();
    DevCtx ctx{l, WAVE};
    const int rc = potrf_tile(a, ldiag, ctx);
    trinv_tile(a, xdiag, ctx);
    for (int c = 0; c < NB; ++c) {
        Lg[c * NB + l] = diag_L(a, l, c);
        Xg[c * NB + l] = diag_X(a, xdiag, l, c);
    }
    if (l == 0) {
        double s = 0.0;
        for (int c = 0; c < NB; ++c) s += log(ldiag[c]);
        tlog[k] = s;
        if (rc >= 0) atomicMin(bad, (int)(k * NB + rc));
    }
}

__global__ void ge_logdet_kernel(int64_t T, const double* __restrict__ tlog, double* logdet) {
    if (threadIdx.x || blockIdx.x) return;
    double s = 0.0;
    for (int64_t k = 0; k < T; ++k) s += tlog[k];
    *logdet = 2.0 * s;
}

// entries [0, n_ent): J; then N rows of b; then the identity on the padding
__global__ void __launch_bounds__(BLOCK) ge_assemble_kernel(int64_t N, int64_t Np, int64_t n_ent, const int32_t* __restrict__ ent_row,
                                                            const int32_t* __restrict__ ent_col, const int64_t* __restrict__ ent_ptr,
                                                            const int64_t* __restrict__ ent_mid, const double* __restrict__ vals,
                                                            const int64_t* __restrict__ b_ptr, const double* __restrict__ b_vals,
                                                            double* Jt, double* b) {
    int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (e < n_ent) {
        const int64_t r = ent_row[e], c = ent_col[e];
        if (r < 0 || r >= N || c < 0 || c > r) return;
        double s1 = 0.0, s2 = 0.0;
        for (int64_t p = ent_ptr[e]; p < ent_mid[e]; ++p) s1 += vals[p];
        for (int64_t p = ent_mid[e]; p < ent_ptr[e + 1]; ++p) s2 += vals[p];
        if (r == c) s2 = s1;
        Jt[elem_off(r, c)] = -(s1 + s2);
        return;
    }
    e -= n_ent;
    if (e < N) {
        double s = 0.0;
        for (int64_t p = b_ptr[e]; p < b_ptr[e + 1]; ++p) s += b_vals[p];
        b[e] = s;
        return;
    }
    if (e < Np) Jt[elem_off(e, e)] = 1.0;
}

__global__ void __launch_bounds__(BLOCK) ge_pack_kernel(int64_t N, const double* __restrict__ A, double* Jt) {
    int64_t i, j;
    tile_of_index(blockIdx.x, i, j);
    double* T = Jt + tile_off(i, j);
    for (int e = threadIdx.x; e < TILE; e += BLOCK) {
        const int64_t gi = i * NB + e % NB, gj = j * NB + e / NB;
        T[e] = gi < N && gj < N ? -(A[gi * N + gj] + A[gj * N + gi]) : (gi == gj ? 1.0 : 0.0);
    }
}

// tile (i, j): py = X_ij b_j (rows), pv = squared column norms
__global__ void __launch_bounds__(WAVE) ge_moments1_kernel(const double* __restrict__ Xt, const double* __restrict__ b, double* py,
                                                           double* pv) {
    int64_t i, j;
    tile_of_index(blockIdx.x, i, j);
    const double* X = Xt + (int64_t)blockIdx.x * TILE;
    py[(int64_t)blockIdx.x * NB + threadIdx.x] = tile_row_dot(X, threadIdx.x, b + j * NB);
    pv[(int64_t)blockIdx.x * NB + threadIdx.x] = tile_col_sq(X, threadIdx.x);
}

// tile (i, j): pm = X_ij^T y_i (columns)
__global__ void __launch_bounds__(WAVE) ge_moments2_kernel(const double* __restrict__ Xt, const double* __restrict__ y, double* pm) {
    int64_t i, j;
    tile_of_index(blockIdx.x, i, j);
    pm[(int64_t)blockIdx.x * NB + threadIdx.x] = tile_col_dot(Xt + (int64_t)blockIdx.x * TILE, threadIdx.x, y + i * NB);
}

// out[i NB + l] = sum_{j <= i} part[(i, j)][l], ascending j
__global__ void __launch_bounds__(WAVE) ge_reduce_rows_kernel(const double* __restrict__ part, double* out) {
    const int64_t i = blockIdx.x;
    double s = 0.0;
    for (int64_t j = 0; j <= i; ++j) s += part[tile_index(i, j) * NB + threadIdx.x];
    out[i * NB + threadIdx.x] = s;
}

// out[j NB + l] = sum_{i >= j} part[(i, j)][l], ascending i
__global__ void __launch_bounds__(WAVE) ge_reduce_cols_kernel(int64_t T, const double* __restrict__ part, double* out) {
    const int64_t j = blockIdx.x;
    double s = 0.0;
    for (int64_t i = j; i < T; ++i) s += part[tile_index(i, j) * NB + threadIdx.x];
    out[j * NB + threadIdx.x] = s;
}

// out[a][b] = sum_i X[i][cols[a]] X[i][cols[b]]: a lane takes the rows i = lane (mod 64) in ascending order, then a tree
__global__ void __launch_bounds__(WAVE) ge_cov_kernel(int64_t N, int64_t T, const double* __restrict__ Xt, int S,
                                                      const int32_t* __restrict__ cols, double* out) {
    __shared__ double sh[WAVE];
    const int64_t ca = cols[blockIdx.x], cb = cols[blockIdx.y];
    double s = 0.0;
    if (ca >= 0 && ca < N && cb >= 0 && cb < N) {
        const int64_t ta = ca / NB, tb = cb / NB;
        for (int64_t ti = ta > tb ? ta : tb; ti < T; ++ti)
            s = fma(Xt[tile_off(ti, ta) + (ca % NB) * NB + threadIdx.x], Xt[tile_off(ti, tb) + (cb % NB) * NB + threadIdx.x], s);
    }
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = WAVE / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[(int64_t)blockIdx.x * S + blockIdx.y] = sh[0];
}

constexpr int64_t MAX_TILES = 46340;     // T (T + 1) / 2 workgroups fit a 31-bit grid

static int size_check(int64_t N) {
    if (N < 0) return LHVI_E_ARG;
    if (tiles_of(N) > MAX_TILES) return LHVI_E_UNSUPPORTED;
    return LHVI_OK;
}

}  // namespace gauss
}  // namespace lhvi

using namespace lhvi;
using namespace lhvi::gauss;

extern "C" {

size_t lhvi_gauss_exact_tri_doubles(int64_t N) {
    if (N < 0) return 0;
    return (size_t)(tri_tiles(tiles_of(N)) * TILE);
}

size_t lhvi_gauss_exact_ws_doubles(int64_t N) {
    if (N < 0) return 0;
    const int64_t T = tiles_of(N);
    return (size_t)(3 * tri_tiles(T) * NB + T * NB);
}

int lhvi_gauss_exact_assemble(int64_t N, int64_t n_ent, const int32_t* ent_row, const int32_t* ent_col, const int64_t* ent_ptr,
                              const int64_t* ent_mid, const double* vals, const int64_t* b_ptr, const double* b_vals, double* Jt,
                              double* b, void* stream) {
    const int rc = size_check(N);
    if (rc) return rc;
    if (n_ent < 0 || !Jt || !b || !b_ptr || (n_ent && (!ent_row || !ent_col || !ent_ptr || !ent_mid))) return LHVI_E_ARG;
    if (N == 0) return LHVI_OK;
    const int64_t Np = tiles_of(N) * NB, work = n_ent + Np;
    if ((work + BLOCK - 1) / BLOCK > 0x7fffffff) return LHVI_E_UNSUPPORTED;
    hipLaunchKernelGGL(ge_assemble_kernel, dim3(grid_for(work)), dim3(BLOCK), 0, as_stream(stream), N, Np, n_ent, ent_row, ent_col,
                       ent_ptr, ent_mid, vals, b_ptr, b_vals, Jt, b);
    return check_launch();
}

int lhvi_gauss_exact_pack(int64_t N, const double* A, double* Jt, void* stream) {
    const int rc = size_check(N);
    if (rc) return rc;
    if (N == 0) return LHVI_OK;
    if (!A || !Jt) return LHVI_E_ARG;
    hipLaunchKernelGGL(ge_pack_kernel, dim3((unsigned)tri_tiles(tiles_of(N))), dim3(BLOCK), 0, as_stream(stream), N, A, Jt);
    return check_launch();
}

int lhvi_gauss_exact_factor(int64_t N, double* Lt, double* Xt, double* tlog, int32_t* bad, double* logdet, void* stream) {
    const int rc = size_check(N);
    if (rc) return rc;
    if (N == 0) return LHVI_OK;
    if (!Lt || !Xt || !tlog || !bad || !logdet) return LHVI_E_ARG;
    hipStream_t st = as_stream(stream);
    const int64_t T = tiles_of(N);
    for (int64_t k = 0; k < T; ++k) {
        hipLaunchKernelGGL(ge_potrf_kernel, dim3(1), dim3(WAVE), 0, st, Lt, Xt, k, tlog, bad);
        const int64_t m = T - k - 1;
        if (m > 0) {
            hipLaunchKernelGGL(ge_trsm_kernel, dim3((unsigned)m), dim3(GT), 0, st, Lt, (const double*)Xt, k);
            hipLaunchKernelGGL(ge_syrk_kernel, dim3((unsigned)tri_tiles(m)), dim3(GT), 0, st, Lt, k);
        }
    }
    hipLaunchKernelGGL(ge_logdet_kernel, dim3(1), dim3(WAVE), 0, st, T, (const double*)tlog, logdet);
    return check_launch();
}

int lhvi_gauss_exact_inverse(int64_t N, const double* Lt, double* Xt, void* stream) {
    const int rc = size_check(N);
    if (rc) return rc;
    if (N == 0) return LHVI_OK;
    if (!Lt || !Xt) return LHVI_E_ARG;
    hipStream_t st = as_stream(stream);
    const int64_t T = tiles_of(N);
    for (int64_t k = 0; k < T; ++k) {
        if (k > 0) hipLaunchKernelGGL(ge_xrow_kernel, dim3((unsigned)k), dim3(GT), 0, st, Xt, k);
        const int64_t m = T - k - 1;
        if (m > 0)     // (k + 1 <= MAX_TILES < 65536: the grid's second dimension fits)
            hipLaunchKernelGGL(ge_xupd_kernel, dim3((unsigned)m, (unsigned)(k + 1)), dim3(GT), 0, st, Lt, Xt, k);
    }
    return check_launch();
}

int lhvi_gauss_exact_moments(int64_t N, const double* Xt, const double* b, double* ws, double* mu, double* var, void* stream) {
    const int rc = size_check(N);
    if (rc) return rc;
    if (N == 0) return LHVI_OK;
    if (!Xt || !b || !ws || !mu || !var) return LHVI_E_ARG;
    hipStream_t st = as_stream(stream);
    const int64_t T = tiles_of(N), nt = tri_tiles(T);
    double *py = ws, *pv = py + nt * NB, *pm = pv + nt * NB, *y = pm + nt * NB;
    hipLaunchKernelGGL(ge_moments1_kernel, dim3((unsigned)nt), dim3(WAVE), 0, st, Xt, b, py, pv);
    hipLaunchKernelGGL(ge_reduce_rows_kernel, dim3((unsigned)T), dim3(WAVE), 0, st, (const double*)py, y);
    hipLaunchKernelGGL(ge_reduce_cols_kernel, dim3((unsigned)T), dim3(WAVE), 0, st, T, (const double*)pv, var);
    hipLaunchKernelGGL(ge_moments2_kernel, dim3((unsigned)nt), dim3(WAVE), 0, st, Xt, (const double*)y, pm);
    hipLaunchKernelGGL(ge_reduce_cols_kernel, dim3((unsigned)T), dim3(WAVE), 0, st, T, (const double*)pm, mu);
    return check_launch();
}

int lhvi_gauss_exact_cov(int64_t N, const double* Xt, int32_t S, const int32_t* cols, double* out, void* stream) {
    const int rc = size_check(N);
    if (rc) return rc;
    if (S < 0 || S > 65535) return LHVI_E_ARG;
    if (S == 0) return LHVI_OK;
    if (N == 0 || !Xt || !cols || !out) return LHVI_E_ARG;
    hipLaunchKernelGGL(ge_cov_kernel, dim3(S, S), dim3(WAVE), 0, as_stream(stream), N, tiles_of(N), Xt, (int)S, cols, out);
    return check_launch();
}

int lhvi_gauss_exact_host(int64_t N, const double* J, const double* b, double* mu, double* var, double* logdet, int64_t* bad_col) {
    const int rc = size_check(N);
    if (rc) return rc;
    if (bad_col) *bad_col = -1;
    if (N == 0) {
        if (logdet) *logdet = 0.0;
        return LHVI_OK;
    }
    if (!J || !b || !mu || !var || !logdet) return LHVI_E_ARG;
    const int64_t T = tiles_of(N), nt = tri_tiles(T), Np = T * NB;
    double* Lt = new double[2 * nt * TILE + 3 * nt * NB + 3 * Np + T];
    double *Xt = Lt + nt * TILE, *py = Xt + nt * TILE, *pv = py + nt * NB, *pm = pv + nt * NB, *bp = pm + nt * NB, *y = bp + Np,
           *out = y + Np, *tlog = out + Np;
    for (int64_t i = 0; i < T; ++i)
        for (int64_t j = 0; j <= i; ++j) {
            double *Lg = Lt + tile_off(i, j), *Xg = Xt + tile_off(i, j);
            for (int e = 0; e < TILE; ++e) {
                const int64_t gi = i * NB + e % NB, gj = j * NB + e / NB;
                Lg[e] = gi < N && gj < N ? J[gi * N + gj] : (gi == gj ? 1.0 : 0.0);
                Xg[e] = 0.0;
            }
        }
    for (int64_t p = 0; p < Np; ++p) bp[p] = p < N ? b[p] : 0.0;
    int64_t bad = -1;
    double a[NB * LDT], xdiag[NB], ldiag[NB];
    for (int64_t k = 0; k < T; ++k) {
        double *Lg = Lt + tile_off(k, k), *Xg = Xt + tile_off(k, k);
        for (int r = 0; r < NB; ++r)
            for (int c = 0; c < NB; ++c) a[r * LDT + c] = Lg[c * NB + r];
        const int col = potrf_tile(a, ldiag, HostCtx());
        trinv_tile(a, xdiag, HostCtx());
        for (int r = 0; r < NB; ++r)
            for (int c = 0; c < NB; ++c) {
                Lg[c * NB + r] = diag_L(a, r, c);
                Xg[c * NB + r] = diag_X(a, xdiag, r, c);
            }
        double s = 0.0;
        for (int c = 0; c < NB; ++c) s += log(ldiag[c]);
        tlog[k] = s;
        if (col >= 0 && bad < 0) bad = k * NB + col;
        for (int64_t i = k + 1; i < T; ++i) tile_gemm_host<true, false>(Lt + tile_off(i, k), Lt + tile_off(i, k), Xg);
        for (int64_t i = k + 1; i < T; ++i)
            for (int64_t j = k + 1; j <= i; ++j)
                tile_gemm_host<true, true>(Lt + tile_off(i, j), Lt + tile_off(i, k), Lt + tile_off(j, k));
    }
    for (int64_t k = 0; k < T; ++k) {
        for (int64_t j = 0; j < k; ++j) tile_gemm_host<false, false>(Xt + tile_off(k, j), Xt + tile_off(k, k), Xt + tile_off(k, j));
        for (int64_t i = k + 1; i < T; ++i)
            for (int64_t j = 0; j <= k; ++j)
                tile_gemm_host<false, true>(Xt + tile_off(i, j), Lt + tile_off(i, k), Xt + tile_off(k, j));
    }
    for (int64_t i = 0; i < T; ++i)
        for (int64_t j = 0; j <= i; ++j)
            for (int l = 0; l < NB; ++l) {
                const int64_t t = tile_index(i, j);
                py[t * NB + l] = tile_row_dot(Xt + t * TILE, l, bp + j * NB);
                pv[t * NB + l] = tile_col_sq(Xt + t * TILE, l);
            }
    for (int64_t i = 0; i < T; ++i)
        for (int l = 0; l < NB; ++l) {
            double s = 0.0;
            for (int64_t j = 0; j <= i; ++j) s += py[tile_index(i, j) * NB + l];
            y[i * NB + l] = s;
        }
    for (int64_t i = 0; i < T; ++i)
        for (int64_t j = 0; j <= i; ++j)
            for (int l = 0; l < NB; ++l) pm[tile_index(i, j) * NB + l] = tile_col_dot(Xt + tile_off(i, j), l, y + i * NB);
    for (int pass = 0; pass < 2; ++pass) {
        const double* part = pass ? pm : pv;
        for (int64_t j = 0; j < T; ++j)
            for (int l = 0; l < NB; ++l) {
                double s = 0.0;
                for (int64_t i = j; i < T; ++i) s += part[tile_index(i, j) * NB + l];
                out[j * NB + l] = s;
            }
        for (int64_t p = 0; p < N; ++p) (pass ? mu : var)[p] = out[p];
    }
    double s = 0.0;
    for (int64_t k = 0; k < T; ++k) s += tlog[k];
    *logdet = 2.0 * s;
    delete[] Lt;
    if (bad_col) *bad_col = bad;
    return bad >= 0 ? LHVI_E_NOT_PD : LHVI_OK;
}

}  // extern "C"
