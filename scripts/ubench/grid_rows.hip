// micro-benchmark (tuning aid, not part of the product): the integral-point block of a heavy f2v edge on a uniform grid,
//   S_t = sum_j G0_j q_j^t,  G0_j = exp(a_j + b_j x_0), q_j = exp(b_j h),  t < 32, j < 64,
// with the kernel's surroundings (two exp_core per lane, log_table, the store of one point per lane pair), formed
// (A) as grid_sums32 of csrc/pbp.hip does: lane = partner j walks all 32 points, six folds over lane bits 5 ... 0;
// (B) in quarter-wave lane groups (grid_sums32_rows): lane 16 k + c walks points 8 k ... 8 k + 7 for partners c, c + 16, c + 32,
//     c + 48 after a 4 x 4 transpose of the values at points 0, 8, 16, 24 and an all-gather of the ratios; four folds over
//     lane bits 3 ... 0.
// Prints the time per launch, nanoseconds and (at the clock given on the command line, default 2.0 GHz) cycles per edge and
// SIMD for both, and the largest relative difference of the two forms' sums (each form stores into the slot of the point it owns,
// so the comparison also checks the owned-point maps).
// build: hipcc -O3 --offload-arch=gfx950 -I../../lifted-hybrid-variational-inference_amd/csrc -I../../include grid_rows.hip -o grid_rows
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <vector>
#include "fastmath.hpp"

using namespace lhvi;

struct Rec { double a, b; };

template <int CTRL, int BANK>
__device__ __forceinline__ double dpp_into(double old, double src) {      // lanes of the enabled banks take src[permuted], the rest keep old
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(src), CTRL, 0xf, BANK, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(src), CTRL, 0xf, BANK, false);
    return __hiloint2double(hi, lo);
}
template <int CTRL>
__device__ __forceinline__ double dpp_mov(double v) {
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ void swap32(double& x, double& y) {           // bit 5 clear: (own x, partner's x); set: (partner's y, own y)
    auto lo = __builtin_amdgcn_permlane32_swap(__double2loint(x), __double2loint(y), false, false);
    auto hi = __builtin_amdgcn_permlane32_swap(__double2hiint(x), __double2hiint(y), false, false);
    x = __hiloint2double(hi[0], lo[0]); y = __hiloint2double(hi[1], lo[1]);
}
__device__ __forceinline__ void swap16(double& x, double& y) {
    auto lo = __builtin_amdgcn_permlane16_swap(__double2loint(x), __double2loint(y), false, false);
    auto hi = __builtin_amdgcn_permlane16_swap(__double2hiint(x), __double2hiint(y), false, false);
    x = __hiloint2double(hi[0], lo[0]); y = __hiloint2double(hi[1], lo[1]);
}
// x kept by the lanes whose bit is 0, y by the others; returns own-kept + partner's copy of the same value
__device__ __forceinline__ double fold32(double x, double y) { swap32(x, y); return x + y; }
__device__ __forceinline__ double fold16(double x, double y) { swap16(x, y); return x + y; }
__device__ __forceinline__ double fold8(double x, double y) { return dpp_into<0x128, 0x3>(y, x) + dpp_into<0x128, 0xc>(x, y); }
__device__ __forceinline__ double fold4(double x, double y) { return dpp_into<0x104, 0x5>(y, x) + dpp_into<0x114, 0xa>(x, y); }
__device__ __forceinline__ double fold2(double x, double y, bool bit1) {
    const double send = bit1 ? x : y, keep = bit1 ? y : x;
    return keep + dpp_mov<0x4e>(send);
}
__device__ __forceinline__ double fold1(double x) { return x + dpp_mov<0xb1>(x); }

__device__ __forceinline__ int owned_seq(int lane) {
    return 8 * (2 * ((lane >> 1) & 1) + ((lane >> 2) & 1)) + 4 * ((lane >> 3) & 1) + 2 * ((lane >> 4) & 1) + ((lane >> 5) & 1);
}
__device__ __forceinline__ int owned_rows(int lane) {
    return 8 * (lane >> 4) + ((lane >> 3) & 1) + 2 * ((lane >> 2) & 1) + 4 * ((lane >> 1) & 1);
}

__device__ __forceinline__ double sums_seq(double g, double q, int lane) {
    double z[4];
#pragma unroll
    for (int bt = 0; bt < 4; ++bt) {
        double v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) { v[i] = g; g *= q; }
        const double u0 = fold16(fold32(v[0], v[1]), fold32(v[2], v[3]));
        const double u1 = fold16(fold32(v[4], v[5]), fold32(v[6], v[7]));
        z[bt] = fold8(u0, u1);
    }
    return fold1(fold2(fold4(z[0], z[1]), fold4(z[2], z[3]), (lane >> 1) & 1));
}
__device__ __forceinline__ double sums_rows(double g, double q, int lane) {
    double qr[4];
    {
        double lo = q, hi = q;
        swap32(lo, hi);
        qr[0] = lo; qr[1] = lo; swap16(qr[0], qr[1]);
        qr[2] = hi; qr[3] = hi; swap16(qr[2], qr[3]);
    }
    const double q2 = q * q, q4 = q2 * q2;
    double s[4];
    s[0] = g;
#pragma unroll
    for (int m = 1; m < 4; ++m) s[m] = (s[m - 1] * q4) * q4;
    swap32(s[0], s[2]); swap32(s[1], s[3]);
    swap16(s[0], s[1]); swap16(s[2], s[3]);
    double w[2];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        double u[2];
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
            const double v0 = (s[0] + s[1]) + (s[2] + s[3]);
#pragma unroll
            for (int m = 0; m < 4; ++m) s[m] *= qr[m];
            const double v1 = (s[0] + s[1]) + (s[2] + s[3]);
            if (half + pr < 2) {
#pragma unroll
                for (int m = 0; m < 4; ++m) s[m] *= qr[m];
            }
            u[pr] = fold8(v0, v1);
        }
        w[half] = fold4(u[0], u[1]);
    }
    return fold1(fold2(w[0], w[1], (lane >> 1) & 1));
}

// MODE 0: (A), 1: (B), 2: the surroundings alone (exponentials, log_table of the start value, store)
template <int MODE>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(7, 7))) grid_kernel(const Rec* __restrict__ recs, int nrec,
                                                                                            double* __restrict__ out, int edges, double x0, double h) {
    __shared__ double sh_tab[EXP_TAB_N];
    __shared__ LogRec sh_log[LOG_TAB_N];
    load_log_table(sh_log);
    load_exp_table(sh_tab);
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wave = blockIdx.x * 4 + wid;
    double check = 0.0;
    for (int e = 0; e < edges; ++e) {
        const Rec r = recs[(size_t)((wave * 17 + e) % nrec) * 64 + lane];
        const double g = exp_core(fma(r.b, x0, r.a), sh_tab);
        const double q = exp_core(r.b * h, sh_tab);
        const double res = MODE == 0 ? sums_seq(g, q, lane) : MODE == 1 ? sums_rows(g, q, lane) : g + q;
        const int t = MODE == 0 ? owned_seq(lane) : owned_rows(lane);
        const double lg = log_table(res, sh_log);
        if (!(lane & 1)) out[(size_t)wave * 32 + t] = lg + check;
        check += 1e-30 * lg;
    }
}

int main(int argc, char** argv) {
    const double clk = argc > 1 ? atof(argv[1]) * 1e9 : 2.0e9;
    const int nrec = 4096, edges = 400, reps = 5;
    std::vector<Rec> h_recs((size_t)nrec * 64);
    unsigned s = 12345;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (s >> 8) * (1.0 / 16777216.0); };
    for (auto& r : h_recs) { r.a = -60.0 + 120.0 * rnd(); r.b = -5.0 + 10.0 * rnd(); }
    Rec* d_recs; double* d_out[3];
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, 0) != hipSuccess) { fprintf(stderr, "no device\n"); return 1; }
    const int blocks = prop.multiProcessorCount * 7, waves = blocks * 4;
    hipMalloc(&d_recs, h_recs.size() * sizeof(Rec));
    hipMemcpy(d_recs, h_recs.data(), h_recs.size() * sizeof(Rec), hipMemcpyHostToDevice);
    for (int m = 0; m < 3; ++m) { hipMalloc(&d_out[m], (size_t)waves * 32 * sizeof(double)); hipMemset(d_out[m], 0, (size_t)waves * 32 * sizeof(double)); }
    const double x0 = -10.0, hh = 20.0 / 31.0;
    float best[3] = {1e30f, 1e30f, 1e30f};
    hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
    for (int rep = 0; rep < reps; ++rep) {              // the forms alternate; the first pass warms up
        for (int m = 0; m < 3; ++m) {
            hipEventRecord(a);
            if (m == 0) hipLaunchKernelGGL(grid_kernel<0>, dim3(blocks), dim3(256), 0, 0, d_recs, nrec, d_out[0], edges, x0, hh);
            else if (m == 1) hipLaunchKernelGGL(grid_kernel<1>, dim3(blocks), dim3(256), 0, 0, d_recs, nrec, d_out[1], edges, x0, hh);
            else hipLaunchKernelGGL(grid_kernel<2>, dim3(blocks), dim3(256), 0, 0, d_recs, nrec, d_out[2], edges, x0, hh);
            hipEventRecord(b);
            if (hipEventSynchronize(b) != hipSuccess) { fprintf(stderr, "kernel failed: %s\n", hipGetErrorString(hipGetLastError())); return 1; }
            float ms; hipEventElapsedTime(&ms, a, b);
            if (rep > 0) { best[m] = fminf(best[m], ms); printf("rep %d form %d: %.4f ms\n", rep, m, ms); }
        }
    }
    std::vector<double> o0((size_t)waves * 32), o1(o0.size());
    hipMemcpy(o0.data(), d_out[0], o0.size() * 8, hipMemcpyDeviceToHost);
    hipMemcpy(o1.data(), d_out[1], o1.size() * 8, hipMemcpyDeviceToHost);
    double maxd = 0.0; size_t bad = 0;
    for (size_t i = 0; i < o0.size(); ++i) {
        if (!std::isfinite(o0[i]) || !std::isfinite(o1[i]) || o1[i] == 0.0) ++bad;
        maxd = fmax(maxd, fabs(o0[i] - o1[i]));
    }
    const char* name[3] = {"sequential (grid_sums32)   ", "rows (grid_sums32_rows)    ", "surroundings alone         "};
    // 7 waves per SIMD run the loop side by side: time / edges / 7 is the issue time one edge takes of its SIMD
    for (int m = 0; m < 3; ++m)
        printf("%s: best %.4f ms, %.1f ns = %.0f cycles at %.2f GHz per edge and SIMD\n", name[m], best[m], best[m] * 1e6 / edges / 7.0,
               best[m] * 1e-3 * clk / edges / 7.0, clk * 1e-9);
    printf("block alone: sequential %.0f cycles, rows %.0f cycles per edge and SIMD\n", (best[0] - best[2]) * 1e-3 * clk / edges / 7.0,
           (best[1] - best[2]) * 1e-3 * clk / edges / 7.0);
    printf("max |log S_sequential - log S_rows| = %.3e over %zu sums (%zu not finite or unwritten)\n", maxd, o0.size(), bad);
    return bad ? 2 : 0;
}
