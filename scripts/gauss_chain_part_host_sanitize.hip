// gauss_chain_part_host_sanitize.hip -- lhvi_gauss_chain_part_host (the partitioned chain solve's device code with one lane) on
// diagonally dominant random systems at every padded edge, with and without the covariances, every array a heap block of
// exactly its documented size: scripts/gauss_chain_part_host_sanitize.sh runs it under AddressSanitizer and UBSan on the host.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "../include/lhvi.h"

static double rnd() { return (double)rand() / RAND_MAX - 0.5; }

int main() {
    const int cases[][4] = {{1, 3, 1, 2}, {2, 9, 1, 5}, {3, 4, 3, 2}, {2, 11, 3, 6}, {1, 23, 5, 7}, {2, 9, 17, 3}, {2, 7, 33, 3},
                            {1, 5, 65, 2}, {2, 5, 65, 3}, {1, 300, 4, 64}, {1, 6, 128, 3}, {1, 40, 30, 8}};
    for (auto& c : cases) {
        const int64_t B = c[0], M = c[1], n = c[2], S = c[3], nn = n * n;
        for (int keep = 0; keep < 2; ++keep) {
            double* D = (double*)malloc(B * M * nn * 8);
            double* O = (double*)malloc(B * (M - 1) * nn * 8);
            double* h = (double*)malloc(B * M * n * 8);
            for (int64_t i = 0; i < B * M * nn; ++i) D[i] = 0.0;
            for (int64_t b = 0; b < B * M; ++b)
                for (int i = 0; i < n; ++i)
                    for (int j = 0; j <= i; ++j) D[b * nn + i * n + j] = D[b * nn + j * n + i] = i == j ? 3.0 + rnd() : 0.3 * rnd() / n;
            for (int64_t i = 0; i < B * (M - 1) * nn; ++i) O[i] = rnd() / n;
            for (int64_t i = 0; i < B * M * n; ++i) h[i] = rnd();
            size_t wsn = lhvi_gauss_chain_part_ws_doubles(B, M, n, S);
            double* ws = (double*)malloc(wsn * 8);
            double *mu = (double*)malloc(B * M * n * 8), *var = (double*)malloc(B * M * n * 8), *logdet = (double*)malloc(B * 8);
            double* cov = keep ? (double*)malloc(B * M * nn * 8) : nullptr;
            double* cross = keep ? (double*)malloc(B * (M - 1) * nn * 8) : nullptr;
            int32_t* bad = (int32_t*)malloc(B * 8);
            int rc = lhvi_gauss_chain_part_host(B, M, n, S, D, O, h, ws, mu, var, cov, cross, logdet, bad);
            printf("B %ld M %ld n %ld S %ld keep %d rc %d bad %d logdet %g mu0 %g\n", (long)B, (long)M, (long)n, (long)S, keep, rc, bad[0], logdet[0], mu[0]);
            free(D), free(O), free(h), free(ws), free(mu), free(var), free(logdet), free(cov), free(cross), free(bad);
        }
    }
    return 0;
}
