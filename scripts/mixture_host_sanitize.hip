// mixture_host_sanitize.hip -- the host twins of csrc/mixture.hip (lhvi_mix_*_host) in a stand-alone program, to be built with
// the host-side sanitizers and run on the CPU: scripts/mixture_host_sanitize.sh.  It touches no device.  The shapes are the
// edges of the entry points: no observation, one tile plus one, NaN holes, a row group that ends early, repeated rows, a
// discrete value that is no state, rows outside the belief and rows without parameters, bounds that clip every start, and the
// joint MAP with and without discrete / continuous rows.
#include <cmath>
#include <cstdio>
#include <vector>
#include "../lifted-hybrid-variational-inference_amd/csrc/mixture.hip"

namespace lhvi {
thread_local int g_last_hip_error = 0;
}

static double lcg(unsigned long long& s) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(s >> 11) / 9007199254740992.0;
}

int main() {
    const int Nc = 5, Nd = 4, V = Nc + Nd + 1, Dmax = 5;
    int failures = 0;
    double checksum = 0.0;
    for (int K : {1, 3, 33, 128}) {
        unsigned long long s = 12345 + K;
        std::vector<double> w(K), eta_c((size_t)V * K * 2), eta_d((size_t)V * K * Dmax, 0.0), logw(K), rec((size_t)V * K * 3),
            lpi((size_t)V * K * Dmax);
        std::vector<int32_t> nstates(V);
        double tot = 0.0;
        for (int k = 0; k < K; ++k) tot += w[k] = 0.1 + lcg(s);
        for (int k = 0; k < K; ++k) w[k] /= tot;
        for (int v = 0; v < V; ++v) {
            nstates[v] = v < Nc ? 0 : v < Nc + Nd ? 2 + (v - Nc) : -1;      // 2, 3, 4, 5 states; the last row has no parameters
            for (int k = 0; k < K; ++k) {
                eta_c[((size_t)v * K + k) * 2] = 6 * lcg(s) - 3;
                eta_c[((size_t)v * K + k) * 2 + 1] = 0.1 + 3 * lcg(s);
                double t = 0.0;
                for (int d = 0; d < nstates[v]; ++d) t += eta_d[((size_t)v * K + k) * Dmax + d] = 0.05 + lcg(s);
                for (int d = 0; d < nstates[v]; ++d) eta_d[((size_t)v * K + k) * Dmax + d] /= t;
            }
        }
        for (int norm : {LHVI_MIX_GAUSSIAN, LHVI_MIX_VI}) {
            if (lhvi_mix_prepare_host(V, K, Dmax, norm, w.data(), eta_c.data(), eta_d.data(), nstates.data(), logw.data(),
                                      rec.data(), lpi.data()))
                ++failures;
            lhvi_mix_t b{V, K, Dmax, nstates.data(), logw.data(), rec.data(), lpi.data(), eta_d.data()};
            for (int n_obs : {0, 1, 64, 65, 129})
                for (int M : {1, 4, 5}) {
                    std::vector<int32_t> obs(n_obs);
                    std::vector<double> X((size_t)M * n_obs);
                    for (int o = 0; o < n_obs; ++o) {
                        obs[o] = (int)(lcg(s) * (V + 2)) - 1;                  // -1 and V: outside the belief; V - 1: no parameters
                        for (int m = 0; m < M; ++m) {
                            const int ns = obs[o] >= 0 && obs[o] < V ? nstates[obs[o]] : 0;
                            double x = ns > 0 ? (double)(int)(lcg(s) * (ns + 1)) : 6 * lcg(s) - 3;   // ns itself: no state
                            if (lcg(s) < 0.25) x = __builtin_nan("");
                            X[(size_t)m * n_obs + o] = x;
                        }
                    }
                    std::vector<double> ws(lhvi_mix_condition_ws_doubles(M, n_obs, K) + 1), comp((size_t)M * K), logp(M),
                        condw((size_t)M * K);
                    if (lhvi_mix_condition_host(&b, M, n_obs, obs.data(), X.data(), ws.data(), comp.data(), logp.data(),
                                                condw.data()))
                        ++failures;
                    const int n_q = V + 3;
                    std::vector<int32_t> query(n_q), qptr(n_q + 1, 0), qidx;
                    std::vector<double> lo(n_q), hi(n_q), xo((size_t)M * n_q), fo((size_t)M * n_q);
                    for (int q = 0; q < n_q; ++q) {
                        query[q] = q < V ? q : q == V ? -1 : q == V + 1 ? V : 2;
                        lo[q] = q % 3 == 0 ? 0.5 : -10;
                        hi[q] = q % 3 == 0 ? 0.75 : 10;
                        for (int o = 0; o < n_obs; ++o)
                            if (obs[o] == query[q]) qidx.push_back(o);
                        qptr[q + 1] = (int32_t)qidx.size();
                    }
                    qidx.push_back(0);
                    if (lhvi_mix_marginal_map_host(&b, M, condw.data(), n_q, query.data(), lo.data(), hi.data(), n_obs, X.data(),
                                                   qptr.data(), qidx.data(), 100, xo.data(), fo.data()))
                        ++failures;
                    const int P = 3;
                    std::vector<double> x((size_t)n_q * P), out((size_t)M * n_q * P);
                    for (auto& v : x) v = (double)(int)(lcg(s) * 7) - 1;
                    if (lhvi_mix_log_belief_host(&b, M, condw.data(), n_q, query.data(), P, x.data(), out.data())) ++failures;
                    if (n_obs == 65) {                                  // the joint MAP of every row with parameters, from every component
                        std::vector<int32_t> crows, drows;
                        for (int v = 0; v < V; ++v)
                            if (nstates[v] == 0 && (M > 1 || v != 2)) crows.push_back(v);
                            else if (nstates[v] > 0 && M != 4) drows.push_back(v);
                        const int jc = (int)crows.size(), jd = (int)drows.size();
                        std::vector<double> x0((size_t)K * jc + 1), jlo(jc + 1, -3.0), jhi(jc + 1, 3.0), jxc((size_t)K * jc + 1), jobj(K),
                            jws(lhvi_mix_joint_map_ws_doubles(K, jc, jd, Dmax, K) + 1);
                        std::vector<int32_t> xd0((size_t)K * jd + 1, 0), jxd((size_t)K * jd + 1);
                        for (int k = 0; k < K; ++k)
                            for (int n = 0; n < jc; ++n) x0[(size_t)k * jc + n] = eta_c[((size_t)crows[n] * K + k) * 2];
                        if (lhvi_mix_joint_map_host(&b, logw.data(), jc, crows.data(), jlo.data(), jhi.data(), jd, drows.data(), K, x0.data(),
                                                    xd0.data(), 3, 0.05, 0.01, 40, 1e-7, jws.data(), jxc.data(), jxd.data(), jobj.data()))
                            ++failures;
                        for (double v : jobj)
                            if (std::isfinite(v)) checksum += v;
                    }
                    for (const auto* a : {&logp, &xo, &out})
                        for (double v : *a)
                            if (std::isfinite(v)) checksum += v;
                }
        }
    }
    lhvi_mix_t big{0, 129, 1, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (lhvi_mix_condition_host(&big, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != LHVI_E_UNSUPPORTED) ++failures;
    std::printf("mixture host twins: %d failures, checksum %.17g\n", failures, checksum);
    return failures != 0;
}
