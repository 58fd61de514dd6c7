// gmkl_host_sanitize.hip -- the host twin of csrc/gmkl.hip (lhvi_gm_kl_host) in a stand-alone program, to be built with the
// host-side sanitizers and run on the CPU: scripts/gmkl_host_sanitize.sh.  It touches no device.  The shapes are the edges of
// the entry point: one component, zero-weight padding, component counts around the device's chunk, a clipped and an empty
// range, the panel cap (the whole panel list), a narrow component of q (the stack), zero tolerances (the work limit), an
// invalid row, NULL optional outputs.
#include <cmath>
#include <cstdio>
#include <vector>
#include "../lifted-hybrid-variational-inference_amd/csrc/gmkl.hip"

namespace lhvi {
thread_local int g_last_hip_error = 0;
}

static double lcg(unsigned long long& s) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(s >> 11) / 9007199254740992.0;
}

int main() {
    int failures = 0;
    double checksum = 0.0;
    const double inf = __builtin_huge_val();
    for (int Kp : {1, 5, 64, 130})
        for (int Kq : {1, 3, 65}) {
            const int R = 6;
            unsigned long long s = 99 + 1000 * Kp + Kq;
            std::vector<double> wp(R * Kp), mp(R * Kp), vp(R * Kp), wq(R * Kq), mq(R * Kq), vq(R * Kq), a(R, -inf), b(R, inf), kl(R),
                err(R);
            std::vector<int32_t> st(R), ne(R);
            auto fill = [&](std::vector<double>& w, std::vector<double>& m, std::vector<double>& v, int K) {
                for (int r = 0; r < R; ++r) {
                    double tot = 0.0;
                    for (int k = 0; k < K; ++k) {
                        w[r * K + k] = k % 3 == 2 ? 0.0 : 0.1 + lcg(s);         // every third component is padding
                        tot += w[r * K + k];
                        m[r * K + k] = 16 * lcg(s) - 8;
                        v[r * K + k] = std::exp(std::log(1e-3) + lcg(s) * std::log(1e3));
                    }
                    for (int k = 0; k < K; ++k) w[r * K + k] /= tot;
                }
            };
            fill(wp, mp, vp, Kp);
            fill(wq, mq, vq, Kq);
            a[1] = -2.0, b[1] = 3.0;                // clipped
            a[2] = 50.0, b[2] = 60.0;               // empty
            vp[3 * Kp] = 1e-12;                     // the panel cap
            vq[4 * Kq] = 1e-8, mq[4 * Kq] = mp[4 * Kp];             // a spike of q on a mean of p
            vq[5 * Kq + (Kq > 1 ? 1 : 0)] = -1.0;   // invalid
            for (double eps : {1.49e-8, 0.0}) {
                int rc = lhvi_gm_kl_host(R, Kp, wp.data(), mp.data(), vp.data(), Kq, wq.data(), mq.data(), vq.data(), a.data(), b.data(),
                                         eps, eps, kl.data(), err.data(), st.data(), ne.data());
                failures += rc != LHVI_OK;
                failures += !(kl[2] == 0.0 && ne[2] == 0) + (Kp > 1 && !(st[3] & 2)) + !(st[5] == 4 && kl[5] != kl[5]);      // (Kp = 1: 20 sd, three panels)
                if (eps == 0.0) failures += !(st[0] & 1) + !(ne[0] <= 21 * 1024 + 42 * 4096);
                for (int r = 0; r < 5; ++r) checksum += std::isfinite(kl[r]) ? kl[r] : 0.0;
                rc = lhvi_gm_kl_host(R, Kp, wp.data(), mp.data(), vp.data(), Kq, wq.data(), mq.data(), vq.data(), a.data(), b.data(), eps,
                                     eps, kl.data(), nullptr, nullptr, nullptr);
                failures += rc != LHVI_OK;
            }
            failures += lhvi_gm_kl_host(0, Kp, wp.data(), mp.data(), vp.data(), Kq, wq.data(), mq.data(), vq.data(), a.data(), b.data(),
                                        1e-8, 1e-8, kl.data(), nullptr, nullptr, nullptr) != LHVI_E_ARG;
        }
    std::printf("gmkl host twin under the sanitizers: checksum %.17g, %d failures\n", checksum, failures);
    return failures != 0;
}
