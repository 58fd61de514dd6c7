// ais_host_sanitize.hip -- the host twin of csrc/ais.hip (lhvi_ais_chain_host) in a stand-alone program, to be built with the
// host-side sanitizers and run on the CPU: scripts/ais_host_sanitize.sh, which also writes the file of flat models (rand_3_2,
// wide_states, pure_disc, no_disc) this reads.  It touches no device.  Every array has exactly the size the entry point may read
// or write, so an access past it is reported.  Per model and T in {1, 2, 5}: seeded chains with injected draws and with the
// Philox stream, each in one call and split over two (the same bits, finite log weights, digits in range), and the return codes.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>
#include "../lifted-hybrid-variational-inference_amd/csrc/ais.hip"

namespace lhvi {
thread_local int g_last_hip_error = 0;
}

static double lcg(unsigned long long& s) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(s >> 11) / 9007199254740992.0;
}

struct Model {
    std::string name;
    int Nd = 0, Nc = 0, n_quad = 0, n_tab = 0, n_hyb = 0, table_doubles = 0, max_states = 1;
    std::vector<int32_t> ints[12];      // dstates, quad_ptr, quad_desc, tab_ptr, tab_desc, dstate_off, vt_ptr, vt_fac, vh_ptr, vh_fac,
                                        // hyb_quad, hyb_off
    std::vector<double> quad_par, tab_par;

    bool read(FILE* fh) {
        char buf[64];
        if (std::fscanf(fh, "%63s %d %d %d %d %d %d %d", buf, &Nd, &Nc, &n_quad, &n_tab, &n_hyb, &table_doubles, &max_states) != 8)
            return false;
        name = buf;
        for (auto& v : ints) {
            int n = 0;
            if (std::fscanf(fh, "%d", &n) != 1) return false;
            v.resize(n);
            for (auto& x : v)
                if (std::fscanf(fh, "%d", &x) != 1) return false;
        }
        for (auto* v : {&quad_par, &tab_par}) {
            int n = 0;
            if (std::fscanf(fh, "%d", &n) != 1) return false;
            v->resize(n);
            for (auto& x : *v)
                if (std::fscanf(fh, "%la", &x) != 1) return false;
        }
        return true;
    }
    static const int32_t* p(const std::vector<int32_t>& v) { return v.empty() ? nullptr : v.data(); }
    lhvi_gibbs_t view(int its, uint64_t seed) const {
        lhvi_gibbs_t g{};
        lhvi_exact_t& m = g.ex;
        m.Nd = Nd, m.Nc = Nc, m.M = 0, m.dstates = p(ints[0]), m.dstride = nullptr;      // M = 0, no dstride: neither is read
        m.n_quad = n_quad, m.quad_ptr = p(ints[1]), m.quad_desc = p(ints[2]), m.quad_par = quad_par.empty() ? nullptr : quad_par.data();
        m.n_tab = n_tab, m.tab_ptr = p(ints[3]), m.tab_desc = p(ints[4]), m.tab_par = tab_par.empty() ? nullptr : tab_par.data();
        g.dstate_off = p(ints[5]), g.vt_ptr = p(ints[6]), g.vt_fac = p(ints[7]), g.vh_ptr = p(ints[8]), g.vh_fac = p(ints[9]);
        g.n_hyb = n_hyb, g.hyb_quad = p(ints[10]), g.hyb_off = p(ints[11]);
        g.table_doubles = table_doubles, g.max_states = max_states, g.table_scratch = nullptr;
        g.disc_block_its = its, g.num_burnin = 0, g.num_samples = 0, g.seed = seed;
        return g;
    }
};

template <class T>
static T* ptr(std::vector<T>& v) { return v.empty() ? nullptr : v.data(); }

static int run_chains(const Model& md, double& checksum) {
    int failures = 0;
    const std::vector<int32_t>& dstates = md.ints[0];
    const int its = 2;
    for (int T : {1, 2, 5}) {
        unsigned long long s = 91 + T;
        const lhvi_gibbs_t g = md.view(its, 12345);
        std::vector<double> betas(T + 1), mu0(md.Nc), z((size_t)T * md.Nc), u((size_t)T * its * md.Nd);
        for (int t = 0; t <= T; ++t) betas[t] = (double)t / T;
        for (auto& v : mu0) v = lcg(s) - 0.5;
        for (int chain = 0; chain < 6; ++chain) {
            std::vector<int32_t> x0(md.Nd);
            for (int n = 0; n < md.Nd; ++n) {
                const int k = (int)(lcg(s) * dstates[n]);
                x0[n] = k < dstates[n] ? k : dstates[n] - 1;
            }
            for (auto& v : z) v = 4 * lcg(s) - 2;
            for (auto& v : u) v = lcg(s);
            for (int philox = 0; philox < 2; ++philox) {
                const double *zz = philox ? nullptr : ptr(z), *uu = philox ? nullptr : ptr(u);
                std::vector<int32_t> a = x0, b = x0;
                double lwa = 0.0, lwb = 0.0;
                failures += lhvi_ais_chain_host(&g, chain, T, betas.data(), 0, T, 1.3, ptr(mu0), ptr(a), &lwa, zz, uu) != LHVI_OK;
                failures += lhvi_ais_chain_host(&g, chain, T, betas.data(), 0, T / 2, 1.3, ptr(mu0), ptr(b), &lwb, zz, uu) != LHVI_OK;
                failures += lhvi_ais_chain_host(&g, chain, T, betas.data(), T / 2, T, 1.3, ptr(mu0), ptr(b), &lwb, zz, uu) != LHVI_OK;
                failures += !(lwa == lwb) || !std::isfinite(lwa) || a != b;
                for (int n = 0; n < md.Nd; ++n) failures += a[n] < 0 || a[n] >= dstates[n];
                checksum += lwa;
            }
        }
        std::vector<int32_t> x(md.Nd, 0);
        double lw = 0.0;
        failures += lhvi_ais_chain_host(&g, 0, T, betas.data(), 0, T + 1, 1.3, ptr(mu0), ptr(x), &lw, nullptr, nullptr) != LHVI_E_ARG;
        failures += lhvi_ais_chain_host(&g, 0, T, betas.data(), -1, T, 1.3, ptr(mu0), ptr(x), &lw, nullptr, nullptr) != LHVI_E_ARG;
        failures += lhvi_ais_chain_host(&g, 0, T, nullptr, 0, T, 1.3, ptr(mu0), ptr(x), &lw, nullptr, nullptr) != LHVI_E_ARG;
        failures += lhvi_ais_chain_host(&g, 0, T, betas.data(), 0, T, 0.0, ptr(mu0), ptr(x), &lw, nullptr, nullptr) != LHVI_E_ARG;
        failures += lhvi_ais_chain_host(&g, 0, T, betas.data(), 0, T, 1.3, ptr(mu0), ptr(x), nullptr, nullptr, nullptr) != LHVI_E_ARG;
        failures += lhvi_ais_chain_host(&g, -1, T, betas.data(), 0, T, 1.3, ptr(mu0), ptr(x), &lw, nullptr, nullptr) != LHVI_E_ARG;
        if (md.Nc && md.Nd)     // one injected stream without the other
            failures += lhvi_ais_chain_host(&g, 0, T, betas.data(), 0, T, 1.3, ptr(mu0), ptr(x), &lw, ptr(z), nullptr) != LHVI_E_ARG;
        failures += lhvi_ais_chain_host(&g, 0, T, betas.data(), T, T, 1.3, ptr(mu0), ptr(x), &lw, nullptr, nullptr) != LHVI_OK;
    }
    failures += lhvi_ais_chain_host(nullptr, 0, 1, nullptr, 0, 0, 1.0, nullptr, nullptr, nullptr, nullptr, nullptr) != LHVI_E_ARG;
    std::printf("%s: Nd = %d, Nc = %d\n", md.name.c_str(), md.Nd, md.Nc);
    return failures;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s <file of flat models>\n", argv[0]);
        return 2;
    }
    FILE* fh = std::fopen(argv[1], "r");
    if (!fh) {
        std::perror(argv[1]);
        return 2;
    }
    int failures = 0, models = 0;
    double checksum = 0.0;
    for (Model md; md.read(fh); ++models) failures += run_chains(md, checksum);
    std::fclose(fh);
    failures += models != 4;
    std::printf("ais host twin under the sanitizers: %d models, checksum %.17g, %d failures\n", models, checksum, failures);
    return failures != 0;
}
