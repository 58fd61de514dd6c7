// pt_host_sanitize.hip -- the host twin of csrc/pt.hip (lhvi_pt_ladder_host) in a stand-alone program, to be built with the
// host-side sanitizers and run on the CPU: scripts/pt_host_sanitize.sh, which also writes the file of flat models (rand_3_2,
// wide_states, pure_disc, no_disc, two_wells) this reads.  It touches no device.  Every array has exactly the size the entry point
// may read or write, so an access past it is reported.  Per model, R in {1, 2, 3, 5} and swap_every in {0, 1, 2}: seeded ladders
// with injected draws and with the Philox stream, each in one call and split over two (the same bits, finite samples, digits in
// range, counters that add up), and the return codes.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>
#include "../lifted-hybrid-variational-inference_amd/csrc/pt.hip"

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
    lhvi_gibbs_t view(int its, int burnin, int samples, uint64_t seed) const {
        lhvi_gibbs_t g{};
        lhvi_exact_t& m = g.ex;
        m.Nd = Nd, m.Nc = Nc, m.M = 0, m.dstates = p(ints[0]), m.dstride = nullptr;      // M = 0, no dstride: neither is read
        m.n_quad = n_quad, m.quad_ptr = p(ints[1]), m.quad_desc = p(ints[2]), m.quad_par = quad_par.empty() ? nullptr : quad_par.data();
        m.n_tab = n_tab, m.tab_ptr = p(ints[3]), m.tab_desc = p(ints[4]), m.tab_par = tab_par.empty() ? nullptr : tab_par.data();
        g.dstate_off = p(ints[5]), g.vt_ptr = p(ints[6]), g.vt_fac = p(ints[7]), g.vh_ptr = p(ints[8]), g.vh_fac = p(ints[9]);
        g.n_hyb = n_hyb, g.hyb_quad = p(ints[10]), g.hyb_off = p(ints[11]);
        g.table_doubles = table_doubles, g.max_states = max_states, g.table_scratch = nullptr;
        g.disc_block_its = its, g.num_burnin = burnin, g.num_samples = samples, g.seed = seed;
        return g;
    }
};

template <class T>
static T* ptr(std::vector<T>& v) { return v.empty() ? nullptr : v.data(); }

struct Outputs {
    std::vector<int32_t> x, disc, counts, tries, accs;
    std::vector<double> cont, sum1, sum2;
    Outputs(const Model& md, int R, int samples, const std::vector<int32_t>& x0)
        : x(x0), disc((size_t)samples * md.Nd), counts(md.ints[5].empty() ? 0 : md.ints[5].back()), tries(R - 1), accs(R - 1),
          cont((size_t)samples * md.Nc), sum1(md.Nc), sum2((size_t)md.Nc * (md.Nc + 1) / 2) {}
    bool operator==(const Outputs& o) const {
        return x == o.x && disc == o.disc && counts == o.counts && tries == o.tries && accs == o.accs && cont == o.cont &&
               sum1 == o.sum1 && sum2 == o.sum2;
    }
};

static int run(const lhvi_gibbs_t& g, int64_t ladder, int R, const std::vector<double>& betas, int b, int e, int swap_every,
               std::vector<double>& mu0, Outputs& o, const double* z, const double* u, const double* usw) {
    return lhvi_pt_ladder_host(&g, ladder, R, betas.data(), b, e, swap_every, 1.3, ptr(mu0), ptr(o.x), z, u, usw, ptr(o.disc),
                               ptr(o.cont), ptr(o.counts), ptr(o.sum1), ptr(o.sum2), ptr(o.tries), ptr(o.accs));
}

static int run_ladders(const Model& md, double& checksum) {
    int failures = 0;
    const std::vector<int32_t>& dstates = md.ints[0];
    const int its = 2, burnin = 2, samples = 3, iters = burnin + samples;
    const lhvi_gibbs_t g = md.view(its, burnin, samples, 12345);
    std::vector<double> mu0(md.Nc);
    for (int R : {1, 2, 3, 5})
        for (int swap_every : {0, 1, 2}) {
            unsigned long long s = 91 + 7 * R + swap_every;
            std::vector<double> betas(R), z((size_t)iters * R * md.Nc), u((size_t)iters * R * its * md.Nd),
                usw((size_t)iters * (R > 1 ? R - 1 : 1));
            for (int r = 0; r < R; ++r) betas[r] = R > 1 ? (double)r / (R - 1) : 1.0;
            for (auto& v : mu0) v = lcg(s) - 0.5;
            for (int ladder = 0; ladder < 3; ++ladder) {
                std::vector<int32_t> x0((size_t)R * md.Nd);
                for (int r = 0; r < R; ++r)
                    for (int n = 0; n < md.Nd; ++n) {
                        const int k = (int)(lcg(s) * dstates[n]);
                        x0[(size_t)r * md.Nd + n] = k < dstates[n] ? k : dstates[n] - 1;
                    }
                for (auto& v : z) v = 4 * lcg(s) - 2;
                for (auto& v : u) v = lcg(s);
                for (auto& v : usw) v = lcg(s);
                for (int philox = 0; philox < 2; ++philox) {
                    const double *zz = philox ? nullptr : ptr(z), *uu = philox ? nullptr : ptr(u), *ss = philox ? nullptr : ptr(usw);
                    Outputs a(md, R, samples, x0), b(md, R, samples, x0);
                    failures += run(g, ladder, R, betas, 0, iters, swap_every, mu0, a, zz, uu, ss) != LHVI_OK;
                    failures += run(g, ladder, R, betas, 0, 3, swap_every, mu0, b, zz, uu, ss) != LHVI_OK;
                    failures += run(g, ladder, R, betas, 3, iters, swap_every, mu0, b, zz, uu, ss) != LHVI_OK;
                    failures += !(a == b);
                    for (size_t i = 0; i < a.x.size(); ++i) failures += a.x[i] < 0 || a.x[i] >= dstates[i % md.Nd];
                    int total = 0;
                    for (int c : a.counts) total += c;
                    failures += total != samples * md.Nd;
                    for (int r = 0; r + 1 < R; ++r) {
                        // rounds of pair r: swap rounds s = 0 .. of parity r mod 2
                        int rounds = 0;
                        for (int it = 0; it < iters; ++it)
                            rounds += swap_every > 0 && (it + 1) % swap_every == 0 && (it / swap_every) % 2 == r % 2;
                        failures += a.tries[r] != rounds || a.accs[r] < 0 || a.accs[r] > a.tries[r];
                    }
                    for (double v : a.cont) failures += !std::isfinite(v);
                    for (double v : a.sum2) checksum += v;
                }
            }
            Outputs o(md, R, samples, std::vector<int32_t>((size_t)R * md.Nd, 0));
            failures += run(g, 0, R, betas, -1, iters, swap_every, mu0, o, nullptr, nullptr, nullptr) != LHVI_E_ARG;
            failures += run(g, 0, R, betas, 3, 2, swap_every, mu0, o, nullptr, nullptr, nullptr) != LHVI_E_ARG;
            failures += run(g, 0, R, betas, 0, iters, -1, mu0, o, nullptr, nullptr, nullptr) != LHVI_E_ARG;
            failures += run(g, -1, R, betas, 0, iters, swap_every, mu0, o, nullptr, nullptr, nullptr) != LHVI_E_ARG;
            failures += lhvi_pt_ladder_host(&g, 0, R, nullptr, 0, iters, swap_every, 1.3, ptr(mu0), ptr(o.x), nullptr, nullptr, nullptr,
                                            nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != LHVI_E_ARG;
            failures += lhvi_pt_ladder_host(&g, 0, R, betas.data(), 0, iters, swap_every, 0.0, ptr(mu0), ptr(o.x), nullptr, nullptr,
                                            nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != LHVI_E_ARG;
            if (md.Nc && md.Nd)     // one injected stream without the others
                failures += run(g, 0, R, betas, 0, iters, swap_every, mu0, o, ptr(z), nullptr, nullptr) != LHVI_E_ARG;
            // every output may be absent
            failures += lhvi_pt_ladder_host(&g, 0, R, betas.data(), 0, iters, swap_every, 1.3, ptr(mu0), ptr(o.x), nullptr, nullptr,
                                            nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != LHVI_OK;
            failures += run(g, 0, R, betas, iters, iters, swap_every, mu0, o, nullptr, nullptr, nullptr) != LHVI_OK;
        }
    failures += lhvi_pt_ladder_host(nullptr, 0, 1, nullptr, 0, 0, 1, 1.0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                    nullptr, nullptr, nullptr, nullptr, nullptr) != LHVI_E_ARG;
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
    for (Model md; md.read(fh); ++models) failures += run_ladders(md, checksum);
    std::fclose(fh);
    failures += models != 5;
    std::printf("pt host twin under the sanitizers: %d models, checksum %.17g, %d failures\n", models, checksum, failures);
    return failures != 0;
}
