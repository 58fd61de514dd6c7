// gibbs_rb_host_sanitize.hip -- the host twins of csrc/gibbs_rb.hip (lhvi_exact_config_at_host, lhvi_gibbs_rb_disc_host) in a
// stand-alone program, to be built with the host-side sanitizers and run on the CPU: scripts/gibbs_rb_host_sanitize.sh, which
// also writes the file of flat models (rand_3_2, wide_states) this reads.  It touches no device.  Every array has exactly the
// size the entry points may read or write, so an access past it is reported.  Per model: every configuration's row of digits
// through lhvi_exact_config_at_host (twice, the same bits; with null outputs; with M = 0 and no dstride), 1, 3 and 7 seeded
// samples through lhvi_gibbs_rb_disc_host in one call and split over two (the same bits; every variable's states sum to the
// number of samples), and the return codes of both.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>
#include "../lifted-hybrid-variational-inference_amd/csrc/gibbs_rb.hip"

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
    lhvi_gibbs_t view(int num_samples) const {
        lhvi_gibbs_t g{};
        lhvi_exact_t& m = g.ex;
        m.Nd = Nd, m.Nc = Nc, m.M = 0, m.dstates = p(ints[0]), m.dstride = nullptr;      // M = 0, no dstride: neither is read
        m.n_quad = n_quad, m.quad_ptr = p(ints[1]), m.quad_desc = p(ints[2]), m.quad_par = quad_par.empty() ? nullptr : quad_par.data();
        m.n_tab = n_tab, m.tab_ptr = p(ints[3]), m.tab_desc = p(ints[4]), m.tab_par = tab_par.empty() ? nullptr : tab_par.data();
        g.dstate_off = p(ints[5]), g.vt_ptr = p(ints[6]), g.vt_fac = p(ints[7]), g.vh_ptr = p(ints[8]), g.vh_fac = p(ints[9]);
        g.n_hyb = n_hyb, g.hyb_quad = p(ints[10]), g.hyb_off = p(ints[11]);
        g.table_doubles = table_doubles, g.max_states = max_states, g.table_scratch = nullptr;
        g.disc_block_its = 1, g.num_burnin = 0, g.num_samples = num_samples, g.seed = 0;
        return g;
    }
};

static int run_configs(const Model& md, double& checksum) {
    int failures = 0;
    const lhvi_gibbs_t g = md.view(0);
    const lhvi_exact_t& m = g.ex;
    const std::vector<int32_t>& dstates = md.ints[0];
    std::vector<int32_t> row(md.Nd, 0);
    std::vector<double> mean(md.Nc), var(md.Nc), mean2(md.Nc), var2(md.Nc);
    int64_t count = 0;
    for (bool more = true; more; ++count) {
        double lp = 0, lp2 = 0;
        failures += lhvi_exact_config_at_host(&m, row.data(), &lp, mean.data(), var.data()) != LHVI_OK;
        failures += lhvi_exact_config_at_host(&m, row.data(), &lp2, mean2.data(), var2.data()) != LHVI_OK;
        failures += lhvi_exact_config_at_host(&m, row.data(), nullptr, nullptr, nullptr) != LHVI_OK;
        failures += !(lp == lp2) || !std::isfinite(lp);
        for (int j = 0; j < md.Nc; ++j) failures += !(mean[j] == mean2[j]) || !(var[j] == var2[j]) || !(var[j] > 0);
        checksum += lp;
        more = false;
        for (int d = md.Nd - 1; d >= 0; --d) {              // the next configuration's digits
            if (++row[d] < dstates[d]) { more = true; break; }
            row[d] = 0;
        }
    }
    // a digit outside its range, a missing row, a missing model
    if (md.Nd) {
        row[md.Nd - 1] = dstates[md.Nd - 1];
        failures += lhvi_exact_config_at_host(&m, row.data(), nullptr, mean.data(), var.data()) != LHVI_E_ARG;
        row[md.Nd - 1] = -1;
        failures += lhvi_exact_config_at_host(&m, row.data(), nullptr, mean.data(), var.data()) != LHVI_E_ARG;
        failures += lhvi_exact_config_at_host(&m, nullptr, nullptr, mean.data(), var.data()) != LHVI_E_ARG;
    }
    failures += lhvi_exact_config_at_host(nullptr, row.data(), nullptr, nullptr, nullptr) != LHVI_E_ARG;
    std::printf("%s: %lld configurations\n", md.name.c_str(), (long long)count);
    return failures;
}

static int run_rb_disc(const Model& md, double& checksum) {
    int failures = 0;
    const std::vector<int32_t>& dstates = md.ints[0];
    const std::vector<int32_t>& off = md.ints[5];
    const int n_states = md.Nd ? off[md.Nd] : 0;
    for (int S : {1, 3, 7}) {
        unsigned long long s = 77 + S;
        const lhvi_gibbs_t g = md.view(S);
        std::vector<int32_t> disc((size_t)S * md.Nd);
        std::vector<double> cont((size_t)S * md.Nc), one(n_states, 0.0), two(n_states, 0.0);
        for (int r = 0; r < S; ++r) {
            for (int n = 0; n < md.Nd; ++n) {
                const int k = (int)(lcg(s) * dstates[n]);
                disc[(size_t)r * md.Nd + n] = k < dstates[n] ? k : dstates[n] - 1;
            }
            for (int j = 0; j < md.Nc; ++j) cont[(size_t)r * md.Nc + j] = 4 * lcg(s) - 2;
        }
        failures += lhvi_gibbs_rb_disc_host(&g, 0, S, disc.data(), cont.data(), one.data()) != LHVI_OK;
        failures += lhvi_gibbs_rb_disc_host(&g, 0, S / 2, disc.data(), cont.data(), two.data()) != LHVI_OK;
        failures += lhvi_gibbs_rb_disc_host(&g, S / 2, S, disc.data(), cont.data(), two.data()) != LHVI_OK;
        for (int i = 0; i < n_states; ++i) failures += !(one[i] == two[i]);
        for (int n = 0; n < md.Nd; ++n) {
            double total = 0;
            for (int i = off[n]; i < off[n + 1]; ++i) total += one[i], checksum += one[i] * (i + 1);
            failures += !(std::fabs(total - S) <= S * 4e-16 * dstates[n]);
        }
        failures += lhvi_gibbs_rb_disc_host(&g, 0, S + 1, disc.data(), cont.data(), one.data()) != LHVI_E_ARG;
        failures += lhvi_gibbs_rb_disc_host(&g, -1, S, disc.data(), cont.data(), one.data()) != LHVI_E_ARG;
        failures += lhvi_gibbs_rb_disc_host(&g, 0, S, nullptr, cont.data(), one.data()) != LHVI_E_ARG;
        failures += lhvi_gibbs_rb_disc_host(&g, 0, S, disc.data(), cont.data(), nullptr) != LHVI_E_ARG;
        failures += lhvi_gibbs_rb_disc_host(&g, S, S, nullptr, nullptr, nullptr) != LHVI_OK;      // an empty range reads nothing
        disc[0] = dstates[0];
        failures += lhvi_gibbs_rb_disc_host(&g, 0, S, disc.data(), cont.data(), one.data()) != LHVI_E_ARG;
    }
    failures += lhvi_gibbs_rb_disc_host(nullptr, 0, 0, nullptr, nullptr, nullptr) != LHVI_E_ARG;
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
    for (Model md; md.read(fh); ++models) {
        failures += run_configs(md, checksum);
        failures += run_rb_disc(md, checksum);
    }
    std::fclose(fh);
    failures += models != 2;
    std::printf("gibbs_rb host twins under the sanitizers: %d models, checksum %.17g, %d failures\n", models, checksum, failures);
    return failures != 0;
}
