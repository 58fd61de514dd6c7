// npvi_host_sanitize.hip -- the host twins of csrc/npvi.hip (lhvi_npvi_grad_host, lhvi_npvi_run_host) or, built with
// -DLHVI_SANITIZE_ONESHOT, of csrc/oneshot.hip (lhvi_oneshot_grad_host, lhvi_oneshot_run_host; csrc/npvi.hip is then linked as a
// second translation unit, for the kernels oneshot.hip only declares) in a stand-alone program, to be built with the host-side
// sanitizers and run on the CPU: scripts/npvi_host_sanitize.sh.  It touches no device.  The models of tests/npvi_models.py and
// tests/oneshot_models.py arrive as a text file; every array has exactly the size the entry point may read or write, so an access
// past it is reported.  Per model: one gradient, then 4 updates with fix_mix_its = 2; a checksum (FNV-1a over the bytes) of every
// output is printed, so that two builds of the library can be compared line by line, and the return codes of the refused arguments
// are checked.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#ifdef LHVI_SANITIZE_ONESHOT
#include "oneshot.hip"
static const char* const SOLVER = "oneshot";
#else
#include "npvi.hip"
static const char* const SOLVER = "npvi";
#endif

namespace lhvi {
thread_local int g_last_hip_error = 0;
}

static int grad_host(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const double* var_count, const double* fac_count,
                     const double* var_coef, double* obj, double* g_tau, double* g_c, double* g_rho) {
#ifdef LHVI_SANITIZE_ONESHOT
    return lhvi_oneshot_grad_host(g, pots, p, var_count, fac_count, var_coef, obj, g_tau, g_c, g_rho);
#else
    return lhvi_npvi_grad_host(g, pots, p, var_count, fac_count, obj, g_tau, g_c, g_rho);
#endif
}
static int run_host(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const lhvi_npvi_opt_t* o, const double* var_coef,
                    int32_t iterations, int32_t fix_mix_its, double* obj_log) {
#ifdef LHVI_SANITIZE_ONESHOT
    return lhvi_oneshot_run_host(g, pots, p, o, var_coef, iterations, fix_mix_its, obj_log);
#else
    return lhvi_npvi_run_host(g, pots, p, o, iterations, fix_mix_its, obj_log);
#endif
}

static std::vector<int32_t> read_ints(FILE* fh) {
    long n = 0;
    if (fscanf(fh, "%ld", &n) != 1) { fprintf(stderr, "bad model file\n"); exit(2); }
    std::vector<int32_t> v((size_t)n);
    for (auto& x : v) { long long t; if (fscanf(fh, "%lld", &t) != 1) exit(2); x = (int32_t)t; }
    return v;
}
static std::vector<double> read_doubles(FILE* fh) {
    long n = 0;
    if (fscanf(fh, "%ld", &n) != 1) exit(2);
    std::vector<double> v((size_t)n);
    char buf[64];
    for (auto& x : v) { if (fscanf(fh, "%63s", buf) != 1) exit(2); x = strtod(buf, nullptr); }
    return v;
}
// NULL for an array the model does not have (the counts, var_coef)
static const double* opt(const std::vector<double>& v) { return v.empty() ? nullptr : v.data(); }

static unsigned long long fnv(const std::vector<double>& v) {
    unsigned long long h = 1469598103934665603ull;
    const unsigned char* b = reinterpret_cast<const unsigned char*>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(double); ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #c, name); return 1; } } while (0)

int main(int argc, char** argv) {
    FILE* fh = argc < 2 ? nullptr : fopen(argv[1], "r");
    if (!fh) return 2;
    char name[64], lo[64], hi[64];
    int V, F, E, D, P, interpreted, K, T, Dmax, max_slots, max_arity;
    while (fscanf(fh, "%63s %d %d %d %d %d %d %d %d %d %d %d %63s %63s", name, &V, &F, &E, &D, &P, &interpreted, &K, &T, &Dmax, &max_slots,
                  &max_arity, lo, hi) == 14) {
        auto fac_ptr = read_ints(fh), edge_var = read_ints(fh), edge_fac = read_ints(fh), var_ptr = read_ints(fh), var_edge = read_ints(fh);
        auto fac_pot = read_ints(fh), var_dom = read_ints(fh), dom_cont = read_ints(fh), dom_ptr = read_ints(fh);
        auto kind = read_ints(fh), off = read_ints(fh), edge_axis = read_ints(fh);
        auto var_value = read_doubles(fh), dom_lo = read_doubles(fh), dom_hi = read_doubles(fh), dom_val = read_doubles(fh);
        auto param = read_doubles(fh), gh_x = read_doubles(fh), gh_w = read_doubles(fh), mu_lo = read_doubles(fh), mu_hi = read_doubles(fh);
        auto var_count = read_doubles(fh), fac_count = read_doubles(fh), var_coef = read_doubles(fh);
        auto tau = read_doubles(fh), theta_c = read_doubles(fh), rho = read_doubles(fh);
        auto w = read_doubles(fh), eta_c = read_doubles(fh), eta_d = read_doubles(fh);
        REQUIRE((int)tau.size() == K && (int)theta_c.size() == V * K * 2 && (int)rho.size() == V * K * Dmax && (int)edge_axis.size() == E * 4);
        REQUIRE((int)w.size() == K && eta_c.size() == theta_c.size() && eta_d.size() == rho.size() && (int)gh_x.size() == T);
        lhvi_graph_t g{};
        g.V = V; g.F = F; g.E = E; g.nnz = (int32_t)var_edge.size(); g.D = D;
        g.fac_ptr = fac_ptr.data(); g.edge_var = edge_var.data(); g.edge_fac = edge_fac.data(); g.var_ptr = var_ptr.data();
        g.var_edge = var_edge.data(); g.fac_pot = fac_pot.data(); g.var_value = var_value.data(); g.var_dom = var_dom.data();
        g.dom_cont = dom_cont.data(); g.dom_lo = dom_lo.data(); g.dom_hi = dom_hi.data(); g.dom_ptr = dom_ptr.data(); g.dom_val = dom_val.data();
        lhvi_pots_t pots{P, kind.data(), off.data(), param.data(), interpreted};
        lhvi_vi_t p{};
        p.K = K; p.T = T; p.Dmax = Dmax; p.quirks = LHVI_VI_GAUSSIAN_PDF;
        p.gh_x = gh_x.data(); p.gh_w = gh_w.data(); p.w = w.data(); p.eta_c = eta_c.data(); p.eta_d = eta_d.data(); p.edge_axis = edge_axis.data();
        const double* coef = opt(var_coef);

        // one gradient
        std::vector<double> obj(1), g_tau(tau.size()), g_c(theta_c.size()), g_rho(rho.size());
        REQUIRE(grad_host(&g, &pots, &p, opt(var_count), opt(fac_count), coef, obj.data(), g_tau.data(), g_c.data(), g_rho.data()) == LHVI_OK);
        printf("%s %s K %d T %d grad: obj %.17g %016llx g_tau %016llx g_c %016llx g_rho %016llx\n", SOLVER, name, K, T, obj[0], fnv(obj),
               fnv(g_tau), fnv(g_c), fnv(g_rho));

        // 4 updates, the weights fixed during the first 2
        const int its = 4;
        std::vector<double> m_tau(tau.size()), s_tau(tau.size()), m_c(theta_c.size()), s_c(theta_c.size()), m_rho(rho.size()), s_rho(rho.size());
        std::vector<double> log((size_t)its);
        lhvi_npvi_opt_t o{};
        o.tau = tau.data(); o.theta_c = theta_c.data(); o.rho = rho.data();
        o.m_tau = m_tau.data(); o.s_tau = s_tau.data(); o.m_c = m_c.data(); o.s_c = s_c.data(); o.m_rho = m_rho.data(); o.s_rho = s_rho.data();
        o.g_tau = g_tau.data(); o.g_c = g_c.data(); o.g_rho = g_rho.data(); o.obj = obj.data();
        o.w = w.data(); o.eta_c = eta_c.data(); o.eta_d = eta_d.data(); o.mu_lo = mu_lo.data(); o.mu_hi = mu_hi.data();
        o.lvar_lo = strtod(lo, nullptr); o.lvar_hi = strtod(hi, nullptr);
        o.var_count = opt(var_count); o.fac_count = opt(fac_count);
        o.lr = 0.05; o.b1 = 0.9; o.b2 = 0.999; o.eps = 1e-8; o.t = 0;
        o.max_slots = max_slots; o.max_arity = max_arity;
        REQUIRE(run_host(&g, &pots, &p, &o, coef, its, 2, log.data()) == LHVI_OK);
        for (double x : log) REQUIRE(x == x);
        printf("%s %s K %d T %d run: obj_log %.17g %016llx tau %016llx theta_c %016llx rho %016llx\n", SOLVER, name, K, T, log[its - 1], fnv(log),
               fnv(tau), fnv(theta_c), fnv(rho));
        printf("    moments %016llx %016llx %016llx %016llx %016llx %016llx view %016llx %016llx %016llx gradient %016llx %016llx %016llx\n",
               fnv(m_tau), fnv(s_tau), fnv(m_c), fnv(s_c), fnv(m_rho), fnv(s_rho), fnv(w), fnv(eta_c), fnv(eta_d), fnv(g_tau), fnv(g_c), fnv(g_rho));
        // without a log the objective goes to o.obj; no update: nothing but the checks runs
        REQUIRE(run_host(&g, &pots, &p, &o, coef, 1, 0, nullptr) == LHVI_OK && obj[0] == obj[0]);
        REQUIRE(run_host(&g, &pots, &p, &o, coef, 0, 0, nullptr) == LHVI_OK);

        // refused arguments
        REQUIRE(grad_host(&g, &pots, &p, opt(var_count), opt(fac_count), coef, nullptr, g_tau.data(), g_c.data(), g_rho.data()) == LHVI_E_ARG);
        REQUIRE(run_host(&g, &pots, &p, &o, coef, -1, 0, log.data()) == LHVI_E_ARG);
        lhvi_vi_t p0 = p;
        p0.K = 0;
        REQUIRE(grad_host(&g, &pots, &p0, opt(var_count), opt(fac_count), coef, obj.data(), g_tau.data(), g_c.data(), g_rho.data()) == LHVI_E_ARG);
        REQUIRE(run_host(&g, &pots, &p0, &o, coef, its, 2, log.data()) == LHVI_E_ARG);
        lhvi_npvi_opt_t o0 = o;
        o0.obj = nullptr;
        REQUIRE(run_host(&g, &pots, &p, &o0, coef, its, 2, log.data()) == LHVI_E_ARG);
#ifdef LHVI_SANITIZE_ONESHOT
        REQUIRE(grad_host(&g, &pots, &p, opt(var_count), opt(fac_count), nullptr, obj.data(), g_tau.data(), g_c.data(), g_rho.data()) == LHVI_E_ARG);
        REQUIRE(run_host(&g, &pots, &p, &o, nullptr, its, 2, log.data()) == LHVI_E_ARG);
#endif
    }
    fclose(fh);
    return 0;
}
