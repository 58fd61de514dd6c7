// fgibbs_host_sanitize.hip -- the host twin of csrc/fgibbs.hip (lhvi_fgibbs_chain_host: the device's update code with one "lane")
// in a stand-alone program, to be built with the host-side sanitizers and run on the CPU: scripts/fgibbs_host_sanitize.sh.  It
// touches no device.  The models of tests/fgibbs_models.py arrive as a text file; every array has exactly the size the entry
// point may read or write, so an access past it is reported.  Per model: 3 chains of 6 iterations (burn-in 1, 3 kept at thin 2)
// from the Philox stream with every output, in one call and in three; the two must agree, the counters must add up, and the
// return codes of the refused arguments are checked.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../lifted-hybrid-variational-inference_amd/csrc/fgibbs.hip"

namespace lhvi {
thread_local int g_last_hip_error = 0;
}

template <class T>
static std::vector<T> read_ints(FILE* fh) {
    long n = 0;
    if (fscanf(fh, "%ld", &n) != 1) { fprintf(stderr, "bad model file\n"); exit(2); }
    std::vector<T> v((size_t)n);
    for (auto& x : v) { long long t; if (fscanf(fh, "%lld", &t) != 1) exit(2); x = (T)t; }
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

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #c, name); return 1; } } while (0)

int main(int argc, char** argv) {
    FILE* fh = fopen(argv[1], "r");
    if (argc < 2 || !fh) return 2;
    char name[64];
    int V, F, E, D, P, interpreted, n_colours, max_shrink, n_states;
    while (fscanf(fh, "%63s %d %d %d %d %d %d %d %d %d", name, &V, &F, &E, &D, &P, &interpreted, &n_colours, &max_shrink, &n_states) == 10) {
        auto fac_ptr = read_ints<int32_t>(fh), edge_var = read_ints<int32_t>(fh), edge_fac = read_ints<int32_t>(fh);
        auto var_ptr = read_ints<int32_t>(fh), var_edge = read_ints<int32_t>(fh), fac_pot = read_ints<int32_t>(fh);
        auto var_dom = read_ints<int32_t>(fh), dom_cont = read_ints<int32_t>(fh), dom_ptr = read_ints<int32_t>(fh);
        auto kind = read_ints<int32_t>(fh), off = read_ints<int32_t>(fh);
        auto col_ptr = read_ints<int32_t>(fh), col_var = read_ints<int32_t>(fh), hub_ptr = read_ints<int32_t>(fh), hub_var = read_ints<int32_t>(fh);
        auto cnt_off = read_ints<int32_t>(fh), keep_row = read_ints<int32_t>(fh);
        auto var_value = read_doubles(fh), dom_lo = read_doubles(fh), dom_hi = read_doubles(fh), dom_val = read_doubles(fh), param = read_doubles(fh);
        auto init_x = read_doubles(fh);
        lhvi_graph_t g{};
        g.V = V; g.F = F; g.E = E; g.nnz = (int32_t)var_edge.size(); g.D = D;
        g.fac_ptr = fac_ptr.data(); g.edge_var = edge_var.data(); g.edge_fac = edge_fac.data(); g.var_ptr = var_ptr.data();
        g.var_edge = var_edge.data(); g.fac_pot = fac_pot.data(); g.var_value = var_value.data(); g.var_dom = var_dom.data();
        g.dom_cont = dom_cont.data(); g.dom_lo = dom_lo.data(); g.dom_hi = dom_hi.data(); g.dom_ptr = dom_ptr.data(); g.dom_val = dom_val.data();
        lhvi_pots_t p{P, kind.data(), off.data(), param.data(), interpreted};
        int rows = 0;
        for (int r : keep_row) rows += r >= 0;
        const int64_t C = 3;
        const int burn = 1, ns = 3, thin = 2, iters = burn + (ns - 1) * thin + 1;
        struct Out {
            std::vector<double> x, sum1, sum2, samples;
            std::vector<int32_t> idx, counts, stuck, capped;
            std::vector<int64_t> evals;
        };
        auto run = [&](Out& o, const std::vector<int>& cuts, bool inject_init) {
            o.x.assign((size_t)V * C, 0.0); o.idx.assign((size_t)V * C, 0); o.sum1.assign((size_t)V * C, 0.0); o.sum2.assign((size_t)V * C, 0.0);
            o.samples.assign((size_t)rows * C * ns, 0.0); o.counts.assign((size_t)n_states * C, 0);
            o.stuck.assign(C, 0); o.capped.assign(C, 0); o.evals.assign(C, 0);
            lhvi_fgibbs_t s{};
            s.n_colours = n_colours; s.col_ptr = col_ptr.data(); s.col_var = col_var.data(); s.hub_ptr = hub_ptr.data(); s.hub_var = hub_var.data();
            s.max_shrink = max_shrink; s.hub_degree = 64; s.num_burnin = burn; s.num_samples = ns; s.thin = thin; s.seed = 20261021ull;
            s.init_x = inject_init ? init_x.data() : nullptr;
            s.cnt_off = cnt_off.data(); s.counts = o.counts.data(); s.sum1 = o.sum1.data(); s.sum2 = o.sum2.data();
            s.keep_row = keep_row.data(); s.samples = o.samples.data(); s.stuck = o.stuck.data(); s.capped = o.capped.data(); s.evals = o.evals.data();
            for (int64_t c = 0; c < C; ++c) {
                int done = 0;
                for (size_t k = 0; k < cuts.size(); ++k) {
                    const int rc = lhvi_fgibbs_chain_host(&g, &p, &s, C, c, k == 0, done, cuts[k], o.x.data(), o.idx.data());
                    if (rc) return rc;
                    done = cuts[k];
                }
            }
            return 0;
        };
        const bool has_init = !init_x.empty();
        Out one, three;
        REQUIRE(run(one, {iters}, has_init) == 0);
        REQUIRE(run(three, {1, 4, iters}, has_init) == 0);
        REQUIRE(one.x == three.x && one.idx == three.idx && one.sum1 == three.sum1 && one.sum2 == three.sum2);
        REQUIRE(one.samples == three.samples && one.counts == three.counts);
        REQUIRE(one.stuck == three.stuck && one.capped == three.capped && one.evals == three.evals);
        long kept = 0, hidden_disc = 0;
        for (int c : one.counts) kept += c;
        for (int v = 0; v < V; ++v) hidden_disc += cnt_off[v] >= 0;
        REQUIRE(kept == hidden_disc * ns * C);
        for (int64_t c = 0; c < C; ++c) REQUIRE(one.evals[c] > 0 || n_colours == 0);
        // refused arguments
        lhvi_fgibbs_t s{};
        s.thin = 1;
        REQUIRE(lhvi_fgibbs_chain_host(&g, &p, &s, C, C, 0, 0, 0, one.x.data(), one.idx.data()) == LHVI_E_ARG);
        REQUIRE(lhvi_fgibbs_chain_host(&g, &p, &s, C, 0, 0, 2, 1, one.x.data(), one.idx.data()) == LHVI_E_ARG);
        s.max_shrink = 511;
        REQUIRE(lhvi_fgibbs_chain_host(&g, &p, &s, C, 0, 0, 0, 0, one.x.data(), one.idx.data()) == LHVI_E_UNSUPPORTED);
        s.max_shrink = 4; s.thin = 0;
        REQUIRE(lhvi_fgibbs_chain_host(&g, &p, &s, C, 0, 0, 0, 0, one.x.data(), one.idx.data()) == LHVI_E_ARG);
        const double one_count = 1.0;
        g.edge_count = &one_count; s.thin = 1;
        REQUIRE(lhvi_fgibbs_chain_host(&g, &p, &s, C, 0, 0, 0, 0, one.x.data(), one.idx.data()) == LHVI_E_UNSUPPORTED);
        printf("%s: V %d, F %d, %d colours, %d iterations x %lld chains: clean (evals %lld, stuck %d, capped %d)\n", name, V, F, n_colours, iters,
               (long long)C, (long long)(one.evals[0] + one.evals[1] + one.evals[2]), one.stuck[0] + one.stuck[1] + one.stuck[2],
               one.capped[0] + one.capped[1] + one.capped[2]);
    }
    fclose(fh);
    return 0;
}
