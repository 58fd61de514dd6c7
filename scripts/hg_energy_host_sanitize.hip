// hg_energy_host_sanitize.hip -- the host twins of csrc/hg_energy.hip (lhvi_hg_energy_host, lhvi_argmax_first_host) in a
// stand-alone program, to be built with the host-side sanitizers and run on the CPU: scripts/hg_energy_host_sanitize.sh.  It
// touches no device.  Every array has exactly the size the entry points may read or write, so an access past it is reported.
// The shapes are the edges of the entry points: Nc = 1, 7 and 64 with two discrete variables (a hybrid scope in reverse order,
// a table of arity 2), a discrete-only chain of 40 binary variables, a Gaussian-only model (Nd = 0, M = 1), S = 1, 63, 64, 65
// and 130 in both addressing modes, the return codes, and the arg-max at n = 0 .. 257 with ties, NaN, -inf and signed zeros.
#include <cmath>
#include <cstdio>
#include <vector>
#include "../lifted-hybrid-variational-inference_amd/csrc/hg_energy.hip"

namespace lhvi {
thread_local int g_last_hip_error = 0;
}

static double lcg(unsigned long long& s) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(s >> 11) / 9007199254740992.0;
}

struct Model {
    std::vector<int32_t> dstates, quad_ptr{0}, quad_desc, tab_ptr{0}, tab_desc;
    std::vector<int64_t> dstride;
    std::vector<double> quad_par, tab_par;
    int Nc = 0;
    int64_t M = 1;

    void strides() {
        dstride.assign(dstates.size(), 1);
        for (int d = (int)dstates.size() - 2; d >= 0; --d) dstride[d] = dstride[d + 1] * dstates[d + 1];
        M = dstates.empty() ? 1 : dstride[0] * dstates[0];
    }
    // scope: (variable, local stride) pairs; cont: continuous scope; `local` blocks of nc^2 + nc + 1 seeded doubles
    void quad(const std::vector<int32_t>& scope, const std::vector<int32_t>& cont, int local, unsigned long long& s) {
        const int nc = (int)cont.size();
        quad_desc.push_back((int32_t)scope.size() / 2);
        quad_desc.push_back(nc);
        quad_desc.push_back((int32_t)quad_par.size());
        quad_desc.insert(quad_desc.end(), scope.begin(), scope.end());
        quad_desc.insert(quad_desc.end(), cont.begin(), cont.end());
        quad_ptr.push_back((int32_t)quad_desc.size());
        for (int i = 0; i < local * (nc * nc + nc + 1); ++i) quad_par.push_back(2 * lcg(s) - 1);
    }
    void table(const std::vector<int32_t>& scope, int local, unsigned long long& s) {
        tab_desc.push_back((int32_t)scope.size() / 2);
        tab_desc.push_back((int32_t)tab_par.size());
        tab_desc.insert(tab_desc.end(), scope.begin(), scope.end());
        tab_ptr.push_back((int32_t)tab_desc.size());
        for (int i = 0; i < local; ++i) tab_par.push_back(2 * lcg(s) - 1);
    }
    lhvi_exact_t view() const {
        lhvi_exact_t m{};
        m.Nd = (int32_t)dstates.size(), m.Nc = Nc, m.M = M;
        m.dstates = dstates.empty() ? nullptr : dstates.data(), m.dstride = dstride.empty() ? nullptr : dstride.data();
        m.n_quad = (int32_t)quad_ptr.size() - 1, m.quad_ptr = quad_ptr.data(), m.quad_desc = quad_desc.data(), m.quad_par = quad_par.data();
        m.n_tab = (int32_t)tab_ptr.size() - 1, m.tab_ptr = tab_ptr.data(), m.tab_desc = tab_desc.data(), m.tab_par = tab_par.data();
        return m;
    }
};

static int run_model(const Model& md, unsigned long long seed, double& checksum) {
    int failures = 0;
    const lhvi_exact_t m = md.view();
    const int Nd = m.Nd, Nc = m.Nc;
    for (int64_t S : {1, 63, 64, 65, 130}) {
        unsigned long long s = seed + S;
        std::vector<int32_t> x_d((size_t)S * Nd);
        std::vector<double> x_c((size_t)S * Nc), a(S), b(S);
        const int64_t begin = md.M > S ? (md.M - S) / 2 : 0;          // implicit rows: wrap inside [0, M) by construction below
        const int64_t count = md.M - begin < S ? md.M - begin : S;   // the rows both modes share
        for (int64_t r = 0; r < S; ++r) {
            const int64_t cfg = (begin + r) % md.M;
            for (int d = 0; d < Nd; ++d) x_d[r * Nd + d] = (int32_t)((cfg / md.dstride[d]) % md.dstates[d]);
            for (int j = 0; j < Nc; ++j) x_c[r * Nc + j] = 20 * lcg(s) - 10;
        }
        failures += lhvi_hg_energy_host(&m, S, 0, Nd ? x_d.data() : nullptr, Nc ? x_c.data() : nullptr, a.data()) != LHVI_OK;
        failures += lhvi_hg_energy_host(&m, count, begin, nullptr, Nc ? x_c.data() : nullptr, b.data()) != LHVI_OK;
        for (int64_t r = 0; r < count; ++r) failures += !(a[r] == b[r]);
        for (int64_t r = 0; r < S; ++r) checksum += a[r];
        failures += lhvi_hg_energy_host(&m, 0, 0, nullptr, nullptr, nullptr) != LHVI_OK;
        failures += lhvi_hg_energy_host(&m, -1, 0, nullptr, x_c.data(), a.data()) != LHVI_E_ARG;
        failures += lhvi_hg_energy_host(&m, S, 0, nullptr, Nc ? x_c.data() : nullptr, nullptr) != LHVI_E_ARG;
        if (Nc) failures += lhvi_hg_energy_host(&m, S, 0, nullptr, nullptr, a.data()) != LHVI_E_ARG;
    }
    return failures;
}

static int run_argmax() {
    int failures = 0;
    const double inf = __builtin_huge_val(), nan = __builtin_nan("");
    int64_t idx;
    double val;
    for (int64_t n : {0, 1, 63, 64, 65, 257}) {
        std::vector<double> v(n);
        unsigned long long s = 7 + n;
        auto expect = [&](int64_t want, const char* what) {
            const int rc = lhvi_argmax_first_host(n, n ? v.data() : nullptr, &idx, &val);
            const bool ok = rc == LHVI_OK && idx == want && (want < 0 ? val != val : val == v[want] && std::signbit(val) == std::signbit(v[want]));
            if (!ok) std::printf("arg-max: n = %lld, %s: index %lld, expected %lld\n", (long long)n, what, (long long)idx, (long long)want);
            failures += !ok;
        };
        if (!n) {
            expect(-1, "empty");
            continue;
        }
        for (auto& x : v) x = lcg(s);
        v[n / 2] = 3.0, v[n - 1] = 3.0;
        expect(n / 2, "duplicated maximum");
        v[0] = 3.0;
        expect(0, "maximum at index 0");
        for (auto& x : v) x = -inf;
        expect(0, "all -inf");
        for (auto& x : v) x = nan;
        expect(-1, "all NaN");
        v[n - 1] = -inf;
        expect(n - 1, "NaN, then -inf");
        for (int64_t i = 0; i < n; ++i) v[i] = i % 2 ? 0.0 : -0.0;
        expect(0, "signed zeros");
    }
    failures += lhvi_argmax_first_host(-1, nullptr, &idx, &val) != LHVI_E_ARG;
    failures += lhvi_argmax_first_host(3, nullptr, &idx, &val) != LHVI_E_ARG;
    return failures;
}

int main() {
    int failures = 0;
    double checksum = 0.0;
    for (int Nc : {1, 7, 64}) {
        unsigned long long s = 1000 + Nc;
        Model md;
        md.dstates = {3, 2}, md.Nc = Nc;
        md.strides();
        std::vector<int32_t> all(Nc);
        for (int j = 0; j < Nc; ++j) all[j] = Nc - 1 - j;
        md.quad({}, all, 1, s);                                                   // dense, scope in reverse order
        md.quad({1, 3, 0, 1}, Nc > 1 ? std::vector<int32_t>{Nc - 1, 0} : std::vector<int32_t>{0}, 6, s);   // scope (1, 0): strides (3, 1)
        md.quad({0, 1}, {Nc / 2}, 3, s);
        md.table({1, 3, 0, 1}, 6, s);
        md.table({1, 1}, 2, s);
        failures += run_model(md, 11 * Nc, checksum);
    }
    {
        unsigned long long s = 2000;
        Model md;                                                                 // discrete only: a chain of 40 binary variables
        md.dstates.assign(40, 2);
        md.strides();
        for (int32_t i = 0; i + 1 < 40; ++i) md.table(i % 2 ? std::vector<int32_t>{i + 1, 2, i, 1} : std::vector<int32_t>{i, 2, i + 1, 1}, 4, s);
        failures += run_model(md, 40, checksum);
    }
    {
        unsigned long long s = 3000;
        Model md;                                                                 // Gaussian only: Nd = 0, M = 1
        md.Nc = 3;
        md.strides();
        md.quad({}, {2, 0, 1}, 1, s);
        md.quad({}, {1}, 1, s);
        failures += run_model(md, 3, checksum);
    }
    {
        Model md;                                                                 // more continuous variables than supported
        md.Nc = LHVI_EXACT_MAX_NC + 1;
        md.strides();
        const lhvi_exact_t m = md.view();
        double x[LHVI_EXACT_MAX_NC + 1] = {0}, out = 0;
        failures += lhvi_hg_energy_host(&m, 1, 0, nullptr, x, &out) != LHVI_E_UNSUPPORTED;
        failures += lhvi_hg_energy_host(nullptr, 1, 0, nullptr, x, &out) != LHVI_E_ARG;
    }
    failures += run_argmax();
    std::printf("hg_energy host twins under the sanitizers: checksum %.17g, %d failures\n", checksum, failures);
    return failures != 0;
}
