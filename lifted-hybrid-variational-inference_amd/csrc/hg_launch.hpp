// hg_launch.hpp -- the launch side the hybrid-Gaussian samplers share (gibbs.hip, ais.hip, pt.hip, gibbs_rb.hip; exact.hip takes
// the lane context, the lanes test and the launch shape): the device's lane context, where the reduced tables live, the checks
// of a model, the grid of a one-wavefront workgroup with a group of `lanes` lanes per item, and the workspace of a host twin.
// Nothing here is arithmetic of a kernel.
#pragma once
#include "common.hpp"
#include "gibbs.hpp"

namespace lhvi {
namespace hg {

constexpr size_t LDS_LIMIT = 64 * 1024;

// a lane of a group of `lanes` lanes on the device (exact::HostCtx is the host's one "lane")
struct DevCtx {
    int lane, lanes;
    __device__ __forceinline__ void sync() const { __syncthreads(); }
};

// disc_doubles of gibbs::ws_doubles: the reduced tables live in the workspace unless the model names a scratch row for them
LHVI_HD int lds_disc_doubles(const lhvi_gibbs_t& g) { return g.max_states + (g.table_scratch ? 0 : g.table_doubles); }

inline bool lanes_ok(int32_t lanes) { return lanes >= 1 && lanes <= WAVE && !(lanes & (lanes - 1)); }

// an exact model without M and dstride (lhvi_exact_configs asks for those on top): the flat model every sampler reads
inline int exact_check(const lhvi_exact_t* m) {
    if (!m || m->Nd < 0 || m->Nc < 0 || m->n_quad < 0 || m->n_tab < 0) return LHVI_E_ARG;
    if (m->Nd && !m->dstates) return LHVI_E_ARG;
    if (m->n_quad && (!m->quad_ptr || !m->quad_desc || !m->quad_par)) return LHVI_E_ARG;
    if (m->n_tab && (!m->tab_ptr || !m->tab_desc || !m->tab_par)) return LHVI_E_ARG;
    if (m->Nc > LHVI_EXACT_MAX_NC) return LHVI_E_UNSUPPORTED;
    return LHVI_OK;
}

// the counts of a lhvi_gibbs_t an entry point reads, and so tests: the annealed sampler reads neither num_burnin nor
// num_samples, the Rao-Blackwellised read-out only num_samples
enum Counts { ITS = 1, BURNIN = 2, SAMPLES = 4, ALL_COUNTS = ITS | BURNIN | SAMPLES };

inline int gibbs_check(const lhvi_gibbs_t* g, int counts) {
    if (!g) return LHVI_E_ARG;
    const int rc = exact_check(&g->ex);
    if (rc == LHVI_E_ARG) return rc;
    if (g->n_hyb < 0 || g->table_doubles < 0 || g->max_states < 1) return LHVI_E_ARG;
    if (((counts & ITS) && g->disc_block_its < 0) || ((counts & BURNIN) && g->num_burnin < 0) ||
        ((counts & SAMPLES) && g->num_samples < 0))
        return LHVI_E_ARG;
    if (g->ex.Nd && (!g->dstate_off || !g->vt_ptr || !g->vh_ptr)) return LHVI_E_ARG;
    if (g->ex.n_tab && !g->vt_fac) return LHVI_E_ARG;
    if (g->n_hyb && (!g->hyb_quad || !g->hyb_off || !g->vh_fac)) return LHVI_E_ARG;
    return rc;
}

// ---- a one-wavefront workgroup: WAVE / lanes groups, a workspace of ws_doubles (rounded up to even) per group ------------------
inline size_t wave_lds_bytes(int lanes, int ws_doubles) {
    return (size_t)(WAVE / lanes) * (((size_t)ws_doubles + 1) & ~(size_t)1) * sizeof(double);
}

struct WaveShape {
    int gpb;            // groups of a workgroup
    int64_t blocks;
    size_t lds;         // bytes
};
// the shape of `items` groups (0: nothing to launch, the workgroup is still sized); LHVI_E_UNSUPPORTED beyond the LDS of a
// workgroup or the blocks of a grid
inline int wave_shape(int64_t items, int lanes, int ws_doubles, WaveShape& s) {
    s.gpb = WAVE / lanes;
    s.lds = wave_lds_bytes(lanes, ws_doubles);
    s.blocks = (items + s.gpb - 1) / s.gpb;
    return s.lds > LDS_LIMIT || s.blocks > 0x7fffffff ? LHVI_E_UNSUPPORTED : LHVI_OK;
}

// ---- the workspace of a host twin: the model with its reduced tables inside the workspace, `doubles` doubles of its own --------
struct HostWork {
    lhvi_gibbs_t g;
    int dd;             // lds_disc_doubles(g)
    double* W = nullptr;
    explicit HostWork(const lhvi_gibbs_t& m) : g(m) {
        g.table_scratch = nullptr;
        dd = lds_disc_doubles(g);
    }
    HostWork(const HostWork&) = delete;
    HostWork& operator=(const HostWork&) = delete;
    ~HostWork() { delete[] W; }
    double* alloc(int doubles) { return W = new double[doubles]; }
    void digits_in(const gibbs::Workspace& w, const int32_t* x_d) const {
        for (int n = 0; n < g.ex.Nd; ++n) w.dig[n] = x_d[n];
    }
    void digits_out(const gibbs::Workspace& w, int32_t* x_d) const {
        for (int n = 0; n < g.ex.Nd; ++n) x_d[n] = w.dig[n];
    }
};

}  // namespace hg
}  // namespace lhvi
