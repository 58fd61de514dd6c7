/*
 * lhvi.h -- C ABI of the MI355X (gfx950) message-passing library `liblhvi.so`.
 *
 * This is the drop-in boundary of the hot path.  The reference
 * (leodd/Lifted-Hybrid-Variational-Inference) has no FFI: its boundary is the Python method surface
 * of the solver classes.  Each entry point below replaces the *body* of one of those methods and
 * cites it; the Python classes in lifted-hybrid-variational-inference_amd/lhvi/ keep the reference's
 * signatures and call these through ctypes (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - plain C, no torch / C++ types; every pointer inside the structs and every array argument is a
 *     DEVICE pointer (hipMalloc'd or a torch tensor's data_ptr()); the structs themselves live on the host.
 *   - all calls are asynchronous on the caller's `hipStream_t` (passed as void*; NULL = default stream),
 *     allocate nothing, keep no global state, and are re-entrant per stream.
 *   - return 0 on success, a negative LHVI_E_* code otherwise; nothing throws across the boundary.
 *   - all floating point is IEEE fp64, like the reference (Python floats).
 *   - a Gaussian message is two doubles (mu, var); var = NaN encodes the reference's `None`
 *     variance (pure linear term, GaBP.py:126), var = +Inf the vacuous message (GaBP.py:138).
 */
#ifndef LHVI_H
#define LHVI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LHVI_ABI_VERSION 32 /* 2: lhvi_graph_t gained edge_value / slot_var / hub_vars, lhvi_pbp_t the heavy / light descriptor lists, 128-byte descriptors;
                              * 3: lhvi_pbp_t gained var_lo / var_hi;  4: f2v_ticket;  5: prop_desc;  6: lhvi_vi_t gained obs_var, lhvi_gabp_plan_t;  7: lhvi_pbp_t gained pair_desc;
                              * 8: lhvi_pbp_t gained cq_desc / n_cq, lhvi_pbp_classify takes the particle state, lhvi_pbp_describe_cq; the colour
                              *    refinement calls take a method and return four result words; lhvi_vi_t gained var_N; lhvi_vi_opt_t, lhvi_vi_adam_run;
                              *    lhvi_gabp_plan_t.n_hub_rows, lhvi_gabp_graph_*; lhvi_pbp_t gained v2f_wide / v2f_narrow / v2f_hub / v2f_mid16 / v2f_mid32, prop_hub / prop_partial, resample_vars, small16_desc / small32_desc; 16 ticket words; lhvi_pbp_boundary_reduce;
                              * 9: lhvi_vi_t gained fac_list / n_cc / n_tiny / n_grp3 / n_grp6 / n_rest3 / n_rest6 / edge_axis; lhvi_color_first_members, lhvi_color_segment_sums, lhvi_pbp_halo_pack / _unpack; lhvi_gabp_plan_t.rec;
                              * 10: lhvi_pbp_t gained halo_off / halo_buf, LHVI_PBP_NO_UNIQ, edge_canon may name rows beyond E; lhvi_pbp_map_brent, lhvi_pbp_quad;
                              * 11: LHVI_PBP_V2F_RECORDS (v2f_wide as 8-word records), LHVI_PBP_WIDE_PAIRS, LHVI_PBP_SHARE_CUS;
                              * 12: lhvi_vi_map_bfgs;
                              * 13: lhvi_pbp_f2v selects the kernel families it launches with LHVI_PBP_F2V_* (replacing five bits that skipped kernels);
                              * 14: lhvi_mws_t, lhvi_mws_init / lhvi_mws_flips, lhvi_lbfgsb_host, lhvi_wall_clock_khz;
                              * 15: lhvi_exact_t, lhvi_exact_*, LHVI_E_NOT_PD;
                              * 16: lhvi_gibbs_t, lhvi_gibbs_*;
                              * 17: lhvi_gauss_exact_*, LHVI_GAUSS_EXACT_NB;
                              * 18: lhvi_mix_t, lhvi_mix_*, LHVI_MIX_*;
                              * 19: lhvi_gm_fit, lhvi_gm_fit_host, LHVI_GMFIT_MAX_K;
                              * 20: lhvi_npvi_opt_t, lhvi_npvi_*, LHVI_NPVI_MAX_K, LHVI_NPVI_MAX_SLOTS, LHVI_VI_GAUSSIAN_PDF;
                              * 21: lhvi_oneshot_*;
                              * 22: lhvi_pbp_var_fused64;
                              * 23: lhvi_gauss_chain_*, LHVI_GAUSS_CHAIN_MAX_BLOCK;
                              * 24: lhvi_gm_kl, lhvi_gm_kl_ws_doubles, lhvi_gm_kl_host, LHVI_GMKL_MAX_PANELS;
                              * 25: lhvi_hg_energy, lhvi_hg_energy_host, lhvi_argmax_first, lhvi_argmax_first_ws_bytes, lhvi_argmax_first_host;
                              * 26: lhvi_pbp_kl, lhvi_gm_kl_fn_host;
                              * 27: lhvi_exact_configs_at, lhvi_exact_config_at_host, lhvi_gibbs_rb_disc, lhvi_gibbs_rb_disc_host;
                              * 28: lhvi_gauss_chain_part_*, lhvi_gauss_chain_segments;
                              * 29: lhvi_ais_*, LHVI_AIS_REDUCE_OUT, LHVI_AIS_REDUCE_WS;
                              * 30: lhvi_pt_*;
                              * 31: lhvi_fgibbs_t, lhvi_fgibbs_*, LHVI_FGIBBS_MAX_STATES;
                              * 32: LHVI_PBP_NO_SPLIT_ROUND */
#define LHVI_MAX_ARITY 6

/* error codes */
#define LHVI_OK 0
#define LHVI_E_ARG (-1)        /* null pointer / negative size / inconsistent struct */
#define LHVI_E_LAUNCH (-2)     /* hipLaunch failed; see lhvi_last_hip_error() */
#define LHVI_E_UNSUPPORTED (-3)/* e.g. arity > LHVI_MAX_ARITY, n not supported */
#define LHVI_E_NODEVICE (-4)   /* no HIP device visible */
#define LHVI_E_NOT_PD (-5)     /* exact baseline, block Gibbs: a precision matrix is not positive definite */

/* potential kinds (pot_kind[]); parameter layouts are documented in csrc/potential.hpp */
#define LHVI_POT_GENERIC 0
#define LHVI_POT_TABLE 1
#define LHVI_POT_GAUSSIAN 2
#define LHVI_POT_QUADRATIC 3
#define LHVI_POT_HYBRID_QUADRATIC 4
#define LHVI_POT_LINEAR_GAUSSIAN 5
#define LHVI_POT_X2 6
#define LHVI_POT_XY 7
#define LHVI_POT_MLN 8
#define LHVI_POT_MLN_HARD 9
#define LHVI_POT_IMAGE_NODE 10
#define LHVI_POT_IMAGE_EDGE 11

/* Flat factor graph (ground or lifted).  Built by lhvi/flat.py from Graph / CompressedGraph objects
 * (Graph.py:137-209, CompressedGraphWithObs.py:178-271).  Edges are (factor, argument) incidences,
 * factor-major: the edges of factor f are fac_ptr[f] .. fac_ptr[f+1]-1 in argument order. */
typedef struct lhvi_graph {
    int32_t V, F, E, nnz;       /* nnz = length of var_edge (== E unless a lifted factor repeats a cluster) */
    const int32_t* fac_ptr;     /* [F+1] */
    const int32_t* edge_var;    /* [E] variable of edge e */
    const int32_t* edge_fac;    /* [E] factor of edge e */
    const int32_t* edge_canon;  /* [E] canonical edge of the (factor, variable) pair, or NULL if all e: the ROW of the message arrays that
                                 * holds the pair's messages.  An edge with edge_canon[e] != e is served by no kernel (its messages are
                                 * another row's).  (ABI 10) edge_canon[e] >= E is allowed for the particle sweep: a row of the caller's
                                 * v -> f array BEHIND the graph's own E rows, where a message computed elsewhere arrives in place
                                 * (the ghost edges of the owner-computes split, lhvi/dist.py::OwnerPlan.ghost_rows) */
    const int32_t* var_ptr;     /* [V+1] */
    const int32_t* var_edge;    /* [nnz] canonical edge ids in rv.nb order */
    const double* edge_count;   /* [E] lifted multiplicity rv.count[f], or NULL (ground: all 1) */
    const int32_t* fac_pot;     /* [F] index into the potential table */
    const double* var_value;    /* [V] evidence value, NaN = hidden */
    const int32_t* var_dom;     /* [V] domain id */
    const double* var_mult;     /* [V] |cluster| (len(rv.rvs)), or NULL */
    const double* fac_mult;     /* [F] |cluster| (len(f.factors)), or NULL */
    int32_t D;                  /* number of domains */
    const int32_t* dom_cont;    /* [D] 1 = continuous */
    const double* dom_lo;       /* [D] */
    const double* dom_hi;       /* [D] */
    const int32_t* dom_ptr;     /* [D+1] into dom_val */
    const double* dom_val;      /* discrete: the states; continuous: the integral points */
    /* optional denormalised copies that turn random gathers of the Gaussian sweep into contiguous reads (NULL = gather) */
    const double* edge_value;   /* [E] var_value[edge_var[e]] */
    const int32_t* slot_var;    /* [nnz] variable of CSR slot k (the v with var_ptr[v] <= k < var_ptr[v+1]) */
    /* optional: the variables with more than LHVI_HUB_DEGREE incident edges (template variables of relational models).
     * Kernels that walk a variable's CSR row give these a wavefront each; without the list (NULL) the hub kernels
     * scan all V variables for them (colour refinement, variational gather) or the row is walked by one thread
     * (Gaussian v2f / marginals, which keep the reference's summation order up to 512 edges and use the list beyond:
     * direct O(deg^2) leave-one-out sums). */
    const int32_t* hub_vars;    /* [n_hubs] ascending variable ids */
    int32_t n_hubs;
} lhvi_graph_t;
#define LHVI_HUB_DEGREE 64

/* Potential table: one row per distinct (potential object, scope domains). */
typedef struct lhvi_pots {
    int32_t P;
    const int32_t* kind;        /* [P] LHVI_POT_* */
    const int32_t* off;         /* [P+1] into param */
    const double* param;
    int32_t interpreted;        /* (ABI 10) how many rows are formulas the device evaluates by interpreting their bytecode: MLN rows without a
                                 * conditional-quadratic block (cq_off = 0) and MLN_HARD rows.  0 (every formula the reference ships): the
                                 * kernels that evaluate general potentials run the builds compiled without the interpreter.  A caller that
                                 * does not know passes -1 (treated as "some") */
} lhvi_pots_t;

int lhvi_version(void);
const char* lhvi_strerror(int code);
int lhvi_last_hip_error(void);       /* hipError_t of the last failed launch on this thread */
int lhvi_device_count(void);

/* ---- Gaussian BP (GaBP.py / GaLBP.py) ----------------------------------------------------------
 * f2v / v2f: [E][2] doubles (mu, var), indexed by edge id. */

/* all messages (mu,var) = (0,1): GaBP.py:142-145, GaLBP.py:154-157 */
int lhvi_gabp_init(const lhvi_graph_t* g, double* f2v, double* v2f, void* stream);
/* variable -> factor half sweep: GaBP.message_rv_to_f GaBP.py:20-35, GaLBP.py:21-39 */
int lhvi_gabp_v2f(const lhvi_graph_t* g, const double* f2v, double* v2f, void* stream);
/* factor -> variable half sweep: GaBP.message_f_to_rv GaBP.py:37-138, GaLBP.py:41-142 */
int lhvi_gabp_f2v(const lhvi_graph_t* g, const lhvi_pots_t* pots, const double* v2f, double* f2v, void* stream);
/* `iterations` flooding sweeps; the last one skips f2v: GaBP.run GaBP.py:140-169, GaLBP.run GaLBP.py:159-181 */
int lhvi_gabp_run(const lhvi_graph_t* g, const lhvi_pots_t* pots, double* f2v, double* v2f, int iterations, void* stream);
/* Pull form of the Gaussian sweep (one launch per iteration; replaces the pair lhvi_gabp_v2f + lhvi_gabp_f2v of
 * GaBP.run GaBP.py:152-165 / GaLBP.run GaLBP.py:160-177 for graphs whose factors are unary or pairwise -- every factor
 * GaBP.message_f_to_rv knows a closed form for, GaBP.py:37-138).  Messages live in variable-CSR ("slot") order,
 * slot k = (variable slot_var[k], edge var_edge[k]); the f -> v message of a slot is recomputed from the partner's
 * previous v -> f message instead of being stored.  The caller builds the plan once per graph:
 *   pslot[k]  slot of the partner argument's (canonical) edge when the partner variable is hidden; -1 - (partner variable)
 *             when it is observed (its value is read from var_value); unused for codes 0 and 3
 *   info[k]   4 * potential index + code; code 0 = unary factor, 1 / 2 = pairwise factor with this variable at
 *             position 0 / 1, 3 = any other arity (vacuous message (0, Inf), GaBP.py:138)
 *   count[k]  lifted graphs: rv.count[f] of the slot (GaLBP.py:24-34); NULL on a ground graph
 * Results equal the two-kernel path bit for bit (same expressions, same summation order). */
typedef struct lhvi_gabp_plan {
    const int32_t* pslot;
    const int32_t* info;
    const double* count;
    int32_t n_hub_rows;     /* variables with more than 512 incident edges (served by the wave-parallel hub kernel); 0 skips that
                             * launch, -1 = not counted (the kernel is launched whenever the graph lists hub_vars) */
    const int32_t* rec;     /* (ABI 9) [nnz][4] or NULL: per slot {pslot[k], info[k], position of k in its row | row length << 10 |
                             * variable hidden << 20 | row longer than 512 << 21, 0}: with it a slot needs no lookup through
                             * slot_var / var_ptr / var_value (GaBP.message_rv_to_f, GaBP.py:20-35, reads rv.nb and rv.value) */
    const double* pot_words;/* (ABI 9) [P][12], required with rec: per potential its first eleven parameters (zero padded; the closed forms
                             * of GaBP.message_f_to_rv, GaBP.py:37-138, read at most par[10]) and its kind as a double -- one record
                             * instead of the walk pots.kind -> pots.off -> pots.param */
    const int32_t* seg;     /* (ABI 9) [n_seg][2], required with rec: the slot order cut into segments [lo, hi) of whole rows -- the rows
                             * of at most 512 entries that start inside one window of 256 slots, up to the next row of more than 512
                             * entries (those belong to the hub kernel) -- one workgroup each.  BOUND: hi - lo <= 768 (the kernel
                             * stages a segment whole in LDS: window - 1 + 512 slots at most, window <= 256); a longer segment is
                             * left unswept */
    int32_t n_seg;
} lhvi_gabp_plan_t;
size_t lhvi_gabp_pull_workspace_bytes(const lhvi_graph_t* g);
/* one sweep: v_next[k] = message_rv_to_f of slot k given the f -> v messages implied by v_prev (first != 0: given the
 * initial messages (0, 1); v_prev is not read).  v_prev, v_next: [nnz][2], distinct. */
int lhvi_gabp_pull(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_gabp_plan_t* plan, const double* v_prev,
                   double* v_next, int first, void* stream);
/* lhvi_gabp_run through the pull form: same f2v [E][2] / v2f [E][2] (edge order) on return.  ws: caller-owned scratch of
 * lhvi_gabp_pull_workspace_bytes(g) bytes. */
int lhvi_gabp_run_pull(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_gabp_plan_t* plan, double* f2v, double* v2f,
                       int iterations, void* ws, size_t ws_bytes, void* stream);

/* The whole of GaBP.run + the marginals (lhvi_gabp_run_pull, then lhvi_gabp_marginals into mu_var [V][2]) recorded once as a
 * hipGraph over the caller's buffers and replayed with ONE launch: on template-sized graphs (BASELINE cfg 2: 20 k edges, 23
 * launches) the launches are the run.  The handle owns only the executable graph; rebuild it when the graph, the plan, a
 * buffer or `iterations` changes.  Evidence values are read from g->var_value at replay time, so new evidence in the same
 * buffer needs no rebuild. */
int lhvi_gabp_graph_create(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_gabp_plan_t* plan, double* f2v, double* v2f,
                           double* mu_var, int iterations, void* ws, size_t ws_bytes, void** handle_out);
int lhvi_gabp_graph_launch(void* handle, void* stream);
int lhvi_gabp_graph_destroy(void* handle);

/* per-variable product of incoming messages -> mu_var [V][2]; evidence rows get (value, 0):
 * GaBP.get_belief_params GaBP.py:187-200, GaLBP.map GaLBP.py:201-217 */
int lhvi_gabp_marginals(const lhvi_graph_t* g, const double* f2v, double* mu_var, void* stream);

/* utils.log_likelihood (utils.py:6-15) of a full assignment x [V] on flat arrays: out[0] = -sum_f log phi_f(x_scope),
 * or -inf when some factor is 0 at x (the reference's convention).  Discrete arguments are matched to their states. */
size_t lhvi_log_likelihood_workspace_bytes(const lhvi_graph_t* g);
int lhvi_log_likelihood(const lhvi_graph_t* g, const lhvi_pots_t* pots, const double* x, double* out, void* ws, size_t ws_bytes,
                        void* stream);

/* ---- Particle BP (EPBPLogVersion.py / HybridLBPLogVersion.py) -----------------------------------
 * Log messages are tabulated per edge: f2v [E][n+T] (first n = at the variable's particles, next T = at
 * the variable's integral points), v2f [E][n]. */

#define LHVI_PBP_EP 1u            /* proposal_approximation == 'EP' (else 'simple') */
#define LHVI_PBP_EPBP_DISCRETE 2u /* EPBP applies importance weights to discrete rvs too (EPBP.py:157) */
#define LHVI_PBP_SKIP_TERMS 16u   /* lhvi_pbp_f2v: the quadratic-family kernels skip their term loops -- results are
                                   * meaningless; isolates the per-edge load/store cost when tuning */
#define LHVI_PBP_LEAVE_ROOM 256u /* lhvi_pbp_f2v: the persistent kernels launch cus/8 workgroups fewer than fill the device, so that
                                   * another stream's kernels (RCCL's copy kernels of an overlapped exchange) find free slots at
                                   * any time instead of waiting for a persistent workgroup to retire.  Set by sharded runs. */
#define LHVI_PBP_CQ 512u         /* route MLN factors whose formula is conditionally quadratic (lhvi/expr.py::cq_block: a polynomial of degree <= 2
                                   * in the continuous arguments for every state of the discrete ones, e.g. x[0] * eq_op(x[1], x[2]),
                                   * Demo/Data/HMLN/GeneratorPaperPopularity.py:28-40) to the quadratic-family kernels instead of the
                                   * generic interpreter kernel: set it for lhvi_pbp_classify / _describe / _describe_cq AND lhvi_pbp_f2v */
#define LHVI_PBP_BOUNDARY_TOTALS 2048u /* sharded runs: a boundary variable's one listed row of s->recv holds the finished total over all ranks
                                        * (lhvi_pbp_boundary_reduce); without it the rows are the peers' sums and the kernels add them */
#define LHVI_PBP_NO_UNIQ 4096u   /* lhvi_pbp_resample_uniq with a resample_vars list: draw the particles only, leave uniq_out untouched (ghost variables of
                                  * the owner-computes split: their first-occurrence masks are read by nobody on this rank) */
#define LHVI_PBP_V2F_RECORDS 8192u /* v2f_wide holds one 8-word record per variable instead of its id: 0 variable  1 incident edges  2 particles (np)
                                    * 3 domain  4-7 the first four incident edges, in row order (a shorter row: its last edge repeated).  The
                                    * kernel then reaches the f -> v rows after ONE dependent load instead of three (id -> var_ptr / np -> var_edge) */
#define LHVI_PBP_WIDE_PAIRS 16384u /* lhvi_pbp_f2v: the pair_desc list always through the one-entry-per-wavefront kernel, also when n <= 32 would let
                                   * four / two entries share a wavefront (testing aid: the two kernels give the same bits) */
#define LHVI_PBP_SHARE_CUS 32768u /* lhvi_pbp_f2v: the persistent grids of the long kernels (heavy_desc, small16 / small32) take one workgroup per CU less than
                                   * fits, so that the kernels of the other families, launched by another call on ANOTHER stream (disjoint
                                   * rows of f2v), find a wave slot and LDS on every CU and run beside them */
#define LHVI_PBP_NO_GRID 128u    /* lhvi_pbp_f2v: integral points always by the direct form (one exponential per term), never by the
                                   * uniform-grid recurrence (testing / profiling aid) */
#define LHVI_PBP_NO_SPLIT_ROUND 16777216u /* lhvi_pbp_f2v: the heavy kernel's full particle round (64 target particles on 64 lanes) through the loop of
                                   * every other round (a record read per term) instead of the split round (the half-waves share a point pair
                                   * and split the chains: a record read per two terms).  Same bits either way (testing / profiling aid) */
#define LHVI_PBP_FUSED_RECORDS16 131072u /* lhvi_pbp_var_fused: desc holds SIXTEEN 32-bit words per variable (64-byte aligned) -- words 0-7 as documented
                                   * there, then 8 particles of the variable (s->np[v])  9 g->var_ptr[v]  10-15 its first six incident edges
                                   * (var_edge[var_ptr[v] + 0 .. 5]; unused ones 0) -- so that a variable's rows hang on one load behind its record */
/* lhvi_pbp_f2v: the kernel families a call launches, in this order.  No family bit set: every family.  A half sweep split over
 * several calls (lhvi/pbp.py::_launch_f2v) names each family in exactly one of them. */
#define LHVI_PBP_F2V_HEAVY 262144u   /* heavy_desc */
#define LHVI_PBP_F2V_SMALL 524288u   /* small16_desc and small32_desc */
#define LHVI_PBP_F2V_PAIR 1048576u   /* pair_desc (through the pair_small or the pair kernel), or light_desc when there is no pair list */
#define LHVI_PBP_F2V_FAST 2097152u   /* fast_edges, or every edge when the caller gives no work lists */
#define LHVI_PBP_F2V_CQ 4194304u     /* cq_desc */
#define LHVI_PBP_F2V_GENERIC 8388608u /* the generic-potential kernel: generic_edges, or every edge when the caller gives no work lists */
#define LHVI_PBP_F2V_ALL (LHVI_PBP_F2V_HEAVY | LHVI_PBP_F2V_SMALL | LHVI_PBP_F2V_PAIR | LHVI_PBP_F2V_FAST | LHVI_PBP_F2V_CQ | LHVI_PBP_F2V_GENERIC)
#define LHVI_PBP_POW2_GROUPS 65536u /* lhvi_pbp_f2v: the small16 / small32 lists always through lane groups of 16 / 32 lanes (four / two edges per
                                   * wavefront), also when s->n would let up to eight edges share one (narrower groups, two particles per lane; testing / profiling aid) */

typedef struct lhvi_pbp {
    int32_t n;                  /* particle slots per variable */
    int32_t T;                  /* integral-point slots per variable (max over domains) */
    uint32_t flags;
    double var_threshold;       /* EPBP 3, HybridLBP 5 */
    double max_log_value;       /* 700 */
    const double* particles;    /* [V][n] current sample */
    const double* old_particles;/* [V][n] sample the v2f messages were computed on */
    const int32_t* np;          /* [V] valid particles: n (continuous hidden), #states (discrete hidden), 0 (observed) */
    const uint8_t* uniq;        /* [V][n] 1 = first occurrence of that value among the variable's particles */
    const double* q;            /* [V][2] proposal (mu, var) */
    /* optional work lists for lhvi_pbp_f2v (from lhvi_pbp_classify); NULL = classify every edge on the fly */
    const int32_t* fast_edges;  /* [n_fast] edges whose log phi is quadratic in the target (LDS-staged kernel) */
    int32_t n_fast;
    const int32_t* generic_edges; /* [n_generic] all other edges with a hidden target */
    int32_t n_generic;
    int32_t generic_pts_log2;   /* ceil(log2(max output points of a generic edge)), clamped to [0, 6]: lanes per edge */
    const void* fast_desc;      /* [n_fast][LHVI_PBP_DESC_BYTES] from lhvi_pbp_describe, or NULL (built on the fly) */
    const void* heavy_desc;     /* [n_heavy][LHVI_PBP_DESC_BYTES] descriptors of the edges served by the specialised kernel:
                                 * class 1, constant x^2 coefficient (kind != HYBRID_QUADRATIC), nj <= 64, and either np + T <= 128 or a uniform
                                 * grid (word 15) of T <= 128 points with nj >= 24 and np <= 128; disjoint from fast_edges */
    int32_t n_heavy;
    const void* light_desc;     /* [n_light] descriptors with word 14 != 0: HybridQuadratic edges with a binary (or observed)
                                 * discrete side, served by their own kernel; disjoint from fast_edges and heavy_desc */
    int32_t n_light;
    /* edge-sharded runs only (all NULL on a single GPU).  A boundary variable (edges on several ranks) owns one row per
     * peer rank in the exchange buffers; row r of the send buffer and row r of the receive buffer belong to the same
     * (variable, peer) because both ends list their shared variables in ascending global id.  A row of a continuous
     * variable is n + 2 doubles: [sum over the sender's local edges of count * f2v[e][j], j < n | sum of count/var, sum of
     * count*mu/var of its sites]; a row of a discrete variable is np doubles (the sums at its states; it has no proposal).
     * Rows are packed back to back, peer-major; brow_off gives each row's element offset in either buffer. */
    const int32_t* bslot;       /* [V] index of the variable in the boundary list, -1 for interior / observed variables */
    const int32_t* brow_ptr;    /* [nb+1] CSR over exchange rows per boundary variable, rows in ascending peer rank */
    const int64_t* brow_off;    /* [rows] element offset of the row (the same offsets address the send and the receive buffer) */
    const int32_t* brow_peer;   /* [rows] peer rank of each listed row */
    const double* recv;         /* received rows of this sweep, packed like the send buffer */
    int32_t rank;               /* this rank (fixes the summation order of the proposals so that all replicas agree bit for bit) */
    const double* var_degree;   /* [V] global number of incoming messages (sum of counts over ALL ranks' edges) */
    /* variable range of the per-variable entry points (lhvi_pbp_v2f, _proposal, _proposal_partial, _proposal_finish,
     * _resample_uniq): they work on [var_lo, var_hi) when var_hi > var_lo, on every variable when both are 0.  A sharded
     * run numbers its interior variables first and sweeps them while the boundary rows are in flight. */
    int32_t var_lo, var_hi;
    /* optional: LHVI_PBP_TICKET_WORDS 32-bit words of device memory for lhvi_pbp_f2v.  When set, the persistent heavy kernel
     * cuts its work list into one contiguous range per XCD (each XCD has its own L2) and hands each range out in chunks of
     * consecutive entries through an atomic counter, which the call resets on its stream: a wave's descriptors are then
     * neighbours in memory, and a workgroup dispatched late finds less left to do instead of owing a full static share
     * (13.4 -> 12.0 ms per launch on the 10 M-edge benchmark).  NULL: every wave strides over the list.  Words 8 and 9 come
     * back with the launch's grid-recurrence statistics (LHVI_PBP_TICKET_COUNTERS). */
    uint32_t* f2v_ticket;
    /* optional, lhvi_pbp_proposal only: one record of eight 32-bit words per hidden CONTINUOUS variable, host-built --
     *   0 variable   1 degree (entries of its var_edge row)   2 grid base in dom_val   3 T   4-7 the first four incident
     *   edges var_edge[var_ptr[v] + k] (unused: repeat the first) --
     * so that a wave starts from one scalar load instead of the chain var_value / var_dom -> dom_ptr / var_ptr -> var_edge,
     * and no wave is launched for an observed or discrete variable.  NULL: the kernel walks the graph arrays. */
    const int32_t* prop_desc;
    int32_t n_prop_desc;
    /* optional, lhvi_pbp_f2v only: the light edges again, one LHVI_PBP_DESC_BYTES-byte record per FACTOR (both edges of a
     * HybridQuadratic(1 discrete, 1 continuous) factor share its per-state coefficients), host-built from light_desc --
     *   words 0 e_c  1 e_d  (edge to the continuous / discrete variable, -1 = that variable is observed)   2 v_c  3 v_d
     *   4 np_c  5 T  6 grid base  7 live states of v_d   8-9 val_c  10-11 val_d (doubles, NaN = hidden)
     *   12-23 A0 b0 c0 A1 b1 c1 (doubles)   24 / 25 rows of v2f with the discrete / continuous variable's message
     * When set, one kernel over these records replaces the light kernel (twice the bytes in flight per wave, half the
     * descriptor traffic; same messages bit for bit).  NULL: light_desc is used.  With n <= 16 / n <= 32 particles four / two records
     * share a wavefront (same bits again; LHVI_PBP_WIDE_PAIRS keeps one record per wavefront). */
    const void* pair_desc;
    int32_t n_pair;
    /* optional, lhvi_pbp_f2v only: [n_cq][2 * LHVI_PBP_DESC_BYTES] records from lhvi_pbp_describe_cq for the edges of class 4
     * (conditionally quadratic factors with a hidden discrete and a hidden continuous partner, or two hidden continuous
     * partners of a discrete target); served by their own kernel. */
    const void* cq_desc;
    int32_t n_cq;
    /* optional, lhvi_pbp_v2f only (single-GPU runs: not with bslot or a variable range): the hidden variables split by particle
     * count -- v2f_wide: more than four particles, one wavefront each; v2f_narrow: at most four (binary variables, boolean
     * atoms), sixteen per wavefront.  Both or neither; together they must list every hidden variable once.  NULL: one wavefront
     * per variable of the range.  With LHVI_PBP_V2F_RECORDS in flags, v2f_wide is an array of 8-word records (see the flag). */
    const int32_t* v2f_wide;
    int32_t n_v2f_wide;
    const int32_t* v2f_narrow;
    int32_t n_v2f_narrow;
    const int32_t* v2f_hub;     /* optional third part of the split: variables with 5..64 particles and more than 64 incident edges
                                 * (template variables of relational models), a workgroup each; such variables are then NOT in
                                 * v2f_wide */
    int32_t n_v2f_hub;
    const int32_t* v2f_mid16;   /* optional further parts of the split (with v2f_wide / v2f_narrow): variables with 5-16 and with 17-32 particles */
    int32_t n_v2f_mid16;        /* and at most 64 incident edges, four / two per wavefront; such variables are then NOT in v2f_wide */
    const int32_t* v2f_mid32;
    int32_t n_v2f_mid32;
    /* optional, lhvi_pbp_proposal with prop_desc only: variables with long rows (template variables of relational models) listed in
     * prop_desc by SLICES of their var_edge row, a wavefront per slice instead of one per variable.  A slice record has word 1 =
     * -(entries in the slice), word 4 = position of its first entry in the row, word 5 = its slot in prop_partial (words 6-7
     * unused); prop_hub lists each such variable once as (variable, first slot, slices, 0) with its slices in consecutive slots in
     * row order, and a second small kernel adds the slices' information-form sums in that order.  prop_partial: [slots][2]
     * doubles of scratch. */
    const int32_t* prop_hub;
    int32_t n_prop_hub;
    double* prop_partial;
    /* optional, lhvi_pbp_resample_uniq only (n <= 64, not with a variable range): one record of eight 32-bit words per hidden
     * CONTINUOUS variable -- 0 variable   1 its particle count np   2-3 dom_lo   4-5 dom_hi (doubles)   6-7 unused.  The call then
     * draws for these only, two per wavefront, and touches no other row of particles_out / uniq_out -- the rows of discrete and
     * observed variables never change, so the caller fills them once (one call without the list per particle buffer).  NULL:
     * every variable of the range, neighbours two by two.  The draws do not depend on which form is used. */
    const int32_t* resample_vars;
    int32_t n_resample_vars;
    /* optional, lhvi_pbp_f2v only: heavy-class descriptors (same rows as heavy_desc would hold, and NOT in heavy_desc) of the edges
     * whose target AND partner have at most 16 / at most 32 particles (nj <= 16 and np <= 16; the rest with nj <= 32 and np <= 32);
     * any number of integral points.  Served four / two edges per wavefront by their own kernel -- six / ten / eight for the small16
     * list when s->n <= 10 / 12 / 16, six / five / four for the small32 list when s->n <= 20 / 24 / 32 (lane groups as narrow as
     * the particle count allows, two particles per lane beyond 10; no variable may then hold more than s->n particles;
     * LHVI_PBP_POW2_GROUPS keeps four / two): with the particle counts of the
     * reference's demos (10-20) an edge per wavefront is bound by its own latencies, not by its terms.  Integral points on a uniform
     * grid (descriptor word 15) are tabulated by the recurrence along the grid inside the lane group, like the heavy kernel's (to
     * rounding the same values as the direct form; LHVI_PBP_NO_GRID forces that one).  NULL: such edges stay in heavy_desc.  Family
     * LHVI_PBP_F2V_SMALL. */
    const void* small16_desc;
    int32_t n_small16;
    const void* small32_desc;
    int32_t n_small32;
    /* (ABI 10) optional, lhvi_pbp_v2f only -- the owner-computes split of a sharded sweep (lhvi/dist.py::OwnerRunner): halo_off [E],
     * per edge the element offset in halo_buf that its v -> f row is ALSO written to as it is formed (the send buffer of the
     * sweep's all_to_all: no pack pass re-reads the rows), or -1.  NULL: no copies. */
    const int64_t* halo_off;
    double* halo_buf;
} lhvi_pbp_t;

#define LHVI_PBP_DESC_BYTES 128
#define LHVI_PBP_TICKET_WORDS 16     /* the work counters, then two words of statistics of the last lhvi_pbp_f2v call */
#define LHVI_PBP_TICKET_COUNTERS 8   /* words 0-7: one work counter per XCD range; word 8: heavy edges whose integral points were tabulated by the
                                      * uniform-grid recurrence; word 9: eligible edges that failed its range guard and took the direct form */
/* static per-edge descriptors of the fast work list: lets the persistent f2v kernels fetch everything about an edge with
 * scalar loads.  Must be rebuilt when np / the graph / the potentials change.  Layout (32-bit words unless noted):
 *   0 edge   1 target variable   2 partner variable   3 partner's canonical edge   4 class (lhvi_pbp_classify)
 *   5 target position   6 potential kind   7 nj = partner particle count (1 = observed)   8 np = target particle count
 *   9 T = target integral points   10 grid base in dom_val   11 offset into pots.param   12-13 partner value (double,
 *   NaN = hidden)   14 light-kernel type (0 none, 1 continuous target / discrete partner, 2 discrete target /
 *   continuous partner)   15 1 = the target's integral points are a uniform grid (x_t = x0 + t h to a few ulp)   16-27 six doubles: the potential resolved for this edge -- class 1 with a constant
 *   x^2 coefficient: log phi = kx x^2 + (ay y + by) y + c + (axy y + bx) x as (ay, by, c, axy, bx, kx), x = target;
 *   light edges: (A_0, b_0, c_0, A_1, b_1, c_1) of the discrete side's two points   28-31 two doubles (x0, h) of a uniform grid.
 * The host builds heavy_desc / light_desc / fast_desc by splitting the rows on words 4, 6, 7, 8 + 9 and 14. */
int lhvi_pbp_describe(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_pbp_t* s, const int32_t* edges, int32_t count,
                      void* desc_out, void* stream);
/* descriptors of the class-4 edges (2 * LHVI_PBP_DESC_BYTES each).  Layout (32-bit words unless noted):
 *   0 edge   1 target variable   2 type (1 = continuous target, hidden discrete partner z + continuous partner y: the message is
 *   log sum_s sum_j exp(a_sj + b_sj x + k_s x^2); 2 = discrete target, two hidden continuous partners x, y: S sums over the n^2
 *   joint particles)   3 S = coefficient sets (states of z / of the target)   4 np   5 T   6 grid base   7 variable of y
 *   8 v2f row of y   9 particles of y (1 = observed or absent)   10 variable of z (type 2: of x)   11 v2f row of z (type 1: -1 =
 *   none; type 2: of x)   12 states of z (type 2: particles of x)   14-15 value of an observed y (double, NaN = hidden)
 *   16-63 S x six doubles (ay, by, c, axy, bx, kx): log phi_s = kx x^2 + (ay y + by) y + c + (axy y + bx) x
 * EPBP.message_f_to_rv on such factors: EPBP.py:176-194 with MLNPotential.get MLNPotential.py:36-37. */
int lhvi_pbp_describe_cq(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_pbp_t* s, const int32_t* edges, int32_t count,
                         void* desc_out, void* stream);
/* Batched queries (extension; EPBP.belief_rv EPBP:196-202 for every variable at once).  Tabulate the messages at n query
 * points per variable by running lhvi_pbp_f2v with s->particles = the query points [V][n] and s->old_particles = the
 * current sample into a scratch f2v buffer, then
 *   lhvi_pbp_var_sum      out[v][j] = sum over the variable's edges of count * f2v[e][j]   (the log-belief at point j)
 *   lhvi_pbp_domain_grid  x[v][:] = uniform n-point grid on the domain (discrete: the states)
 *   lhvi_pbp_refine_grid  best[v] / best_val[v] = argmax point and value of logb[v][:]; x[v][:] := uniform grid on the
 *                         bracket around it (one step of the batched MAP search, EPBP.map EPBP:377-394 uses fminbound) */
int lhvi_pbp_var_sum(const lhvi_graph_t* g, const lhvi_pbp_t* s, const double* f2v, double* out, void* stream);
int lhvi_pbp_domain_grid(const lhvi_graph_t* g, const lhvi_pbp_t* s, double* x, void* stream);
int lhvi_pbp_refine_grid(const lhvi_graph_t* g, const lhvi_pbp_t* s, const double* logb, double* x, double* best, double* best_val,
                         void* stream);
/* test hook: y[i] = the f2v kernel's exp(x[i]) */
int lhvi_debug_exp(const double* x, double* y, int64_t n, void* stream);
/* test hook: y[i] = exp(x[i] + c[i]) through the accumulating form the f2v term loop uses (c = the per-point constant) */
int lhvi_debug_exp_acc(const double* x, const double* c, double* y, int64_t n, void* stream);
/* the same value through the floor form of the term loop (heavy and cq kernels: records pre-divided by the table step, floor by a
 * round-down addition, csrc/fastmath.hpp::exp_accumulate_floor) */
int lhvi_debug_exp_acc_floor(const double* x, const double* c, double* y, int64_t n, void* stream);
/* test hook: y[i] = log(x[i]), x > 0; which = 0 the table-driven log of the f2v epilogue, 1 the series log */
int lhvi_debug_log(const double* x, double* y, int64_t n, int32_t which, void* stream);

/* edge_class[e]: 0 = no message (observed target / alias edge), 1|2 = quadratic-family (continuous | discrete target),
 * 3 = generic potential, 4 = conditionally quadratic with two hidden partners (only with LHVI_PBP_CQ in s->flags; `s` may be
 * NULL otherwise -- it is read for flags, n and np only).  Static per (graph, evidence, potentials, particle counts); the
 * host turns it into the work lists above. */
int lhvi_pbp_classify(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_pbp_t* s, uint8_t* edge_class, void* stream);

/* uniq[v][j] = no i<j with particles[v][i] == particles[v][j]  (dict-key collapse, EPBP.py:236-242) */
int lhvi_pbp_uniq(const lhvi_graph_t* g, int32_t n, const double* particles, const int32_t* np, uint8_t* uniq, void* stream);
/* EPBP.message_rv_to_f + important_weight + log_message_balance: EPBP.py:156-174,204-215; HLBP.py:173-191,225-236 */
int lhvi_pbp_v2f(const lhvi_graph_t* g, const lhvi_pbp_t* s, const double* f2v, double* v2f, void* stream);
/* EPBP.message_f_to_rv at the new particles + integral points: EPBP.py:176-194,275-285; HLBP.py:193-215.
 * One kernel per work list of `s` on `stream`, in the order of the LHVI_PBP_F2V_* families, which select among them.  With
 * s->f2v_ticket set the heavy family first resets those words on `stream` (a memset). */
int lhvi_pbp_f2v(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_pbp_t* s, const double* v2f, double* f2v, void* stream);
/* update_proposal (sites eta [E][2] in/out, q [V][2] in/out): EPBP.py:83-154; HLBP.py:100-171 */
int lhvi_pbp_proposal(const lhvi_graph_t* g, const lhvi_pbp_t* s, const double* f2v, double* eta, double* q, void* stream);
/* Sharded form of lhvi_pbp_proposal: `partial` updates the local sites and writes, per variable, the information-form sum
 * over its LOCAL edges ph[v] = (sum c/var, sum c*mu/var); `boundary_pack` writes every boundary variable's row into each of
 * its slots of the send buffer; after the all_to_all, lhvi_pbp_v2f reads the received rows through s->recv, and `finish`
 * forms q[v] from ph[v] plus the received sums in rank order -- together they equal lhvi_pbp_proposal on the whole graph. */
int lhvi_pbp_proposal_partial(const lhvi_graph_t* g, const lhvi_pbp_t* s, const double* f2v, double* eta, double* ph, void* stream);
int lhvi_pbp_proposal_finish(const lhvi_graph_t* g, const lhvi_pbp_t* s, const double* ph, double* q, void* stream);
int lhvi_pbp_boundary_pack(const lhvi_graph_t* g, const lhvi_pbp_t* s, const double* f2v, const double* ph, int32_t nb,
                           const int32_t* bvars, double* send, void* stream);
/* Reduce-to-owner form of the exchange (a boundary variable present on k ranks costs 2 (k - 1) rows instead of k (k - 1)): every
 * such variable has one owner among its ranks; the others send it their row, the owner adds the rows in ascending rank order
 * (its own at its position -- the order lhvi_pbp_v2f / _proposal_finish use for the all-to-all form, so both forms give the same
 * bits) and sends the total back.  This call is the owner's sum: item i adds the `width[i]` doubles at in + src_off[r],
 * r in [src_ptr[i], src_ptr[i+1]), and stores the total at out + dst_off[r], r in [dst_ptr[i], dst_ptr[i+1]).  Afterwards
 * lhvi_pbp_v2f / _proposal_finish run with LHVI_PBP_BOUNDARY_TOTALS: each boundary variable lists ONE row (brow_ptr / brow_off into
 * s->recv) holding the total over all ranks. */
int lhvi_pbp_boundary_reduce(int32_t n_items, const int32_t* width, const int32_t* src_ptr, const int64_t* src_off,
                             const int32_t* dst_ptr, const int64_t* dst_off, const double* in, double* out, void* stream);
/* initial_proposal: q=(0,5), sites (0, 5*deg): EPBP.py:72-81; HLBP.py:89-98 */
int lhvi_pbp_init(const lhvi_graph_t* g, const lhvi_pbp_t* s, double* eta, double* q, double* f2v, double* v2f, void* stream);
/* generate_sample with a counter-based device RNG: EPBP.py:61-70.  Philox4x32-10, key = seed, counter = (variable gid, block,
 * iteration); a block yields two normals by Box-Muller, particle j takes block (j & 31) | (j >> 6 << 5) and the cosine (bit 5 of j
 * clear) or the sine.  var_gid may be NULL (gid = local index).  Parity runs inject host particles instead. */
int lhvi_pbp_resample(const lhvi_graph_t* g, const lhvi_pbp_t* s, const int64_t* var_gid, uint64_t seed, uint32_t iteration, double* particles_out, void* stream);
/* message_f_to_rv(x, f, rv, sample) for explicit (edge, point) pairs: qedge [nq] edge ids, x [nq][npts], out [nq][npts].
 * HybridLBP.belief_rv_query (HLBP.py:313-317) sums these over a ground variable's factors. */
int lhvi_pbp_edge_points(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_pbp_t* s, const double* v2f,
                         int32_t nq, const int32_t* qedge, int32_t npts, const double* x, double* out, void* stream);
/* lhvi_pbp_resample followed by lhvi_pbp_uniq on the fresh particles: those two calls themselves when n > 64 (both over the
 * variables [var_lo, var_hi) when s names a range, as lhvi_pbp_resample alone does); for n <= 64 one fused
 * pass that draws from the same Philox blocks but takes the table logarithm and its own square root where lhvi_pbp_resample takes
 * the series logarithm -- its particles agree with lhvi_pbp_resample's to rounding (about 3 % of the drawn values differ in the
 * last bits; clipped ones are the bound in both), not to the bit, and its mask is the exact mask of its own particles
 * (tests/test_gpu_pbp_sampler.py). */
int lhvi_pbp_resample_uniq(const lhvi_graph_t* g, const lhvi_pbp_t* s, const int64_t* var_gid, uint64_t seed, uint32_t iteration,
                           double* particles_out, uint8_t* uniq_out, void* stream);
/* belief_rv(x) = sum_f message_f_to_rv(x, f, rv, sample) at arbitrary points: EPBP.py:196-202; HLBP.py:313-317.
 * qvar [nq] variable ids, x [nq][npts], out [nq][npts]; uses s->particles as the partners' sample. */
int lhvi_pbp_belief_points(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_pbp_t* s, const double* v2f,
                           int32_t nq, const int32_t* qvar, int32_t npts, const double* x, double* out, void* stream);
/* map(rv) of nq query rows in ONE launch: EPBP.map EPBP.py:377-394, HybridLBP.map HLBP.py:405-424.  Every continuous row runs
 * scipy.optimize.fminbound (Brent's bounded minimiser, the reference's call with its defaults xtol = 1e-5, maxfun = 500) on
 * f(x) = -belief_rv(x) over the row's domain [dom_lo, dom_hi], decision for decision, in IEEE double without contraction; a
 * discrete row returns its first state with the largest belief.  row_var [nq]: the variable of g whose domain the row searches.
 * qptr == NULL: the row's belief is belief_rv of row_var[i] (its incident edges, count-weighted on a lifted graph).
 * qptr [nq + 1] / qedge / qmult: the row's belief is sum_k qmult[k] * message_f_to_rv(x, edge qedge[k]) for k in
 * [qptr[i], qptr[i+1]) -- a GROUND variable's factors on the lifted graph (belief_rv_query HLBP.py:313-317).
 * xout [nq] the minimiser, fout [nq] (optional) the log-belief there, nfev [nq] (optional) function evaluations used. */
/* The three per-variable steps of a sweep fused for hidden continuous variables with few particles (s->n <= 32: the particle
 * counts of the reference's demos): message_rv_to_f + log_message_balance (EPBP.py:165-174,204-215; HLBP.py:182-191), then
 * update_proposal (EPBP.py:83-154; HLBP.py:100-171), then generate_sample with the counter-based sampler + the first-occurrence
 * mask (EPBP.py:61-70) -- one pass over a variable's incident f -> v rows instead of three launches' worth.  Same bits as
 * lhvi_pbp_v2f + lhvi_pbp_proposal + lhvi_pbp_resample_uniq on those variables (the caller runs those three on the others).
 * desc: records of eight 32-bit words per variable -- 0 variable  1 incident edges (<= 64)  2 grid base in dom_val  3 T
 * 4-5 dom_lo  6-7 dom_hi (doubles) -- in three blocks: n16 variables with np <= 16 and T <= 32, then n32_t32 with 16 < np <= 32
 * and T <= 32, then n32_t64 with np <= 32 and 32 < T <= 64.  Reads s->particles / s->uniq / s->q (the current sample and
 * proposal), writes v2f rows, eta, q, particles_out (must not be s->particles) and uniq_out rows of the listed variables. */
int lhvi_pbp_var_fused(const lhvi_graph_t* g, const lhvi_pbp_t* s, const double* f2v, double* v2f, double* eta, double* q,
                       const int64_t* var_gid, uint64_t seed, uint32_t iteration, double* particles_out, uint8_t* uniq_out,
                       const int32_t* desc, int32_t n16, int32_t n32_t32, int32_t n32_t64, void* stream);
/* lhvi_pbp_var_fused for 32 < s->n <= 64 particles: one variable per wavefront, lane = particle.  Same bits as lhvi_pbp_v2f +
 * lhvi_pbp_proposal + lhvi_pbp_resample_uniq on the listed variables.  desc: records of SIXTEEN 32-bit words per variable whatever
 * LHVI_PBP_FUSED_RECORDS16 says (words 0-7 as above, 8 particles  9 var_ptr[v]  10-15 the first six incident edges), in two blocks:
 * n64_t32 variables with T <= 32, then n64_t64 with 32 < T <= 64.  Everything else as for lhvi_pbp_var_fused. */
int lhvi_pbp_var_fused64(const lhvi_graph_t* g, const lhvi_pbp_t* s, const double* f2v, double* v2f, double* eta, double* q,
                         const int64_t* var_gid, uint64_t seed, uint32_t iteration, double* particles_out, uint8_t* uniq_out,
                         const int32_t* desc, int32_t n64_t32, int32_t n64_t64, void* stream);
/* The normaliser of EPBP.belief for nq query rows in ONE launch: EPBP.py:325-328 calls scipy.integrate.quad on e ** belief_rv over
 * [lo, hi] (= the domain widened by 20 on both sides).  A thread per row runs QUADPACK's 21-point Gauss-Kronrod rule (dqk21 and
 * its error estimate) inside dqage's globally adaptive bisection (at most 50 intervals) until the summed error estimate meets
 * max(epsabs, epsrel |z|); scipy's quad (dqagse) adds an extrapolation step to the same rule and bisection, so both lie within
 * the tolerance of the integral (scipy's default request: 1.49e-8 for both).  Rows as for lhvi_pbp_map_brent.  z [nq] the integral
 * (NaN where e ** belief_rv overflowed: the reference raises OverflowError there), abserr [nq] (optional) the error estimate,
 * status [nq] (optional) 0 converged / 1 interval limit / 3 overflow. */
int lhvi_pbp_quad(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_pbp_t* s, const double* v2f, int64_t nq,
                  const int32_t* row_var, const int64_t* qptr, const int32_t* qedge, const double* qmult, const double* lo,
                  const double* hi, double epsabs, double epsrel, double* z, double* abserr, int32_t* status, void* stream);
int lhvi_pbp_map_brent(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_pbp_t* s, const double* v2f, int64_t nq,
                       const int32_t* row_var, const int64_t* qptr, const int32_t* qedge, const double* qmult, double xtol,
                       int32_t maxfun, double* xout, double* fout, int32_t* nfev, void* stream);
/* KL(p[r] || belief of query row r) for nq rows in ONE launch: the drivers' kl_err = kl_continuous_logpdf(log_p, log_q) with an EPBP /
 * HybridLBP belief as log_q (osi/hybrid_mln_experiment.py:326-338, osi/utils.py:724-729) and p a scalar Gaussian mixture
 * (wp, mup, varp)[r][0 .. Kp).  Rows exactly as for lhvi_pbp_quad (row_var, or the (edge, multiplicity) lists qptr / qedge / qmult).
 * The method is lhvi_gm_kl's below, unchanged -- the range and the panels from p alone, pass 1, left-to-right depth-first bisection,
 * the two guards, the status bits, neval -- with log q(x) = belief_rv(x) - logz[r] in the place of the second mixture's log density
 * (logz: log of the belief's normaliser, e.g. of lhvi_pbp_quad's z).  One wavefront per row, the lanes on the quadrature nodes, the
 * panel list and the stack in LDS (csrc/gmkl_dev.hpp); no atomics: a row's bits depend neither on nq, nor on its position, nor on the
 * run.  A row whose logz is not finite, whose variable is observed, discrete or not a variable of g, or whose p is invalid (as for
 * lhvi_gm_kl) gets kl = abserr = NaN and status bit 2; the other rows are unaffected.  abserr, status and neval may be NULL.
 * LHVI_E_ARG: nq < 1, Kp < 1, a NULL required pointer, epsabs or epsrel negative or NaN.  docs/kernels_pbkl.md. */
int lhvi_pbp_kl(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_pbp_t* s, const double* v2f, int64_t nq,
                const int32_t* row_var, const int64_t* qptr, const int32_t* qedge, const double* qmult, const double* logz,
                int32_t Kp, const double* wp, const double* mup, const double* varp, const double* a, const double* b,
                double epsabs, double epsrel, double* kl, double* abserr, int32_t* status, int32_t* neval, void* stream);

/* ---- owner-computes exchange of the edge-sharded sweep (lhvi/dist.py::OwnerRunner; csrc/halo.hip) ----------------------------
 * The reference is one process; these two calls move its `message[(rv, f)]` tables (EPBPLogVersion.py:250-258) and proposals
 * `q[rv]` (EPBPLogVersion.py:83-101) of the factors cut by a variable partition between ranks: pack fills the send buffer of the
 * sweep's one all_to_all, unpack scatters the receive buffer.  Row i: `row_width[i]` doubles of v2f row `row_edge[i]` (v2f is
 * [E][n]) at element offset `row_off[i]` of the buffer; proposal i: the two doubles of q row `q_var[i]` at `q_off[i]`. */
int lhvi_pbp_halo_pack(const double* v2f, int32_t n, int32_t n_rows, const int32_t* row_edge, const int64_t* row_off,
                       const int32_t* row_width, const double* q, int32_t n_q, const int32_t* q_var, const int64_t* q_off,
                       double* out, void* stream);
int lhvi_pbp_halo_unpack(const double* in, int32_t n, int32_t n_rows, const int32_t* row_edge, const int64_t* row_off,
                         const int32_t* row_width, double* v2f, int32_t n_q, const int32_t* q_var, const int64_t* q_off,
                         double* q, void* stream);

/* ---- Mixture variational inference (VarInference.py / LiftedVarInference.py) --------------------- */

typedef struct lhvi_vi {
    int32_t K;                  /* mixture components */
    int32_t T;                  /* Gauss-Hermite points */
    int32_t Dmax;               /* max #states of a discrete variable (row stride of eta_d) */
    int32_t quirks;             /* 1 = reproduce VarInference.py:147-150; (ABI 20) | LHVI_VI_GAUSSIAN_PDF: lhvi_vi_map_bfgs
                                 * evaluates the components as normal densities exp(-u^2 / 2 var) / sqrt(2 pi var) (an NPVI fit) instead of
                                 * VarInference.norm_pdf's exp(-u^2 / 2 var) / (2.5066 var) */
    const double* gh_x;         /* [T] hermgauss nodes */
    const double* gh_w;         /* [T] weights / sqrt(pi) */
    const double* w;            /* [K] softmax(w_tau) */
    const double* eta_c;        /* [V][K][2] (mu, var) for continuous hidden variables */
    const double* eta_d;        /* [V][K][Dmax] category probabilities for discrete hidden variables */
    const double* obs_var;      /* [V] or NULL.  C2FVarInference.py:120-136,253-261: obs_var[v] > 0 makes the evidence cluster v
                                 * a Gaussian observation N(var_value[v], obs_var[v]) -- T quadrature nodes in every expectation,
                                 * its pdf in every belief, no parameters; 0 = exact evidence (or not evidence at all) */
    const double* var_N;        /* [V] or NULL: rv.N = number of incident ground factors (the sum of the row's edge_count on a
                                 * lifted graph, LiftedVarInference.py:64-67).  NULL: every (variable, k) thread sums its row itself,
                                 * which serialises on the template variables of a relational model (thousands of entries) */
    /* (ABI 9) the caller's split of the factors among the kernels of expectation() (VarInference.py:40-55), or NULL: a permutation
     * of the factor ids in six segments, in this order --
     *   n_cc    pairwise factors over two distinct continuous / observed variables with a Gaussian / quadratic / linear-Gaussian /
     *           XY potential (thread per (factor, k), per-axis pdf tables in registers);
     *   n_tiny  other factors of arity <= 3 whose grid has at most LHVI_VI_TINY_NODES nodes, K <= 2 (thread per (factor, k) walking
     *           the grid nodes and the points of the pinned expectations as one list; needs edge_axis and tiny_par_words);
     *   n_grp3  other factors of arity <= 3 whose axis lengths sum to <= LHVI_VI_GROUP_SLOTS with K * that <= LHVI_VI_GROUP_COMP
     *           (8 lanes per (factor, k), per-axis tables in LDS);  n_grp6: the same for arity 4 .. LHVI_MAX_ARITY;
     *   n_rest3 / n_rest6  whatever fits neither (thread per (factor, k), arity <= 3 / 4 .. LHVI_MAX_ARITY).
     * NULL: every kernel classifies the factors itself (thread-per-factor kernels only). */
    const int32_t* fac_list;
    int32_t n_cc, n_grp3, n_grp6, n_rest3, n_rest6;
    int32_t n_tiny;            /* (sits between n_cc and n_grp3 in the list) */
    int32_t tiny_par_words;    /* pots.off[P], the length of pots.param in doubles: the tiny-grid kernel keeps the parameter rows (an MLN
                                * formula's program) in LDS; n_tiny > 0 needs 0 < tiny_par_words <= 3072 */
    /* (ABI 9) [E][4] or NULL: per edge {variable, axis length | hidden << 16 | continuous << 17 | Gaussian observation << 18,
     * state index of the observed value (0 unless observed and discrete), offset of the variable's states in dom_val} -- the shape
     * of the factor's quadrature grid, which
     * depends on the graph and the evidence pattern only; NULL: the group kernels derive it per (factor, k) */
    const int32_t* edge_axis;
} lhvi_vi_t;
#define LHVI_VI_GAUSSIAN_PDF 2
#define LHVI_VI_GROUP_SLOTS 24
#define LHVI_VI_GROUP_COMP 48
#define LHVI_VI_TINY_NODES 32

/* state of the optimiser for lhvi_vi_adam_run: the arrays ADAM_update (VarInference.py:249-287) reads and writes.  w, eta_c and
 * eta_d must be the arrays the lhvi_vi_t passed alongside points to (the step must see what it updates). */
typedef struct lhvi_vi_opt {
    double* w_tau;              /* [K] mixture logits */
    double* w;                  /* [K] softmax(w_tau) */
    double* eta_c;              /* [V][K][2] */
    double* tau_d;              /* [V][K][Dmax] category logits */
    double* eta_d;              /* [V][K][Dmax] softmax(tau_d) over each hidden discrete variable's states */
    double *m_w, *s_w, *m_c, *s_c, *m_d, *s_d;   /* ADAM moments, shaped like w_tau / eta_c / tau_d */
    double *g_w, *g_c, *g_d;    /* gradient scratch, same shapes */
    double* fe;                 /* [1] scratch for the free energy of passes that are not logged */
    double lr, b1, b2, eps;     /* VarInference.py:252-254: 0.9, 0.999, 1e-8 */
    double var_min;             /* var_threshold: variances are clipped from below (VarInference.py:11,277) */
    int32_t t;                  /* updates done before this call (bias correction uses t + i + 1) */
} lhvi_vi_opt_t;

/* gradient_w_tau / gradient_mu_var / gradient_category_tau / free_energy: VarInference.py:57-195,
 * LiftedVarInference.py:59-199.  Outputs: g_w [K] (already softmax-projected), g_c [V][K][2],
 * g_d [V][K][Dmax] (already projected), fe [1].  ws: workspace of lhvi_vi_workspace_bytes() bytes. */
size_t lhvi_vi_workspace_bytes(const lhvi_graph_t* g, const lhvi_vi_t* p);
int lhvi_vi_grad(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p,
                 double* g_w, double* g_c, double* g_d, double* fe, void* ws, size_t ws_bytes, void* stream);
/* `iterations` rounds of ADAM_update (VarInference.py:249-300) enqueued back to back, no host work in between: per round one
 * lhvi_vi_grad and ONE update launch for all three parameter arrays (ADAM step, variance clip, both softmaxes).  fe_log: device
 * [iterations] or NULL -- fe_log[i] = the free energy after update i + 1, which is what the next round's gradient pass computes
 * anyway (one extra pass after the last update).  Results equal the per-array calls below bit for bit. */
int lhvi_vi_adam_run(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const lhvi_vi_opt_t* o, int32_t iterations,
                     double* fe_log, void* ws, size_t ws_bytes, void* stream);
/* ADAM_update body: VarInference.py:255-287.  theta/m/s/g are flat arrays of `count` doubles;
 * clip_stride>0 clamps every element with index % clip_stride == clip_stride-1 to >= clip_min (variances). */
int lhvi_adam_step(double* theta, double* m, double* s, const double* g, int64_t count, int32_t t,
                   double lr, double b1, double b2, double eps, int32_t clip_stride, double clip_min, void* stream);
/* softmax over rows of `cols` valid entries (stride `stride`): VarInference.py:32-38 */
int lhvi_softmax_rows(const double* tau, double* out, int64_t rows, int32_t cols, int32_t stride, void* stream);
/* map(rv) (VarInference.py:355-376) of nq rows in ONE launch, a thread each (csrc/vi_map.hip).  row_var [nq]: variables of the
 * solver's graph.  A hidden continuous row runs what the reference calls: scipy.optimize.minimize(-belief, x0 = the first component
 * mean of largest belief), i.e. SciPy 1.15's BFGS with a forward-difference gradient, line_search_wolfe1 (MINPACK dcsrch) and
 * line_search_wolfe2 as fallback -- the same iterates, decision for decision, so that the answer is scipy's and not merely a maximum.
 * gtol / maxiter: minimize's options (1e-5, 200).  xout [nq] res.x; fout [nq] (optional) -res.fun, the belief there; nit / status
 * [nq] (optional) res.nit / res.status (0 converged, 1 maxiter, 2 line search failed, 3 NaN).  A hidden discrete row: xout = the
 * VALUE of the first state of largest sum_k w_k eta_d[v, k, s], fout that sum, status 0.  Observed rows (and indices outside
 * [0, V)): NaN, status -1.  Reads p->K (<= 128), w, eta_c, eta_d, Dmax. */
int lhvi_vi_map_bfgs(const lhvi_graph_t* g, const lhvi_vi_t* p, int64_t nq, const int32_t* row_var, double gtol, int32_t maxiter,
                     double* xout, double* fout, int32_t* nit, int32_t* status, void* stream);

/* ---- Hybrid MaxWalkSAT (HybridMaxWalkSAT.py): MAP local search, one workgroup (one wavefront) per try (csrc/mws.hip) ------
 * The caller (lhvi/mws.py) classifies the factors as the reference does and passes the two clause lists; the device runs the
 * tries' flips.  Per flip of a try (HybridMaxWalkSAT.run, :221-281): the improvement check (:226-230), the unsatisfied scan of
 * the discrete clauses (:82-96), the clause pick (:233-237, random_factor :98-104), then the walk (:239-248) or greedy (:249-273)
 * move, and the score of the new state.  Random numbers: Philox4x32-10 keyed by seed, counter (flip, try id, draw, tag).
 * Continuous moves run SciPy's L-BFGS-B (scipy_opt.hpp): argmax_rv_wrt_factor (:106-112) on -phi, argmax_rvs_wrt_score
 * (:114-144) on the negated local score.  State lives in the caller's arrays, so a run is any number of lhvi_mws_flips calls. */
typedef struct lhvi_mws {
    int32_t T;                  /* tries of this launch (one workgroup each) */
    int32_t max_flips;          /* flips per try (rec_* row length) */
    double epsilon;             /* walk probability (:239) */
    double noise_std;           /* scale of the walk's normal noise (:245) */
    uint64_t seed;              /* Philox key */
    const int32_t* try_id;      /* [T] the try index of each workgroup in the Philox counter */
    const int32_t* disc;        /* [n_disc] discrete clauses (discrete_and_numeric_factors + prune, :59-80), factor order */
    int32_t n_disc;
    const int32_t* num;         /* [n_num] numeric clauses, factor order */
    int32_t n_num;
    const int8_t* fac_class;    /* [F] 1: type(potential) == MLNHardPotential, 2: == MLNPotential, 0: neither (:87-94) */
    double* x;                  /* [T][V] current assignment (observed entries hold their values) */
    double* best_x;             /* [T][V] best assignment of the try */
    double* cur_score;          /* [T] score (:30-40) of x */
    double* best_score;         /* [T] best score of the try (-inf before its first flip) */
    int32_t* status;            /* [T] 0 running, 1 stopped: no clause to pick (the reference's ZeroDivisionError, :99), 2: bad replay input */
    int32_t* err_flip;          /* [T] the flip of that stop */
    double* rec_score;          /* [T][max_flips] score after each flip, or NULL */
    int32_t* rec_zero;          /* [T][max_flips] factors with phi == 0 after each flip, or NULL */
    int64_t* rec_ticks;         /* [T][max_flips] device wall-clock ticks spent in each flip, or NULL */
    /* Replay (the parity tests' input): with rp_clause set, T must be 1 and every flip takes the recorded decisions instead of
     * drawing them, then forces the recorded post-state, so that a trajectory of the reference can be followed flip by flip.
     * All rp_* / out_* NULL: the search draws its own decisions. */
    const double* rp_init;      /* [V] the initial assignment (random_assignment's draw, :17-28) */
    const int32_t* rp_clause;   /* [max_flips] the clause c (factor index), :233-237 */
    const int32_t* rp_walk;     /* [max_flips] 1: the walk branch (rand() < epsilon, :239), 0: greedy */
    const int32_t* rp_walk_k;   /* [max_flips] walk: index of rv among c's hidden variables in c.nb order (:240) */
    const double* rp_noise;     /* [max_flips] walk on a continuous rv: the normal draw added (:245) */
    const double* rp_post;      /* [max_flips][LHVI_MAX_ARITY] values of c's hidden variables after the flip (forced) */
    double* out_score;          /* [max_flips] the device's score at the start of the flip (:227) */
    int32_t* out_unsat;         /* [max_flips][2] the device's hard / soft unsatisfied counts (:232) */
    int32_t* out_winner;        /* [max_flips] greedy winner: index among c's hidden variables (:267); -1 after a walk */
    int32_t* out_accept;        /* [max_flips] 1: the winner applied (:269-270), 0: numeric-term move (:272), -1: walk */
    double* out_val;            /* [max_flips][LHVI_MAX_ARITY] the device's values of c's hidden variables after its move */
} lhvi_mws_t;

/* random_assignment (:17-28) of every try (uniform on dom_lo..dom_hi / over the states; observed rvs keep their value), its
 * score, best_score = -inf, status = 0 */
int lhvi_mws_init(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_mws_t* s, void* stream);
/* flips [flip_begin, flip_end) of every try; a stopped try does nothing.  Arity <= LHVI_MAX_ARITY; every potential must have a
 * device encoding (lhvi_pots_t kind != LHVI_POT_GENERIC). */
int lhvi_mws_flips(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_mws_t* s, int32_t flip_begin, int32_t flip_end,
                   void* stream);
/* scipy.optimize.minimize(fun, x, method='L-BFGS-B') with no bounds and default options, on the host (the code the device runs):
 * x [n] in / out (n <= LHVI_MAX_ARITY), fun(x, ctx) the objective.  out_fun, nit, nfev, status: res.fun / nit / nfev / status. */
int lhvi_lbfgsb_host(int32_t n, double* x, double (*fun)(const double*, void*), void* ctx, double* out_fun, int32_t* nit,
                     int32_t* nfev, int32_t* status);
/* the device wall clock's rate (wall_clock64 ticks per millisecond) of the current device */
int lhvi_wall_clock_khz(int32_t* khz);

/* ---- Exact hybrid-Gaussian baseline (gibbs/hybrid_gaussian_mrf.py, enumeration half; csrc/exact.hip, csrc/exact.hpp) -------
 * p(x_d, x_c) = p(x_d) N(x_c; mu(x_d), J(x_d)^-1): every joint state of the discrete variables is one "configuration",
 * numbered in C order of the table [v_1 .. v_Nd] (first variable most significant).  The caller (lhvi/exact.py) flattens the
 * factors, in factor order, into two descriptor lists of int32 words:
 *   quadratic (LogQuadratic: nd = 0; LogHybridQuadratic): [nd, nc, off, (variable, local stride) * nd, continuous variable * nc]
 *     with quad_par[off + local * (nc * nc + nc + 1)] = A [nc][nc], b [nc], c of the local discrete state;
 *   table (LogTable): [nd, off, (variable, local stride) * nd] with tab_par[off + local] the log potential.
 * All doubles. */
#define LHVI_EXACT_MAX_NC 64
typedef struct lhvi_exact {
    int32_t Nd, Nc;
    int64_t M;                  /* prod(dstates), 1 when Nd = 0 */
    const int32_t* dstates;     /* [Nd] */
    const int64_t* dstride;     /* [Nd] stride of the variable in the configuration index */
    int32_t n_quad;
    const int32_t* quad_ptr;    /* [n_quad + 1] into quad_desc */
    const int32_t* quad_desc;
    const double* quad_par;
    int32_t n_tab;
    const int32_t* tab_ptr;     /* [n_tab + 1] into tab_desc */
    const int32_t* tab_desc;
    const double* tab_par;
} lhvi_exact_t;

/* LDS of one workgroup of lhvi_exact_configs (one wavefront, 64 / lanes configurations); 0 for an invalid `lanes` */
size_t lhvi_exact_lds_bytes(int32_t Nc, int32_t Nd, int32_t lanes);
/* configurations [cfg_begin, cfg_begin + cfg_count): logp [M] = log p~(x_d) (:57-65), means [M][Nc], vars [M][Nc] = diag(J^-1),
 * covs [M][Nc][Nc] = J^-1 or NULL; rows indexed by the configuration.  lanes: lanes per configuration, a power of two <= 64;
 * the results do not depend on it.  bad [1]: the caller sets it to UINT64_MAX; a configuration whose J = -(A + A^T) has a
 * pivot <= 0 lowers it to its index (atomic min), and its outputs are meaningless (the caller raises, LHVI_E_NOT_PD).
 * LHVI_E_UNSUPPORTED: Nc > LHVI_EXACT_MAX_NC or more than 64 KiB of LDS. */
int lhvi_exact_configs(const lhvi_exact_t* m, int64_t cfg_begin, int64_t cfg_count, int32_t lanes, double* logp, double* means,
                       double* vars, double* covs, uint64_t* bad, void* stream);
/* logZ [1] = log sum exp logp (max pass, then a sum in a fixed order), table [M] = exp(logp - logZ); ws: 2048 doubles */
int lhvi_exact_normalize(int64_t M, const double* logp, double* table, double* logZ, double* ws, void* stream);
/* get_drv_marg (:98-109) of every discrete variable: marg [n_states = sum dstates], variable-major */
int lhvi_exact_marginals(const lhvi_exact_t* m, int32_t n_states, const double* table, double* marg, void* stream);
/* per-variable mixture records mix [Nc][M][3] = (log w_k - 1/2 log(2 pi var_kj), mean_kj, 1 / var_kj) (get_crv_marg :76-95) */
int lhvi_exact_mix_prepare(int32_t Nc, int64_t M, const double* table, const double* means, const double* vars, double* mix,
                           void* stream);
/* out [Nc][npts][3] = log density of variable j's mixture at x [Nc][npts] (utils.get_scalar_gm_log_prob), and its first and
 * second derivative in x */
int lhvi_exact_mixture(int32_t Nc, int64_t M, const double* mix, int32_t npts, const double* x, double* out, void* stream);
/* safeguarded Newton on the log density of variable j from each of x [Nc][S] (in / out), clipped to [lo[j], hi[j]]; vmin [Nc]:
 * smallest component variance (gradient-step scale where the second derivative is not negative); out_logf [Nc][S] */
int lhvi_exact_map_polish(int32_t Nc, int64_t M, const double* mix, int32_t S, double* x, const double* lo, const double* hi,
                          const double* vmin, int32_t max_iter, double* out_logf, void* stream);
/* one configuration on the HOST through the device's code (csrc/exact.hpp); every pointer of m and every output is host
 * memory; mean, var, cov may be NULL.  LHVI_E_NOT_PD when J is not positive definite. */
int lhvi_exact_config_host(const lhvi_exact_t* m, int64_t cfg, double* logp, double* mean, double* var, double* cov);

/* ---- Block Gibbs sampling in a hybrid Gaussian MRF (gibbs/hybrid_gaussian_mrf.py::block_gibbs_sample, gibbs/disc_mrf.py;
 * csrc/gibbs.hip, csrc/gibbs.hpp) -------------------------------------------------------------------------------------------
 * Many independent chains.  One outer iteration: x_c | x_d from the Cholesky factor of J(x_d) (x_c = L^-T (L^-1 b + z)), the
 * reduced log table of every strictly hybrid factor at x_c, then disc_block_its sweeps of single-site Gibbs over x_d.
 * ex: the flat model of the exact baseline; ex.M and ex.dstride are not read (a chain is not a configuration index).
 * A "hybrid" factor is a quadratic descriptor with nd > 0; hybrid factor h is quadratic descriptor hyb_quad[h] and its reduced
 * table occupies [hyb_off[h], hyb_off[h + 1]) of the chain's table row, in C order of its discrete scope.
 * The draw of counter (chain, iteration, index, tag) comes from Philox4x32-10 keyed by seed. */
typedef struct lhvi_gibbs {
    lhvi_exact_t ex;
    const int32_t* dstate_off;  /* [Nd + 1] prefix sums of ex.dstates (rows of the state counts) */
    const int32_t* vt_ptr;      /* [Nd + 1] into vt_fac */
    const int32_t* vt_fac;      /* table descriptors with variable n in scope, in factor order */
    const int32_t* vh_ptr;      /* [Nd + 1] into vh_fac */
    const int32_t* vh_fac;      /* hybrid factors (h) with variable n in scope, in factor order */
    int32_t n_hyb;
    const int32_t* hyb_quad;    /* [n_hyb] */
    const int32_t* hyb_off;     /* [n_hyb + 1] */
    int32_t table_doubles;      /* hyb_off[n_hyb] */
    int32_t max_states;         /* max ex.dstates (1 when Nd = 0) */
    double* table_scratch;      /* NULL: the reduced tables live in LDS.  Otherwise one row of table_doubles per chain, for the
                                 * number of chains rounded up to a multiple of 64 */
    int32_t disc_block_its;
    int32_t num_burnin;         /* iterations [num_burnin, num_burnin + num_samples) are kept */
    int32_t num_samples;        /* rows of a chain in the sample arrays */
    uint64_t seed;
} lhvi_gibbs_t;

/* LDS of one workgroup of lhvi_gibbs_run (one wavefront, 64 / lanes chains).  table_doubles: the doubles a chain keeps in LDS
 * for the discrete block = max_states + (the reduced tables when they live in LDS: lhvi_gibbs_t.table_doubles, else 0).
 * 0 for an invalid `lanes`. */
size_t lhvi_gibbs_lds_bytes(int32_t Nc, int32_t Nd, int32_t table_doubles, int32_t lanes);
/* the initial state x_d [chains][Nd] (int32): variable n of chain c = floor(u dstates[n]) with u the uniform of counter
 * (c, n, 0, init tag) */
int lhvi_gibbs_init(const lhvi_gibbs_t* m, int64_t chains, int32_t* x_d, void* stream);
/* iterations [it_begin, it_end) of every chain.  x_d [chains][Nd]: in / out, so a run is any number of calls.  lanes: lanes
 * per chain, a power of two <= 64; a chain's samples depend neither on it, nor on `chains`, nor on the split into calls.
 * z [iters][chains][Nc], u [iters][chains][disc_block_its][Nd]: injected draws (rows by absolute iteration), or NULL for the
 * Philox stream.  Outputs, each NULL or: disc [chains][num_samples][Nd] (int32), cont [chains][num_samples][Nc], and the
 * accumulators over the kept iterations, which the caller zeroes before the first call: counts [chains][sum dstates] (int32),
 * sum1 [chains][Nc] = sum x_c, sum2 [chains][Nc (Nc + 1) / 2] = sum x_c x_c^T, lower triangle by rows.
 * bad [1]: the caller sets it to UINT64_MAX; a chain whose J is not positive definite lowers it to (chain << 32 | iteration)
 * (atomic min), keeps its x_d of that moment and stores nothing more.
 * LHVI_E_UNSUPPORTED: Nc > LHVI_EXACT_MAX_NC or more than 64 KiB of LDS. */
int lhvi_gibbs_run(const lhvi_gibbs_t* m, int64_t chains, int32_t it_begin, int32_t it_end, int32_t lanes, int32_t* x_d,
                   const double* z, const double* u, int32_t* disc, double* cont, int32_t* counts, double* sum1, double* sum2,
                   uint64_t* bad, void* stream);
/* one chain on the HOST through the device's code (csrc/gibbs.hpp) with injected draws z [iters][Nc], u [iters][its][Nd];
 * every pointer of m and every argument is host memory, the outputs are this chain's rows and may be NULL.  m->table_scratch
 * is ignored.  LHVI_E_NOT_PD when a J is not positive definite (x_d then holds the state). */
int lhvi_gibbs_chain_host(const lhvi_gibbs_t* m, int32_t it_begin, int32_t it_end, int32_t* x_d, const double* z, const double* u,
                          int32_t* disc, double* cont, int32_t* counts, double* sum1, double* sum2);

/* ---- Rao-Blackwellised marginals of the block Gibbs sampler (csrc/gibbs_rb.hip, csrc/gibbs_rb.hpp) ---------------------------
 * The conditional Gaussian of explicit discrete states: lhvi_exact_configs with row s of x_d [S][Nd] (int32 digits, each inside
 * [0, dstates[n]): the caller checks) in the place of a configuration index.  logp [S] or NULL, means [S][Nc], vars [S][Nc]; rows
 * indexed by s.  Neither m->M nor m->dstride is read, so a model whose configurations cannot be numbered (M = 0) is served.  The
 * operations are those of lhvi_exact_configs after its digit decode, in the same order: a row of digits gives the bits that call
 * gives for that configuration, whatever `lanes`.  Launch shape and LDS of lhvi_exact_configs (lhvi_exact_lds_bytes).
 * bad [1]: the caller sets it to UINT64_MAX; a row whose J is not positive definite lowers it to s (atomic min).
 * LHVI_E_UNSUPPORTED: Nc > LHVI_EXACT_MAX_NC or more than 64 KiB of LDS. */
int lhvi_exact_configs_at(const lhvi_exact_t* m, int64_t S, const int32_t* x_d, int32_t lanes, double* logp, double* means,
                          double* vars, uint64_t* bad, void* stream);
/* one row of digits on the HOST through the device's code; every pointer is host memory, logp, mean, var may be NULL.
 * LHVI_E_ARG for a digit outside its range, LHVI_E_NOT_PD when J is not positive definite. */
int lhvi_exact_config_at_host(const lhvi_exact_t* m, const int32_t* x_d_row, double* logp, double* mean, double* var);
/* prob_sum [chains][sum dstates] += sum over the kept samples s in [s_begin, s_end) of p(x_n = k | x_d,-n, x_c) at the sample
 * (disc [chains][num_samples][Nd], cont [chains][num_samples][Nc], as lhvi_gibbs_run stored them): the reduced tables of the
 * strictly hybrid factors at the sample's x_c, every variable's log probabilities over its table factors, then its hybrid
 * factors, in factor order with the other digits at the sample's values, and the sampler's softmax exp(v - (max + log sum)),
 * added in sample order by the lane that owns the state.  The caller zeroes prob_sum before the first call; a chain's sums
 * depend neither on `lanes`, nor on `chains`, nor on the split of [0, num_samples) over calls.  Workspace, lanes and the place of
 * the reduced tables (LDS, or m->table_scratch) are those of lhvi_gibbs_run (lhvi_gibbs_lds_bytes).  m->disc_block_its,
 * num_burnin and seed are not read.  LHVI_E_UNSUPPORTED: Nc > LHVI_EXACT_MAX_NC or more than 64 KiB of LDS. */
int lhvi_gibbs_rb_disc(const lhvi_gibbs_t* m, int64_t chains, int32_t s_begin, int32_t s_end, int32_t lanes, const int32_t* disc,
                       const double* cont, double* prob_sum, void* stream);
/* one chain on the HOST through the device's code: disc [num_samples][Nd], cont [num_samples][Nc], prob_sum [sum dstates];
 * m->table_scratch is ignored.  LHVI_E_ARG for a digit outside its range. */
int lhvi_gibbs_rb_disc_host(const lhvi_gibbs_t* m, int32_t s_begin, int32_t s_end, const int32_t* disc, const double* cont,
                            double* prob_sum);

/* ---- Annealed importance sampling for log Z of a hybrid Gaussian MRF (csrc/ais.hip, csrc/ais.hpp; docs/kernels_ais.md) ---------
 * Many independent annealing runs over the model of lhvi_gibbs_t along f_beta = p~^beta f0^(1 - beta), f0 = exp(-tau0 / 2
 * |x_c - mu0|^2) with x_d uniform, for a schedule betas [T + 1] (betas[0] = 0 <= ... <= betas[T] = 1: the caller checks).  x_c
 * is integrated out in closed form: step t adds log m_{betas[t+1]}(x_d) - log m_{betas[t]}(x_d) to the chain's log weight, with
 * log m_beta(x_d) = beta tables + c_beta + Nc / 2 log 2 pi - 1/2 log det J_beta + 1/2 |L_beta^-1 b_beta|^2, then (unless
 * t = T - 1) makes one block Gibbs transition at betas[t + 1]: x_c from the factor just computed, the reduced tables at x_c,
 * m->disc_block_its sweeps over x_d with the log probabilities multiplied by beta.  log Z0 = sum log dstates + Nc / 2
 * log(2 pi / tau0); log Z is estimated by log Z0 + log mean exp(logw).  m->num_burnin and m->num_samples are not read.
 * The draw of counter (chain, step, index, tag) comes from Philox4x32-10 keyed by m->seed, under tags of its own. */
#define LHVI_AIS_REDUCE_OUT 9
#define LHVI_AIS_REDUCE_WS 8192
/* LDS of one workgroup of lhvi_ais_run (one wavefront, 64 / lanes chains): the workspace of lhvi_gibbs_lds_bytes plus mu0.
 * 0 for an invalid `lanes`. */
size_t lhvi_ais_lds_bytes(int32_t Nc, int32_t Nd, int32_t table_doubles, int32_t lanes);
/* steps [t_begin, t_end) of every chain, 0 <= t_begin <= t_end <= T.  x_d [chains][Nd] (int32, from lhvi_gibbs_init before the
 * first call) and logw [chains] (zeroed before the first call) are in / out, so a run is any number of calls.  betas [T + 1],
 * mu0 [Nc]: device arrays; tau0 > 0.  lanes: lanes per chain, a power of two <= 64; a chain's x_d and logw depend neither on
 * it, nor on `chains`, nor on the split into calls.  z [T][chains][Nc], u [T][chains][disc_block_its][Nd]: injected draws (rows
 * by step; the transition of step t reads row t), or NULL for the Philox stream.
 * bad [1]: the caller sets it to UINT64_MAX; a chain that meets a J_beta that is not positive definite lowers it to
 * (chain << 32 | step) (atomic min) and keeps its x_d and logw of that moment.
 * LHVI_E_UNSUPPORTED: Nc > LHVI_EXACT_MAX_NC or more than 64 KiB of LDS. */
int lhvi_ais_run(const lhvi_gibbs_t* m, int64_t chains, int32_t T, const double* betas, int32_t t_begin, int32_t t_end,
                 int32_t lanes, double tau0, const double* mu0, int32_t* x_d, double* logw, const double* z, const double* u,
                 uint64_t* bad, void* stream);
/* out [LHVI_AIS_REDUCE_OUT] over logw [chains], every sum in a fixed order (two stages, no floating-point atomics), with
 * mx = max logw and d = logw - mx: log sum exp(logw), log sum exp(2 logw), sum logw, sum logw^2, mx, sum exp(d), sum exp(2 d),
 * sum d, sum d^2.  ws: LHVI_AIS_REDUCE_WS doubles. */
int lhvi_ais_reduce(int64_t chains, const double* logw, double* out, double* ws, void* stream);
/* steps [t_begin, t_end) of one chain on the HOST through the device's code (csrc/ais.hpp); every pointer of m and every
 * argument is host memory; x_d [Nd] and logw [1] are in / out.  z [T][Nc], u [T][its][Nd]: this chain's injected draws, or both
 * NULL for the Philox stream of chain `chain`.  m->table_scratch is ignored.  LHVI_E_NOT_PD when a J_beta is not positive
 * definite (x_d then holds the state). */
int lhvi_ais_chain_host(const lhvi_gibbs_t* m, int64_t chain, int32_t T, const double* betas, int32_t t_begin, int32_t t_end,
                        double tau0, const double* mu0, int32_t* x_d, double* logw, const double* z, const double* u);

/* ---- Parallel tempering for the block Gibbs sampler (csrc/pt.hip, csrc/pt.hpp; docs/kernels_pt.md) ------------------------------
 * `ladders` independent ladders of R replicas over the model of lhvi_gibbs_t.  Replica r samples f_betas[r] on the path of
 * lhvi_ais_run (betas [R], 0 <= betas[0] <= ... <= betas[R - 1] = 1: the caller checks).  Iteration `it` of a ladder: every
 * replica makes one block Gibbs transition at its beta (at beta = 1 the operations of lhvi_gibbs_run); from iteration
 * m->num_burnin on replica R - 1 stores its sample and adds to the accumulators like lhvi_gibbs_run, `chains` read as `ladders`;
 * then, when swap_every > 0 and (it + 1) % swap_every == 0, swap round s = it / swap_every proposes to exchange the digits of the
 * pairs (r, r + 1), r = s mod 2, s mod 2 + 2, ...: accepted iff log(1 - u) <= log m_{b_r}(d_{r+1}) + log m_{b_{r+1}}(d_r)
 * - log m_{b_r}(d_r) - log m_{b_{r+1}}(d_{r+1}) with log m_beta the collapsed mass of lhvi_ais_run.  The draws come from
 * Philox4x32-10 keyed by m->seed: normals and sweep uniforms of counter (ladder * R + r, it, index, tag), the swap uniform of
 * pair r of counter (ladder, it, r, tag), under tags of their own. */
/* LDS of one workgroup of lhvi_pt_run: per ladder R workspaces of lhvi_ais_run's chains plus the exchange slots; a workgroup is
 * R * lanes threads rounded up to whole wavefronts and holds 64 / (R * lanes) ladders when R * lanes <= 32.  0 for an invalid
 * `lanes`, R < 1 or R * lanes > 256. */
size_t lhvi_pt_lds_bytes(int32_t Nc, int32_t Nd, int32_t table_doubles, int32_t R, int32_t lanes);
/* iterations [it_begin, it_end) of every ladder.  x_d [ladders][R][Nd] (int32; lhvi_gibbs_init over ladders * R rows before the
 * first call) is in / out, so a run is any number of calls.  betas [R], mu0 [Nc]: device arrays; tau0 > 0.  lanes: lanes per
 * replica, a power of two <= 64; a ladder's outputs depend neither on it, nor on `ladders`, nor on the split into calls.
 * z [iters][ladders * R][Nc], u [iters][ladders * R][disc_block_its][Nd], usw [iters][ladders][max(R - 1, 1)]: injected draws
 * (rows by absolute iteration), or NULL for the Philox stream.  disc, cont, counts, sum1, sum2: the outputs of lhvi_gibbs_run
 * over `ladders` rows (each may be NULL; counts and sums zeroed before the first call).  swap_try, swap_acc [ladders][R - 1]
 * (int32, zeroed before the first call, may be NULL): proposed and accepted swaps per pair.  m->table_scratch: NULL, or
 * ladders * R rows of table_doubles.
 * bad [1]: the caller sets it to UINT64_MAX; a ladder one of whose replicas meets a J_beta that is not positive definite lowers
 * it to (ladder << 32 | iteration) (atomic min), keeps its x_d of that moment and stores, counts and swaps nothing more.
 * LHVI_E_UNSUPPORTED: Nc > LHVI_EXACT_MAX_NC, R * lanes > 256 or more than 64 KiB of LDS. */
int lhvi_pt_run(const lhvi_gibbs_t* m, int64_t ladders, int32_t R, const double* betas, int32_t it_begin, int32_t it_end,
                int32_t swap_every, int32_t lanes, double tau0, const double* mu0, int32_t* x_d, const double* z, const double* u,
                const double* usw, int32_t* disc, double* cont, int32_t* counts, double* sum1, double* sum2, int32_t* swap_try,
                int32_t* swap_acc, uint64_t* bad, void* stream);
/* iterations [it_begin, it_end) of one ladder on the HOST through the device's code (csrc/pt.hpp), the replicas in order; every
 * pointer of m and every argument is host memory; x_d [R][Nd] is in / out.  z [iters][R][Nc], u [iters][R][its][Nd],
 * usw [iters][max(R - 1, 1)]: this ladder's injected draws, or all NULL for the Philox stream of ladder `ladder`.  The outputs
 * are one ladder's rows.  m->table_scratch is ignored.  LHVI_E_NOT_PD when a J_beta is not positive definite. */
int lhvi_pt_ladder_host(const lhvi_gibbs_t* m, int64_t ladder, int32_t R, const double* betas, int32_t it_begin, int32_t it_end,
                        int32_t swap_every, double tau0, const double* mu0, int32_t* x_d, const double* z, const double* u,
                        const double* usw, int32_t* disc, double* cont, int32_t* counts, double* sum1, double* sum2,
                        int32_t* swap_try, int32_t* swap_acc);

/* ---- Single-site Gibbs / slice sampling on a ground flat graph (csrc/fgibbs.hip, csrc/fgibbs.hpp; docs/kernels_fgibbs.md) ---------
 * `chains` independent chains over the hidden variables of a GROUND lhvi_graph_t (edge_count, var_mult, fac_mult NULL), any
 * potential kind.  State: x [V][chains] (doubles) and idx [V][chains] (int32: the state index of a discrete variable, 0 of a
 * continuous one), chain fastest; an observed variable holds its value.  The conditional log density of hidden variable v at t is
 * g_v(t) = sum over v's var_edge row, in row order, of log phi_f(x with x_v = t): the evaluator's value where it is a logarithm,
 * else log(value) (phi == 0: -inf).
 *   discrete v (S <= LHVI_FGIBBS_MAX_STATES states): lp[j] = g_v(s_j); all -inf: the state stays and stuck[chain] += 1; else the
 *     softmax and inverse-CDF pick of lhvi_gibbs_run with ONE uniform (draw 0).
 *   continuous v (Neal's slice sampler, shrinkage only): y = g_v(x0) + log(1 - u_0); L = dom_lo, R = dom_hi; for k = 1 ..
 *     max_shrink: x1 = L + u_k (R - L) (product rounded, then added); accept when g_v(x1) >= y, else L = x1 if x1 < x0 else R = x1.
 *     Nothing accepted: x0 stays and capped[chain] += 1.
 * Iteration `it` visits the colours 0, 1, ... (one launch each, plus one for the colour's hub list); no factor holds two hidden
 * variables of one colour, so the launch equals the sequential visit of col_var in list order.  From iteration num_burnin on,
 * every thin-th iteration is kept (sample s = (it - num_burnin) / thin < num_samples) and added to the accumulators by the thread
 * that owns (variable, chain), in iteration order, without atomics.
 * Draws: Philox4x32-10 keyed by seed; uniforms 2 p and 2 p + 1 of (chain, it, v) come from counter
 * (chain | p << 24, it, v, "FGSU"); the initial state from (chain, 0, v, "FGXI").  chains <= 2^24, max_shrink <= 510. */
#define LHVI_FGIBBS_MAX_STATES 16
typedef struct lhvi_fgibbs {
    int32_t n_colours;
    const int32_t* col_ptr;     /* [n_colours + 1] into col_var */
    const int32_t* col_var;     /* the hidden variables colour by colour, ascending ids within a colour */
    const int32_t* hub_ptr;     /* [n_colours + 1] into hub_var */
    const int32_t* hub_var;     /* per colour, the variables of col_var with more than hub_degree incident edges: a wavefront each */
    int32_t max_shrink;
    int32_t hub_degree;
    int32_t num_burnin;
    int32_t num_samples;
    int32_t thin;
    uint64_t seed;
    const double* u;            /* injected uniforms [iterations][chains][V][1 + max_shrink], rows by absolute iteration, or NULL */
    const double* init_x;       /* injected initial state [chains][V] (hidden rows are read), or NULL */
    /* outputs: each may be NULL; the caller zeroes them before the first call */
    const int32_t* cnt_off;     /* [V] first row of the variable's states in counts (hidden discrete variables), else -1 */
    int32_t* counts;            /* [sum of states][chains] kept samples per state */
    double* sum1;               /* [V][chains] sum of the kept x (hidden continuous rows) */
    double* sum2;               /* [V][chains] sum of the kept x * x (product rounded, then added) */
    const int32_t* keep_row;    /* [V] row of the variable in samples, or -1 */
    double* samples;            /* [rows][chains * num_samples]: sample s of chain c at column c * num_samples + s */
    int32_t* stuck;             /* [chains] discrete updates that met only -inf */
    int32_t* capped;            /* [chains] slice updates that accepted nothing */
    int64_t* evals;             /* [chains] evaluations of g_v */
} lhvi_fgibbs_t;
/* the initial state into x, idx [V][chains]: observed variables their value (a discrete one the index of its state, 0 when it
 * is none of them), hidden discrete ones state floor(u S), hidden continuous ones lo + u (hi - lo); s->init_x replaces the draws */
int lhvi_fgibbs_init(const lhvi_graph_t* g, const lhvi_fgibbs_t* s, int64_t chains, double* x, int32_t* idx, void* stream);
/* iterations [it_begin, it_end) of every chain; x, idx in / out, so a run is any number of calls.  col_ptr_host, hub_ptr_host:
 * HOST copies of s->col_ptr / s->hub_ptr (the launch sizes).  A chain's samples depend neither on `chains`, nor on the split into
 * calls, nor on hub_degree up to the summation order of g_v (lane form: row order; hub form: 64 strided partial sums, then the
 * fixed tree of the wave reduction).  LHVI_E_UNSUPPORTED: a lifted graph, chains > 2^24, max_shrink > 510. */
int lhvi_fgibbs_run(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_fgibbs_t* s, int64_t chains, int32_t it_begin,
                    int32_t it_end, const int32_t* col_ptr_host, const int32_t* hub_ptr_host, double* x, int32_t* idx, void* stream);
/* chain `chain` of `chains` on the HOST through the device's code (csrc/fgibbs.hpp) with one "lane", in the sequential order:
 * every pointer is host memory, the arrays have the device's layout and the chain touches its own column only.  init != 0: set
 * the chain's initial state first. */
int lhvi_fgibbs_chain_host(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_fgibbs_t* s, int64_t chains, int64_t chain,
                           int32_t init, int32_t it_begin, int32_t it_end, double* x, int32_t* idx);

/* ---- Exact Gaussian-MRF marginals: dense blocked fp64 Cholesky (osi/utils.py get_gaussian_mean_params_from_quadratic_params;
 * csrc/gauss_exact.hip, csrc/gauss_exact.hpp) ----------------------------------------------------------------------------------
 * p(x) ~ exp(x'Ax + b'x + c) over N hidden variables, J = -(A + A^T) = L L^T, X = L^-1, Sig = X^T X, mu = X^T (X b),
 * var_j = sum_i X_ij^2, log det J = 2 sum log L_ii.  A matrix on the device is a "packed triangle": padded to T = ceil(N / NB)
 * tiles a side (identity on the padding), lower block triangle only, tile (i, j) at (i (i + 1) / 2 + j) NB^2 doubles,
 * column-major inside a tile.  All indices are 64-bit.  N = 0: every call returns LHVI_OK without a launch.
 * LHVI_E_UNSUPPORTED: more than 46340 tiles a side. */
#define LHVI_GAUSS_EXACT_NB 64
/* doubles of one packed triangle / of the workspace of lhvi_gauss_exact_moments */
size_t lhvi_gauss_exact_tri_doubles(int64_t N);
size_t lhvi_gauss_exact_ws_doubles(int64_t N);
/* J and b from the contributions of the conditioned factors, sorted by the host: entry e is J[ent_row[e]][ent_col[e]], row >=
 * col, each pair once; vals[ent_ptr[e] .. ent_mid[e]) are the terms of A[row][col] and vals[ent_mid[e] .. ent_ptr[e + 1]) those
 * of A[col][row], each in the reference's (factor, i, j) order (a diagonal entry has the first range only); b_vals[b_ptr[r] ..
 * b_ptr[r + 1]) the terms of b[r].  One thread sums one entry in that order: the same input gives the same bits.
 * Jt (a packed triangle) and b [T NB] must be zero on entry. */
int lhvi_gauss_exact_assemble(int64_t N, int64_t n_ent, const int32_t* ent_row, const int32_t* ent_col, const int64_t* ent_ptr,
                              const int64_t* ent_mid, const double* vals, const int64_t* b_ptr, const double* b_vals, double* Jt,
                              double* b, void* stream);
/* Jt = -(A + A^T) from a dense row-major A [N][N] */
int lhvi_gauss_exact_pack(int64_t N, const double* A, double* Jt, void* stream);
/* J -> L in place (Lt), blocked right-looking: per step a diagonal-tile kernel, a panel solve, a trailing update.  Xt: a second
 * packed triangle, zero on entry; its diagonal tiles receive L_kk^-1.  tlog [T]: scratch; logdet [1] = log det J.
 * bad [1]: the caller sets it to INT32_MAX; a pivot <= 0 or NaN lowers it to its column (atomic min on the integer) and is
 * taken as 1, so every kernel of the run ends normally and the outputs are meaningless (the caller raises, LHVI_E_NOT_PD). */
int lhvi_gauss_exact_factor(int64_t N, double* Lt, double* Xt, double* tlog, int32_t* bad, double* logdet, void* stream);
/* X = L^-1 by blocked forward substitution, after lhvi_gauss_exact_factor on the same two triangles */
int lhvi_gauss_exact_inverse(int64_t N, const double* Lt, double* Xt, void* stream);
/* mu, var [T NB] (entries >= N: padding) from X and b [T NB]; sums in a fixed order.  ws: lhvi_gauss_exact_ws_doubles(N) */
int lhvi_gauss_exact_moments(int64_t N, const double* Xt, const double* b, double* ws, double* mu, double* var, void* stream);
/* out [S][S] = Sig[cols[a]][cols[b]] from the columns of X; S <= 65535; a column outside [0, N) gives zeros */
int lhvi_gauss_exact_cov(int64_t N, const double* Xt, int32_t S, const int32_t* cols, double* out, void* stream);
/* the whole computation on the HOST through the same tile routines in the same order (csrc/gauss_exact.hpp): J [N][N] dense
 * row-major (its lower triangle is read), b, mu, var [N], logdet [1]; bad_col (may be NULL): the first column with a pivot <= 0
 * or NaN, else -1.  LHVI_E_NOT_PD when there is one. */
int lhvi_gauss_exact_host(int64_t N, const double* J, const double* b, double* mu, double* var, double* logdet, int64_t* bad_col);

/* ---- Exact Gaussian chains: batched block-tridiagonal fp64 Cholesky with the covariance recursion (the conditioned relational
 * Kalman filters of Demo/RKF; csrc/gauss_chain.hip, csrc/gauss_chain.hpp, docs/kernels_gauss_chain.md) --------------------------
 * B independent systems of M blocks of edge n, all row-major: D [B][M][n][n] the symmetric diagonal blocks of J (the lower
 * triangle is read), O [B][M-1][n][n] = J[block t, block t + 1] (rows: block t; may be NULL when M == 1), h [B][M][n].
 * Results: mu, var [B][M][n]; cov [B][M][n][n] = Sig[t, t] and cross [B][M-1][n][n] = Sig[t, t + 1], each written unless NULL;
 * logdet [B] = log det J; bad [B][2] = (block, column) of the first pivot <= 0 or NaN of a system, (-1, -1) when there is
 * none: such a pivot is taken as 1, the kernel ends normally, that system's results are meaningless and the others' are
 * untouched.  ws: lhvi_gauss_chain_ws_doubles(B, M, n) doubles (W_t, C_t, y_t of every block for the backward pass, and
 * the working tiles of a system when n > 32).  One workgroup per system, time sequential; fixed order, no atomics: a
 * system's bits do not depend on B or on its position.  B == 0 or M == 0: nothing is launched.
 * LHVI_E_ARG: n < 1, negative B or M, a NULL array.  LHVI_E_UNSUPPORTED: n > LHVI_GAUSS_CHAIN_MAX_BLOCK. */
#define LHVI_GAUSS_CHAIN_MAX_BLOCK 128
size_t lhvi_gauss_chain_ws_doubles(int64_t B, int64_t M, int64_t n);
int lhvi_gauss_chain_solve(int64_t B, int64_t M, int64_t n, const double* D, const double* O, const double* h, double* ws, double* mu,
                           double* var, double* cov, double* cross, double* logdet, int32_t* bad, void* stream);
/* the same on the HOST through the same code with one "lane" (host pointers); LHVI_E_NOT_PD when some system has a bad pivot */
int lhvi_gauss_chain_host(int64_t B, int64_t M, int64_t n, const double* D, const double* O, const double* h, double* ws, double* mu,
                          double* var, double* cov, double* cross, double* logdet, int32_t* bad);
/* The same systems solved in S segments along time (one level of nested dissection; csrc/gauss_chain_part.hip,
 * docs/kernels_gauss_chain.md): S_eff = max(1, min(S, (M + 1) / 2)); S_eff - 1 single-block separators between S_eff interiors
 * of (M - S_eff + 1) / S_eff blocks, the first (M - S_eff + 1) % S_eff of them one block longer.  lhvi_gauss_chain_segments
 * writes the first and last block of every interior to first, last [S_eff] (either may be NULL) and returns S_eff (0 when
 * M < 1 or S < 1); separator p is block last[p] + 1.  Three launches on the stream: one workgroup per (system, interior) solves
 * the interior and its two spikes; the reduced chain of the separators is assembled and solved by the serial kernel; one
 * workgroup per (system, interior) corrects the interior.  No atomics and a fixed order: with (M, n, S) fixed a system's
 * bits do not depend on B, on its position or on cov / cross being NULL; they differ from the serial solve's and between
 * different S.  S_eff == 1 is lhvi_gauss_chain_solve itself.  bad [B][2]: the bad pivot with the lowest block index among
 * those met in the interiors and in the reduced chain (reported at its separator's block); the position may differ from
 * the serial solve's, (-1, -1) holds for exactly the same systems.  ws: lhvi_gauss_chain_part_ws_doubles(B, M, n, S) doubles.
 * Return codes as lhvi_gauss_chain_solve, and LHVI_E_ARG for S < 1. */
size_t lhvi_gauss_chain_part_ws_doubles(int64_t B, int64_t M, int64_t n, int64_t S);
int lhvi_gauss_chain_part_solve(int64_t B, int64_t M, int64_t n, int64_t S, const double* D, const double* O, const double* h,
                                double* ws, double* mu, double* var, double* cov, double* cross, double* logdet, int32_t* bad,
                                void* stream);
int lhvi_gauss_chain_part_host(int64_t B, int64_t M, int64_t n, int64_t S, const double* D, const double* O, const double* h,
                               double* ws, double* mu, double* var, double* cov, double* cross, double* logdet, int32_t* bad);
int64_t lhvi_gauss_chain_segments(int64_t M, int64_t S, int64_t* first, int64_t* last);

/* ---- Conditional queries on a fitted mixture belief (osi/mixture_beliefs.py:505-746, osi/utils.py:21-98; csrc/mixture.hip,
 * csrc/mixture.hpp) ---------------------------------------------------------------------------------------------------------
 * q(x) = sum_k w_k prod_v q_vk(x_v) over V "rows" (ground variables or lifted clusters); q_vk is N(mu_vk, var_vk) or a
 * categorical pi_vk.  Conditioning on observed rows re-weights the components: w' = softmax(log w + sum_o log q_ok(x_o)).
 * Variables enter every call as int32 row indices, repeats allowed.  Evidence is X [M][n_obs] doubles: a value (continuous
 * row) or a state index (discrete row), NaN = not observed in that evidence row. */
#define LHVI_MIX_MAX_K 128      /* the limit of lhvi_vi_map_bfgs; beyond it every call returns LHVI_E_UNSUPPORTED */
#define LHVI_MIX_TILE 64        /* observed variables of one stage-1 partial sum of lhvi_mix_condition */
#define LHVI_MIX_ROWS 4         /* evidence rows that share one pass over the records */
#define LHVI_MIX_GAUSSIAN 0     /* normaliser: c = -1/2 log 2 pi + 1/2 log(1 / var) (osi/mixture_beliefs.py:538) */
#define LHVI_MIX_VI 1           /* normaliser: c = -log(2.506628274631 var), the density of VarInference.norm_pdf */
typedef struct lhvi_mix {
    int32_t V, K, Dmax;
    const int32_t* nstates;     /* [V] 0: continuous row, > 0: discrete row of that many states, < 0: row without parameters */
    const double* logw;         /* [K] log w */
    const double* rec;          /* [V][K][3] (c, mu, 1 / var), c by the normaliser; the layout of lhvi_exact_mix_prepare */
    const double* lpi;          /* [V][K][Dmax] log pi (-inf beyond the row's states), or NULL without discrete rows */
    const double* pi;           /* [V][K][Dmax] pi, the caller's eta_d itself, or NULL without discrete rows */
} lhvi_mix_t;
/* logw, rec and lpi (may be NULL when no row is discrete) from w [K], eta_c [V][K][2] (mean, variance; may be NULL when no
 * row is continuous), eta_d [V][K][Dmax] and nstates [V]: the arrays of lhvi_vi_t, read in place */
int lhvi_mix_prepare(int32_t V, int32_t K, int32_t Dmax, int32_t normaliser, const double* w, const double* eta_c,
                     const double* eta_d, const int32_t* nstates, double* logw, double* rec, double* lpi, void* stream);
/* doubles of the workspace of lhvi_mix_condition: M * tiles * K, tiles = ceil(n_obs / LHVI_MIX_TILE) */
size_t lhvi_mix_condition_ws_doubles(int64_t M, int32_t n_obs, int32_t K);
/* comp [M][K] = sum_o log q_ok(X[m][o]), logp [M] = logsumexp_k(log w + comp), condw [M][K] = exp(log w + comp - logp); each
 * output may be NULL.  Two stages, no atomics: a thread sums one tile of observed variables in index order for one component
 * and LHVI_MIX_ROWS evidence rows, then a thread per evidence row adds the tiles in index order.  The launch geometry depends on
 * (n_obs, K) only: a row's bits depend neither on M, nor on its position, nor on the run.  n_obs = 0: comp = 0, condw = w.
 * A discrete observation that is no state of its row gives NaN (the caller validates). */
int lhvi_mix_condition(const lhvi_mix_t* b, int64_t M, int32_t n_obs, const int32_t* obs_rows, const double* X, double* ws,
                       double* comp, double* logp, double* condw, void* stream);
/* marginal MAP of every (evidence row m, query q) under the weights condw [M][K] (marginal_map :723-746): xout / fout [M][n_q].
 * Discrete row: the index of the first state of largest sum_k condw[m][k] pi[q][k][s] (drv_belief_map :693-708) and that
 * probability.  Continuous row: the mode of sum_k condw[m][k] N(x; mu_qk, var_qk) inside [lo[q], hi[q]] and its log density
 * (get_scalar_gm_mode, osi/utils.py:66-98): a safeguarded Newton iteration (at most max_iter steps) from every component mean
 * clipped to the bounds, the best start kept, ties to the lowest component.  lanes: lanes per item, a power of two <= 64; the
 * answer does not depend on it.  qobs_ptr [n_q + 1] / qobs_idx (or NULL / NULL, then X is not read): the positions of query q
 * in the observed list of X [M][n_obs]; a query that row m observes there returns that value (fout NaN).  A row without
 * parameters returns NaN. */
int lhvi_mix_marginal_map(const lhvi_mix_t* b, int64_t M, const double* condw, int32_t n_q, const int32_t* query_rows,
                          const double* lo, const double* hi, int32_t n_obs, const double* X, const int32_t* qobs_ptr,
                          const int32_t* qobs_idx, int32_t lanes, int32_t max_iter, double* xout, double* fout, void* stream);
/* out [M][n_q][P] = log sum_k condw[m][k] q_qk(x[q][p]), x [n_q][P]: values (continuous row) or state indices (discrete) */
int lhvi_mix_log_belief(const lhvi_mix_t* b, int64_t M, const double* condw, int32_t n_q, const int32_t* query_rows, int32_t P,
                        const double* x, double* out, void* stream);
/* joint MAP of Nd discrete rows (drows) and Nc continuous rows (crows, bounds lo / hi [Nc]) under the log weights logw [K]:
 * joint_map_from_belief_params (:771-867) with get_multivar_gm_mode(init_xs=[xc]) (osi/utils.py:101-161), S starts, one workgroup
 * each.  Start s: x0 [S][Nc] (joint_map: column k of Mu, NOT clipped) and xd0 [S][Nd] (joint_map: argmax_s pi[n][k][s]).  Per
 * coordinate iteration (at most coord_its): projected gradient ascent with Polyak averaging on the continuous block (gamma = 0.05,
 * grad_lr = 0.01, at most grad_its = 500 steps, tol = 1e-7 in the reference), then one sweep over the discrete rows, each set to
 * the first state of largest joint density.  Outputs per start: xc [S][Nc] of the best coordinate iteration, xd [S][Nd] of the
 * LAST sweep (the reference's best_xd aliases xd, :848), best_obj [S]; the caller takes the first start of largest best_obj.
 * A start stops early when a whole coordinate iteration changed neither xd nor a bit of xc (the rest would repeat it).
 * ws: lhvi_mix_joint_map_ws_doubles() doubles.  Rows and xd0 must be valid (the caller checks). */
size_t lhvi_mix_joint_map_ws_doubles(int32_t K, int32_t Nc, int32_t Nd, int32_t Dmax, int32_t S);
int lhvi_mix_joint_map(const lhvi_mix_t* b, const double* logw, int32_t Nc, const int32_t* crows, const double* lo, const double* hi,
                       int32_t Nd, const int32_t* drows, int32_t S, const double* x0, const int32_t* xd0, int32_t coord_its,
                       double gamma, double grad_lr, int32_t grad_its, double tol, double* ws, double* xc, int32_t* xd,
                       double* best_obj, void* stream);
/* the same entry points on the HOST through the device's code (csrc/mixture.hpp) with one "lane"; every pointer is host memory */
int lhvi_mix_prepare_host(int32_t V, int32_t K, int32_t Dmax, int32_t normaliser, const double* w, const double* eta_c,
                          const double* eta_d, const int32_t* nstates, double* logw, double* rec, double* lpi);
int lhvi_mix_condition_host(const lhvi_mix_t* b, int64_t M, int32_t n_obs, const int32_t* obs_rows, const double* X, double* ws,
                            double* comp, double* logp, double* condw);
int lhvi_mix_marginal_map_host(const lhvi_mix_t* b, int64_t M, const double* condw, int32_t n_q, const int32_t* query_rows,
                               const double* lo, const double* hi, int32_t n_obs, const double* X, const int32_t* qobs_ptr,
                               const int32_t* qobs_idx, int32_t max_iter, double* xout, double* fout);
int lhvi_mix_log_belief_host(const lhvi_mix_t* b, int64_t M, const double* condw, int32_t n_q, const int32_t* query_rows,
                             int32_t P, const double* x, double* out);
int lhvi_mix_joint_map_host(const lhvi_mix_t* b, const double* logw, int32_t Nc, const int32_t* crows, const double* lo,
                            const double* hi, int32_t Nd, const int32_t* drows, int32_t S, const double* x0, const int32_t* xd0,
                            int32_t coord_its, double gamma, double grad_lr, int32_t grad_its, double tol, double* ws, double* xc,
                            int32_t* xd, double* best_obj);

/* ---- Scalar Gaussian mixtures fitted to samples by EM (sampling_utils.fit_scalar_gm_from_samples: scikit-learn's
 * GaussianMixture(n_components=K, covariance_type='diag') on one column; csrc/gmfit.hip, csrc/gmfit.hpp,
 * docs/kernels_gmfit.md) ----------------------------------------------------------------------------------------------------
 * Every row of x [R][n] is fitted on its own, one workgroup per row, the whole fit in one launch.  Per row: y = x - mean(x);
 * the start is init [R][3][K] = (w0, mu0, var0) or, with init NULL, deterministic: centres sd * Phi^-1((k + 1/2) / K), kmeans_its
 * Lloyd iterations (an empty cluster keeps its centre), one M-step from the hard assignments.  Then at most max_iter EM
 * iterations with scikit-learn's formulas (nk = sum r_k + 10 DBL_EPSILON, mu = sum r_k y / nk, var = sum r_k y^2 / nk - mu^2 +
 * reg_covar, w = nk / n renormalised), stopped when |lower bound - previous| < tol (the first previous is -inf).  Outputs are
 * the parameters after the M-step of the last iteration (mu with the mean added back), the last lower bound (the mean over
 * the samples of logsumexp_k), the iterations done and flags: bit 0 converged, bit 1 the row holds a non-finite sample (its
 * other outputs are then NaN / 0).  Sums are formed in a fixed order without atomics: a row's bits depend neither on R, nor on
 * its position, nor on the run.  LHVI_E_ARG: R < 1, n < K, K < 1 or K > LHVI_GMFIT_MAX_K, max_iter < 1, kmeans_its < 0,
 * reg_covar < 0 or NaN, a NULL array. */
#define LHVI_GMFIT_MAX_K 16
int lhvi_gm_fit(int32_t R, int64_t n, int32_t K, const double* x, const double* init, double reg_covar, double tol,
                int32_t max_iter, int32_t kmeans_its, double* w, double* mu, double* var, double* lower_bound, int32_t* n_iter,
                int32_t* flags, void* stream);
/* the same on the HOST through the device's code (csrc/gmfit.hpp) with one "lane": every sum runs in index order */
int lhvi_gm_fit_host(int32_t R, int64_t n, int32_t K, const double* x, const double* init, double reg_covar, double tol,
                     int32_t max_iter, int32_t kmeans_its, double* w, double* mu, double* var, double* lower_bound,
                     int32_t* n_iter, int32_t* flags);

/* ---- KL(p || q) of scalar Gaussian mixtures, a batch of rows in one launch (utils.kl_continuous_logpdf where both sides are
 * mixture marginals; csrc/gmkl.hip, csrc/gmkl.hpp, docs/kernels_gmkl.md) ------------------------------------------------------
 * Row r: p = (wp, mup, varp)[r][0 .. Kp), q = (wq, muq, varq)[r][0 .. Kq) (row-major [R][K]; a component of weight 0 is skipped,
 * so ragged rows are padded with zeros), bounds a[r] <= b[r] (+-inf allowed).  The integrand is f(x) = exp(lp) (lp - lq) with
 * lp, lq the log densities by a max-shifted log-sum-exp, and f = 0 where exp(lp) == 0.
 *   range     L = max(a, min_k(mu_k - 10 sd_k)), U = min(b, max_k(mu_k + 10 sd_k)) over p's components; U <= L: kl = 0, status 0
 *   panels    P = ceil((U - L) / (8 sd_min)) equal panels, sd_min of p's narrowest component, at least 1 and at most
 *             LHVI_GMKL_MAX_PANELS (the cap sets status bit 1; the result is still returned): no component of p can fall
 *             between the nodes of the first pass
 *   pass 1    QUADPACK's 21-point Gauss-Kronrod rule with its error estimate (dqk21) on every panel; area0 = the sum of the
 *             panel results in order; bound = max(epsabs, epsrel |area0|)
 *   pass 2    panel by panel, left to right, depth-first bisection: an interval is accepted when its estimate is
 *             <= bound * width / (U - L), or at depth 40 (status bit 0 when the estimate is not met there); an interval whose
 *             estimate is not finite, and every interval after 4096 bisections of the row, is accepted as it stands (status
 *             bit 0).  Accepted results and estimates are added in that left-to-right order.
 * Outputs per row: kl, abserr (the sum of the accepted estimates), status, neval (integrand evaluations); abserr, status and
 * neval may be NULL.  A row with a non-finite parameter or bound NaN, a variance <= 0, a negative weight or all-zero weights
 * on either side gets kl = abserr = NaN and status bit 2; the other rows are unaffected.  Where q underflows and p does not the
 * integrand, and with it kl, is +inf.  One wavefront per row, no atomics: a row's bits depend neither on R, nor on its position,
 * nor on the run.  ws: lhvi_gm_kl_ws_doubles(R) doubles, or NULL when that is 0 (it is: the panel list and the stack of a row are
 * in LDS).  LHVI_E_ARG: R < 1, Kp < 1, Kq < 1, a NULL required pointer, epsabs or epsrel negative or NaN. */
#define LHVI_GMKL_MAX_PANELS 1024
size_t lhvi_gm_kl_ws_doubles(int32_t R);
int lhvi_gm_kl(int32_t R, int32_t Kp, const double* wp, const double* mup, const double* varp, int32_t Kq, const double* wq,
               const double* muq, const double* varq, const double* a, const double* b, double epsabs, double epsrel, double* ws,
               double* kl, double* abserr, int32_t* status, int32_t* neval, void* stream);
/* the same on the HOST through the device's code (csrc/gmkl.hpp), the nodes one after another */
int lhvi_gm_kl_host(int32_t R, int32_t Kp, const double* wp, const double* mup, const double* varp, int32_t Kq, const double* wq,
                    const double* muq, const double* varq, const double* a, const double* b, double epsabs, double epsrel,
                    double* kl, double* abserr, int32_t* status, int32_t* neval);
/* the same on the HOST with ANY log density as q: logq(x, r, user) is log q(x) of row r (the reference's kl_continuous_logpdf with
 * log_p a mixture and log_q any callable).  p, the bounds, the tolerances, the outputs and the invalid rows as above; where logq
 * returns -inf and p does not vanish the integrand, and with it kl, is +inf (status bit 0).  LHVI_E_ARG also for logq == NULL. */
int lhvi_gm_kl_fn_host(int32_t R, int32_t Kp, const double* wp, const double* mup, const double* varp,
                       double (*logq)(double x, int64_t row, void* user), void* user, const double* a, const double* b,
                       double epsabs, double epsrel, double* kl, double* abserr, int32_t* status, int32_t* neval);

/* ---- Joint log potentials of assignments of a hybrid Gaussian MRF and the first-index arg-max (the joint MAP of the exact and
 * Gibbs baselines, osi/hybrid_mln_experiment.py:267-279 with osi/utils.py::eval_joint_assignment_energy; csrc/hg_energy.hip,
 * csrc/hg_energy.hpp, docs/kernels_hg_energy.md) ----------------------------------------------------------------------------
 * Row s of S is one joint assignment of the flat model m.  Its discrete state: with x_d == NULL the digits of configuration
 * cfg_begin + s (from dstride / dstates, as lhvi_exact_configs numbers them), else x_d [S][Nd] and cfg_begin is ignored (m->M and
 * m->dstride are then not read).  Its continuous point: x_c [S][Nc] (may be NULL when Nc == 0).
 * out [s] = the sum of the quadratic descriptors, in descriptor order, each (sum_a sum_j P[a][j] x_a x_j, row-major, one term
 * after the other) + (sum_a b_a x_a) + c at the local discrete state, then the table descriptors in descriptor order: the same
 * order on the device and on the host.  One lane per row; a row's bits depend neither on S nor on its position.
 * S == 0: LHVI_OK without a launch.  LHVI_E_UNSUPPORTED: Nc > LHVI_EXACT_MAX_NC.  LHVI_E_ARG: a NULL required pointer, S < 0,
 * cfg_begin < 0 without x_d.  Nd is not limited.  A digit outside its variable's range is the caller's error. */
int lhvi_hg_energy(const lhvi_exact_t* m, int64_t S, int64_t cfg_begin, const int32_t* x_d, const double* x_c, double* out,
                   void* stream);
/* the same on the HOST through the device's code (csrc/hg_energy.hpp); every pointer is host memory */
int lhvi_hg_energy_host(const lhvi_exact_t* m, int64_t S, int64_t cfg_begin, const int32_t* x_d, const double* x_c, double* out);
/* index [0] = the smallest index that attains the maximum over the non-NaN entries of v [n], value [0] = that entry; n == 0 or
 * all NaN: index -1, value NaN.  -inf wins when nothing is larger; +0 and -0 tie.  Two stages, 64-bit indices; a comparison
 * reduction, so the result is the definition's for every n.  ws: lhvi_argmax_first_ws_bytes(n) bytes of device memory. */
size_t lhvi_argmax_first_ws_bytes(int64_t n);
int lhvi_argmax_first(int64_t n, const double* v, int64_t* index, double* value, void* ws, void* stream);
int lhvi_argmax_first_host(int64_t n, const double* v, int64_t* index, double* value);

/* ---- Nonparametric variational inference (osi/NPVI.py: Gershman-style NPVI on a K-component product mixture; csrc/npvi.hip,
 * csrc/npvi.hpp, docs/kernels_npvi.md) -----------------------------------------------------------------------------------------
 * Parameters: tau [K] (w = softmax(tau)), theta_c [V][K][2] = (mu, log var) of the hidden continuous variables, rho [V][K][Dmax]
 * (pi = softmax(rho) over a hidden discrete variable's own states).  The lhvi_vi_t passed alongside is the parameter VIEW the
 * kernels and every query read: K, T, gh_x, gh_w, Dmax, edge_axis (required) and w, eta_c = (mu, var), eta_d = pi, which the update
 * keeps in step with tau / theta_c / rho.  obs_var must be NULL; quirks (LHVI_VI_GAUSSIAN_PDF for the queries) and the factor lists
 * are not read.
 * Objective (NPVI.py:133-159): obj = sum_f c_f sum_k w_k E_{q_k}[-log phi_f] (Gauss-Hermite on the factor's grid,
 * mixture_beliefs.py:160-256 / :293-340 with neg_lpot_only) + sum_k w_k logsumexp_j(L[k][j] + log w_j), L[k][j] = sum_v c_v l_v(k, j)
 * (the Jensen bound on the mixture entropy, :903-942).  The gradient is that of the reference's auxiliary objective: the grid
 * nodes and node weights are constants (tf.stop_gradient), the factor term is differentiated through log b alone; the entropy
 * term is differentiated fully.  Sums are formed in a fixed order without atomics: a run's bits do not depend on the run.
 * A factor's axis lengths (T per hidden continuous argument, #states per hidden discrete one, 1 per observed one) must sum to at
 * most LHVI_NPVI_MAX_SLOTS; a longer factor makes obj NaN (the caller checks: max_slots). */
#define LHVI_NPVI_MAX_K 16
#define LHVI_NPVI_MAX_SLOTS 24
typedef struct lhvi_npvi_opt {
    double* tau;                /* [K] mixture logits */
    double* theta_c;            /* [V][K][2] (mu, log var) */
    double* rho;                /* [V][K][Dmax] category logits */
    double *m_tau, *s_tau, *m_c, *s_c, *m_rho, *s_rho;   /* Adam moments, shaped like tau / theta_c / rho */
    double *g_tau, *g_c, *g_rho;/* gradient scratch, same shapes */
    double* obj;                /* [1] scratch for the objective when it is not logged */
    double* w;                  /* [K]: the arrays the lhvi_vi_t passed alongside points to (the step writes what the view reads) */
    double* eta_c;              /* [V][K][2] (mu, var = exp(log var)) */
    double* eta_d;              /* [V][K][Dmax] softmax(rho) */
    const double* mu_lo;        /* [V] the variable's domain: mu is clipped to [mu_lo, mu_hi] after every step (NPVI.py:123) */
    const double* mu_hi;        /* [V] */
    double lvar_lo, lvar_hi;    /* log of Var_bds (NPVI.py:107,124) */
    const double* var_count;    /* [V] sharing_count of the variables (cluster sizes), NULL = ones */
    const double* fac_count;    /* [F] sharing_count of the factors, NULL = ones */
    double lr, b1, b2, eps;     /* tf.train.AdamOptimizer: lr, 0.9, 0.999, 1e-8 */
    int32_t t;                  /* updates done before this call (the step size uses t + i + 1) */
    /* hints, 0 = unknown: the largest sum of axis lengths of a factor and the largest arity.  With max_arity <= 3 and no interpreted
     * formula (lhvi_pots_t.interpreted == 0) the factor kernel's lean builds run (max_slots <= 8: the one with the smaller LDS
     * tables).  A factor beyond a hint makes obj NaN. */
    int32_t max_slots;
    int32_t max_arity;
} lhvi_npvi_opt_t;
size_t lhvi_npvi_workspace_bytes(const lhvi_graph_t* g, const lhvi_vi_t* p);
/* obj [1] and the gradient of the auxiliary objective at the view's parameters: g_tau [K] (through the softmax), g_c [V][K][2]
 * (d/d mu, d/d log var; zero rows for other variables), g_rho [V][K][Dmax] (through the softmax; zero beyond a variable's states
 * and for other variables).  LHVI_E_ARG: K < 1, K > LHVI_NPVI_MAX_K, T < 1, a NULL array (edge_axis included). */
int lhvi_npvi_grad(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const double* var_count,
                   const double* fac_count, int32_t max_slots, int32_t max_arity, double* obj, double* g_tau, double* g_c,
                   double* g_rho, void* ws, size_t ws_bytes, void* stream);
/* `iterations` updates (NPVI.run, NPVI.py:230-263) enqueued back to back, no host work in between: per update one gradient pass
 * and ONE launch for TensorFlow's Adam on tau / rho / theta_c (lr_t = lr sqrt(1 - b2^t) / (1 - b1^t), theta -= lr_t m /
 * (sqrt(v) + eps)), the clips of mu and log var, tau := 0 while the update's index < fix_mix_its (its moments keep running), both
 * softmaxes and eta_c.  obj_log: device [iterations] or NULL -- obj_log[i] = the objective at the parameters before update i. */
int lhvi_npvi_run(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const lhvi_npvi_opt_t* o, int32_t iterations,
                  int32_t fix_mix_its, double* obj_log, void* ws, size_t ws_bytes, void* stream);
/* the same on the HOST through the device's code (csrc/npvi.hpp) with one "lane": every pointer is host memory, sums run in index order */
int lhvi_npvi_grad_host(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const double* var_count,
                        const double* fac_count, double* obj, double* g_tau, double* g_c, double* g_rho);
int lhvi_npvi_run_host(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const lhvi_npvi_opt_t* o,
                       int32_t iterations, int32_t fix_mix_its, double* obj_log);

/* ---- OneShot (osi/OneShot.py: the same K-component product mixture fitted to the Bethe free energy; csrc/oneshot.hip,
 * csrc/oneshot.hpp, docs/kernels_oneshot.md) ------------------------------------------------------------------------------------
 * Parameters, parameter view, lhvi_npvi_opt_t, limits (LHVI_NPVI_MAX_K, LHVI_NPVI_MAX_SLOTS), hints and the update are NPVI's.
 * Objective (OneShot.py:53-150): obj = sum_f c_f E_b[-log phi_f + log b_f] (the factor grid of NPVI with log b inside the expectant,
 * mixture_beliefs.py:160-256 / :293-340 with neg_lpot_only=False) + sum_v var_coef[v] E_b[log b_v] (:441-502; Gauss-Hermite at the K * T
 * nodes of a continuous variable, the states of a discrete one).  var_coef [V], required: c_v (1 - deg_v) for a hidden variable --
 * c_v its sharing count, deg_v the number of ground factors a (member) variable touches -- and 0 for an observed one; rows with 0
 * are not evaluated.  The gradient is that of the reference's auxiliary objective: nodes, node weights and the expectant are
 * constants, both terms are differentiated through log b alone.  Fixed-order sums, no atomics.
 * LHVI_E_ARG: as for lhvi_npvi_*, and a NULL var_coef. */
size_t lhvi_oneshot_workspace_bytes(const lhvi_graph_t* g, const lhvi_vi_t* p);
int lhvi_oneshot_grad(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const double* var_count,
                      const double* fac_count, const double* var_coef, int32_t max_slots, int32_t max_arity, double* obj, double* g_tau,
                      double* g_c, double* g_rho, void* ws, size_t ws_bytes, void* stream);
/* `iterations` updates (OneShot.run, OneShot.py:221-254: the loop of NPVI.run) enqueued back to back; obj_log as in lhvi_npvi_run */
int lhvi_oneshot_run(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const lhvi_npvi_opt_t* o,
                     const double* var_coef, int32_t iterations, int32_t fix_mix_its, double* obj_log, void* ws, size_t ws_bytes,
                     void* stream);
/* the same on the HOST through the device's code (csrc/npvi.hpp, csrc/oneshot.hpp) with one "lane": host pointers, sums in index order */
int lhvi_oneshot_grad_host(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const double* var_count,
                           const double* fac_count, const double* var_coef, double* obj, double* g_tau, double* g_c, double* g_rho);
int lhvi_oneshot_run_host(const lhvi_graph_t* g, const lhvi_pots_t* pots, const lhvi_vi_t* p, const lhvi_npvi_opt_t* o,
                          const double* var_coef, int32_t iterations, int32_t fix_mix_its, double* obj_log);

/* ---- Colour refinement (CompressedGraphWithObs.py / CompressedGraphSorted.py) --------------------
 * One half-round each; colours are dense int32 ids (the rank of the item's 64-bit signature fingerprint among the distinct
 * fingerprints).  ws: lhvi_color_workspace_bytes(g) bytes.
 * result: device int32[4] = {number of colours, fingerprint collision (two items agree on the first 64-bit fingerprint and
 * differ on the second: the Python callers raise LhviError -- the seed is a constant, nothing is retried), table overflow
 * (method 0 only: repeat the call with method 1), 0}.
 * method 0: the signature kernel finds-or-inserts each fingerprint in a 1 M-slot hash table and only the distinct keys are
 *           sorted (the answer has few of them: ~30 k on a 10 M-edge relational graph);
 * method 1: radix sort of all items' fingerprints.  Both give the same colours. */
#define LHVI_COLOR_HASH 0
#define LHVI_COLOR_SORT 1
size_t lhvi_color_workspace_bytes(const lhvi_graph_t* g);
/* SuperF.split_by_structure CGWO.py:152-175: signature = (old colour, nb rv colours [sorted iff symmetric]) */
int lhvi_color_refine_factors(const lhvi_graph_t* g, const uint8_t* pot_symmetric_per_factor, const int32_t* rv_color,
                              const int32_t* f_color, int32_t* f_color_out, int32_t* result,
                              void* ws, size_t ws_bytes, int32_t method, void* stream);
/* SuperRV.split_by_structure CGWO.py:47-76: signature = (old colour, sorted multiset of nb factor colours) */
int lhvi_color_refine_rvs(const lhvi_graph_t* g, const int32_t* f_color, const int32_t* rv_color,
                          int32_t* rv_color_out, int32_t* result, void* ws, size_t ws_bytes, int32_t method, void* stream);

/* the representative of every cluster: first_out[c] = smallest i with color[i] == c, or n when colour c has no member
 * (SuperRV.update_nb CompressedGraphWithObs.py:41-45 and SuperF.update_nb :148-150 read the neighbourhood of
 * `next(iter(self.rvs))` / `next(iter(self.factors))` -- any member; this build always takes the first).  color [n] on the
 * device, values in [0, n_colors). */
int lhvi_color_first_members(const int32_t* color, int32_t n, int32_t n_colors, int32_t* first_out, void* stream);

/* sums_out[s] = values[offsets[s]] + values[offsets[s] + 1] + ... in index order (one running sum per segment, like
 * SuperRV.get_value CompressedGraphWithObs.py:24-28 over a cluster's observed members); offsets [n_segments + 1], ascending. */
int lhvi_color_segment_sums(const double* values, const int64_t* offsets, int32_t n_segments, double* sums_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LHVI_H */
