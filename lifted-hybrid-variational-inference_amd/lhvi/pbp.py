"""Particle belief propagation on the GPU: ``EPBP`` (ground) and ``HybridLBP`` (lifted).

Same surface as the reference (``EPBPLogVersion.py:14-394``, ``HybridLBPLogVersion.py:15-536``):
``EPBP(g, n, proposal_approximation).run(iteration)``, ``.belief(x, rv, ...)``, ``.probability(a, b, rv)``,
``.map(rv)``, attributes ``.message .sample .q .eta_message``; class attributes ``var_threshold`` /
``max_log_value`` keep the reference's values.

``run`` keeps all state (particles, log-message tables, proposals) resident in HBM and issues one sweep as
four launches through the C ABI (``csrc/pbp.hip``): v2f, proposal, resample, f2v.

Sampling.  The reference draws particles with ``scipy.stats.norm(...).rvs`` on NumPy's global RNG while
iterating ``g.rvs`` (``EPBPLogVersion.py:61-70``).  ``sampler='host'`` (default) reproduces exactly that stream
(``standard_normal(n) * sqrt(var) + mu`` in ``g.rvs`` order), so a seeded run matches the reference draw for
draw when ``g.rvs`` is ordered; ``sampler='device'`` uses the counter-based Philox generator of
``lhvi_pbp_resample`` (no host round trip; what the benchmark uses); a callable
``sampler(k, flat, q) -> [V, n] array`` injects particles (parity tests inject the reference's draws).
"""
from __future__ import annotations

import os
from math import e, log, sqrt

import numpy as np

from . import _abi, pbp_plan, pbp_query
from .flat import flatten

# Schedules of the f -> v half sweep (_ParticleSweep._launch_f2v): the lhvi_pbp_f2v calls in issue order, each as (stream, kernel
# families, further flags, timed by f2v_events).  Every schedule names each family exactly once.
_F2V_LONG = _abi.PBP_F2V_HEAVY | _abi.PBP_F2V_SMALL
_F2V_SHORT = _abi.PBP_F2V_PAIR | _abi.PBP_F2V_FAST | _abi.PBP_F2V_CQ | _abi.PBP_F2V_GENERIC
F2V_SCHEDULES = {
    'one': (('main', _abi.PBP_F2V_ALL, 0, False),),
    'timed': (('main', _F2V_LONG, 0, True), ('main', _F2V_SHORT, 0, False)),
    'overlap': (('side', _F2V_SHORT, 0, False), ('main', _F2V_LONG, _abi.PBP_SHARE_CUS, True)),
}


def _stream(st):
    """the current stream's pointer unless the caller has it at hand (a null pointer is a stream too: the default one)"""
    return _abi.stream_ptr() if st is None else st


class _ParticleSweep:
    var_threshold = 3
    max_log_value = 700
    _epbp_discrete = True
    verbose = False
    listed_proposal = True          # the proposal kernel starts from per-variable records (else it walks the graph arrays)
    dynamic_f2v = True              # the persistent f2v kernels claim their work in chunks (else static striding)
    paired_light = True             # the light edges are served per factor (pair_desc) instead of per edge (light_desc)
    cq_routing = True               # conditionally quadratic MLN formulas go to the quadratic-family kernels (else: generic kernel)
    small_f2v = True                # heavy-class edges with at most 16 / 32 particles on both sides: four / two edges per wavefront
    long_grid_min_edges = 1 << 16   # edges with np + T > 128 join the heavy kernel's list (grid recurrence, T <= 128) from this many on
    listed_resample = True          # the device sampler draws for the hidden continuous variables only, two per wavefront
    sliced_proposal = True          # rows of more than prop_slice incident edges are cut into slices, a wavefront per slice
    prop_slice = 64
    packed_v2f = True               # variables with at most four particles share a wavefront in the v -> f half (sixteen each)
    overlap_f2v = True              # the short f -> v kernels (pair / light / cq / generic lists) on a second stream beside the heavy kernel, which
                                    # then leaves a workgroup per CU free (LHVI_PBP_SHARE_CUS): 15.20 -> 14.66 ms per sweep on the headline graph (the
                                    # heavy kernel 10.65 -> 11.26 ms, the 1.25 ms of the others hidden; same bits).  Only for a heavy list of at
    overlap_min_heavy = 1 << 16     # least this many edges: the few-particle kernels lose by it (4.55 -> 4.60 ms at n = 16), small graphs gain nothing
    fused_var_kernel = True         # few particles, device sampler: v -> f, proposal update and the new sample of a continuous variable in
                                    # ONE pass over its rows (lhvi_pbp_var_fused) instead of three launches; same bits
    fused_max_particles = 64        # ... up to this many particles.  With a row's loads in flight together (csrc/pbp.hip, FUSED_CH) the fused kernel
                                    # wins at every width: n = 10 / 16 / 20 / 32: 5.65 / 5.83 / 8.56 / 9.53 -> 4.97 / 5.03 / 8.25 / 9.30 ms per sweep
                                    # (profiles/r05_experiments.md item 7; walked edge by edge it was a draw at n <= 16 and a loss beyond); 33 - 64
                                    # particles take lhvi_pbp_var_fused64, one variable per wavefront (profiles/fused64_experiments.md)
    exact_queries = False           # map / probability / belief answer per-variable calls from ONE batched pass over all
                                    # variables, made at the first call after run() (True: one fminbound / log_area / quad per call)
    map_mode = 'fminbound'          # what the batched map() runs per variable: the reference's fminbound iteration (lhvi_pbp_map_brent)
                                    # or 'global': scan + bracket refinement (map_all)
    # state that is set later than _setup, if at all (class level: on_flat and the coarse-to-fine engine's states skip __init__)
    var_gid = None                  # int64 device tensor: the variables' global ids, which key the device sampler on a shard (lhvi/dist.py)
    _side = None                    # the second stream of the 'overlap' schedule, made by its first launch
    _query_f2v = None               # belief_rv_all's table of messages at the query points
    _stable_partition = False       # (lifted) the sweeps ran on the stable partition: a row is a cluster of equal ground variables
    _ground = None                  # (lifted, on arrays) the ground graph and its colours, for the queries of ground variables

    # ---- set-up ------------------------------------------------------------------------------
    def _setup(self, graph_like, flat=None, edge_key=None, sides='vf', edge_skip=None, owned=None):
        """`edge_key` (sharded runs): 0 / 1 per edge; every f2v work list is ordered key-0 edges first and ``part_counts``
        gives the length of that first part per list (heavy, light, fast, generic).
        `edge_skip` (owner-computes shards): boolean per edge; the f -> v message of a marked edge is somebody else's to compute,
        it enters no work list.
        `owned` (owner-computes shards): the per-variable lists of the v -> f half and of the proposal update hold the variables
        below this index only (the rank's own; the sampler's list keeps all of them: ghosts are drawn here too).
        `sides`: which half sweeps this state will run -- 'v' (v -> f, proposal, sampling: the variable-side state of a
        coarse-to-fine sweep), 'f' (f -> v and the queries: its factor-side state) or both; the work lists of the other half
        are not built."""
        flat = flat if flat is not None else flatten(graph_like, require_device_potentials=True)
        self.flat = flat
        self.dg = dg = _abi.DeviceGraph(flat)
        torch = _abi.require_gpu()
        n = self.n
        # which variable goes to which kernel, and the records those kernels read (lhvi/pbp_plan.py)
        plan = pbp_plan.var_side_plan(flat, n, owned=owned, opts=self._plan_options())
        self.np_host, self.T = plan.np_host, plan.T
        S = n + self.T
        self.f2v = dg.zeros(flat.E, S)
        self.v2f = dg.zeros(flat.E, n)
        self.eta = dg.zeros(flat.E, 2)
        self.q_dev = dg.zeros(flat.V, 2)
        self.particles = dg.zeros(flat.V, n)
        self.old_particles = dg.zeros(flat.V, n)
        self.uniq = torch.zeros(flat.V, n, dtype=torch.uint8, device=dg.device)
        self.f2v_ticket = torch.zeros(16, dtype=torch.int32, device=dg.device)    # work counters + statistics of the heavy f2v kernel (LHVI_PBP_TICKET_WORDS)
        self.flags = (_abi.PBP_EP if self.proposal_approximation == 'EP' else 0) | \
                     (_abi.PBP_EPBP_DISCRETE if self._epbp_discrete else 0) | \
                     (_abi.PBP_CQ if self.cq_routing and bool((flat.pot_kind == 8).any()) else 0) | \
                     (_abi.PBP_POW2_GROUPS if os.environ.get('LHVI_PBP_POW2_GROUPS', '0') == '1' else 0) | \
                     (_abi.PBP_NO_SPLIT_ROUND if os.environ.get('LHVI_PBP_SPLIT_ROUND', '1') == '0' else 0) | \
                     plan.flags                                 # (LHVI_PBP_POW2_GROUPS: tuning aid, scripts/diag/narrow_groups.sh;
                                                                #  LHVI_PBP_SPLIT_ROUND=0: the heavy kernel's full round by the one-term-per-read loop, profiles/split_round_experiments.md)
        self._views, self._batched = {}, {}
        self._draws = 0
        self._static_rows = False           # the rows no listed draw writes are filled once, by the first draw (_generate_sample)
        # the per-variable lists go to the device in one copy
        self.var_lists = plan.on(_abi.upload(plan.host), dg.zeros(plan.n_prop_partial, 2) if plan.n_prop_partial else None)
        for name, value in self.var_lists.named().items():      # (np_dev, resample_vars, v2f_lists, _fused, ...)
            setattr(self, name, value)
        # static work lists of the f -> v half sweep: which kernel serves which edge (lhvi/pbp_plan.py); none until they are built
        self._has_f_side = 'f' in sides
        self.f2v_lists = pbp_plan.F2vLists.empty(torch.zeros(1, dtype=torch.int32, device=dg.device))
        if self._has_f_side:
            cls = torch.zeros(max(flat.E, 1), dtype=torch.uint8, device=dg.device)
            _abi.check(_abi.lib().lhvi_pbp_classify(dg.g, dg.p, self._struct(), _abi.ptr(cls), _abi.stream_ptr()))
            self.f2v_lists = pbp_plan.f_side_plan(
                cls[:flat.E], flat, self.np_host, describe=self._describe,
                describe_cq=lambda edges: self._describe(edges, 'lhvi_pbp_describe_cq', 2 * _abi.PBP_DESC_BYTES),
                skip=None if edge_skip is None else _abi.to_dev(np.ascontiguousarray(edge_skip, dtype=bool)),
                key=None if edge_key is None else _abi.to_dev(np.ascontiguousarray(edge_key, dtype=np.int32)),
                paired_light=self.paired_light, small_f2v=self.small_f2v, long_grid_min_edges=self.long_grid_min_edges)
        for name, value in self.f2v_lists.named().items():      # (fast_edges, heavy_desc, n_heavy, part_counts, ...)
            setattr(self, name, value)

    def _describe(self, edges, entry='lhvi_pbp_describe', nbytes=_abi.PBP_DESC_BYTES):
        """the descriptors of `edges` (int32 device tensor), `nbytes` each (include/lhvi.h, lhvi_pbp_describe / lhvi_pbp_describe_cq)"""
        torch = _abi.require_gpu()
        k = int(edges.numel())
        desc = torch.empty(k * nbytes, dtype=torch.uint8, device=edges.device)
        _abi.check(getattr(_abi.lib(), entry)(self.dg.g, self.dg.p, self._struct(), _abi.ptr(edges), k, _abi.ptr(desc), _abi.stream_ptr()))
        return desc

    def _plan_options(self):
        """what the variable-side plan depends on besides the graph: the class attributes and the tuning variables, each read here"""
        env = os.environ.get
        return pbp_plan.PlanOptions(
            sampler_on_device=self.sampler == 'device', listed_proposal=self.listed_proposal, listed_resample=self.listed_resample,
            sliced_proposal=self.sliced_proposal, prop_slice=self.prop_slice, packed_v2f=self.packed_v2f,
            v2f_records=env('LHVI_PBP_V2F_REC', '1') != '0',                                   # (tuning aid: scripts/diag/v2f_records.sh)
            fused=self.fused_var_kernel and env('LHVI_PBP_FUSED', '1') != '0',
            fused_max_particles=int(env('LHVI_PBP_FUSED_MAX', self.fused_max_particles)),      # (tuning aid: scripts/diag/fused_batch.sh)
            fused_records16=env('LHVI_PBP_FUSED_REC16', '1') != '0')

    def _struct(self, var_range=None, leave_room=False):
        """`var_range`: (lo, hi) = this launch addresses the variables by range (0, 0: all of them), not through their lists;
        `leave_room`: a collective is in flight beside the persistent f -> v kernels (LHVI_PBP_LEAVE_ROOM)"""
        s = _abi.PbpStruct()
        s.n, s.T, s.flags = self.n, self.T, self.flags | (_abi.PBP_LEAVE_ROOM if leave_room else 0)
        s.var_threshold, s.max_log_value = float(self.var_threshold), float(self.max_log_value)
        s.particles, s.old_particles = _abi.ptr(self.particles), _abi.ptr(self.old_particles)
        s.uniq, s.q = _abi.ptr(self.uniq), _abi.ptr(self.q_dev)
        self.f2v_lists.install(s)
        if var_range is None:
            self.var_lists.install(s, self.listed_proposal)
        else:
            self.var_lists.install_range(s, *var_range)
        s.f2v_ticket = _abi.ptr(self.f2v_ticket) if self.dynamic_f2v else None
        return s

    # ---- the launches of a sweep: each entry point's argument list, once.  `st`: the current stream's pointer, when the caller
    # has looked it up already (on a small graph a sweep is host time, and a look-up is not free: one serves a whole phase)
    def _launch_init(self, s, st=None):
        _abi.check(_abi.lib().lhvi_pbp_init(self.dg.g, s, _abi.ptr(self.eta), _abi.ptr(self.q_dev), _abi.ptr(self.f2v), _abi.ptr(self.v2f),
                                            _stream(st)))

    def _launch_v2f(self, s, st=None):
        _abi.check(_abi.lib().lhvi_pbp_v2f(self.dg.g, s, _abi.ptr(self.f2v), _abi.ptr(self.v2f), _stream(st)))

    def _launch_proposal(self, s, st=None):
        _abi.check(_abi.lib().lhvi_pbp_proposal(self.dg.g, s, _abi.ptr(self.f2v), _abi.ptr(self.eta), _abi.ptr(self.q_dev), _stream(st)))

    def _launch_proposal_partial(self, s, ph, st=None):
        """the sites and information-form partial sums of a rank's local edges, into `ph` ([V, 2])"""
        _abi.check(_abi.lib().lhvi_pbp_proposal_partial(self.dg.g, s, _abi.ptr(self.f2v), _abi.ptr(self.eta), _abi.ptr(ph), _stream(st)))

    def _launch_proposal_finish(self, s, ph, st=None):
        _abi.check(_abi.lib().lhvi_pbp_proposal_finish(self.dg.g, s, _abi.ptr(ph), _abi.ptr(self.q_dev), _stream(st)))

    def _launch_draw(self, s, st=None):
        """the device draw of the sample `_new_sample` has started, for the variables `s` lists or ranges over"""
        _abi.check(_abi.lib().lhvi_pbp_resample_uniq(self.dg.g, s, _abi.ptr(self.var_gid), int(self.seed), int(self._draws - 1),
                                                     _abi.ptr(self.particles), _abi.ptr(self.uniq), _stream(st)))

    def _launch_fused(self, s, st=None):
        """v -> f, proposal update and the NEXT sample of the fused pass's variables, drawn into the buffer `_new_sample` makes current"""
        l, F, st = _abi.lib(), self.var_lists.fused, _stream(st)
        args = (self.dg.g, s, _abi.ptr(self.f2v), _abi.ptr(self.v2f), _abi.ptr(self.eta), _abi.ptr(self.q_dev), _abi.ptr(self.var_gid),
                int(self.seed), int(self._draws), _abi.ptr(self.old_particles), _abi.ptr(self.uniq))
        if sum(F.counts):
            _abi.check(l.lhvi_pbp_var_fused(*args, _abi.ptr(F.desc), *F.counts, st))
        if F.desc64 is not None:
            _abi.check(l.lhvi_pbp_var_fused64(*args, _abi.ptr(F.desc64), *F.counts64, st))

    def _new_sample(self):
        """start a new sample: the current particles become the old ones, and whatever was read off the old state is dropped"""
        self.old_particles, self.particles = self.particles, self.old_particles
        self._draws += 1
        self._views, self._batched = {}, {}

    # ---- sampling ----------------------------------------------------------------------------
    def _host_draw(self):
        """the reference's generate_sample stream: NumPy global RNG, g.rvs order (EPBP:61-70)"""
        flat = self.flat
        q = self.q_dev.cpu().numpy()
        out = np.zeros((flat.V, self.n))
        rows = np.flatnonzero(flat.var_hidden & flat.var_cont)
        if rows.size:
            # one call for all rows: the legacy generator fills a (rows, n) array in order and keeps its spare Box-Muller value in
            # its state, so this is the stream of one standard_normal(n) per variable in g.rvs order
            z = np.random.standard_normal((rows.size, self.n))
            d = flat.var_dom[rows]
            out[rows] = np.clip(z * np.sqrt(q[rows, 1])[:, None] + q[rows, 0][:, None], flat.dom_lo[d][:, None], flat.dom_hi[d][:, None])
        return out

    def _install(self, host_particles):
        flat = self.flat
        p = np.nan_to_num(np.array(host_particles, dtype=np.float64), nan=0.0)
        disc = np.flatnonzero(flat.var_hidden & ~flat.var_cont)
        if disc.size:                                  # the particles of a discrete variable are its states
            d = flat.var_dom[disc]
            nst = (flat.dom_ptr[d + 1] - flat.dom_ptr[d]).astype(np.int64)
            k = np.arange(int(nst.max()))[None, :]
            live = k < nst[:, None]
            rows, cols = np.nonzero(live)
            p[disc[rows], cols] = flat.dom_val[flat.dom_ptr[d][rows] + cols]
        self.old_particles, self.particles = self.particles, self.old_particles
        self.particles.copy_(_abi.to_dev(p))

    def _generate_sample(self, rest_only=False):
        """`rest_only`: the fused kernel has already drawn for its variables into the other buffer (``_launch_fused``): start the
        sample, then draw for the remaining listed variables only"""
        L = self.var_lists
        if self.sampler == 'device':
            self._new_sample()
            s = self._struct()
            listed = self.listed_resample and self.n <= 64 and L.resample_vars is not None
            by_list = rest_only or (listed and self._static_rows)
            if rest_only:
                L.install_rest(s, 'sampler')
            elif by_list:
                L.install_sampler(s)
            # else the full (unlisted) draw.  As the first device draw of a listed state it goes into the CURRENT buffer only -- the
            # other one may hold the particles the v -> f messages were evaluated at (a coarse-to-fine state, or one a host sampler
            # filled) and must keep them; it only receives the rows no later listed draw writes: the states of the discrete
            # variables and the rows of the observed ones
            if not by_list or s.n_resample_vars:
                self._launch_draw(s)
            if listed and not self._static_rows:
                if L.static_idx is not None:
                    self.old_particles.index_copy_(0, L.static_idx, self.particles.index_select(0, L.static_idx))
                self._static_rows = True
            return
        k = self._draws
        self._draws += 1
        if callable(self.sampler):
            self._install(self.sampler(k, self.flat, self.q_dev.cpu().numpy()))
        else:
            self._install(self._host_draw())
        _abi.check(_abi.lib().lhvi_pbp_uniq(self.dg.g, self.n, _abi.ptr(self.particles), _abi.ptr(L.np_dev), _abi.ptr(self.uniq),
                                            _abi.stream_ptr()))
        self._views, self._batched = {}, {}

    # ---- the sweep (EPBP.run EPBP:225-289; HybridLBP.run with c2f=-1 HLBP:430-536) -------------
    def _run_sweeps(self, iteration):
        self._launch_init(self._struct())
        self._generate_sample()
        for i in range(iteration):
            self.sweep(last=(i == iteration - 1))
        self._views, self._batched = {}, {}

    def sweep(self, last=False, f2v_events=None):
        """one flooding sweep: v2f, and unless `last`: proposal update, new sample, f2v.
        `f2v_events`: optional (start, end) torch.cuda.Event pair recorded around the f2v launch on its stream"""
        L, st = self.var_lists, _abi.stream_ptr()
        if not last and L.fused is not None and self._static_rows and self.sampler == 'device':
            # few particles: one pass per continuous variable does its v -> f messages, its proposal update and its new sample
            # (lhvi_pbp_var_fused, into the buffer the new sample makes current); the three kernels serve the other variables, each
            # from its rest list
            s = self._struct()
            self._launch_fused(s, st)
            L.install_rest(s, 'v2f')
            self._launch_v2f(s, st)
            L.install_rest(s, 'proposal')
            self._launch_proposal(s, st)
            self._generate_sample(rest_only=True)
            self._launch_f2v(self._struct(), f2v_events, st)
            return
        self._launch_v2f(self._struct(), st)
        if last:
            self._batched = {}              # the queries read v2f: what was answered from the previous messages is dropped
        else:
            self._launch_proposal(self._struct(), st)
            self._generate_sample()
            self._launch_f2v(self._struct(), f2v_events, st)

    def _f2v_schedule(self, timed=False):
        """the F2V_SCHEDULES key of this state's f -> v half sweep; `timed`: f2v_events are given"""
        want = os.environ.get('LHVI_PBP_OVERLAP')                     # (tuning aid: scripts/diag/f2v_overlap.sh)
        if (self.overlap_f2v or want == '1') and want != '0' and self.n_heavy >= self.overlap_min_heavy:
            # the long kernels of the half sweep on this stream, one workgroup per CU short of a full device; the short kernels
            # (pair / light, fast, cq, generic: other rows of f2v) on a second stream beside them.  The heavy kernel is bound
            # by VALU issue and the LDS and indifferent to 6 or 7 waves per SIMD; the pair kernel waits for its loads most of its
            # 1.1 ms -- side by side the second one costs next to nothing.
            return 'overlap'
        return 'timed' if timed else 'one'

    def _call_f2v(self, s, out=None, st=None):
        """ONE ``lhvi_pbp_f2v`` call on the current stream: the kernel families `s.flags` names (none named: all), into `out` (the
        f -> v table unless given).  What bypasses the schedules calls this."""
        _abi.check(_abi.lib().lhvi_pbp_f2v(self.dg.g, self.dg.p, s, _abi.ptr(self.v2f), _abi.ptr(self.f2v if out is None else out),
                                           _stream(st)))

    def _launch_f2v(self, s, f2v_events=None, st=None):
        """the f -> v half sweep (`lhvi_pbp_f2v`) by the schedule of _f2v_schedule.  `f2v_events`: (start, end) events recorded
        on this stream around the long kernels (heavy and small lists); the other families then run in a call of their own."""
        if not self._has_f_side:
            raise _abi.LhviError('this state was set up for the v -> f half only (sides="v")')
        st = _stream(st)
        calls = F2V_SCHEDULES[self._f2v_schedule(bool(f2v_events))]
        side = any(stream == 'side' for stream, _, _, _ in calls)
        if side:
            torch = _abi.require_gpu()
            main = torch.cuda.current_stream()
            if self._side is None:
                self._side = torch.cuda.Stream(device=self.dg.device)
                self._fork, self._join = torch.cuda.Event(), torch.cuda.Event()
            self._fork.record(main)
            self._side.wait_event(self._fork)
        base = s.flags
        for stream, families, extra, timed in calls:
            s.flags = base | families | extra
            if stream == 'side':
                with torch.cuda.stream(self._side):
                    self._call_f2v(s)
                self._join.record(self._side)
                continue
            if timed and f2v_events:
                f2v_events[0].record()
            self._call_f2v(s, st=st)
            if timed and f2v_events:
                f2v_events[1].record()
        s.flags = base
        if side:
            main.wait_event(self._join)

    # ---- dict views with the reference's keys ------------------------------------------------------
    def _host(self, name):
        if name not in self._views:
            self._views[name] = getattr(self, name).cpu().numpy()
        return self._views[name]

    @property
    def sample(self):
        flat, P = self.flat, self._host('particles')
        out = {}
        for v, rv in enumerate(flat.rvs):
            if flat.var_hidden[v]:
                out[rv] = P[v].copy() if flat.var_cont[v] else rv.domain.values
        return out

    @property
    def q(self):
        flat, Q = self.flat, self._host('q_dev')
        return {rv: (float(Q[v, 0]), float(Q[v, 1])) for v, rv in enumerate(flat.rvs)
                if flat.var_hidden[v] and (flat.var_cont[v] or self._epbp_discrete)}

    @property
    def eta_message(self):
        flat, E = self.flat, self._host('eta')
        out = {}
        for k in range(flat.var_edge.size):
            e = int(flat.var_edge[k])
            v = flat.edge_var[e]
            if flat.var_hidden[v] and (flat.var_cont[v] or self._epbp_discrete):
                out[(flat.factors[flat.edge_fac[e]], flat.rvs[v])] = (float(E[e, 0]), float(E[e, 1]))
        return out

    @property
    def message(self):
        """log messages as dicts keyed by point, like the reference (built on demand; large graphs: use .f2v/.v2f)"""
        flat, n = self.flat, self.n
        F2V, V2F, P = self._host('f2v'), self._host('v2f'), self._host('particles')
        out = {}
        for k in range(flat.var_edge.size):
            e = int(flat.var_edge[k])
            v = flat.edge_var[e]
            if not flat.var_hidden[v]:
                continue
            rv, f = flat.rvs[v], flat.factors[flat.edge_fac[e]]
            npv = self.np_host[v]
            pts = [float(x) for x in P[v, :npv]]
            m = {x: float(F2V[e, j]) for j, x in enumerate(pts)}
            if flat.var_cont[v]:
                d = flat.var_dom[v]
                grid = flat.dom_val[flat.dom_ptr[d]:flat.dom_ptr[d + 1]]
                m.update({float(x): float(F2V[e, n + t]) for t, x in enumerate(grid)})
            out[(f, rv)] = m
            out[(rv, f)] = {x: float(V2F[e, j]) for j, x in enumerate(pts)}
        return out

    # ---- the launches of the point and grid queries: each entry point's argument list, once (``_brent``, ``quad_all`` and
    # ``kl_from`` below hold those of lhvi_pbp_map_brent, lhvi_pbp_quad and lhvi_pbp_kl) ------------------------------------------
    def _launch_belief_points(self, qvar_t, x_t):
        """``belief_rv`` (EPBP:196-202) of the variables `qvar_t` (int32 [R]) at the points `x_t` ([R, m]), as a tensor like `x_t`"""
        out = _abi.require_gpu().empty_like(x_t)
        _abi.check(_abi.lib().lhvi_pbp_belief_points(self.dg.g, self.dg.p, self._struct(), _abi.ptr(self.v2f), int(x_t.shape[0]),
                                                     _abi.ptr(qvar_t), int(x_t.shape[1]), _abi.ptr(x_t), _abi.ptr(out), _abi.stream_ptr()))
        return out

    def _launch_edge_points(self, edge_t, x_t):
        """the f -> v messages of the edges `edge_t` (int32 [R]) at the points `x_t` ([R, m]), as a tensor like `x_t`; no rows, no launch"""
        out = _abi.require_gpu().empty_like(x_t)
        if x_t.shape[0]:
            _abi.check(_abi.lib().lhvi_pbp_edge_points(self.dg.g, self.dg.p, self._struct(), _abi.ptr(self.v2f), int(x_t.shape[0]),
                                                       _abi.ptr(edge_t), int(x_t.shape[1]), _abi.ptr(x_t), _abi.ptr(out), _abi.stream_ptr()))
        return out

    def _launch_domain_grid(self):
        """a new [V, n] tensor: per row a uniform grid on a continuous hidden variable's domain, the states of a discrete one"""
        x = _abi.require_gpu().empty_like(self.particles)
        _abi.check(_abi.lib().lhvi_pbp_domain_grid(self.dg.g, self._struct(), _abi.ptr(x), _abi.stream_ptr()))
        return x

    def _need_stable_rows(self):
        """the batched queries take a row of the solver's graph for a variable.  A lifted query walks the GROUND variable's factors
        (HLBP:313-317); that equals the count-weighted sum over the cluster's edges only when the partition is stable"""
        if self.flat.lifted and not self._stable_partition:
            raise NotImplementedError('batched queries on a lifted graph need a stable partition (run(c2f=-1))')

    # ---- queries (A8) ------------------------------------------------------------------------
    def _belief_rv_points(self, v, xs):
        """belief_rv(x) for one variable index at a batch of points, on the device (EPBP:196-202)"""
        xs = np.atleast_1d(np.asarray(xs, dtype=np.float64))
        out = self._launch_belief_points(_abi.to_dev(np.array([v], dtype=np.int32)), _abi.to_dev(xs.reshape(1, -1)))
        return out.cpu().numpy().reshape(-1)

    def belief_rv_batch(self, rvs, xs):
        """log-beliefs of many variables at `xs[i]` points each, one launch (extension, not in the reference)"""
        idx = np.array([self._var_of(rv) for rv in rvs], dtype=np.int32)
        x = _abi.to_dev(np.asarray(xs, dtype=np.float64).reshape(len(rvs), -1))
        return self._launch_belief_points(_abi.to_dev(idx), x).cpu().numpy()

    # ---- batched queries: every variable at once (extension) ------------------------
    def belief_rv_all(self, x):
        """log-beliefs ``belief_rv`` (EPBP:196-202) of EVERY variable at ``x[v, :]`` (n points per variable; a device
        tensor or array of shape (V, n)): one f2v launch with the query points in the place of the target particles
        tabulates all messages, one pass adds them up per variable (count-weighted on a lifted graph with a stable
        partition: rows are clusters then).  Returns a (V, n) device tensor; rows of observed variables are 0."""
        torch = _abi.require_gpu()
        self._need_stable_rows()
        l, st = _abi.lib(), _abi.stream_ptr()
        xq = x if torch.is_tensor(x) else _abi.to_dev(np.ascontiguousarray(x, dtype=np.float64))
        assert tuple(xq.shape) == (self.flat.V, self.n) and xq.is_contiguous()
        if self._query_f2v is None or self._query_f2v.shape != self.f2v.shape:
            self._query_f2v = torch.empty_like(self.f2v)
        s = self._struct()
        s.particles, s.old_particles = _abi.ptr(xq), _abi.ptr(self.particles)      # partners: the current sample
        self._call_f2v(s, out=self._query_f2v)
        out = torch.empty_like(xq)
        _abi.check(l.lhvi_pbp_var_sum(self.dg.g, s, _abi.ptr(self._query_f2v), _abi.ptr(out), st))
        return out

    def map_all(self, steps=5, scan=64):
        """MAP of every variable at once: a uniform scan of the domain with at least `scan` points (ceil(scan / n) passes
        of n points, so a solver with few particles still sees a narrow mode), then ``steps - 1`` times a new n-point grid
        on the bracket around the best point (the bracket shrinks by (n-1)/2 per step; 5 steps with n = 64 resolve 1e-6 of
        the domain width, the reference's fminbound stops at 1e-5).  Finds the mode the scan sees, where ``EPBP.map``
        (EPBP:377-394) finds the one fminbound's golden section runs into.  Returns (map, log-belief) as arrays of length
        V; observed variables return their value."""
        torch = _abi.require_gpu()
        l, st = _abi.lib(), _abi.stream_ptr()
        n, flat = self.n, self.flat
        x = self._launch_domain_grid()
        best = torch.empty(flat.V, dtype=torch.float64, device=x.device)
        val = torch.empty_like(best)
        s = self._struct()
        passes = -(-int(scan) // n) if n >= 3 else 1
        if passes > 1 and bool((flat.var_hidden & flat.var_cont).any()):
            cont = _abi.to_dev(flat.var_hidden & flat.var_cont)[:, None]
            lo, hi = (_abi.to_dev(t)[:, None] for t in pbp_query.domain_bounds(flat))
            h = (hi - lo) / (passes * (n - 1))
            j = torch.arange(n, dtype=torch.float64, device=x.device)[None, :]
            bx = bv = None
            for p in range(passes):                  # pass p covers [lo + p (n-1) h, lo + (p+1)(n-1) h], ends shared
                xp = torch.where(cont, lo + (p * (n - 1) + j) * h, x)
                vp, ap = self.belief_rv_all(xp).max(dim=1)
                xb = xp.gather(1, ap[:, None])[:, 0]
                if bx is None:
                    bx, bv = xb, vp
                else:
                    better = vp > bv                 # first maximum, like the reference's argmax over a list
                    bx, bv = torch.where(better, xb, bx), torch.where(better, vp, bv)
            a, b = torch.maximum(bx[:, None] - h, lo), torch.minimum(bx[:, None] + h, hi)
            x = torch.where(cont, a + (b - a) * (j / (n - 1)), x).contiguous()
        for _ in range(max(int(steps), 1)):
            logb = self.belief_rv_all(x)
            _abi.check(l.lhvi_pbp_refine_grid(self.dg.g, s, _abi.ptr(logb), _abi.ptr(x), _abi.ptr(best), _abi.ptr(val), st))
        return best.cpu().numpy(), val.cpu().numpy()

    def _brent(self, row_var, pairs=None, xtol=1e-5, maxfun=500):
        """``lhvi_pbp_map_brent`` on the rows `row_var` (variables of the solver's graph; with `pairs` = (ptr, edge, mult) the rows'
        beliefs are sums over explicit (edge, multiplicity) lists).  Returns device tensors (x, log-belief, evaluations)."""
        torch = _abi.require_gpu()
        rv_t = row_var if torch.is_tensor(row_var) else _abi.to_dev(np.ascontiguousarray(row_var, dtype=np.int32))
        rv_t = rv_t.to(torch.int32).contiguous()
        nq = int(rv_t.numel())
        x = torch.empty(nq, dtype=torch.float64, device=rv_t.device)
        fx = torch.empty_like(x)
        nfev = torch.empty(nq, dtype=torch.int32, device=rv_t.device)
        qptr = qedge = qmult = None
        if pairs is not None:
            qptr, qedge, qmult = (t.contiguous() for t in pairs)
            assert qptr.dtype == torch.int64 and qedge.dtype == torch.int32 and qmult.dtype == torch.float64 and qptr.numel() == nq + 1
        _abi.check(_abi.lib().lhvi_pbp_map_brent(self.dg.g, self.dg.p, self._struct(), _abi.ptr(self.v2f), nq, _abi.ptr(rv_t),
                                                 _abi.ptr(qptr), _abi.ptr(qedge), _abi.ptr(qmult), float(xtol), int(maxfun),
                                                 _abi.ptr(x), _abi.ptr(fx), _abi.ptr(nfev), _abi.stream_ptr()))
        return x, fx, nfev

    def map_fminbound_all(self, xtol=1e-5, maxfun=500):
        """MAP of every variable of the solver's graph the way the reference finds it (EPBP:377-394, HLBP:405-424): every
        continuous hidden variable runs ``scipy.optimize.fminbound``'s iteration on ``-belief_rv`` over its domain -- all of
        them in ONE launch, a thread each (``lhvi_pbp_map_brent``) -- and every discrete one takes its first state with the
        largest belief.  Returns (map [V], log-belief [V], evaluations [V]) as host arrays; observed rows hold their value."""
        flat = self.flat
        self._need_stable_rows()
        hid = np.flatnonzero(flat.var_hidden).astype(np.int32)
        out = np.nan_to_num(np.array(flat.var_value, dtype=np.float64), nan=0.0)
        val, nfev = np.zeros(flat.V), np.zeros(flat.V, dtype=np.int32)
        if hid.size:
            x, fx, k = self._brent(hid, xtol=xtol, maxfun=maxfun)
            out[hid], val[hid], nfev[hid] = x.cpu().numpy(), fx.cpu().numpy(), k.cpu().numpy()
        return out, val, nfev

    def quad_all(self, margin=20.0, epsabs=1.49e-8, epsrel=1.49e-8):
        """The normaliser of ``EPBP.belief`` (EPBP:325-328: ``quad`` of ``e ** belief_rv`` over the domain widened by 20 on both
        sides) of every continuous hidden variable in ONE launch (``lhvi_pbp_quad``: QUADPACK's 21-point Gauss-Kronrod rule in its
        adaptive bisection, to scipy's default tolerances; agrees with ``scipy.integrate.quad`` to ~1e-7 relative).  Returns host
        arrays (z [V], status [V]); z is NaN where the integrand overflowed (the reference raises OverflowError there) and for
        rows that are not continuous hidden variables."""
        torch = _abi.require_gpu()
        flat = self.flat
        self._need_stable_rows()
        rows = np.flatnonzero(flat.var_hidden & flat.var_cont).astype(np.int32)
        z, st = np.full(flat.V, np.nan), np.zeros(flat.V, dtype=np.int32)
        if rows.size:
            dom = flat.var_dom[rows]
            rv_t = _abi.to_dev(rows)
            lo, hi = _abi.to_dev(flat.dom_lo[dom] - margin), _abi.to_dev(flat.dom_hi[dom] + margin)
            zt = torch.empty(rows.size, dtype=torch.float64, device=rv_t.device)
            et = torch.empty_like(zt)
            stt = torch.empty(rows.size, dtype=torch.int32, device=rv_t.device)
            _abi.check(_abi.lib().lhvi_pbp_quad(self.dg.g, self.dg.p, self._struct(), _abi.ptr(self.v2f), int(rows.size), _abi.ptr(rv_t),
                                                None, None, None, _abi.ptr(lo), _abi.ptr(hi), float(epsabs), float(epsrel),
                                                _abi.ptr(zt), _abi.ptr(et), _abi.ptr(stt), _abi.stream_ptr()))
            z[rows], st[rows] = zt.cpu().numpy(), stt.cpu().numpy()
        return z, st

    def _kl_rows(self, rows):
        """the query rows of ``kl_from`` as an int32 array; ``ValueError`` for a row that is no continuous hidden variable"""
        flat = self.flat
        cont = flat.var_hidden & flat.var_cont
        if rows is None:
            return np.flatnonzero(cont).astype(np.int32)
        index = getattr(flat, 'var_index', None) or {}

        def one(r):         # an index, a random variable of the graph, or (lifted) a ground variable through its cluster
            if isinstance(r, (int, np.integer)):
                return int(r)
            key = r if r in index else getattr(r, 'cluster', None)
            if key not in index:
                raise ValueError('rows must name variables of the solver\'s graph')
            return index[key]
        rows = np.asarray([one(r) for r in (rows.tolist() if hasattr(rows, 'tolist') else list(rows))], dtype=np.int64).reshape(-1)
        if rows.size and (rows.min() < 0 or rows.max() >= flat.V):
            raise ValueError('rows must name variables of the solver\'s graph, 0 .. %d' % (flat.V - 1))
        bad = rows[~cont[rows]]
        if bad.size:
            raise ValueError('kl_from compares continuous hidden variables; rows %s are observed or discrete' % bad[:8].tolist())
        return rows.astype(np.int32)

    def _kl_logz(self):
        """``log`` of every row's belief normaliser as a host array [V] (NaN: not a continuous hidden row, or the normaliser
        overflowed).  The base class normalises like ``HybridLBP.belief`` (HLBP:343-382): the 20-point ``log_area`` over the
        domain, ``log(area) + shift``."""
        z, shift = self._cached_area()
        with np.errstate(invalid='ignore', divide='ignore'):
            return np.log(z) + shift

    def kl_from(self, p, rows=None, a=-np.inf, b=np.inf, epsabs=1.49e-8, epsrel=1.49e-8, info=False):
        """``KL(p[r] || belief of variable rows[r])`` for every row in ONE launch (``lhvi_pbp_kl``, docs/kernels_pbkl.md): the
        drivers' ``kl_err = kl_continuous_logpdf(log_p, curry_epbp_belief(bp, rv, log_belief=True))`` with ``p`` the baseline's
        mixture marginals.  ``p``: a ``ScalarMixtures`` or a ``(w, mu, var)`` tuple, broadcast as in ``kl_scalar_mixtures`` (a
        one-row ``p`` serves every row); ``rows``: variable indices of the solver's graph (or its random variables), default
        every continuous hidden variable in index order; ``a``, ``b``: scalars or [R].  The belief is normalised as the solver's
        own ``belief`` does it: for ``EPBP`` by ``quad_all``'s ``z`` (EPBP:321-331), for ``HybridLBP`` by the 20-point
        ``log_area`` over the domain (HLBP:343-382).  A row whose normaliser overflowed is NaN with status bit 2, the others are
        unaffected.  Device tensors in give device tensors out, arrays in give arrays out; ``info=True`` returns
        ``(kl, dict(abserr=, status=, neval=))``.  ``ValueError`` before any launch for an observed or discrete row, or when the
        number of rows does not match ``p``."""
        from . import gmkl
        rows = self._kl_rows(rows)
        R = int(rows.size)
        parts = list(gmkl._parts(p, 'p')) + [a, b]
        tensors = [t for t in parts if gmkl._is_tensor(t)]
        if not (float(epsabs) >= 0 and float(epsrel) >= 0):
            raise ValueError('epsabs and epsrel must not be negative')
        shapes = [tuple(t.shape) if hasattr(t, 'shape') else np.shape(t) for t in parts]
        sizes = {int(s[0]) for s in shapes[:3] if len(s) == 2} | {int(np.prod(s)) for s in shapes[3:]}
        if R == 0:
            raise ValueError('no rows to compare')
        if sizes - {1, R}:
            raise ValueError('p, a and b must have one row or as many as rows (%d): %s' % (R, sorted(sizes - {1, R})))
        self._need_stable_rows()
        torch = _abi.require_gpu()
        kind = gmkl._Torch(torch, self.particles.device)
        wp, mup, varp = gmkl._mixture(kind, p, 'p')
        Kp = int(mup.shape[1])
        wp, mup, varp = (kind.rows(t, (R, Kp)) for t in (wp, mup, varp))
        a, b = kind.rows(kind.array(a).reshape(-1), (R,)), kind.rows(kind.array(b).reshape(-1), (R,))
        logz = _abi.to_dev(np.ascontiguousarray(self._query_cache('kl_logz', self._kl_logz)[rows], dtype=np.float64))
        rv_t = _abi.to_dev(rows)
        kl, abserr = kind.empty(R, np.float64), kind.empty(R, np.float64)
        status, neval = kind.empty(R, np.int32), kind.empty(R, np.int32)
        _abi.check(_abi.lib().lhvi_pbp_kl(self.dg.g, self.dg.p, self._struct(), _abi.ptr(self.v2f), R, _abi.ptr(rv_t), None, None, None,
                                          _abi.ptr(logz), Kp, _abi.ptr(wp), _abi.ptr(mup), _abi.ptr(varp), _abi.ptr(a), _abi.ptr(b),
                                          float(epsabs), float(epsrel), _abi.ptr(kl), _abi.ptr(abserr), _abi.ptr(status),
                                          _abi.ptr(neval), _abi.stream_ptr()))
        if not tensors:
            kl, abserr, status, neval = (t.cpu().numpy() for t in (kl, abserr, status, neval))
        return (kl, dict(abserr=abserr, status=status, neval=neval)) if info else kl

    def _per_var(self, a):
        torch = _abi.require_gpu()
        t = torch.as_tensor(np.broadcast_to(np.asarray(a, dtype=np.float64), (self.flat.V,)).copy()) if not torch.is_tensor(a) else a
        return t.to(self.particles.device, torch.float64)

    def log_area_all(self, a, b, npts=20, shift=None):
        """``log_area`` (EPBP:291-308, HLBP:318-341) of every continuous hidden variable at once: trapezoid of
        exp(belief_rv - shift) on linspace(a[v], b[v], npts), shift = ``log_message_balance`` of the tabulated values
        unless given.  `a`, `b`: scalars or arrays / tensors of length V.  Returns device tensors
        (area [V], shift [V]); rows of discrete and observed variables are NaN."""
        torch = _abi.require_gpu()
        if npts < 2:
            raise ValueError('npts must be at least 2')
        a, b = self._per_var(a), self._per_var(b)
        n = self.n
        x = self._launch_domain_grid()
        cont = _abi.to_dev(self.flat.var_hidden & self.flat.var_cont)
        step = (b - a) / (npts - 1)                                   # numpy.linspace: start + i * step, last point = stop
        lin = torch.arange(npts, dtype=torch.float64, device=a.device)[None, :] * step[:, None] + a[:, None]
        lin[:, npts - 1] = b
        y = torch.empty_like(lin)
        for c in range(0, npts, n):                                   # n query points per variable and pass
            w = min(n, npts - c)
            x[:, :w] = torch.where(cont[:, None], lin[:, c:c + w], x[:, :w])
            y[:, c:c + w] = self.belief_rv_all(x)[:, :w]
        if shift is None:
            mean, mx = y.mean(dim=1), y.max(dim=1).values
            shift = torch.where(mx - mean > self.max_log_value, mx - self.max_log_value, mean)
        w = torch.exp(y - shift[:, None])
        area = (w[:, :-1] + w[:, 1:]).sum(dim=1) * (lin[:, 1] - lin[:, 0]) * 0.5
        nan = torch.full_like(area, float('nan'))
        return torch.where(cont, area, nan), torch.where(cont, shift, nan)

    def belief_all(self, x):
        """normalised beliefs of EVERY variable (``HybridLBP.belief`` HLBP:343-382 for all of them at once; for EPBP the
        same 20-point trapezoid normaliser in the place of ``scipy.integrate.quad``).  `x`: (V, m) query points, m <= n.
        Continuous hidden rows: exp(belief_rv(x) - shift) / area over the domain; discrete hidden rows: the normalised
        beliefs of the variable's states in columns [0, #states) (x is ignored there); observed rows: 1 where x equals
        the value.  Returns a (V, m) device tensor."""
        torch = _abi.require_gpu()
        flat = self.flat
        xq = x if torch.is_tensor(x) else _abi.to_dev(np.ascontiguousarray(x, dtype=np.float64))
        xq = xq.reshape(flat.V, -1)
        m = xq.shape[1]
        if m > self.n:
            raise ValueError('at most n query points per variable')
        z, shift = self._domain_area()
        grid = self._launch_domain_grid()
        cont = _abi.to_dev(flat.var_hidden & flat.var_cont)
        grid[:, :m] = torch.where(cont[:, None], xq, grid[:, :m])     # discrete rows keep their states
        logb = self.belief_rv_all(grid)
        out = torch.exp(logb[:, :m] - shift[:, None] - torch.log(z)[:, None])
        disc = _abi.to_dev(flat.var_hidden & ~flat.var_cont)
        if bool(disc.any()):
            nst = _abi.to_dev(self.np_host.astype(np.int64))
            live = torch.arange(self.n, device=xq.device)[None, :] < nst[:, None]
            w = torch.where(live, torch.exp(logb), torch.zeros_like(logb))
            w = w / w.sum(dim=1, keepdim=True)
            out = torch.where(disc[:, None], w[:, :m], out)
        obs = _abi.to_dev(~flat.var_hidden)
        val = _abi.to_dev(np.nan_to_num(flat.var_value, nan=0.0))
        return torch.where(obs[:, None], (xq == val[:, None]).to(torch.float64), out)

    def probability_all(self, a, b):
        """``probability(a, b, rv)`` (EPBP:356-375, HLBP:384-403) of every continuous hidden variable at once: 5-point
        trapezoid on [a[v], b[v]] over the 20-point one on the domain.  Returns a device tensor [V] (NaN elsewhere)."""
        z, shift = self._domain_area()
        num, _ = self.log_area_all(a, b, 5, shift=shift)
        return num / z

    # ---- per-variable queries answered from one batched pass (the reference's callers loop `infer.map(rv)` over every rv:
    # Demo/RGM/demo.py:32-35, Demo/HMLN/DemoPaperPopularity.py:44-47) --------------------------------------------------------
    def _query_cache(self, name, fill):
        c = self.__dict__.setdefault('_batched', {})
        if name not in c:
            c[name] = fill()
        return c[name]

    def _cached_map(self):
        """MAP of every row of the solver's graph as a host array: the reference's ``fminbound`` iterates for all rows in one
        launch (``map_fminbound_all``); with ``map_mode = 'global'`` the scan + bracket refinement of ``map_all`` (the highest
        mode a 64-point scan sees, which need not be the one Brent's golden section runs into)"""
        if self.map_mode == 'global':
            return self._query_cache('map_global', lambda: self.map_all(steps=6 if self.n >= 32 else 9)[0])
        return self._query_cache('map', lambda: self.map_fminbound_all()[0])

    def _domain_area(self):
        """(z, shift) of ``log_area`` over the domain with 20 points for every row (``log_area_all``): the normaliser of ``belief_all``
        and ``probability_all``, as device tensors, computed once per sample"""
        return self._query_cache('domain_area', lambda: self.log_area_all(*pbp_query.domain_bounds(self.flat), 20))

    def _cached_area(self):
        """``_domain_area`` as host arrays"""
        return self._query_cache('area', lambda: tuple(t.cpu().numpy() for t in self._domain_area()))

    def log_message_balance(self, message):
        """EPBP.log_message_balance (EPBP:204-215) on a host dict"""
        shift = pbp_query.balance_shift(list(message.values()), self.max_log_value)
        for k in message:
            message[k] = message[k] - shift
        return shift

    def log_area(self, f, a, b, n, shift=None):
        """``log_area`` with the reference's signature (EPBP:291-308, HLBP:324-341): trapezoid of exp(f(x) - shift) on
        linspace(a, b, n) for a callable log-density ``f``; returns (area, shift)"""
        x = np.linspace(a, b, n)
        return pbp_query.balanced_trapezoid([f(v) for v in x], x[1] - x[0], shift, self.max_log_value)

    @staticmethod
    def get_cluster(instance):
        return instance.cluster

    def _log_area(self, v, a, b, npts, shift=None):
        """EPBP.log_area (EPBP:291-308): trapezoid of exp(belief_rv - shift) on linspace(a, b, npts)"""
        x = np.linspace(a, b, npts)
        return pbp_query.balanced_trapezoid(self._belief_rv_points(v, x).tolist(), x[1] - x[0], shift, self.max_log_value)

    @staticmethod
    def message_normalization(message):
        z = 0
        for k, v in message.items():
            z = z + v
        for k, v in message.items():
            message[k] = v / z

    @staticmethod
    def norm_pdf(x, mu, sig):
        u = (x - mu) / sig
        return np.exp(-u * u * 0.5) / (2.506628274631 * sig)

    # ---- the reference's per-variable calls (EPBP:310-394, HLBP:343-424).  A solver says how a call maps to a row of a batched pass
    # (`_row_of`: ('cluster', row of its graph), ('ground', row of the ground graph) or (None, None): one scipy run per call) and
    # which normaliser its ``belief`` divides by (`_normaliser`) ----------------------------------------------------------------------
    def _batched_rows(self, how, what):
        """the batched answer to `what` ('map': values; 'area': (z, shift) of the 20-point ``log_area`` over the domain), each
        indexed by the rows of `how`"""
        return self._cached_map() if what == 'map' else self._cached_area()

    def _area_of(self, rv):
        """(z, shift) of the 20-point ``log_area`` over rv's domain (EPBP:364-366, HLBP:361-365), batched when possible"""
        how, row = self._row_of(rv)
        if how is None:
            return self._log_area(self._var_of(rv), rv.domain.values[0], rv.domain.values[1], 20)
        z, shift = self._batched_rows(how, 'area')
        return float(z[row]), float(shift[row])

    def _state_beliefs(self, rv):
        """{state: normalised belief} of a discrete hidden variable"""
        vals = rv.domain.values
        b = dict(zip(vals, (e ** t for t in self._belief_rv_points(self._var_of(rv), vals).tolist())))
        self.message_normalization(b)
        return b

    def _belief(self, x, rv, log_belief=False, inf_integral=False):
        if rv.value is not None:
            if log_belief:
                return 0 if x == rv.value else -np.inf
            return 1 if x == rv.value else 0
        if rv.domain.continuous:
            z, shift = self._normaliser(rv, inf_integral)
            lb_x = float(self._belief_rv_points(self._var_of(rv), [x])[0]) - shift - log(z)
            return lb_x if log_belief else e ** lb_x
        b = self._state_beliefs(rv)
        return log(b[x]) if log_belief else b[x]

    def probability(self, a, b, rv):
        if rv.value is None and rv.domain.continuous:
            z, shift = self._area_of(rv)
            num, _ = self._log_area(self._var_of(rv), a, b, 5, shift)
            return num / z
        return None

    def map(self, rv):
        if rv.value is not None:
            return rv.value
        how, row = self._row_of(rv)
        if how is not None:
            return pbp_query.typed_value(rv, self._batched_rows(how, 'map')[row])
        v = self._var_of(rv)
        if rv.domain.continuous:
            from scipy.optimize import fminbound
            return fminbound(lambda val: -float(self._belief_rv_points(v, [val])[0]),
                             rv.domain.values[0], rv.domain.values[1], disp=False)
        vals = list(rv.domain.values)           # (the particles of a discrete variable are its states)
        return vals[int(np.argmax(self._belief_rv_points(v, vals)))]


class EPBP(_ParticleSweep):
    """Expectation particle BP on a ground graph (``EPBPLogVersion.py``)."""

    var_threshold = 3
    max_log_value = 700
    _epbp_discrete = True

    def __init__(self, g=None, n=50, proposal_approximation='EP', sampler='host', seed=0):
        self.g = g
        self.n = n
        self.proposal_approximation = proposal_approximation
        self.sampler, self.seed = sampler, seed
        self.cache = dict()

    def run(self, iteration=10, log_enable=False):
        self._setup(self.g)
        self.cache = dict()
        self._run_sweeps(iteration)

    def _var_of(self, rv):
        return self.flat.var_index[rv]

    def belief_rv(self, x, rv, sample=None):
        return float(self._belief_rv_points(self._var_of(rv), [x])[0])

    def _row_of(self, rv):
        return (None, None) if self.exact_queries else ('cluster', self._var_of(rv))

    def _normaliser(self, rv, inf_integral=False):
        """(z, shift = 0) of ``EPBP.belief`` (EPBP:321-331): adaptive quadrature of exp(belief_rv), kept per variable in ``cache``"""
        if rv not in self.cache:
            v = self._var_of(rv)
            if not self.exact_queries and not inf_integral:
                # the normalisers of all variables from one launch (quad_all), made at the first call after run()
                zs, status = self._query_cache('quad', self.quad_all)
                if status[v] == 3:
                    raise OverflowError('(34, \'Numerical result out of range\')')      # e ** belief_rv overflowed, as in the reference (EPBP:326)
                z = float(zs[v])
            else:
                from scipy.integrate import quad
                lb, ub = (-np.inf, np.inf) if inf_integral else (rv.domain.values[0] - 20, rv.domain.values[1] + 20)
                z = quad(lambda val: e ** float(self._belief_rv_points(v, [val])[0]), lb, ub)[0]
            self.cache[rv] = (z, 0)
        return self.cache[rv]

    def belief(self, x, rv, log_belief=False, inf_integral=False):
        """EPBP.belief (EPBP:310-354): normaliser by adaptive quadrature of exp(belief_rv)"""
        return self._belief(x, rv, log_belief, inf_integral)

    def _kl_logz(self):
        """``log`` of ``quad_all()``'s ``z`` (the cache ``belief`` fills too): the normaliser of ``EPBP.belief`` (EPBP:321-331);
        NaN where ``e ** belief_rv`` overflowed (status 3), which ``kl_from`` reports as an invalid row"""
        zs, _ = self._query_cache('quad', self.quad_all)
        with np.errstate(invalid='ignore', divide='ignore'):
            return np.log(zs)


class HybridLBP(_ParticleSweep):
    """Lifted particle BP (``HybridLBPLogVersion.py``): colour passing, then the counted sweep."""

    var_threshold = 5
    max_log_value = 700
    _epbp_discrete = False

    def __init__(self, g, n=50, k_mean_k=2, k_mean_iteration=10, proposal_approximation='EP', sampler='host', seed=0):
        from .lifting import CompressedGraph
        self.g = CompressedGraph(g)
        self.n = n
        self.k_mean_k = k_mean_k
        self.k_mean_iteration = k_mean_iteration
        self.proposal_approximation = proposal_approximation
        self.sampler, self.seed = sampler, seed
        self.query_cache = dict()

    c2f_on_objects = False          # run(c2f >= 0) through Python objects per cluster (lhvi.c2f.run_c2f) instead of arrays
    c2f_observer = None             # called by a coarse-to-fine run before every draw but the first (lhvi.c2f.run_c2f)
    c2f_keep_history = False        # run_flat(c2f >= 0) keeps the partition of every sweep in c2f_history

    @classmethod
    def on_flat(cls, flat, n=50, k_mean_k=2, k_mean_iteration=10, proposal_approximation='EP', sampler='device', seed=0):
        """The lifted sweep on arrays -- no Python object per ground atom anywhere.  `flat` is either a ready-made lifted
        ``FlatGraph`` (``lifting.lift_flat`` of a stable partition) or a GROUND one (``RelationalGraph.ground_flat``,
        ``flatten(g)``, ``build_flat``): then ``run_flat`` does the lifting itself, to the stable partition (``c2f=-1``) or coarse
        to fine (``c2f >= 0``).  Query with the batched calls (``belief_rv_all``, ``map_all``, ``belief_all``,
        ``probability_all``: rows are clusters, stable partition) or per ground variable with ``belief_rv_ground``."""
        self = cls.__new__(cls)
        self.g = None
        self.n, self.k_mean_k, self.k_mean_iteration = n, k_mean_k, k_mean_iteration
        self.proposal_approximation, self.sampler, self.seed = proposal_approximation, sampler, seed
        self.query_cache = dict()
        self._flat_in = flat
        return self

    def run_flat(self, iteration=10, c2f=-1, timing=None):
        """``run(iteration, c2f)`` for a solver made by ``on_flat``.  ``timing``: dict that receives the per-sweep seconds of a
        coarse-to-fine run (``lhvi.c2f.run_c2f_flat``)."""
        self.query_cache = dict()
        flat = self._flat_in
        if flat.lifted:
            if c2f != -1:
                raise ValueError('a coarse-to-fine run starts from the GROUND graph (on_flat(ground_flat))')
            self._setup(None, flat=flat)
            self._run_sweeps(iteration)
            self._stable_partition = True
            return
        from .lifting import initial_colors_device, lift_flat, refine_flat
        dg = _abi.DeviceGraph(flat)
        if c2f == -1:
            rvc0, fc0, sym = initial_colors_device(flat, dg, True)
            rvc, fc = refine_flat(flat, sym, rvc0, fc0, dg=dg, device_out=True)
            self._ground = dict(flat=flat, dg=dg, rvc=rvc, fc=fc)
            self._setup(None, flat=lift_flat(flat, rvc, fc, dg=dg))
            self._run_sweeps(iteration)
            self._stable_partition = True
            return
        self._run_c2f_arrays(flat, dg, iteration, c2f, timing, keep_history=self.c2f_keep_history)

    def _c2f_draw(self):
        def draw(k, flat, q_host):
            if callable(self.sampler):
                return self.sampler(k, flat, q_host)
            if self.sampler == 'device':
                return None                       # engine.install draws on the device
            out = np.zeros((flat.V, self.n))      # the reference's stream: standard_normal in cluster order (HLBP:75-87)
            rows = np.flatnonzero(flat.var_hidden & flat.var_cont)
            if rows.size:                         # (one call: the same stream as one standard_normal(n) per cluster, see _host_draw)
                z = np.random.standard_normal((rows.size, self.n))
                dmn = flat.var_dom[rows]
                out[rows] = np.clip(z * np.sqrt(q_host[rows, 1])[:, None] + q_host[rows, 0][:, None], flat.dom_lo[dmn][:, None],
                                    flat.dom_hi[dmn][:, None])
            return out
        return draw

    def _run_c2f_arrays(self, gflat, dg, iteration, c2f, timing=None, keep_history=False):
        """``run(iteration, c2f >= 0)`` on arrays (``lhvi.c2f.run_c2f_flat``): colours, refinement and both re-liftings of every
        sweep on the device"""
        from . import c2f as _c2f
        from .lifting import initial_colors_device
        rvc0, fc0, sym = initial_colors_device(gflat, dg, False)                     # HLBP:432
        st, G2, rvc, fc, history = _c2f.run_c2f_flat(
            gflat, dg, _DeviceEngine(self), _c2f.FlatRefiner(gflat, dg, sym), iteration, c2f, self.k_mean_k, self.k_mean_iteration,
            self._c2f_draw(), rvc0, fc0, observer=self.c2f_observer, keep_history=keep_history, timing=timing)
        self.c2f_history = history
        self._stable_partition = False
        self.__dict__.update({k: v for k, v in st.__dict__.items()})
        self._ground = dict(flat=gflat, dg=dg, rvc=rvc, fc=fc)
        self._views, self._batched = {}, {}

    def run(self, iteration=10, log_enable=False, c2f=-1):
        """``HybridLBP.run`` (HLBP:430-536).  ``c2f == -1``: colour passing to the stable partition, then the sweeps.
        ``c2f >= 0``: coarse start (continuous evidence merged regardless of value), evidence clusters are split by
        k-means while their variance exceeds a shrinking threshold, rv / factor clusters are refined once per sweep and
        every new cluster inherits the messages, sites, proposal and particles of the cluster it came from."""
        self.query_cache = dict()
        self._stable_partition = False
        self._ground = None
        if c2f == -1:
            self.g.init_cluster(True)
            prev = -1
            while self.g.num_rv_clusters != prev:         # HLBP:433-438
                prev = self.g.num_rv_clusters
                self.g.split_factors()
                self.g.split_rvs()
            self.g.array_flat = True                        # (stable: lifting.lifted_flat instead of walking the cluster objects)
            self._setup(self.g)
            self._run_sweeps(iteration)
            self.g.split_factors()                          # HLBP:536 (a no-op on a stable partition)
            self._stable_partition = True
            return
        from . import c2f as _c2f
        ground = self.g.g
        if not self.c2f_on_objects:
            # the ground objects are flattened once; clusters become objects again only at the end, for the rv.cluster queries
            from .lifting import CompressedGraph
            gflat = flatten(ground, require_device_potentials=True)
            self._run_c2f_arrays(gflat, _abi.DeviceGraph(gflat), iteration, c2f, keep_history=True)
            cg = CompressedGraph(ground)
            cg.set_colors(self._ground['rvc'].cpu().numpy(), self._ground['fc'].cpu().numpy())
            self.g = cg
            lf = self.flat
            lf.rvs, lf.factors = sorted(cg.rvs), sorted(cg.factors)
            lf.var_index = {c: i for i, c in enumerate(lf.rvs)}
            lf.fac_index = {c: i for i, c in enumerate(lf.factors)}
            return
        engine = _DeviceEngine(self)
        refiner = _c2f.DeviceRefiner(ground)
        st, flat, cg, rvc, fc, history = _c2f.run_c2f(ground, engine, refiner, iteration, c2f, self.k_mean_k,
                                                      self.k_mean_iteration, self._c2f_draw(),
                                                      observer=self.c2f_observer)
        self.c2f_history = history
        self.g = cg
        # adopt the final factor-side state for the queries
        self.__dict__.update({k: v for k, v in st.__dict__.items()})
        self._views, self._batched = {}, {}

    # ---- queries of GROUND variables on arrays (a solver made by on_flat) --------------------------------------------------------
    def _ground_pairs(self):
        """(ground variable, lifted edge, multiplicity) of every distinct pair: ``belief_rv_query`` (HLBP:313-317) walks the
        GROUND rv's factors f and evaluates the message of (f.cluster, position of the rv)"""
        G = self._ground
        if 'pairs' not in G:
            torch = _abi.require_gpu()
            gf, lf, dg = G['flat'], self.flat, G['dg']
            fcl = G['fc'].long()
            dev = fcl.device
            efac = dg.t['edge_fac'].long()
            pos = torch.arange(gf.E, device=dev) - dg.t['fac_ptr'].long()[efac]
            lifted_e = _abi.to_dev(lf.edge_canon.astype(np.int64))[_abi.to_dev(lf.fac_ptr.astype(np.int64))[fcl[efac]] + pos]
            slot_edge = dg.t['var_edge'].long()
            slot_var = dg.t['slot_var'].long()
            key, cnt = torch.unique(slot_var * max(lf.E, 1) + lifted_e[slot_edge], return_counts=True)     # sorted: grouped per variable
            var = key // max(lf.E, 1)
            ptr = torch.zeros(gf.V + 1, dtype=torch.int64, device=dev)
            torch.cumsum(torch.bincount(var, minlength=gf.V), 0, out=ptr[1:])
            G['pairs'] = (ptr, (key % max(lf.E, 1)).to(torch.int32), cnt.to(torch.float64))
        return G['pairs']

    def belief_rv_ground(self, vs, xs):
        """log-beliefs ``belief_rv_query(x, rv)`` of the GROUND variables `vs` (indices into the ground FlatGraph) at `xs[i, :]`
        (the same number of points each), one launch.  Works after any ``run_flat`` (the partition need not be stable)."""
        torch = _abi.require_gpu()
        ptr, edge, mult = self._ground_pairs()
        vs_t = _abi.to_dev(np.asarray(vs, dtype=np.int64))
        x = xs if torch.is_tensor(xs) else _abi.to_dev(np.ascontiguousarray(xs, dtype=np.float64))
        x = x.reshape(vs_t.numel(), -1)
        _, owner, idx = pbp_query.expand_rows(ptr, vs_t)
        out = self._launch_edge_points(edge[idx].contiguous(), x[owner].contiguous())
        res = torch.zeros_like(x)
        res.index_add_(0, owner, out * mult[idx][:, None])
        return res

    def _var_of(self, ground_rv):
        return ground_rv                      # queries walk the GROUND rv's factors, like belief_rv_query (HLBP:313-317)

    def _ground_edges(self, ground_rv):
        """(lifted edge id, multiplicity) of every ground factor of `ground_rv`: edge = (f.cluster, position of the rv)"""
        flat, acc = self.flat, {}
        for f in ground_rv.nb:
            fi = flat.fac_index[f.cluster]
            pos = next(i for i, r in enumerate(f.nb) if r is ground_rv)
            e = int(flat.edge_canon[flat.fac_ptr[fi] + pos])
            acc[e] = acc.get(e, 0) + 1
        return acc

    def _belief_rv_points(self, ground_rv, xs):
        """belief_rv_query(x, rv) = sum over the ground rv's factors f of message_f_to_rv(x, f.cluster, rv.cluster)"""
        xs = np.atleast_1d(np.asarray(xs, dtype=np.float64))
        acc = self._ground_edges(ground_rv)
        edges = np.array(list(acc), dtype=np.int32)
        mult = np.array([acc[e] for e in acc], dtype=np.float64)
        out = self._launch_edge_points(_abi.to_dev(edges), _abi.to_dev(np.tile(xs, (edges.size, 1))))
        return (out.cpu().numpy() * mult[:, None]).sum(axis=0)

    def belief_rv_batch(self, rvs, xs):
        xs = np.asarray(xs, dtype=np.float64).reshape(len(rvs), -1)
        return np.stack([self._belief_rv_points(rv, x) for rv, x in zip(rvs, xs)])

    def belief_rv_query(self, x, rv, sample=None):
        return float(self._belief_rv_points(rv, [x])[0])

    # ---- batched queries of GROUND variables (any partition): what the per-variable calls below are answered from ---------------
    def _ground_rows(self):
        """hidden ground variables of the run's ground graph, their domain bounds and kind (arrays path only)"""
        G = self._ground
        if 'rows' not in G:
            gf = G['flat']
            hid = np.flatnonzero(gf.var_hidden)
            G['rows'] = (hid, gf.var_cont[hid], *pbp_query.domain_bounds(gf, hid))
        return G['rows']

    def ground_map_all(self, scan=64, steps=6):
        """MAP of every hidden GROUND variable in a few batched passes of ``belief_rv_ground``: a uniform scan of the domain
        with `scan` points, then `steps` times a new 17-point grid on the bracket around the best point (the bracket shrinks 8x
        per step: 1e-6 of the domain width after 6).  Discrete variables: the first state with the largest belief.  Returns
        (ground variable ids, MAP values)."""
        torch = _abi.require_gpu()
        hid, cont, lo, hi = self._ground_rows()
        gf = self._ground['flat']
        out = np.zeros(hid.size)
        ci = np.flatnonzero(cont)
        if ci.size:
            dev = self.particles.device
            lo_t, hi_t = _abi.to_dev(lo[ci])[:, None], _abi.to_dev(hi[ci])[:, None]
            j = torch.arange(scan, dtype=torch.float64, device=dev)[None, :]
            x = lo_t + (hi_t - lo_t) * (j / (scan - 1))
            vals = self.belief_rv_ground(hid[ci], x)
            bv, arg = vals.max(dim=1)
            bx = x.gather(1, arg[:, None])[:, 0]
            h = ((hi_t - lo_t) / (scan - 1))[:, 0]
            m = 17
            jj = torch.arange(m, dtype=torch.float64, device=dev)[None, :]
            for _ in range(steps):
                a = torch.maximum(bx - h, lo_t[:, 0])[:, None]
                b = torch.minimum(bx + h, hi_t[:, 0])[:, None]
                x = (a + (b - a) * (jj / (m - 1))).contiguous()
                vals = self.belief_rv_ground(hid[ci], x)
                v2, arg = vals.max(dim=1)
                better = v2 >= bv
                bx = torch.where(better, x.gather(1, arg[:, None])[:, 0], bx)
                bv = torch.where(better, v2, bv)
                h = ((b - a) / (m - 1))[:, 0]
            out[ci] = bx.cpu().numpy()
        di = np.flatnonzero(~cont)
        if di.size:
            nst = gf.var_nstates[hid[di]]
            D = int(nst.max())
            states = np.zeros((di.size, D))
            for r, v in enumerate(hid[di]):
                d = gf.var_dom[v]
                vals = gf.dom_val[gf.dom_ptr[d]:gf.dom_ptr[d + 1]]
                states[r, :vals.size] = vals
                states[r, vals.size:] = vals[0]
            lb = self.belief_rv_ground(hid[di], states).cpu().numpy()
            lb[np.arange(D)[None, :] >= nst[:, None]] = -np.inf
            out[di] = states[np.arange(di.size), lb.argmax(axis=1)]
        return hid, out

    def ground_log_area_all(self, npts=20):
        """``log_area`` (HLBP:324-341) over the domain of every hidden continuous GROUND variable: (ids, area, shift)"""
        torch = _abi.require_gpu()
        hid, cont, lo, hi = self._ground_rows()
        ci = np.flatnonzero(cont)
        lin = np.linspace(lo[ci], hi[ci], npts, axis=1)          # the per-call form's abscissae, bit for bit (numpy.linspace per row)
        y = self.belief_rv_ground(hid[ci], lin).cpu().numpy() if ci.size else np.zeros((0, npts))
        mean, mx = y.mean(axis=1), y.max(axis=1)
        shift = np.where(mx - mean > self.max_log_value, mx - self.max_log_value, mean)
        w = np.exp(y - shift[:, None])
        area = (w[:, :-1] + w[:, 1:]).sum(axis=1) * (lin[:, 1] - lin[:, 0]) * 0.5
        return hid[ci], area, shift

    def ground_map_fminbound_all(self, xtol=1e-5, maxfun=500):
        """MAP of every hidden GROUND variable the way ``HybridLBP.map`` finds it (HLBP:405-424: ``fminbound`` on
        ``-belief_rv_query``; discrete: first state with the largest belief), all in one launch; works on any partition.
        Returns (ground variable ids, MAP values)."""
        hid = self._ground_rows()[0]
        ptr, edge, mult = self._ground_pairs()
        torch = _abi.require_gpu()
        hid_t = _abi.to_dev(hid.astype(np.int64))
        qptr, _, idx = pbp_query.expand_rows(ptr, hid_t)
        rows = self._ground['rvc'].to(torch.int32)[hid_t]
        x, _, _ = self._brent(rows, pairs=(qptr, edge[idx], mult[idx]), xtol=xtol, maxfun=maxfun)
        return hid, x.cpu().numpy()

    # ---- the per-variable calls (_ParticleSweep.map / probability / _belief): rows, batched tables and the normaliser -----------------
    def _row_of(self, ground_rv):
        """a stable partition: rows are clusters; an unstable one: the ground arrays of the arrays path, if the run kept them"""
        if self.exact_queries:
            return None, None
        index = self.flat.var_index
        if self._stable_partition and getattr(ground_rv, 'cluster', None) in index:
            return 'cluster', index[ground_rv.cluster]
        G = self._ground
        if G is not None and ground_rv in G['flat'].var_index:
            return 'ground', G['flat'].var_index[ground_rv]
        return None, None

    def _batched_rows(self, how, what):
        if how != 'ground':
            return super()._batched_rows(how, what)
        glob = self.map_mode == 'global'

        def fill():                 # keyed by ground variable id: only the hidden ones have a row
            if what == 'map':
                ids, vals = self.ground_map_all() if glob else self.ground_map_fminbound_all()
                return dict(zip(ids.tolist(), vals.tolist()))
            ids, area, shift = (t.tolist() for t in self.ground_log_area_all(20))
            return dict(zip(ids, area)), dict(zip(ids, shift))
        return self._query_cache('ground_' + ('map_global' if what == 'map' and glob else what), fill)

    def _sig(self, rv):
        """the key of ``query_cache``: ground variables with the same cluster and the same lifted edges share their beliefs"""
        return rv.cluster, frozenset(self._ground_edges(rv).items())

    def _normaliser(self, rv, inf_integral=False):
        """(z, shift) of ``HybridLBP.belief`` (HLBP:361-365): the 20-point trapezoid over the domain, kept in ``query_cache``"""
        sig = self._sig(rv)
        if sig not in self.query_cache:
            self.query_cache[sig] = self._area_of(rv)
        return self.query_cache[sig]

    def _state_beliefs(self, rv):
        sig = self._sig(rv)
        if sig not in self.query_cache:
            self.query_cache[sig] = super()._state_beliefs(rv)
        return self.query_cache[sig]

    def belief(self, x, rv, inf_integral=False):
        """HybridLBP.belief (HLBP:343-382): 20-point trapezoid normaliser, cached per cluster"""
        return self._belief(x, rv)


class _DeviceEngine:
    """lhvi.c2f engine backed by the HIP kernels: every state is a solver-shaped object holding one lifted graph's arrays"""

    _names = {'q': 'q_dev'}

    def __init__(self, owner):
        self.owner = owner
        self.draws = 0

    def make(self, flat, sides='vf'):
        o = self.owner
        st = HybridLBP.__new__(HybridLBP)
        st.n, st.proposal_approximation, st.sampler, st.seed = o.n, o.proposal_approximation, o.sampler, o.seed
        st.query_cache = dict()
        st._setup(None, flat=flat, sides=sides)
        return st

    def get(self, st, name):
        return getattr(st, self._names.get(name, name))

    def set(self, st, name, value):
        setattr(st, self._names.get(name, name), value)

    def init(self, st):
        st._launch_init(st._struct())

    def v2f(self, st):
        st._launch_v2f(st._struct())

    def proposal(self, st):
        st._launch_proposal(st._struct())

    def f2v(self, st):
        st._call_f2v(st._struct())

    def install(self, st, host_particles):
        st._draws = self.draws
        self.draws += 1
        if host_particles is None:
            st.sampler = 'device'
        else:
            st.sampler = lambda kk, flat, q: host_particles
        st._generate_sample()

    @staticmethod
    def host(t):
        return t.cpu().numpy()

    @staticmethod
    def gather(t, index):
        return t.index_select(0, _abi.to_dev(np.asarray(index, dtype=np.int64))).contiguous()

