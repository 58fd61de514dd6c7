"""Graphs and the parity check for the owner-computes split of the particle sweep (``lhvi/dist.py::OwnerPlan`` / ``OwnerRunner``).

``assert_owner_equals_single`` runs `world` simulated ranks in one process (``dist.LoopbackGroup``) beside the single-GPU sweep and
holds every array a rank computes or receives to the single-GPU array BIT FOR BIT after every sweep.  It returns, per rank, what
the run exercised (``RankStats``), so that a case can assert it tested what it is there for: a graph or a partition that stops
reaching a path must fail its case, not pass it quietly.

The graphs are the smallest at which each path of the sharded sweep still exists:

* ``zoo``: ``pbp_f2v_models.zoo_graph(T=8, reps=4)`` -- every row of the routing table of docs/kernels_particle.md 4.3 under every
  evidence pattern.  Its factors share no variable, so only an ownership that ignores the graph cuts anything: ``round_robin``.
  Discrete ghosts of 2, 3, 4 and 5 states; factors of three variables whose ghosts have different owners (rows for several peers).
* ``hmln``: the paper-popularity hybrid MLN, 220 three-argument conditional-quadratic factors; at world 8 the refined partition
  leaves a rank that owns nothing.
* ``hmln_hub``: the same with 60 papers: the two hidden topic popularities have 68 incident factors each (> LHVI_HUB_DEGREE).
* ``mrf_small``: the synthetic pairwise MRF at an odd grid size, for the few-particle kernels.

Nothing here imports ``lhvi`` or ``torch`` at module level."""
import functools
from collections import namedtuple

import numpy as np

HUB_DEGREE = 64                 # LHVI_HUB_DEGREE (include/lhvi.h): rows longer than this take the hub kernels
SEED = 3

# n_send_more: rows the pack pass copies for a second, third ... peer;  n_cut_factors: local factors with a ghost;
# n_cont_ghost_edges: continuous rows read where they arrived;  ghost_row_widths: widths of the discrete rows received;
# n_hub_rows / n_prop_hubs: owned variables in the v -> f half's hub list / the proposal kernel's sliced rows;
# owned_hubs_cut: owned hidden variables of more than HUB_DEGREE edges with an edge of a cut factor;
# families: global edge id -> f -> v family of every edge the rank computes;  cut_families: the families of its cut edges;
# n_cut_cq_cont_ghost: cut conditional-quadratic factors with a continuous ghost;  res_lists: OwnerRunner.res_lists;
# split_f2v: the f -> v schedule that ran;  n_owned: owned variables (0: the rank takes part in every phase as a no-op);
# n_interior_edges: computed edges of factors without a ghost (the first of the two f -> v launches);
# cq_ghost_families: the families of the computed edges of the cut conditional-quadratic factors with a continuous ghost
RankStats = namedtuple('RankStats', 'n_send_more n_cut_factors n_cont_ghost_edges ghost_row_widths n_hub_rows n_prop_hubs owned_hubs_cut '
                                    'families cut_families n_cut_cq_cont_ghost res_lists split_f2v n_owned n_interior_edges cq_ghost_families')


# ---- graphs ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def graph(name):
    from lhvi import synth
    if name == 'zoo':
        import pbp_f2v_models as fm
        flat = fm.zoo_graph(T=8, reps=4)[0]
        assert (flat.V, flat.F, flat.E) == (312, 144, 312)
        return flat
    if name == 'hmln':
        flat = synth.paper_popularity_flat(P=40, T=5, seed=1, points=8)[0]
        assert (flat.V, flat.F, flat.E) == (265, 260, 700)
        return flat
    if name == 'hmln_hub':
        return synth.paper_popularity_flat(P=60, T=5, seed=1, points=8)[0]
    if name == 'mrf_small':
        return synth.hybrid_mrf_flat(V=600, deg=4, seed=6, T=7)
    raise KeyError(name)


def round_robin(flat, world):
    return (np.arange(flat.V) % world).astype(np.int32)


@functools.lru_cache(maxsize=None)
def ownership(name, world, kind):
    """'round_robin': variable v belongs to rank v % world;  'refined': ``dist.partition_variables``"""
    from lhvi import dist
    flat = graph(name)
    return round_robin(flat, world) if kind == 'round_robin' else dist.partition_variables(flat, world)


def hidden_hubs(flat):
    return np.flatnonzero(np.isnan(flat.var_value) & (np.diff(flat.var_ptr) > HUB_DEGREE))


def has_cq_block(flat):
    """bool [F]: the factor's potential is an MLN formula with a conditional-quadratic block (word 2 of its row: the block's offset)"""
    pot = flat.fac_pot.astype(np.int64)
    lo, hi = flat.pot_off[pot].astype(np.int64), flat.pot_off[pot + 1].astype(np.int64)
    head = np.where(hi - lo > 2, flat.pot_param[np.minimum(lo + 2, flat.pot_param.size - 1)], 0.0)
    return (flat.pot_kind[pot] == 8) & (head != 0)


# ---- which list of a sweep state serves which edge -------------------------------------------------------------------------------------
_DESC_BYTES = {'heavy': 128, 'small16': 128, 'small32': 128, 'light': 128, 'cq': 256}


def edge_families(bp):
    """local edge id -> family of ``pbp_f2v_models.FAMILIES``, read from the work lists of the sweep state `bp` the way
    tests/test_gpu_pbp_lists.py reads them (word 0 of a record: its edge; a pair record: words 0 and 1).  The light edges are
    'pair' when the state serves them per factor.  Every listed edge is in exactly one list."""
    import torch
    L = bp.f2v_lists
    out = {}

    def put(edges, fam):
        for e in edges.tolist():
            assert e not in out, 'edge %d is in two lists (%s, %s)' % (e, out[e], fam)
            out[e] = fam
    for name, fam in (('heavy', 'heavy'), ('small16', 'small'), ('small32', 'small'), ('cq', 'cq')):
        if getattr(L, 'n_' + name):
            put(getattr(L, name + '_desc').view(torch.int32).view(-1, _DESC_BYTES[name] // 4)[:, 0].cpu(), fam)
    if L.pair_desc is not None and L.n_pair:
        w = L.pair_desc.view(torch.int32).view(-1, 32)[:, :2].cpu().reshape(-1)
        put(w[w >= 0], 'pair')
    elif L.n_light:
        put(L.light_desc.view(torch.int32).view(-1, 32)[:, 0].cpu(), 'light')
    put(L.fast_edges.cpu(), 'fast')
    put(L.generic_edges.cpu(), 'generic')
    return out


# ---- the single-GPU run: made once per (graph, particles, proposal), kept unchanged --------------------------------------------------
SingleRun = namedtuple('SingleRun', 'flat bp families sweeps')       # sweeps: per sweep a dict of clones of q, particles, v2f, f2v
_single = {}


def single_run(flat, n, proposal, sweeps, seed=SEED):
    from lhvi import dist
    from lhvi.pbp import EPBP
    key = (id(flat), n, proposal, sweeps, seed, EPBP.paired_light)
    if key not in _single:
        bp = EPBP(None, n=n, proposal_approximation=proposal, sampler='device', seed=seed)
        bp._setup(None, flat=flat)
        single = dist.SingleRunner(bp)
        single.init()
        snaps = []
        for _ in range(sweeps):
            single.sweep()
            snaps.append({k: getattr(bp, k).clone() for k in ('q_dev', 'particles', 'v2f', 'f2v')})
        _single[key] = SingleRun(flat, bp, edge_families(bp), snaps)
    return _single[key]


# ---- the parity check --------------------------------------------------------------------------------------------------------------------
def rank_stats(runner):
    plan, lf = runner.plan, runner.plan.flat
    if runner.bp is None:
        return RankStats(0, 0, 0, (), 0, 0, 0, {}, frozenset(), 0, None, runner.split_f2v, 0, 0, frozenset())
    bp = runner.bp
    local = edge_families(bp)
    computed = np.flatnonzero(~plan.edge_skip)
    # the lists hold exactly the edges whose message is this rank's to compute
    assert sorted(local) == computed.tolist()
    ghost = (np.arange(lf.V) >= plan.n_owned) & (np.arange(lf.V) < plan.n_owned + plan.n_ghost)
    fac_cut = plan.edge_key[lf.fac_ptr[:-1]].astype(bool)
    cont_ghost = np.maximum.reduceat((ghost & lf.var_cont)[lf.edge_var].astype(np.int8), lf.fac_ptr[:-1]).astype(bool)
    deg = np.diff(lf.var_ptr)
    owned_h = (np.arange(lf.V) < plan.n_owned) & np.isnan(lf.var_value)
    cut_at = np.zeros(lf.V, dtype=bool)
    cut_at[lf.edge_var[plan.edge_key.astype(bool)]] = True
    R = runner.lay['recv']
    cq_ghost = fac_cut & cont_ghost & has_cq_block(lf)
    return RankStats(
        n_send_more=int(runner.n_send_more), n_cut_factors=int(fac_cut.sum()), n_cont_ghost_edges=int(R['cont_edge'].size),
        ghost_row_widths=tuple(sorted(set(R['row_width'].tolist()))),
        n_hub_rows=int(bp.v2f_lists.n_hub) if bp.v2f_lists is not None else 0, n_prop_hubs=int(bp.n_prop_hub),
        owned_hubs_cut=int((owned_h & (deg > HUB_DEGREE) & cut_at).sum()),
        families={int(plan.edge_ids[e]): fam for e, fam in local.items()},
        cut_families=frozenset(fam for e, fam in local.items() if plan.edge_key[e]),
        n_cut_cq_cont_ghost=int(cq_ghost.sum()),
        res_lists=runner.res_lists, split_f2v=bool(runner.split_f2v), n_owned=int(plan.n_owned),
        n_interior_edges=int((~plan.edge_skip & (plan.edge_key == 0)).sum()),
        cq_ghost_families=frozenset(fam for e, fam in local.items() if cq_ghost[lf.edge_fac[e]]))


def assert_owner_equals_single(flat, n, world, var_owner, proposal, sweeps=3, split_f2v=None, seed=SEED):
    """`world` simulated ranks of the owner-computes split of `flat` (loopback exchange) against the single-GPU sweep with `n`
    particles and the given `proposal` ('simple' / 'EP'): after every sweep, on every rank, ``torch.equal`` on the proposals of the
    owned hidden variables and of the continuous ghosts, the live particle columns of both, the v -> f rows of the edges the rank
    computes and of every hidden edge (ghost edges: the rows received) and the f -> v rows of the computed edges.  Before the
    first sweep: every computed edge is served by the f -> v family that serves it on one GPU.
    `split_f2v`: True / False forces the two-launch / one-launch f -> v schedule (None: ``OwnerRunner.min_interior`` decides).
    Returns [RankStats] by rank."""
    import torch
    from lhvi import dist
    ref = single_run(flat, n, proposal, sweeps, seed)
    group = dist.LoopbackGroup(world)
    runners = [dist.OwnerRunner(flat, n=n, seed=seed, rank=r, world=world, proposal_approximation=proposal, group=group,
                                var_owner=var_owner) for r in range(world)]
    stats = []
    for r in runners:
        if split_f2v is not None:
            r.split_f2v = bool(split_f2v)
        stats.append(rank_stats(r))
        r.init()
    # routing: the family of every computed edge is the family of the same edge in the single-GPU run
    for st in stats:
        wrong = {e: (fam, ref.families.get(e)) for e, fam in st.families.items() if ref.families.get(e) != fam}
        assert not wrong, 'f -> v family on the shard differs from the single-GPU one (edge: shard, single): %s' % dict(list(wrong.items())[:8])
    computed = np.zeros(flat.E, dtype=int)
    for r in runners:
        computed[r.plan.edge_ids[~r.plan.edge_skip]] += 1
    np.testing.assert_array_equal(computed, np.isnan(flat.var_value)[flat.edge_var].astype(int))
    dev = ref.bp.q_dev.device
    for it in range(sweeps):
        one = ref.sweeps[it]
        sends = [r.owned_half() for r in runners]
        for r, s in zip(runners, sends):
            assert s.numel() == sum(r.counts)
            group.post(r.rank, s, r.counts)
        for r in runners:
            r.interior()
        recvs = [group.collect(r.rank, None) for r in runners]
        for r, recv in zip(runners, recvs):
            assert recv.numel() == r.lay['recv']['size']
        for r, recv in zip(runners, recvs):
            r.boundary(recv)
        for r in runners:
            plan = r.plan
            if r.bp is None:
                assert plan.n_owned == 0 and plan.flat.E == 0 and not any(r.counts) and r.lay['recv']['size'] == 0
                continue
            where = 'sweep %d, rank %d of %d' % (it, r.rank, world)
            gid = torch.from_numpy(plan.var_gid).to(dev)
            own = torch.from_numpy((np.arange(plan.flat.V) < plan.n_owned) & plan.flat.var_hidden).to(dev)
            loc = torch.from_numpy((np.arange(plan.flat.V) < plan.n_owned + plan.n_ghost) & plan.flat.var_hidden).to(dev)
            live = torch.from_numpy(np.arange(n)[None, :] < r.bp.np_host[:, None]).to(dev)
            assert torch.equal(r.bp.q_dev[own], one['q_dev'][gid][own]), 'q of the owned variables, ' + where
            cont = torch.from_numpy(plan.flat.var_cont).to(dev)
            assert torch.equal(r.bp.q_dev[loc & cont], one['q_dev'][gid][loc & cont]), 'q of the continuous ghosts, ' + where
            assert torch.equal(torch.where(live, r.bp.particles, 0.0)[loc], torch.where(live, one['particles'][gid], 0.0)[loc]), \
                'particles, ' + where
            eid = torch.from_numpy(plan.edge_ids).to(dev)
            mine = torch.from_numpy(~plan.edge_skip).to(dev)
            le = live[torch.from_numpy(plan.flat.edge_var.astype(np.int64)).to(dev)]
            rows = r.message_rows()                     # (continuous ghost edges: gathered from where their rows arrived)
            assert torch.equal(torch.where(le, rows, 0.0)[mine], torch.where(le, one['v2f'][eid], 0.0)[mine]), 'v2f of the computed edges, ' + where
            bad = (r.bp.f2v[mine] != one['f2v'][eid][mine]).any(dim=1)
            if bool(bad.any()):
                ge = eid[mine][bad].tolist()
                diff = float((r.bp.f2v[mine][bad] - one['f2v'][eid][mine][bad]).abs().max())
                raise AssertionError('f2v of %d computed edges differs by up to %.3g, %s: global edges %s (families %s)' % (
                    len(ge), diff, where, ge[:8], sorted({ref.families.get(e) for e in ge})))
            assert torch.equal(r.bp.f2v[mine], one['f2v'][eid][mine]), 'f2v (NaN), ' + where
            hid_e = torch.from_numpy(plan.flat.var_hidden[plan.flat.edge_var]).to(dev)
            assert torch.equal(torch.where(le, rows, 0.0)[hid_e], torch.where(le, one['v2f'][eid], 0.0)[hid_e]), 'v2f of the hidden edges, ' + where
    assert torch.isfinite(ref.sweeps[-1]['q_dev'][torch.from_numpy(flat.var_hidden).to(dev)]).all()
    return stats


# ---- plan invariants (host only) -------------------------------------------------------------------------------------------------------
def send_more_rows(plan, n):
    """the rows of the send layout beyond the first place of their edge, as ``OwnerRunner`` finds them: (edges, offsets, the peer
    whose block each offset lies in, the peer of the edge's first place)"""
    S = plan.layout(n)['send']
    edge, off, _ = plan.rows_of(S, n)
    first = np.unique(edge, return_index=True)[1]
    more = np.setdiff1d(np.arange(edge.size), first)
    ends = np.cumsum(S['counts'])
    peer_of = lambda o: np.searchsorted(ends, o, side='right')
    first_peer = dict(zip(edge[first].tolist(), peer_of(off[first]).tolist()))
    return edge[more], off[more], peer_of(off[more]), np.array([first_peer[e] for e in edge[more].tolist()], dtype=np.int64)


def assert_plan_invariants(flat, owner, world, particle_counts=(10, 16, 64, 100)):
    """what tests/test_dist.py::test_owner_plan_invariants asserts, on any graph and ownership: every message computed exactly
    once; both ends of every pair list the same rows and proposals in the same order; per particle count the layouts do not
    overlap, are padded to whole rows, keep continuous rows on multiples of n, and ``ghost_rows`` names exactly those rows.
    Returns the plans."""
    from lhvi.dist import OwnerPlan
    plans = [OwnerPlan(flat, r, world, var_owner=owner) for r in range(world)]
    hid = np.isnan(flat.var_value)
    computed = np.zeros(flat.E, dtype=int)
    for p in plans:
        lf = p.flat
        np.testing.assert_array_equal(p.var_gid[lf.edge_var], flat.edge_var[p.edge_ids])
        own = np.arange(lf.V) < p.n_owned
        assert (owner[p.var_gid[own]] == p.rank).all() and (owner[p.var_gid[~own]] != p.rank).all()
        # an owned hidden variable has ALL its edges here, in the order of its row in the whole graph
        for v in np.flatnonzero(own & np.isnan(lf.var_value)):
            g = p.var_gid[v]
            np.testing.assert_array_equal(p.edge_ids[lf.var_edge[lf.var_ptr[v]:lf.var_ptr[v + 1]]], flat.var_edge[flat.var_ptr[g]:flat.var_ptr[g + 1]])
        computed[p.edge_ids[~p.edge_skip]] += 1
        ghost = (np.arange(lf.V) >= p.n_owned) & (np.arange(lf.V) < p.n_owned + p.n_ghost)
        assert np.isnan(lf.var_value[ghost]).all()
        want_key = np.repeat(np.maximum.reduceat(ghost[lf.edge_var].astype(np.int8), lf.fac_ptr[:-1]), np.diff(lf.fac_ptr)) if lf.F else np.zeros(0)
        np.testing.assert_array_equal(p.edge_key.astype(bool), want_key.astype(bool))
    np.testing.assert_array_equal(computed, hid[flat.edge_var].astype(int))
    for p in plans:
        lf = p.flat
        got_rows = np.concatenate([p.recv_rows[s] for s in range(world) if s != p.rank])
        ghost = (np.arange(lf.V) >= p.n_owned) & (np.arange(lf.V) < p.n_owned + p.n_ghost)
        # every ghost edge receives exactly one row
        np.testing.assert_array_equal(np.sort(got_rows), np.flatnonzero(ghost[lf.edge_var]))
        for s in range(world):
            if s != p.rank:
                q = plans[s]
                np.testing.assert_array_equal(p.edge_ids[p.send_rows[s]], q.edge_ids[q.recv_rows[p.rank]])
                np.testing.assert_array_equal(p.var_gid[p.send_q[s]], q.var_gid[q.recv_q[p.rank]])
        for n in particle_counts:
            lay = p.layout(n)
            for side in ('send', 'recv'):
                L = lay[side]
                e, o, w = p.rows_of(L, n)
                used = int(w.sum()) + 2 * L['q_var'].size
                assert sum(L['counts']) == L['size'] and all(c % n == 0 for c in L['counts']) and 0 <= L['size'] - used < n * world
                offs = np.concatenate([np.repeat(o, w) + np.concatenate([np.arange(k) for k in w] or [np.zeros(0, int)]),
                                       np.repeat(L['q_off'], 2) + np.tile([0, 1], L['q_var'].size)])
                assert np.unique(offs).size == offs.size == used and offs.min(initial=0) >= 0 and offs.max(initial=-1) < L['size']
                assert (L['cont_off'] % n == 0).all() and lf.var_cont[lf.edge_var[L['cont_edge']]].all()
                # a discrete row is as wide as its variable has states
                assert (L['row_width'] == lf.var_nstates[lf.edge_var[L['row_edge']]]).all() and (L['row_width'] <= n).all()
            canon, extra = p.ghost_rows(n)
            R = lay['recv']
            assert (canon[R['cont_edge']] == lf.E + R['cont_off'] // n).all() and extra * n >= R['size']
            rest = np.setdiff1d(np.arange(lf.E), R['cont_edge'])
            assert (canon[rest] == rest).all()
            # the continuous ghost edges are exactly the rows read in place
            np.testing.assert_array_equal(np.sort(R['cont_edge']), np.flatnonzero((ghost & lf.var_cont)[lf.edge_var]))
            for s in range(world):
                if s != p.rank:
                    assert lay['send']['counts'][s] == plans[s].layout(n)['recv']['counts'][p.rank]
    return plans
