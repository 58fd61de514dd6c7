"""Every f -> v kernel family of csrc/pbp.hip (heavy, small16 / small32, light, pair, fast, cq, generic) point by point against
the longdouble twin of tests/pbp_f2v_models.py, on hand-built states: a solver is set up on the state's graph, the state's
particles, old particles and v -> f messages are copied over its tensors, and ``lhvi_pbp_f2v`` runs with ONE family flag set into
an output filled with NaN -- no sweep.

Bounds: ``pbp_f2v_models.f2v_bound`` (derived there: a few 1e-13 for ordinary messages, 2e-12 to 3e-12 at the edge of the regular
class) for every regular point, ``== -700.0`` for every dead point; no point is left out.  The integral points of an edge that
may take the uniform-grid recurrence (heavy: at least 24 partner particles; small and cq: any) are held to the recurrence's bound
whichever way the range guard decided, all other points to the direct (or ocml) bound.

The generic kernel refuses an edge that ``classify_edge`` does not call generic, so the second opinion on the quadratic-family
classes comes from ``lhvi_pbp_edge_points``: the same ``f2v_point_generic`` (potential evaluated from the parameter row, one
``exp`` per term), with the partners' particles handed over as the sample.  The conditionally quadratic edges also go through the
generic kernel itself, as its work list with the routing flag cleared."""
import numpy as np
import pytest

import pbp_f2v_models as fm

pytestmark = pytest.mark.gpu

COUNTERS = 8            # LHVI_PBP_TICKET_COUNTERS: work counters, then the grid / fallback edge counts
GRID_MIN_NJ = 24

# (state, n, T, options of the state / the solver, families that must have work)
CASES = {
    'n64 T32': ('zoo', 64, 32, {}, ('heavy', 'pair', 'fast', 'cq', 'generic')),
    'n64 T100 uniform': ('zoo', 64, 100, {'long_grid': True}, ('heavy', 'pair', 'fast', 'generic')),
    'n64 T128 uniform': ('zoo', 64, 128, {'long_grid': True}, ('heavy', 'pair', 'fast', 'generic')),
    'n64 T100 uneven': ('zoo', 64, 100, {'uneven': True, 'long_grid': True}, ('pair', 'fast', 'generic')),
    'n64 T70': ('zoo', 64, 70, {}, ('pair', 'fast', 'generic')),
    'n100 T20': ('zoo', 100, 20, {}, ('heavy', 'pair', 'fast', 'generic')),
    'n33 T7': ('zoo', 33, 7, {}, ('heavy', 'pair', 'fast', 'cq', 'generic')),
    'n5 T20': ('zoo', 5, 20, {}, ('small', 'pair', 'fast', 'cq', 'generic')),
    'n64 T0': ('zoo', 64, 0, {}, ('heavy', 'pair', 'fast', 'cq', 'generic')),
    'ranges n64 T32': ('ranges', 64, 32, {}, ('heavy', 'pair', 'fast', 'cq', 'generic')),
    'ranges n64 T100 uniform': ('ranges', 64, 100, {'long_grid': True, 'both_guards': True}, ('heavy', 'pair', 'fast', 'generic')),
    'ranges n16 T32': ('ranges', 16, 32, {}, ('small', 'pair', 'fast', 'cq', 'generic')),
    'lifted n16': ('lifted', 16, 20, {}, ('small', 'generic')),
}
for _n, _T in ((10, 20), (12, 20), (16, 32), (20, 32), (24, 32), (32, 100)):
    for _pow2 in (False, True):
        CASES['n%d T%d%s' % (_n, _T, ' pow2' if _pow2 else '')] = ('zoo', _n, _T, {'pow2': _pow2}, ('small', 'pair', 'fast', 'cq', 'generic'))
KNOBS = {'paired_light off': {'paired_light': False}, 'cq_routing off': {'cq_routing': False}, 'small_f2v off': {'small_f2v': False}}


@pytest.fixture(scope='module')
def api():
    from lhvi import _abi
    _abi.require_gpu()
    return _abi


_states = {}


def state(kind, n, T, uneven=False):
    key = (kind, n, T, uneven)
    if key not in _states:
        _states[key] = fm.lifted(n, T) if kind == 'lifted' else fm.ranges(n, T) if kind == 'ranges' else fm.zoo(n, T, uneven=uneven)
    return _states[key]


def make_solver(api, st, long_grid=False, **knobs):
    """a solver on the state's graph with the state's particles, old particles and v -> f messages copied over its own; no sweep"""
    from lhvi.pbp import EPBP, HybridLBP
    if st.epbp:
        bp = EPBP(None, n=st.n, proposal_approximation='simple', sampler='device', seed=1)
    else:
        bp = HybridLBP.on_flat(st.flat, n=st.n, proposal_approximation='simple', sampler='device', seed=1)
    for name, value in knobs.items():
        setattr(bp, name, value)
    if long_grid:
        bp.long_grid_min_edges = 0
    bp._setup(None, flat=st.flat)
    api.check(api.lib().lhvi_pbp_init(bp.dg.g, bp._struct(), api.ptr(bp.eta), api.ptr(bp.q_dev), api.ptr(bp.f2v), api.ptr(bp.v2f),
                                      api.stream_ptr()))
    assert tuple(bp.particles.shape) == st.particles.shape and tuple(bp.v2f.shape) == st.v2f.shape
    assert (bp.np_host == st.counts).all()
    bp.particles.copy_(api.to_dev(st.particles))
    bp.old_particles.copy_(api.to_dev(st.old_particles))
    bp.v2f.copy_(api.to_dev(st.v2f))
    return bp


def family_flags(api, bp):
    """the seven families by the flag that runs them alone; the light edges are one flag, served per factor ('pair') when the solver
    holds pair records and per edge ('light') otherwise"""
    light = 'pair' if bp.paired_light and bp.n_pair else 'light'
    return {'heavy': api.PBP_F2V_HEAVY, 'small': api.PBP_F2V_SMALL, light: api.PBP_F2V_PAIR, 'fast': api.PBP_F2V_FAST,
            'cq': api.PBP_F2V_CQ, 'generic': api.PBP_F2V_GENERIC}


def run_family(api, bp, flag, extra=0):
    """the [E, n + T] table after one ``lhvi_pbp_f2v`` of one family into NaN, and the ticket words"""
    import torch
    out = torch.full_like(bp.f2v, float('nan'))
    s = bp._struct()
    s.flags |= flag | extra
    tick = torch.zeros(16, dtype=torch.int32, device=out.device)
    s.f2v_ticket = api.ptr(tick)
    api.check(api.lib().lhvi_pbp_f2v(bp.dg.g, bp.dg.p, s, api.ptr(bp.v2f), api.ptr(out), api.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy(), tick.cpu().numpy()


def own_points(st):
    """[E, n + T] mask: the points a sweep computes -- [0, np) and [n, n + T) of the rows of the hidden, canonical edges"""
    fl = st.flat
    S = st.n + (int(fl.var_nstates[fl.var_cont].max()) if fl.var_cont.any() else 0)
    mask = np.zeros((fl.E, S), dtype=bool)
    for e in st.edges():
        tw = st.twin(e)
        mask[e, :tw.np_] = True
        mask[e, st.n:st.n + tw.x.size - tw.np_] = True
    return mask


def bounds_of(st, e, family):
    """the bound of every point of edge e when `family` serves it"""
    fl = st.flat
    tw = st.twin(e)
    T = tw.x.size - tw.np_
    bound = fm.f2v_bound(tw.M, tw.n_terms, tw.L, fm.PATH_OF_FAMILY[family])
    f = fl.edge_fac[e]
    if family in ('heavy', 'small', 'cq') and st.uniform and 2 <= T <= 128 and fl.var_cont[fl.edge_var[e]]:
        nj = max([int(st.counts[fl.edge_var[r]]) for r in range(fl.fac_ptr[f], fl.fac_ptr[f + 1])
                  if r != e and fl.var_hidden[fl.edge_var[r]] and fl.var_cont[fl.edge_var[r]]], default=1)
        if family != 'heavy' or nj >= GRID_MIN_NJ:
            g = fm.grid_deviation(fl, fl.var_dom[fl.edge_var[e]])
            bound[tw.np_:] = fm.f2v_bound(tw.M[tw.np_:].max(), tw.n_terms, tw.L[tw.np_:], 'recurrence', t=np.arange(T), grid_dev=g)
    return bound


def hold_to_twin(st, table, served_by, what, edges=None):
    """every point of every hidden, canonical edge: regular ones within the bound of the family that served the edge, dead ones at
    the floor.  Prints the worst |out - L| / bound per family and returns them"""
    worst, dead_points = {}, 0
    for e in st.edges() if edges is None else edges:
        tw = st.twin(e)
        regular, dead = fm.classify(tw)
        got = np.concatenate([table[e, :tw.np_], table[e, st.n:st.n + tw.x.size - tw.np_]])
        fam = served_by[e]
        assert np.isfinite(got).all(), (what, e, fam)
        ratio = np.abs(got[regular] - tw.L[regular].astype(np.float64)) / bounds_of(st, e, fam)[regular]
        if ratio.size:
            k = int(np.argmax(ratio))
            if ratio[k] > worst.get(fam, (0.0,))[0]:
                worst[fam] = (float(ratio[k]), int(e), st.labels[st.flat.edge_fac[e]], float(got[regular][k]))
        assert (got[dead] == fm.FLOOR).all(), (what, e, fam, got[dead])
        dead_points += int(dead.sum())
    print('%s: worst |out - L| / bound per family: %s; %d dead points at -700' %
          (what, ', '.join('%s %.3f (edge %d, %s, L = %.4g)' % ((k,) + v) for k, v in sorted(worst.items())), dead_points))
    bad = {k: v for k, v in worst.items() if not v[0] <= 1.0}
    assert not bad, (what, bad)
    return worst


def partition(api, st, bp, extra=0, **routing):
    """one run per family: the families' writes are disjoint, together they are exactly the points a sweep computes, and every edge
    was written by the family the routing table names.  Returns (the assembled table, family per edge, ticket words of the heavy run)"""
    own = own_points(st)
    written = np.zeros(own.shape, dtype=np.int32)
    table = np.full(own.shape, np.nan)
    served_by, tick_heavy = {}, None
    for fam, flag in family_flags(api, bp).items():
        out, tick = run_family(api, bp, flag, extra)
        if fam == 'heavy':
            tick_heavy = tick
        w = ~np.isnan(out)
        assert not (w & ~own).any(), (fam, 'wrote outside [0, np) and [n, n + T) of its edges', np.argwhere(w & ~own)[:5])
        written += w
        table[w] = out[w]
        for e in np.flatnonzero(w.any(axis=1)):
            assert e not in served_by, (e, fam, served_by[e])
            served_by[int(e)] = fam
            assert (w[e] == own[e]).all(), (fam, e)
    assert (written == own).all()                   # every point by exactly one family: each NaN pattern is the complement of the others' union
    for e in st.edges():
        want = fm.expected_family(st, e, **routing)
        assert served_by[int(e)] == want, (e, st.labels[st.flat.edge_fac[e]], int(st.flat.edge_pos[e]), served_by[int(e)], want)
    return table, served_by, tick_heavy


@pytest.mark.parametrize('case', list(CASES))
def test_families_partition_the_edges_and_meet_the_twin(api, case):
    kind, n, T, opt, reach = CASES[case]
    st = state(kind, n, T, opt.get('uneven', False))
    bp = make_solver(api, st, long_grid=opt.get('long_grid', False))
    extra = api.PBP_POW2_GROUPS if opt.get('pow2') else 0
    table, served_by, tick = partition(api, st, bp, extra, long_grid=opt.get('long_grid', False))
    have = set(served_by.values())
    assert set(reach) <= have, (case, sorted(have))
    lists = {'heavy': bp.n_heavy, 'small': bp.n_small16 + bp.n_small32, 'pair': bp.n_pair, 'fast': int(bp.fast_edges.numel()),
             'cq': bp.n_cq, 'generic': int(bp.generic_edges.numel())}
    assert all(lists[f] > 0 for f in reach), lists
    if 'uniform' in case:
        assert int(tick[COUNTERS]) > 0                              # the recurrence did run
    if opt.get('both_guards'):
        assert int(tick[COUNTERS]) > 0 and int(tick[COUNTERS + 1]) > 0, tick     # ... and the range guard tripped on other edges
    hold_to_twin(st, table, served_by, case)


@pytest.mark.parametrize('knob', list(KNOBS))
@pytest.mark.parametrize('n', [64, 16])
def test_knobs_change_the_route_not_the_bound(api, knob, n):
    """paired_light / cq_routing / small_f2v off: the same state, the edges on the lists the routing table names without the
    knob, the same bound"""
    st = state('zoo', n, 32)
    bp = make_solver(api, st, **KNOBS[knob])
    table, served_by, _ = partition(api, st, bp, **KNOBS[knob])
    if knob == 'paired_light off':
        assert bp.n_pair == 0 and bp.n_light > 0 and 'light' in served_by.values() and 'pair' not in served_by.values()
    if knob == 'cq_routing off':
        assert bp.n_cq == 0 and 'cq' not in served_by.values()
    if knob == 'small_f2v off':
        assert bp.n_small16 + bp.n_small32 == 0 and 'small' not in served_by.values()
    hold_to_twin(st, table, served_by, '%s, n = %d' % (knob, n))


@pytest.mark.parametrize('kind, n', [('zoo', 64), ('zoo', 16), ('ranges', 16), ('lifted', 16)])
def test_generic_evaluation_as_a_second_opinion(api, kind, n):
    """the quadratic-family classes through ``f2v_point_generic`` (``lhvi_pbp_edge_points`` with the partners' particles as the
    sample): the potential from its parameter row, not from a descriptor -- held to the twin with the ocml bound, so two device
    paths with different coefficient resolution agree with one host value"""
    import torch
    st = state(kind, n, 20 if kind == 'lifted' else 32)
    bp = make_solver(api, st)
    fl = st.flat
    quad = set(fm.PAIR_KINDS) | {'hybrid2', 'hybrid3', 'hybrid4', 'cq1', 'cq3', 'ring', 'repeat'}
    edges = [int(e) for e in st.edges() if st.labels[fl.edge_fac[e]] in quad]
    table = np.full((fl.E, bp.f2v.shape[1]), np.nan)
    by_count = {}
    for e in edges:
        by_count.setdefault(st.twin(e).x.size, []).append(e)
    s = bp._struct()
    s.particles = api.ptr(bp.old_particles)
    for npts, es in by_count.items():
        x = api.to_dev(np.stack([st.twin(e).x for e in es]))
        q = api.to_dev(np.asarray(es, dtype=np.int32))
        out = torch.full_like(x, float('nan'))
        api.check(api.lib().lhvi_pbp_edge_points(bp.dg.g, bp.dg.p, s, api.ptr(bp.v2f), len(es), api.ptr(q), npts, api.ptr(x),
                                                 api.ptr(out), api.stream_ptr()))
        for e, row in zip(es, out.cpu().numpy()):
            k = st.twin(e).np_
            table[e, :k], table[e, st.n:st.n + npts - k] = row[:k], row[k:]
    assert len(edges) >= 16
    hold_to_twin(st, table, {e: 'generic' for e in edges}, 'generic evaluation on %s, n = %d' % (kind, n), edges=edges)
    # the conditionally quadratic edges through the generic KERNEL: handed over as its list, with the routing flag cleared for the
    # launch so that its classifier lets them pass (tests/test_gpu_pbp.py::test_conditionally_quadratic_routing_equals_the_generic_kernel
    # switches the routing off for a whole run)
    cq = [e for e in edges if st.labels[fl.edge_fac[e]] in ('cq1', 'cq3')]
    if cq:
        lst = api.to_dev(np.asarray(cq, dtype=np.int32))
        out = torch.full_like(bp.f2v, float('nan'))
        s = bp._struct()
        s.flags = (s.flags & ~api.PBP_CQ) | api.PBP_F2V_GENERIC
        s.generic_edges, s.n_generic, s.generic_pts_log2 = api.ptr(lst), len(cq), 6
        api.check(api.lib().lhvi_pbp_f2v(bp.dg.g, bp.dg.p, s, api.ptr(bp.v2f), api.ptr(out), api.stream_ptr()))
        out = out.cpu().numpy()
        assert np.isnan(out[np.setdiff1d(np.arange(fl.E), cq)]).all()
        hold_to_twin(st, out, {e: 'generic' for e in cq}, 'generic kernel on the conditionally quadratic edges of %s, n = %d' % (kind, n), edges=cq)
