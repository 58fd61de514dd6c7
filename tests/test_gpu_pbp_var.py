"""The per-variable kernels of csrc/pbp.hip value by value against the longdouble twin of tests/pbp_var_models.py, on hand-built
states: a solver is set up on the state's graph (``_setup`` + ``lhvi_pbp_init``, no sweep), the state's ``f2v``, ``particles``,
``uniq``, ``q`` and ``eta`` are copied over its tensors, the outputs are filled with a sentinel and ONE entry point is called once
through the solver's own struct and lists.

  ``lhvi_pbp_v2f``        range walk (``packed_v2f`` off), the five lists one by one and together, the wide list as records and as
                          a plain list; ground and lifted, both flag sets, n from 5 to 129
  ``lhvi_pbp_proposal``   both rules; range walk, records, slices at ``prop_slice`` 64 and 8; ``lhvi_pbp_proposal_partial`` +
                          ``lhvi_pbp_proposal_finish`` on one rank; count totals summed and handed over (``var_degree``)
  ``lhvi_pbp_var_fused`` / ``lhvi_pbp_var_fused64``   called with the plan's records: every sub-class 16, 32a, 32b, 64a, 64b

Per call: every live value within its bound (``pbp_var_models``: derived there), every kept site and every floored variance bit
for bit, every value of an observed variable, of a lane >= np and of an edge the route does not own still the sentinel; no value is
left out.  The worst |out - twin| / bound is printed per route."""
import functools

import numpy as np
import pytest

import pbp_var_models as vm

pytestmark = pytest.mark.gpu

SEED, ITERATION = (1 << 40) + 12345, 3


@pytest.fixture(scope='module')
def api():
    from lhvi import _abi
    _abi.require_gpu()
    return _abi


@functools.lru_cache(maxsize=None)
def state(family, n, epbp, ep, lifted, thr=None, var_degree=False):
    return vm.build(n, family=family, epbp=epbp, ep=ep, lifted=lifted, var_threshold=thr, var_degree=var_degree)


def make_solver(api, st, **knobs):
    """a solver on the state's graph (the variable side alone) with the state's arrays copied over its own; no sweep"""
    from lhvi.pbp import EPBP, HybridLBP
    rule = 'EP' if st.ep else 'simple'
    if st.epbp:
        bp = EPBP(None, n=st.n, proposal_approximation=rule, sampler='device', seed=1)
    else:
        bp = HybridLBP.on_flat(st.flat, n=st.n, proposal_approximation=rule, sampler='device', seed=1)
    bp.var_threshold = st.var_threshold
    for name, value in knobs.items():
        setattr(bp, name, value)
    bp._setup(None, flat=st.flat, sides='v')
    api.check(api.lib().lhvi_pbp_init(bp.dg.g, bp._struct(), api.ptr(bp.eta), api.ptr(bp.q_dev), api.ptr(bp.f2v), api.ptr(bp.v2f),
                                      api.stream_ptr()))
    assert tuple(bp.f2v.shape) == st.f2v.shape and (bp.np_host == st.counts).all()
    if 'init' in {t for tags in st.tags.values() for t in tags}:
        # the state holds what pbp_init_kernel writes: the sites and proposals of the continuous variables
        eta, q = bp.eta.cpu().numpy(), bp.q_dev.cpu().numpy()
        for v in st.cont():
            assert (q[v] == st.q[v]).all() and (eta[st.rows(v)] == st.eta[st.rows(v)]).all(), v
    for name, value in (('f2v', st.f2v), ('particles', st.particles), ('uniq', st.uniq), ('q_dev', st.q), ('eta', st.eta)):
        getattr(bp, name).copy_(api.to_dev(value))
    return bp


def list_vars(lists, name):
    t, cnt = getattr(lists, name).cpu().numpy(), getattr(lists, 'n_' + name)
    return (t[:cnt, 0] if t.ndim == 2 else t[:cnt]).astype(np.int64)


def edges_of(st, variables):
    mask = np.zeros(st.flat.E, dtype=bool)
    for v in variables:
        mask[st.rows(v)] = True
    return mask


def hold_v2f(st, out, own, what):
    """`own` [E]: the edges the call owns.  Their live values within the bound; everything else still NaN.  Returns the worst ratio"""
    tw = st.v2f()
    live = tw.live & own[:, None]
    assert np.isnan(out[~live]).all(), (what, 'wrote outside its rows', np.argwhere(~np.isnan(out) & ~live)[:5])
    assert live.any(), what
    r = vm.ratio(out[live], tw.out[live], tw.bound[live])
    k = int(np.argmax(r))
    e, j = np.argwhere(live)[k]
    print('%s: %d values, worst |out - twin| / bound = %.3f (edge %d of variable %d, particle %d, bound %.2e)' %
          (what, r.size, r[k], e, st.flat.edge_var[e], j, tw.bound[e, j]))
    assert r[k] <= 1.0, (what, int(e), int(j), float(r[k]), float(out[e, j]), float(tw.out[e, j]))
    return float(r[k])


def run_v2f(api, bp, only=None):
    """one ``lhvi_pbp_v2f`` into NaN; `only`: a list name -- the other lists' counts are zero for this launch"""
    import torch
    out = torch.full_like(bp.v2f, float('nan'))
    s = bp._struct()
    if only is not None:
        for name in ('wide', 'narrow', 'hub', 'mid16', 'mid32'):
            if name != only:
                setattr(s, 'n_v2f_' + name, 0)
    api.check(api.lib().lhvi_pbp_v2f(bp.dg.g, s, api.ptr(bp.f2v), api.ptr(out), api.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


# (family, n, EPBP flags, lifted)
V2F_CASES = [('zoo', 64, True, False), ('ranges', 64, False, True), ('ranges', 20, True, True), ('zoo', 16, False, True),
             ('ranges', 5, True, False), ('zoo', 10, False, False), ('ranges', 17, True, True), ('zoo', 32, True, False),
             ('ranges', 33, False, True), ('zoo', 48, True, True), ('ranges', 65, True, True), ('ranges', 100, True, True),
             ('zoo', 129, False, False), ('ranges', 129, True, True)]


@pytest.mark.parametrize('family, n, epbp, lifted', V2F_CASES)
def test_v2f_routes_meet_the_twin(api, monkeypatch, family, n, epbp, lifted):
    st = state(family, n, epbp, False, lifted)
    what = '%s n = %d %s %s' % (family, n, 'EPBP' if epbp else 'HLBP', 'lifted' if lifted else 'ground')
    every = np.ones(st.flat.E, dtype=bool)
    # the range walk: one wavefront per variable, np > 64 in chunks with the second balancing pass
    bp = make_solver(api, st, packed_v2f=False)
    assert bp.v2f_lists is None
    hold_v2f(st, run_v2f(api, bp), every, what + ', range walk')
    # the lists, one by one and together; the wide list as records
    bp = make_solver(api, st)
    L = bp.v2f_lists
    assert L is not None and bp.flags & api.PBP_V2F_RECORDS
    served = np.zeros(st.flat.V, dtype=int)
    classes = ('wide', 'narrow', 'hub', 'mid16', 'mid32')
    for name in classes:
        vs = list_vars(L, name)
        served[vs] += 1
        if vs.size:
            hold_v2f(st, run_v2f(api, bp, only=name), edges_of(st, vs), '%s, %s list alone' % (what, name))
    assert (served[st.hidden()] == 1).all() and served.sum() == st.hidden().size
    have = {name: getattr(L, 'n_' + name) for name in classes}
    # narrow: np <= 4; hub: a row of more than 64 edges at np <= 64; mid16 / mid32: np <= 16 / 32 (the continuous variables at
    # n <= 32, else the discrete ones of 5, 7 / 20 states); wide: the rest -- the continuous variables at n > 32
    want = ['narrow', 'hub', 'mid16'] + (['mid32'] if n >= 17 else []) + (['wide'] if n > 32 else [])
    assert all(have[name] > 0 for name in want) and (n > 32 or have['wide'] == 0), (what, have)
    if n > 64:                                              # a hub row at np > 64 is the one-wave kernel's
        deg = np.diff(st.flat.var_ptr)
        wide = list_vars(L, 'wide')
        assert (deg[wide] > 64).any() and (st.counts[list_vars(L, 'hub')] <= 64).all()
    hold_v2f(st, run_v2f(api, bp), every, what + ', the five lists (wide as records)')
    if have['wide']:
        monkeypatch.setenv('LHVI_PBP_V2F_REC', '0')
        bp = make_solver(api, st)
        assert bp.v2f_lists is not None and not bp.flags & api.PBP_V2F_RECORDS and bp.v2f_lists.n_wide == have['wide']
        hold_v2f(st, run_v2f(api, bp, only='wide'), edges_of(st, list_vars(bp.v2f_lists, 'wide')), what + ', wide as a plain list')


# ---- proposal ------------------------------------------------------------------------------------------------------------------------
def hold_sites(st, eta, q, own_vars, what, q_written=True):
    """eta [E, 2] and q [V, 2] after a call that owns the continuous hidden variables `own_vars`: live sites within their bound,
    kept sites and floored variances bit for bit (bound 0), every other site the input's bits, every other q still NaN"""
    pr = st.proposal()
    own_v = np.zeros(st.flat.V, dtype=bool)
    own_v[own_vars] = True
    assert (own_v <= pr.q_live).all()
    own_e = edges_of(st, own_vars)
    assert (own_e <= pr.owned).all()
    assert (eta[~own_e] == st.eta[~own_e]).all(), (what, 'wrote a site it does not own')
    keep = own_e & pr.kept
    assert (eta[keep] == st.eta[keep]).all(), (what, 'a kept site changed', np.flatnonzero(keep & (eta != st.eta).any(axis=1))[:5])
    worst = {}
    for k, name in ((0, 'eta mu'), (1, 'eta sig')):
        r = vm.ratio(eta[own_e, k], pr.eta[own_e, k], pr.eta_bound[own_e, k])
        i = int(np.argmax(r))
        worst[name] = (float(r[i]), int(np.flatnonzero(own_e)[i]))
    if q_written:
        assert np.isnan(q[~own_v]).all(), (what, 'wrote a proposal it does not own')
        for k, name in ((0, 'q mu'), (1, 'q sig')):
            r = vm.ratio(q[own_v, k], pr.q[own_v, k], pr.q_bound[own_v, k])
            i = int(np.argmax(r))
            worst[name] = (float(r[i]), int(np.flatnonzero(own_v)[i]))
    print('%s: %d sites (%d kept, %d floored, %d under the cavity), worst |out - twin| / bound: %s' %
          (what, own_e.sum(), keep.sum(), (own_e & pr.floored).sum(), (own_e & pr.cavity).sum(),
           ', '.join('%s %.3f (at %d)' % ((k,) + v) for k, v in worst.items())))
    bad = {k: v for k, v in worst.items() if not v[0] <= 1.0}
    assert not bad, (what, bad)
    return worst


def run_proposal(api, bp, st, s, partial=False):
    import torch
    eta = api.to_dev(st.eta)
    q = torch.full_like(bp.q_dev, float('nan'))
    if st.var_degree is not None:
        deg = api.to_dev(st.var_degree)
        s.var_degree = api.ptr(deg)
    if partial:
        ph = torch.full_like(bp.q_dev, float('nan'))
        api.check(api.lib().lhvi_pbp_proposal_partial(bp.dg.g, s, api.ptr(bp.f2v), api.ptr(eta), api.ptr(ph), api.stream_ptr()))
        api.check(api.lib().lhvi_pbp_proposal_finish(bp.dg.g, s, api.ptr(ph), api.ptr(q), api.stream_ptr()))
        torch.cuda.synchronize()
        return eta.cpu().numpy(), q.cpu().numpy(), ph.cpu().numpy()
    api.check(api.lib().lhvi_pbp_proposal(bp.dg.g, s, api.ptr(bp.f2v), api.ptr(eta), api.ptr(q), api.stream_ptr()))
    torch.cuda.synchronize()
    return eta.cpu().numpy(), q.cpu().numpy()


# (family, n, EPBP flags, EP rule, lifted, var_threshold, count totals handed over)
PROPOSAL_CASES = [('zoo', 64, True, False, False, None, False), ('zoo', 20, False, True, True, 0.02, False),
                  ('zoo', 33, True, True, False, 0.02, False), ('init', 16, True, True, False, None, False),
                  ('init', 48, False, False, True, None, False), ('zoo', 100, False, True, True, 0.02, True),
                  ('zoo', 10, True, False, True, None, True)]


@pytest.mark.parametrize('family, n, epbp, ep, lifted, thr, var_degree', PROPOSAL_CASES)
def test_proposal_routes_meet_the_twin(api, family, n, epbp, ep, lifted, thr, var_degree):
    st = state(family, n, epbp, ep, lifted, thr, var_degree)
    what = '%s n = %d %s %s %s%s' % (family, n, 'EPBP' if epbp else 'HLBP', 'EP' if ep else 'simple', 'lifted' if lifted else 'ground',
                                     ', totals handed over' if var_degree else '')
    cont = st.cont()
    deg = np.diff(st.flat.var_ptr)
    # records, no slices
    bp = make_solver(api, st, sliced_proposal=False)
    assert bp.n_prop_hub == 0 and bp.n_prop_desc == cont.size
    first = hold_sites(st, *run_proposal(api, bp, st, bp._struct()), cont, what + ', records')
    # the range walk, and the partial / finish pair of a sharded run on one rank: the same q
    eta_r, q_r = run_proposal(api, bp, st, bp._struct(var_range=(0, 0)))
    hold_sites(st, eta_r, q_r, cont, what + ', range walk')
    eta_p, q_p, ph = run_proposal(api, bp, st, bp._struct(var_range=(0, 0)), partial=True)
    hold_sites(st, eta_p, q_p, cont, what + ', partial + finish')
    assert (eta_p == eta_r).all() and np.array_equal(q_p, q_r, equal_nan=True)
    pr = st.proposal()
    assert np.isnan(ph[~pr.q_live]).all()
    r = vm.ratio(1.0 / ph[cont, 0], pr.q[cont, 1], pr.q_bound[cont, 1])
    assert r.max() <= 1.0, (what, 'partial sums', float(r.max()))
    # slices
    for length in (64, 8):
        bp = make_solver(api, st, sliced_proposal=True, prop_slice=length)
        hubs = int((deg[cont] > length).sum())
        assert bp.n_prop_hub == hubs > 0 and bp.n_prop_desc > cont.size
        hold_sites(st, *run_proposal(api, bp, st, bp._struct()), cont, '%s, slices of %d (%d rows sliced)' % (what, length, hubs))
    assert first


# ---- the fused one-pass kernels -----------------------------------------------------------------------------------------------------
# (family, n, EPBP flags, EP rule, lifted, var_threshold, sub-classes that must have work)
FUSED_CASES = [('zoo', 16, True, False, False, None, ('16', '32b')), ('zoo', 16, False, True, True, 0.02, ('16', '32b')),
               ('ranges', 20, True, True, False, 0.02, ('32a', '32b')), ('zoo', 32, False, False, True, None, ('32a', '32b')),
               ('zoo', 33, False, True, True, 0.02, ('64a', '64b')), ('ranges', 64, True, False, False, None, ('64a', '64b')),
               ('zoo', 64, True, True, True, 0.02, ('64a', '64b')), ('init', 10, True, True, False, None, ('16', '32b'))]


@pytest.mark.parametrize('family, n, epbp, ep, lifted, thr, reach', FUSED_CASES)
def test_fused_kernels_meet_the_twin(api, family, n, epbp, ep, lifted, thr, reach):
    import torch
    st = state(family, n, epbp, ep, lifted, thr)
    what = 'fused, %s n = %d %s %s %s' % (family, n, 'EPBP' if epbp else 'HLBP', 'EP' if ep else 'simple', 'lifted' if lifted else 'ground')
    bp = make_solver(api, st)
    F = bp._fused
    assert F is not None
    counts = dict(zip(('16', '32a', '32b'), F['counts']))
    counts.update(zip(('64a', '64b'), F['counts64']))
    assert all(counts[k] > 0 for k in reach) and sum(counts.values()) == sum(counts[k] for k in reach), (what, counts)
    lib, s = api.lib(), bp._struct()
    v2f = torch.full_like(bp.v2f, float('nan'))
    eta = api.to_dev(st.eta)
    q = torch.full_like(bp.q_dev, float('nan'))
    particles = torch.full_like(bp.particles, float('nan'))
    uniq = torch.full_like(bp.uniq, 7)
    args = (bp.dg.g, s, api.ptr(bp.f2v), api.ptr(v2f), api.ptr(eta), api.ptr(q), api.ptr(None), SEED, ITERATION, api.ptr(particles),
            api.ptr(uniq))
    if n <= 32:
        api.check(lib.lhvi_pbp_var_fused(*args, api.ptr(F.desc), *F['counts'], api.stream_ptr()))
        fused = F.desc.cpu().numpy().reshape(-1, 16 if bp.flags & api.PBP_FUSED_RECORDS16 else 8)[:sum(F['counts']), 0]
    else:
        api.check(lib.lhvi_pbp_var_fused64(*args, api.ptr(F.desc64), *F['counts64'], api.stream_ptr()))
        fused = F.desc64.cpu().numpy().reshape(-1, 16)[:sum(F['counts64']), 0]
    torch.cuda.synchronize()
    fused = fused.astype(np.int64)
    # the fused pass owns the continuous variables with at most 64 incident edges and at most 64 integral points
    deg = np.diff(st.flat.var_ptr)
    cont = st.cont()
    want = cont[(deg[cont] <= 64) & (np.array([st.grid(v).size for v in cont]) <= 64)]
    assert sorted(fused.tolist()) == sorted(want.tolist())
    hold_v2f(st, v2f.cpu().numpy(), edges_of(st, fused), what + ', v2f')
    hold_sites(st, eta.cpu().numpy(), q.cpu().numpy(), fused, what)
    # the new sample: what lhvi_pbp_resample_uniq draws from the q this pass wrote, bit for bit (the draw itself is held to its twin
    # in tests/test_gpu_pbp_sampler.py)
    s2 = bp._struct()
    bp.var_lists.install_sampler(s2)
    s2.q = api.ptr(q)
    p2, u2 = torch.full_like(bp.particles, float('nan')), torch.full_like(bp.uniq, 7)
    api.check(lib.lhvi_pbp_resample_uniq(bp.dg.g, s2, api.ptr(None), SEED, ITERATION, api.ptr(p2), api.ptr(u2), api.stream_ptr()))
    torch.cuda.synchronize()
    particles, uniq, p2, u2 = (t.cpu().numpy() for t in (particles, uniq, p2, u2))
    rest = np.setdiff1d(np.arange(st.flat.V), fused)
    assert np.isnan(particles[rest]).all() and (uniq[rest] == 7).all()
    assert not np.isnan(particles[fused]).any()
    assert (particles[fused].view(np.int64) == p2[fused].view(np.int64)).all() and (uniq[fused] == u2[fused]).all()
    assert ((uniq[fused] == 0) | (uniq[fused] == 1)).all() and (uniq[fused, 0] == 1).all()
