"""GPU: every kernel of the Gaussian sweep (csrc/gabp.hip) slot by slot against the longdouble twin of tests/gabp_models.py.

The kernels are driven one half sweep at a time from hand-built messages (`None`, infinite and negative variances and zero means at
the first / last entry of a row, at the ends of a middle chunk and inside the last chunk's remainder), on star forests with every
row length at which a kernel changes what it does, ground and lifted, and on one factor per closed form.  Every message is held
to ``gabp_models.bound`` (derived in that module, never widened), NaN / infinity patterns must be identical, and where gabp.hip
promises the reference's summation order -- rows of at most 512 entries in the pair form and the array pull kernel, of at most 32 in
the record pull kernels, every non-hub row of a lifted graph -- the bits must be the C oracle's.  Worst error / bound ratios of the
run that accompanied this file: docs/kernels_gaussian.md, "How it is tested"."""
import copy
import types

import numpy as np
import pytest

import gabp_models as gm
from gabp_models import model, covered, oracle_marginals, oracle_pull

pytestmark = pytest.mark.gpu

SENTINEL = 7.0


@pytest.fixture(scope='module')
def api():
    from lhvi import _abi
    _abi.require_gpu()
    return _abi


_STATE = {}


def state(api, name, monkeypatch):
    """device graph, pull plan (host and device) and the plan structs of the three pull paths of a model, built once"""
    if name in _STATE:
        return _STATE[name]
    from lhvi.gabp import pull_plan
    flat = model(name)
    monkeypatch.setenv('LHVI_GABP_WINDOW', '256' if name == 'layout256' else '64')
    st = types.SimpleNamespace(flat=flat, name=name)
    st.host = pull_plan(flat)
    st.dg = api.DeviceGraph(flat)
    st.dev = {k: (api.to_dev(a) if a is not None else None) for k, a in st.host.items()}
    st.n_hub_rows = int((np.diff(flat.var_ptr) > gm.HUB).sum())
    if flat.pot_kind.size <= 32:
        # more potentials than the record kernels keep in LDS: pad the table (the padding rows are never referenced)
        wide = copy.copy(flat)
        wide.__dict__.pop('_view_cache', None)
        wide.pot_kind = np.concatenate([flat.pot_kind, np.full(64, flat.pot_kind[0], dtype=flat.pot_kind.dtype)])
        wide.pot_off = np.concatenate([flat.pot_off, np.full(64, flat.pot_off[-1], dtype=flat.pot_off.dtype)])
        st.dgw = api.DeviceGraph(wide)
        st.wide_words = api.to_dev(pull_plan(wide)['pot_words'])
    else:
        st.dgw, st.wide_words = st.dg, st.dev['pot_words']
    _STATE[name] = st
    return st


PATHS = ('arrays', 'records', 'records_global')


def plan_of(api, st, path, seg=None):
    """(graph struct, potentials struct, plan struct, keep-alive) of one pull path; `seg`: hand-built segments instead of the plan's"""
    p = api.GabpPlanStruct()
    p.pslot, p.info, p.count = (api.ptr(st.dev[k]) for k in ('pslot', 'info', 'count'))
    p.n_hub_rows = st.n_hub_rows
    seg_dev = st.dev['seg'] if seg is None else api.to_dev(np.ascontiguousarray(seg, dtype=np.int32))
    p.seg, p.n_seg = api.ptr(seg_dev), int(seg_dev.shape[0])
    p.rec = api.ptr(st.dev['rec']) if path != 'arrays' else None
    dg = st.dgw if path == 'records_global' else st.dg
    words = st.wide_words if path == 'records_global' else st.dev['pot_words']
    p.pot_words = api.ptr(words)
    return dg, p, (seg_dev, words)


def dev_pull(api, st, path, vprev, first, seg=None):
    dg, p, keep = plan_of(api, st, path, seg)
    nnz = int(st.flat.var_edge.size)
    prev = api.to_dev(np.ascontiguousarray(vprev if vprev is not None else np.zeros((nnz, 2))))
    nxt = api.to_dev(np.full((nnz, 2), SENTINEL))
    api.check(api.lib().lhvi_gabp_pull(dg.g, dg.p, p, api.ptr(prev), api.ptr(nxt), int(first), api.stream_ptr()))
    return nxt.cpu().numpy()


def dev_v2f(api, dg_g, flat, f2v):
    a, b = api.to_dev(np.ascontiguousarray(f2v)), api.to_dev(np.full((flat.E, 2), SENTINEL))
    api.check(api.lib().lhvi_gabp_v2f(dg_g, api.ptr(a), api.ptr(b), api.stream_ptr()))
    return b.cpu().numpy()


def dev_f2v(api, st, v2f, f2v_before):
    a, b = api.to_dev(np.ascontiguousarray(v2f)), api.to_dev(np.ascontiguousarray(f2v_before))
    api.check(api.lib().lhvi_gabp_f2v(st.dg.g, st.dg.p, api.ptr(a), api.ptr(b), api.stream_ptr()))
    return b.cpu().numpy()


def dev_marginals(api, dg_g, flat, f2v):
    a, b = api.to_dev(np.ascontiguousarray(f2v)), api.to_dev(np.full((flat.V, 2), SENTINEL))
    api.check(api.lib().lhvi_gabp_marginals(dg_g, api.ptr(a), api.ptr(b), api.stream_ptr()))
    return b.cpu().numpy()


def same_bits(a, b):
    """equal as fp64 values including the sign of zero; NaN equals NaN (payloads are not part of the reference's semantics)"""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a) & np.isnan(b)
    return nan | ((a == b) & (np.signbit(a) == np.signbit(b)))


def assert_bits(what, got, want, rows_mask):
    ok = same_bits(got, want)[rows_mask]
    print('%-58s %7d values  bit-identical to the C oracle: %s' % (what + ' [bits]', ok.size, bool(ok.all())))
    assert ok.all(), '%s: %d of %d values differ from the C oracle in their bits' % (what, int((~ok).sum()), ok.size)


def slot_deg(flat):
    deg = np.diff(flat.var_ptr)
    return deg[np.repeat(np.arange(flat.V), deg)]


def edge_deg(flat):
    out = np.zeros(flat.E, dtype=np.int64)
    out[flat.var_edge] = slot_deg(flat)
    return out


PAIR_MODELS = ['rows', 'lifted_counts', 'closed_forms', 'alias', 'layout256']


@pytest.mark.parametrize('name', PAIR_MODELS)
def test_pair_kernels_against_the_twin(api, name, monkeypatch):
    """lhvi_gabp_v2f and lhvi_gabp_marginals on hand-built f -> v messages of every class, lhvi_gabp_f2v on the twin's v -> f
    messages: within the bound, same NaN / infinity pattern, observed rows (NaN, NaN) -- hub rows too --, f -> v entries of
    observed targets and alias edges untouched; rows of at most 512 entries carry the C oracle's bits"""
    from oracle import oracle
    st = state(api, name, monkeypatch)
    flat = st.flat
    f2v = gm.messages(flat, np.random.default_rng(1))
    cov = covered(flat)
    got = dev_v2f(api, st.dg.g, flat, f2v)
    tw = gm.v2f(flat, f2v)
    gm.compare(name + ' lhvi_gabp_v2f', got, tw, cov)
    assert (got[~cov] == SENTINEL).all()                            # alias edges: the canonical edge owns the message
    obs = ~np.isnan(flat.var_value)[flat.edge_var] & cov
    assert np.isnan(got[obs]).all()
    if name in ('rows', 'lifted_counts', 'layout256'):
        assert (obs & (edge_deg(flat) > gm.HUB)).any()              # an observed hub row
        hub = cov & (edge_deg(flat) > gm.HUB) & ~obs
        gm.compare(name + ' lhvi_gabp_v2f, hub rows alone', got, tw, hub)
    ov2f, of2v = oracle.gabp_half_sweeps(flat, f2v, np.full((flat.E, 2), SENTINEL))
    assert_bits(name + ' lhvi_gabp_v2f', got, ov2f, cov & (edge_deg(flat) <= gm.HUB))
    # f -> v from the twin's (rounded) v -> f messages
    v_in = tw.array()
    v_in[~cov] = SENTINEL
    before = np.full((flat.E, 2), SENTINEL)
    got_f = dev_f2v(api, st, v_in, before)
    gm.compare_f2v(name + ' lhvi_gabp_f2v', got_f, gm.f2v(flat, v_in, before))
    of = gm.oracle_f2v(flat, v_in, before)
    assert_bits(name + ' lhvi_gabp_f2v', got_f, of, np.ones(flat.E, dtype=bool))
    # marginals
    got_m = dev_marginals(api, st.dg.g, flat, f2v)
    has_row = np.diff(flat.var_ptr) > 0
    gm.compare(name + ' lhvi_gabp_marginals', got_m, gm.marginals(flat, f2v), has_row)
    assert_bits(name + ' lhvi_gabp_marginals', got_m, oracle_marginals(flat, f2v), has_row & (np.diff(flat.var_ptr) <= gm.HUB))


def test_closed_forms_on_every_class_of_partner_message(api, monkeypatch):
    """lhvi_gabp_f2v on hand-built v -> f messages: proper, `None`, infinite, negative variance, zero mean, per closed form"""
    from oracle import oracle
    st = state(api, 'closed_forms', monkeypatch)
    flat, v_in = gm.closed_forms()
    before = np.full((flat.E, 2), SENTINEL)
    got = dev_f2v(api, st, v_in, before)
    gm.compare_f2v('closed forms, every partner class: lhvi_gabp_f2v', got, gm.f2v(flat, v_in, before))
    of = gm.oracle_f2v(flat, v_in, before)
    assert_bits('closed forms, every partner class: lhvi_gabp_f2v', got, of, np.ones(flat.E, dtype=bool))


PULL_MODELS = ['rows', 'layout64', 'layout256', 'lifted_counts', 'closed_forms', 'alias', 'pots32', 'pots33']


@pytest.mark.parametrize('name', PULL_MODELS)
def test_every_pull_path_against_the_twin(api, name, monkeypatch):
    """lhvi_gabp_pull(first = 0) from hand-built v -> f messages in slot order, and first = 1, on the graph arrays, on the slot
    records with the potentials in LDS and with the potentials in global memory: every slot within the bound of the twin's
    composite, no slot left unwritten; the C oracle's bits where the kernel keeps the reference's order of summation"""
    st = state(api, name, monkeypatch)
    flat = st.flat
    if name == 'pots32':
        assert st.dg.p.P == 32
    if name == 'pots33':
        assert st.dg.p.P == 33                                       # 'records' reads the table from global memory by itself
    vprev = gm.slot_messages(flat, np.random.default_rng(2))
    deg = slot_deg(flat)
    want = {0: gm.pull(flat, vprev, 0), 1: gm.pull(flat, None, 1)}
    f2v1 = np.zeros((flat.E, 2))
    f2v1[:, 1] = 1.0
    from oracle import oracle
    ora = {0: oracle_pull(flat, vprev), 1: oracle.gabp_half_sweeps(flat, f2v1, f2v1)[0][flat.var_edge]}
    seg = st.host['seg'].astype(np.int64)
    longest = seg[np.argmax(seg[:, 1] - seg[:, 0])] if seg.size else None
    for path in PATHS:
        for first in (0, 1):
            got = dev_pull(api, st, path, vprev, first)
            what = '%s lhvi_gabp_pull %s first=%d' % (name, path, first)
            gm.compare(what, got, want[first])
            if flat.lifted or path == 'arrays':
                exact = deg <= gm.HUB
            else:
                exact = deg <= gm.ROW_DIRECT
            assert_bits(what, got, ora[first], exact)
            if name.startswith('layout'):
                # the longest segment the plan can make (767 slots at a window of 256) and the 512-row across two block ends,
                # slot by slot
                window = 256 if name == 'layout256' else 64
                assert longest[1] - longest[0] == window - 1 + 512
                in_seg = np.zeros(deg.size, dtype=bool)
                in_seg[longest[0]:longest[1]] = True
                gm.compare(what + ', longest segment', got, want[first], in_seg)
                hidden = np.isnan(flat.var_value)[np.repeat(np.arange(flat.V), np.diff(flat.var_ptr))]
                gm.compare(what + ', the 512-row', got, want[first], (deg == 512) & hidden)


def test_a_segment_of_exactly_the_lds_stage(api, monkeypatch):
    """the record kernel serves any row-aligned segment of up to 768 slots (lhvi_gabp_plan_t.seg): a hand-built plan whose
    segments are single rows, except one of exactly 768 slots = rows of 128, 512 and 128 entries"""
    st = state(api, 'layout256', monkeypatch)
    flat = st.flat
    deg = np.diff(flat.var_ptr)
    rows = np.flatnonzero((deg > 0) & (deg <= gm.HUB))
    seg = np.stack([flat.var_ptr[rows], flat.var_ptr[rows + 1]], axis=1).astype(np.int64)
    merged = (seg[:, 0] >= 127) & (seg[:, 1] <= 895)
    assert merged.sum() == 3
    seg = np.concatenate([seg[seg[:, 1] <= 127], [[127, 895]], seg[seg[:, 0] >= 895]])
    assert (seg[:, 1] - seg[:, 0]).max() == 768
    vprev = gm.slot_messages(flat, np.random.default_rng(2))
    want = gm.pull(flat, vprev, 0)
    for path in PATHS[1:]:
        got = dev_pull(api, st, path, vprev, 0, seg=seg)
        gm.compare('hand-built 768-slot segment, %s' % path, got, want)


def test_dominant_entry_hub_and_chunk_paths_stay_within_the_bound(api, monkeypatch):
    """a row whose one entry carries 1e9 times the precision of all the others: the slot of that entry is the cancellation case
    of total-minus-own (hub kernels) and of total-minus-own-chunk (record kernel, rows of 33-512 entries); the bound there is
    (n + 4) u sum |p| / |P| ~ 1e-5 relative.  Prints the measured error next to the direct sum's."""
    flat, f2v, vprev, slots = gm.dominant()
    st = state(api, 'dominant', monkeypatch)
    cov = covered(flat)
    tw = gm.v2f(flat, f2v)
    got = dev_v2f(api, st.dg.g, flat, f2v)
    gm.compare('dominant lhvi_gabp_v2f (577: hub kernel, 66: direct)', got, tw, cov)
    # the same kernel without the hub list: direct leave-one-out sums for every row
    g_direct = type(st.dg.g).from_buffer_copy(st.dg.g)
    g_direct.hub_vars, g_direct.n_hubs = None, 0
    direct = dev_v2f(api, g_direct, flat, f2v)
    gm.compare('dominant lhvi_gabp_v2f, direct sums', direct, tw, cov)
    e = flat.var_edge[slots]
    rel = lambda a, i: float(abs((a[i, 1].astype(gm.LD) - tw.var[i]) / tw.var[i]))
    print('dominant slot of the 577-row, relative error of the variance: hub kernel %.3e, direct sum %.3e, bound %.3e'
          % (rel(got, e[0]), rel(direct, e[0]), gm.bound(tw)[1][e[0]] / abs(float(tw.var[e[0]]))))
    got_m = dev_marginals(api, st.dg.g, flat, f2v)
    gm.compare('dominant lhvi_gabp_marginals', got_m, gm.marginals(flat, f2v))
    want = gm.pull(flat, vprev, 0)
    bvar = gm.bound(want)[1]
    ora = oracle_pull(flat, vprev)
    for path in PATHS:
        out = dev_pull(api, st, path, vprev, 0)
        gm.compare('dominant lhvi_gabp_pull %s' % path, out, want)
        for row, k in zip((577, 66), slots):
            r = lambda a: float(abs((a[k, 1].astype(gm.LD) - want.var[k]) / want.var[k]))
            print('dominant slot of the %d-row, %s: relative error of the variance %.3e, direct sum (C oracle) %.3e, bound %.3e'
                  % (row, path, r(out), r(ora), bvar[k] / abs(float(want.var[k]))))


def _run(api, st, how, iterations):
    """(f2v, v2f, marginals, v2f in slot order) after `iterations` sweeps through lhvi_gabp_run ('pair') or lhvi_gabp_run_pull (a
    pull path)"""
    import torch
    flat = st.flat
    l, s = api.lib(), api.stream_ptr()
    dg = st.dg
    f2v, v2f, mv = dg.empty(flat.E, 2), dg.empty(flat.E, 2), dg.empty(flat.V, 2)
    if how == 'pair':
        api.check(l.lhvi_gabp_run(dg.g, dg.p, api.ptr(f2v), api.ptr(v2f), iterations, s))
    else:
        dg, p, keep = plan_of(api, st, how)
        nbytes = int(l.lhvi_gabp_pull_workspace_bytes(dg.g))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dg.device)
        api.check(l.lhvi_gabp_run_pull(dg.g, dg.p, p, api.ptr(f2v), api.ptr(v2f), iterations, api.ptr(ws), nbytes, s))
    api.check(l.lhvi_gabp_marginals(dg.g, api.ptr(f2v), api.ptr(mv), s))
    return f2v.cpu().numpy(), v2f.cpu().numpy(), mv.cpu().numpy()


def _check_run(what, flat, runs, k, pull_form):
    """sweep k of a run against the twin applied to the DEVICE's messages of the step before, so that ``bound`` applies per sweep:
    v2f_k = V(f2v_k), f2v_k = F(v2f_{k-1}), marginals = M(f2v_k), and in the pull form v2f_k = pull(v2f_{k-1}) as one step"""
    f2v, v2f, mv = runs[k]
    cov = covered(flat)
    gm.compare('%s, %d sweeps: v2f' % (what, k), v2f, gm.v2f(flat, f2v), cov)
    gm.compare('%s, %d sweeps: marginals' % (what, k), mv, gm.marginals(flat, f2v), np.diff(flat.var_ptr) > 0)
    init = np.zeros((flat.E, 2))
    init[:, 1] = 1.0
    if k == 1:
        assert np.array_equal(f2v, init)
    else:
        v_before = runs[k - 1][1]
        # (edges of observed variables keep their initial f -> v message for the whole run)
        gm.compare_f2v('%s, %d sweeps: f2v' % (what, k), f2v, gm.f2v(flat, v_before, init))
        if pull_form:
            gm.compare('%s, %d sweeps: one pull step' % (what, k), v2f[flat.var_edge], gm.pull(flat, v_before[flat.var_edge], 0))


@pytest.mark.parametrize('name', ['rows', 'alias'])
def test_whole_runs_sweep_by_sweep(api, name, monkeypatch):
    """1, 2 and 7 sweeps through lhvi_gabp_run, lhvi_gabp_run_pull (three plans) and GaBP.run (the recorded graph); every sweep is
    held to the twin applied to the device's own messages of the sweep before (runs of 6 sweeps supply those of the 7th).  On the
    alias-edge graph the lifted marginals are also held to the GROUND twin's marginals from the same messages."""
    from lhvi.gabp import GaBP
    st = state(api, name, monkeypatch)
    flat = st.flat
    for how in ('pair',) + PATHS:
        runs = {k: _run(api, st, how, k) for k in (1, 2, 6, 7)}
        for k in (1, 2, 7):
            _check_run('%s %s' % (name, how), flat, runs, k, how != 'pair')
    runs = {}
    for k in (1, 2, 6, 7):
        bp = GaBP(flat)
        bp.run(k)
        assert len(bp._state['graphs']) == 1                        # (the recorded graph)
        runs[k] = (bp._f2v.copy(), bp._v2f.copy(), bp._mu_var.copy())
    for k in (1, 2, 7):
        _check_run('%s GaBP.run' % name, flat, runs, k, True)
    if name == 'alias':
        ground, lifted, rvc, fc = gm.alias_chain()
        # every ground edge reads the message of the lifted edge of its (factor cluster, variable cluster)
        from lhvi import lifting
        rvc2, fc2 = lifting.refine_flat(ground, np.array([1 if ground.fac_ptr[f + 1] - ground.fac_ptr[f] == 2 else 0 for f in range(ground.F)],
                                                        dtype=np.uint8),
                                       np.where(np.isnan(ground.var_value), 0, 1).astype(np.int32), ground.fac_pot.astype(np.int32))
        from oracle import oracle
        assert oracle.canonical_labels(rvc2) == oracle.canonical_labels(rvc)      # the device's colours = the oracle's
        lifted2 = lifting.lift_flat(ground, rvc2, fc2)
        assert (lifted2.edge_canon != np.arange(lifted2.E)).any()
        for k in (1, 2, 7):
            f2v_l, _, mv_l = runs[k]
            f2v_g = np.zeros((ground.E, 2))
            for e in range(ground.E):
                lf, lv = fc[ground.edge_fac[e]], rvc[ground.edge_var[e]]
                cand = np.flatnonzero((lifted.edge_fac == lf) & (lifted.edge_var == lv))
                f2v_g[e] = f2v_l[lifted.edge_canon[cand[0]]]
            gm.compare('alias, %d sweeps: lifted marginals against the ground twin' % k, mv_l[rvc], gm.marginals(ground, f2v_g),
                       np.diff(ground.var_ptr) > 0)
