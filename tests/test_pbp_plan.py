"""CPU suite: the particle sweep's work lists as pure host functions (``lhvi/pbp_plan.py``), checked against the record layouts
and class definitions of ``include/lhvi.h`` (``lhvi_pbp_t``, ``lhvi_pbp_var_fused``), not against recorded output."""
import functools

import numpy as np
import pytest
import torch

from lhvi import _abi, pbp_plan, synth
from lhvi.pbp_plan import PlanOptions, V2F_CLASSES, var_side_plan

OPTS = PlanOptions(sampler_on_device=True, listed_proposal=True, listed_resample=True, sliced_proposal=True, prop_slice=64,
                   packed_v2f=True, v2f_records=True, fused=True, fused_max_particles=64, fused_records16=True)
NS = (3, 10, 16, 17, 32, 33, 64, 65)


@functools.lru_cache(maxsize=None)
def graph(name):
    if name == 'hmln':          # two hidden continuous variables with more than 64 factors (largest row 156)
        return synth.paper_popularity_flat(150, 4, seed=2)[0]
    return synth.hybrid_mrf_flat(V=300, deg=12 if name == 'deg12' else 4, seed=37, frac_discrete=0.3, T=48 if name == 'T48' else 32)


GRAPHS = ('mrf', 'T48', 'deg12', 'hmln')


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    def refuse():
        raise AssertionError('the plan asked for a device')
    monkeypatch.setattr(_abi, 'require_gpu', refuse)


def row(flat, v):
    return flat.var_edge[flat.var_ptr[v]:flat.var_ptr[v + 1]]


def doubles(words):
    return np.ascontiguousarray(words, dtype=np.int32).view(np.float64).reshape(-1)


def members(lst, count, records):
    """the variables of one v -> f list: `count` entries (records: word 0); what lies beyond the count is one zero row"""
    a = lst
    assert a.dtype == np.int32 and a.shape[0] == max(count, 1)
    if count == 0:
        assert not a.any() and a.shape == ((1, 8) if records else (1,))
        return a[:0].reshape(-1)
    return a[:, 0] if records else a


def check_split(flat, n, lists, want, records):
    """`lists` holds every variable of `want` once, by the class definitions of include/lhvi.h"""
    deg, npv = np.diff(flat.var_ptr), np.where(flat.var_hidden, np.where(flat.var_cont, n, flat.var_nstates), 0)
    got = {name: members(getattr(lists, name), getattr(lists, 'n_' + name), records and name == 'wide') for name in V2F_CLASSES}
    every = np.concatenate(list(got.values()))
    assert every.size == np.unique(every).size                                      # disjoint
    np.testing.assert_array_equal(np.sort(every), want)                             # ... and together all of them
    for name, vs in got.items():
        assert (np.diff(vs) > 0).all()                                              # ascending
        is_hub = (deg[vs] > 64) & (npv[vs] <= 64)
        if name == 'narrow':
            assert (npv[vs] <= 4).all()
        elif name == 'hub':
            assert (npv[vs] > 4).all() and is_hub.all()
        elif name == 'mid16':
            assert ((npv[vs] > 4) & (npv[vs] <= 16)).all() and not is_hub.any()
        elif name == 'mid32':
            assert ((npv[vs] > 16) & (npv[vs] <= 32)).all() and not is_hub.any()
        else:
            assert (npv[vs] > 32).all() and not is_hub.any()
    return got


@pytest.mark.parametrize('owned', [None, 200])
@pytest.mark.parametrize('name', GRAPHS)
def test_v2f_lists_partition_the_hidden_variables_by_class(name, owned):
    flat = graph(name)
    hidden = np.flatnonzero(flat.var_hidden)
    hidden = hidden if owned is None else hidden[hidden < owned]
    for n in NS:
        for records in (True, False):
            plan = var_side_plan(flat, n, owned=owned, opts=OPTS._replace(v2f_records=records))
            assert plan.v2f is not None                                             # (every graph here has binary variables)
            assert plan.flags & _abi.PBP_V2F_RECORDS == (_abi.PBP_V2F_RECORDS if records else 0)
            got = check_split(flat, n, plan.v2f, hidden, records)
            for cls in V2F_CLASSES:
                assert plan.host['v2f_' + cls] is getattr(plan.v2f, cls)
            if name == 'hmln' and owned is None and 4 < n <= 64:
                assert got['hub'].size >= 2
            np.testing.assert_array_equal(plan.np_host, np.where(flat.var_hidden, np.where(flat.var_cont, n, flat.var_nstates), 0))
            assert plan.host['np_dev'] is plan.np_host and plan.np_host.dtype == np.int32
    assert var_side_plan(flat, 16, owned=owned, opts=OPTS._replace(packed_v2f=False)).v2f is None


def test_no_v2f_lists_when_every_variable_is_wide():
    flat = synth.hybrid_mrf_flat(V=120, deg=4, seed=5, frac_discrete=0.0, T=32)
    plan = var_side_plan(flat, 64, owned=None, opts=OPTS)
    assert plan.v2f is None and plan.fused is None and plan.flags == 0 and not any(k.startswith('v2f_') for k in plan.host)


@pytest.mark.parametrize('name', GRAPHS)
def test_sampled_records_name_what_the_graph_holds(name):
    flat = graph(name)
    sizes, deg = np.diff(flat.dom_ptr), np.diff(flat.var_ptr)
    pv = np.flatnonzero(flat.var_hidden & flat.var_cont)
    for n in (10, 64):
        plan = var_side_plan(flat, n, owned=None, opts=OPTS)
        assert plan.T == int(sizes[flat.dom_cont.astype(bool)].max())
        pd = plan.host['prop_desc']
        assert pd.dtype == np.int32 and pd.shape == (plan.n_prop_desc, 8)
        whole = pd[pd[:, 1] >= 0]                                                   # (slices: their own test)
        np.testing.assert_array_equal(whole[:, 0], pv[deg[pv] <= 64])
        wide = plan.v2f.wide
        rr = plan.host['resample_vars']
        np.testing.assert_array_equal(rr[:, 0], pv)
        assert rr.dtype == np.int32 and (rr[:, 1] == n).all() and not rr[:, 6:].any()
        np.testing.assert_array_equal(doubles(rr[:, 2:4]), flat.dom_lo[flat.var_dom[pv]])
        np.testing.assert_array_equal(doubles(rr[:, 4:6]), flat.dom_hi[flat.var_dom[pv]])
        np.testing.assert_array_equal(plan.host['_static_idx'], np.flatnonzero(~(flat.var_hidden & flat.var_cont)))
        assert plan.host['_static_idx'].dtype == np.int64
        for rec in list(whole[::7]) + list(whole[-2:]):
            v, d = int(rec[0]), flat.var_dom[rec[0]]
            r = row(flat, v)
            assert rec[1] == r.size and rec[2] == flat.dom_ptr[d] and rec[3] == sizes[d]
            assert rec[4:].tolist() == [int(r[min(k, r.size - 1)]) for k in range(4)]
        if n == 64:
            assert plan.v2f.n_wide > 0 and wide.shape == (plan.v2f.n_wide, 8)
            for rec in list(wide[::7]) + list(wide[-2:]):
                r = row(flat, int(rec[0]))
                assert rec[1] == r.size and rec[2] == plan.np_host[rec[0]] and rec[3] == flat.var_dom[rec[0]]
                assert rec[4:].tolist() == [int(r[min(k, r.size - 1)]) for k in range(4)]
        F = plan.fused
        fd = F.desc64 if n > 32 else F.desc[:sum(F.counts)]
        assert fd.shape[1] == 16 and fd.shape[0] > 0 and plan.flags & _abi.PBP_FUSED_RECORDS16
        for rec in list(fd[::7]) + list(fd[-2:]):
            v, d = int(rec[0]), flat.var_dom[rec[0]]
            r = row(flat, v)
            assert rec[1] == r.size and rec[2] == flat.dom_ptr[d] and rec[3] == sizes[d]
            assert doubles(rec[4:8]).tolist() == [flat.dom_lo[d], flat.dom_hi[d]]
            assert rec[8] == n and rec[9] == flat.var_ptr[v]
            assert rec[10:].tolist() == [int(r[k]) if k < r.size else 0 for k in range(6)]


def test_v2f_records_name_the_row_the_graph_holds():
    """``lhvi_pbp_t.v2f_wide`` as records (LHVI_PBP_V2F_RECORDS): variable, degree, particle count, domain and the first four
    incident edges in row order -- what ``pbp_v2f_kernel`` would otherwise read through var_ptr / var_edge (host side only)"""
    flat = synth.hybrid_mrf_flat(V=700, deg=4, seed=3)
    np_host = np.where(flat.var_cont, 64, 2).astype(np.int64)
    vs = np.flatnonzero(flat.var_hidden & flat.var_cont)
    rec = pbp_plan.v2f_records(flat, np_host, vs)
    assert rec.shape == (vs.size, 8) and rec.dtype == np.int32
    deg = np.diff(flat.var_ptr)[vs]
    np.testing.assert_array_equal(rec[:, 0], vs)
    np.testing.assert_array_equal(rec[:, 1], deg)
    np.testing.assert_array_equal(rec[:, 2], 64)
    np.testing.assert_array_equal(rec[:, 3], flat.var_dom[vs])
    for i in range(0, vs.size, 37):
        row = flat.var_edge[flat.var_ptr[vs[i]]:flat.var_ptr[vs[i] + 1]]
        want = [row[min(k, row.size - 1)] for k in range(4)] if row.size else [0] * 4
        assert rec[i, 4:].tolist() == [int(x) for x in want]
    assert pbp_plan.v2f_records(flat, np_host, vs[:0]).shape == (1, 8)          # an empty list keeps a non-null pointer


def test_first_edges_pads_by_the_last_edge_or_by_zero():
    flat = graph('mrf')
    vs = np.flatnonzero(np.diff(flat.var_ptr) > 0)
    short = vs[np.diff(flat.var_ptr)[vs] < 6]
    assert short.size                                                               # rows that end before the sixth entry
    for clamp in (True, False):
        got = pbp_plan.first_edges(flat, vs, 6, clamp)
        assert got.dtype == np.int32 and got.shape == (vs.size, 6)
        for i in list(range(0, vs.size, 11)) + [int(np.flatnonzero(vs == short[0])[0])]:
            r = row(flat, vs[i])
            assert got[i].tolist() == [int(r[k]) if k < r.size else (int(r[-1]) if clamp else 0) for k in range(6)]
    assert pbp_plan.first_edges(flat, vs[:0], 4, True).shape == (0, 4)


@pytest.mark.parametrize('name', GRAPHS)
def test_fused_class_and_rest_cover_every_continuous_variable_once(name):
    flat = graph(name)
    sizes, deg = np.diff(flat.dom_ptr), np.diff(flat.var_ptr)
    pv = np.flatnonzero(flat.var_hidden & flat.var_cont)
    hidden = np.flatnonzero(flat.var_hidden)
    pT = sizes[flat.var_dom]
    for n in NS:
        for opts in (OPTS, OPTS._replace(fused_records16=False), OPTS._replace(prop_slice=8)):
            plan = var_side_plan(flat, n, owned=None, opts=opts)
            F = plan.fused
            qualify = pv[(deg[pv] <= min(64, opts.prop_slice)) & (pT[pv] <= 64)]
            if n > 64 or qualify.size == 0:
                assert F is None and not any(k.startswith(('fused', 'prop_desc_rest', 'resample_rest', 'v2f_rest')) for k in plan.host)
                continue
            width = 16 if opts.fused_records16 else 8
            assert bool(plan.flags & _abi.PBP_FUSED_RECORDS16) == opts.fused_records16
            assert F.desc.dtype == np.int32 and F.desc.shape == (max(sum(F.counts), 1), width) and (sum(F.counts) or not F.desc.any())
            assert (F.desc64 is None) == (sum(F.counts64) == 0) and (F.desc64 is None or F.desc64.shape == (sum(F.counts64), 16))
            assert (sum(F.counts) > 0) == (n <= 32) and (sum(F.counts64) > 0) == (n > 32)
            small = F.desc[:sum(F.counts), 0]
            fused = np.concatenate([small, F.desc64[:, 0]]) if F.desc64 is not None else small
            assert fused.size == np.unique(fused).size
            np.testing.assert_array_equal(np.sort(fused), qualify)
            # nothing with a sliced row or more than 64 integral points is fused
            assert (deg[fused] <= min(64, opts.prop_slice)).all() and (pT[fused] <= 64).all()
            # the sub-classes, contiguous in this order with the reported counts (include/lhvi.h, lhvi_pbp_var_fused / _fused64)
            c16, c32a, c32b = F.counts
            v16, v32a, v32b = small[:c16], small[c16:c16 + c32a], small[c16 + c32a:]
            assert (c16 == 0 or n <= 16) and (pT[v16] <= 32).all()
            assert (c32a == 0 or 16 < n <= 32) and (pT[v32a] <= 32).all() and (pT[v32b] > 32).all()
            if F.desc64 is not None:
                c64a, c64b = F.counts64
                assert (pT[F.desc64[:c64a, 0]] <= 32).all() and (pT[F.desc64[c64a:, 0]] > 32).all()
            for block in (v16, v32a, v32b) + ((F.desc64[:F.counts64[0], 0], F.desc64[F.counts64[0]:, 0]) if F.desc64 is not None else ()):
                assert (np.diff(block) > 0).all()
            # each consumer's rest list holds exactly the others
            rest = np.setdiff1d(pv, fused)
            rest_v2f = check_split(flat, n, F.v2f_rest, np.setdiff1d(hidden, fused), opts.v2f_records)
            assert sum(v.size for v in rest_v2f.values()) == hidden.size - fused.size
            pr = F.prop_desc_rest
            assert pr.shape == (max(F.n_prop_rest, 1), 8) and (F.n_prop_rest or not pr.any())
            np.testing.assert_array_equal(np.unique(pr[:F.n_prop_rest, 0]), rest)
            np.testing.assert_array_equal(pr[:F.n_prop_rest], plan.host['prop_desc'][~np.isin(plan.host['prop_desc'][:, 0], fused)])
            rs = F.resample_rest
            assert rs.shape == (max(F.n_resample_rest, 1), 8) and (F.n_resample_rest or not rs.any())
            np.testing.assert_array_equal(rs[:F.n_resample_rest, 0], rest)
            np.testing.assert_array_equal(rs[:F.n_resample_rest], plan.host['resample_vars'][~np.isin(pv, fused)])
            assert plan.host['fused_desc'] is F.desc and plan.host.get('fused64_desc') is F.desc64
            assert plan.host['prop_desc_rest'] is pr and plan.host['resample_rest'] is rs


@pytest.mark.parametrize('change', [dict(fused=False), dict(sampler_on_device=False), dict(listed_proposal=False), dict(listed_resample=False),
                                    dict(packed_v2f=False), dict(fused_max_particles=16), dict(owned=200)])
def test_no_fused_class_without_its_conditions(change):
    owned = change.pop('owned', None)
    plan = var_side_plan(graph('mrf'), 32, owned=owned, opts=OPTS._replace(**change))
    assert plan.fused is None and not plan.flags & _abi.PBP_FUSED_RECORDS16 and 'fused_desc' not in plan.host


@pytest.mark.parametrize('prop_slice', [64, 50])
def test_hub_slices_tile_their_rows(prop_slice):
    flat = graph('hmln')
    deg = np.diff(flat.var_ptr)
    pv = np.flatnonzero(flat.var_hidden & flat.var_cont)
    hubs = pv[deg[pv] > prop_slice]
    assert hubs.size >= 2 and deg[hubs].max() == 156
    plan = var_side_plan(flat, 16, owned=None, opts=OPTS._replace(prop_slice=prop_slice))
    pd, ph = plan.host['prop_desc'], plan.host['prop_hub']
    nslices = int(plan.n_prop_partial)
    assert plan.n_prop_hub == hubs.size and ph.shape == (hubs.size, 4) and ph.dtype == np.int32 and not ph[:, 3].any()
    assert (pd[:nslices, 1] < 0).all() and (pd[nslices:, 1] >= 0).all()            # slices precede the ordinary records
    assert not np.isin(pd[nslices:, 0], hubs).any() and plan.n_prop_desc == nslices + pv.size - hubs.size
    np.testing.assert_array_equal(pd[:nslices, 5], np.arange(nslices))              # slot in prop_partial
    np.testing.assert_array_equal(ph[:, 0], hubs)
    sizes = np.diff(flat.dom_ptr)
    for v, first, count, _ in ph:
        sl = pd[first:first + count]
        assert (sl[:, 0] == v).all() and count == -(-deg[v] // prop_slice)
        assert (-sl[:, 1]).sum() == deg[v] and ((-sl[:, 1])[:-1] == prop_slice).all() and 0 < -sl[-1, 1] <= prop_slice
        np.testing.assert_array_equal(sl[:, 4], np.arange(count) * prop_slice)
        assert (sl[:, 2] == flat.dom_ptr[flat.var_dom[v]]).all() and (sl[:, 3] == sizes[flat.var_dom[v]]).all() and not sl[:, 6:].any()
    assert ph[:, 2].sum() == nslices and ph[0, 1] == 0 and (ph[1:, 1] == np.cumsum(ph[:, 2])[:-1]).all()
    off = var_side_plan(flat, 16, owned=None, opts=OPTS._replace(sliced_proposal=False))
    assert off.n_prop_hub == 0 and off.n_prop_partial == 0 and 'prop_hub' not in off.host and off.n_prop_desc == pv.size


def test_fused_max_particles_bounds_the_fused_class():
    for n, want in ((16, True), (17, False)):
        assert (var_side_plan(graph('mrf'), n, owned=None, opts=OPTS._replace(fused_max_particles=16)).fused is not None) == want


def test_empty_lists_are_one_zero_row():
    flat = graph('mrf')
    plan = var_side_plan(flat, 16, owned=None, opts=OPTS)                           # everything continuous is fused, nothing is a hub
    L, F = plan.v2f, plan.fused
    assert L.n_wide == 0 and L.wide.shape == (1, 8) and not L.wide.any()
    assert L.n_hub == 0 and L.hub.shape == (1,) and not L.hub.any() and L.n_mid32 == 0 and L.mid32.shape == (1,)
    assert F.n_prop_rest == 0 and F.prop_desc_rest.shape == (1, 8) and not F.prop_desc_rest.any()
    assert F.n_resample_rest == 0 and F.resample_rest.shape == (1, 8) and not F.resample_rest.any()
    assert F.v2f_rest.n_mid16 == 0 and F.v2f_rest.mid16.shape == (1,) and F.v2f_rest.n_narrow == L.n_narrow > 0
    assert F['counts'] is F.counts and F['n_prop_rest'] == 0 and F[0] is F.counts   # fields read by name in either spelling
    plan = var_side_plan(flat, 64, owned=None, opts=OPTS)                           # 64 particles: no record in the small fused list
    assert plan.fused.counts == (0, 0, 0) and plan.fused.desc.shape == (1, 16) and not plan.fused.desc.any()
    assert var_side_plan(flat, 16, owned=None, opts=OPTS._replace(v2f_records=False)).v2f.wide.shape == (1,)


def test_plan_is_a_function_of_its_arguments(monkeypatch):
    flat = graph('hmln')
    a = var_side_plan(flat, 16, owned=None, opts=OPTS)
    for k, v in (('LHVI_PBP_V2F_REC', '0'), ('LHVI_PBP_FUSED', '0'), ('LHVI_PBP_FUSED_MAX', '8'), ('LHVI_PBP_FUSED_REC16', '0')):
        monkeypatch.setenv(k, v)
    b = var_side_plan(flat, 16, owned=None, opts=OPTS)
    assert a.flags == b.flags and a.host.keys() == b.host.keys()
    for k in a.host:
        assert (a.host[k] is None and b.host[k] is None) or (a.host[k].dtype == b.host[k].dtype and a.host[k].tobytes() == b.host[k].tobytes())


def test_plan_options_come_from_attributes_and_environment_once(monkeypatch):
    from lhvi.pbp import EPBP
    for k in ('LHVI_PBP_V2F_REC', 'LHVI_PBP_FUSED', 'LHVI_PBP_FUSED_MAX', 'LHVI_PBP_FUSED_REC16'):
        monkeypatch.delenv(k, raising=False)
    bp = EPBP(None, n=16, sampler='device')
    assert bp._plan_options() == OPTS
    assert EPBP(None, n=16)._plan_options() == OPTS._replace(sampler_on_device=False)
    bp.packed_v2f, bp.prop_slice, bp.fused_max_particles = False, 32, 20
    assert bp._plan_options() == OPTS._replace(packed_v2f=False, prop_slice=32, fused_max_particles=20)
    monkeypatch.setenv('LHVI_PBP_FUSED_MAX', '8')
    monkeypatch.setenv('LHVI_PBP_V2F_REC', '0')
    monkeypatch.setenv('LHVI_PBP_FUSED', '0')
    monkeypatch.setenv('LHVI_PBP_FUSED_REC16', '0')
    assert bp._plan_options() == OPTS._replace(packed_v2f=False, prop_slice=32, fused_max_particles=8, v2f_records=False, fused=False,
                                               fused_records16=False)


def test_plan_refuses_what_the_sweep_cannot_run():
    import copy
    flat = graph('mrf')
    with pytest.raises(_abi.LhviError, match='a discrete variable has more states than particle slots n=1'):
        var_side_plan(flat, 1, owned=None, opts=OPTS)
    bare = copy.copy(flat)
    v = int(np.flatnonzero(flat.var_hidden & flat.var_cont)[-1])
    bare.var_ptr = flat.var_ptr.copy()
    bare.var_ptr[v + 1:] -= flat.var_ptr[v + 1] - flat.var_ptr[v]                   # its row is empty now
    with pytest.raises(ZeroDivisionError, match='a hidden continuous variable has no incident factor: its proposal is an empty product'):
        var_side_plan(bare, 16, owned=None, opts=OPTS)


def test_v2f_lists_install_by_name_and_null_in_their_empty_form():
    lists = pbp_plan.V2fLists(**{k: torch.arange(4, dtype=torch.int32) + i for i, k in enumerate(V2F_CLASSES)},
                              **{'n_' + k: i + 1 for i, k in enumerate(V2F_CLASSES)})
    s = _abi.PbpStruct()
    lists.install(s)
    for i, k in enumerate(V2F_CLASSES):
        assert getattr(s, 'v2f_' + k) == getattr(lists, k).data_ptr() and getattr(s, 'n_v2f_' + k) == i + 1
    pbp_plan.V2fLists().install(s)
    for k in V2F_CLASSES:
        assert getattr(s, 'v2f_' + k) is None and getattr(s, 'n_v2f_' + k) == 0


# ---- the variable side's lists as one record -----------------------------------------------------------------------------------
def var_lists(name, n, owned=None):
    """the plan of graph `name` and its lists the way a sweep holds them, on CPU tensors in the place of the uploaded ones"""
    plan = var_side_plan(graph(name), n, owned=owned, opts=OPTS)
    dev = {k: None if a is None else torch.from_numpy(np.ascontiguousarray(a)) for k, a in plan.host.items()}
    partial = torch.zeros(plan.n_prop_partial, 2, dtype=torch.float64) if plan.n_prop_partial else None
    return plan, plan.on(dev, partial)


def list_fields(s):
    """every per-variable list of ``lhvi_pbp_t`` with its count, as the struct holds them"""
    out = {'v2f_' + k: (getattr(s, 'v2f_' + k), getattr(s, 'n_v2f_' + k)) for k in V2F_CLASSES}
    out.update(prop_desc=(s.prop_desc, s.n_prop_desc), prop_hub=(s.prop_hub, s.n_prop_hub), prop_partial=(s.prop_partial, 0),
               resample_vars=(s.resample_vars, s.n_resample_vars))
    return out


def listed(lists, prefix=''):
    return {prefix + k: (getattr(lists, k).data_ptr(), getattr(lists, 'n_' + k)) for k in V2F_CLASSES}


@pytest.mark.parametrize('name,owned', [('hmln', None), ('hmln', 200), ('mrf', None), ('mrf', 200)])
def test_var_lists_install_every_list(name, owned):
    flat = graph(name)
    plan, L = var_lists(name, 16, owned)
    pv = np.flatnonzero(flat.var_hidden & flat.var_cont)
    assert (L.fused is None) == (owned is not None) and L.v2f is not None and L.n_prop_desc == plan.n_prop_desc == L.prop_desc.shape[0]
    # the sampler's list keeps the ghosts; the rows no listed draw writes are all the others
    assert L.n_resample_vars == pv.size == L.resample_vars.shape[0] and L.static_idx.numel() == flat.V - pv.size
    hubs = int((np.diff(flat.var_ptr)[pv if owned is None else pv[pv < owned]] > 64).sum())
    assert L.n_prop_hub == hubs == (2 if name == 'hmln' else 0)                     # (hmln: two rows of more than 64 factors, owned both)
    s = _abi.PbpStruct()
    L.install(s)
    want = listed(L.v2f, 'v2f_')
    want.update(prop_desc=(L.prop_desc.data_ptr(), plan.n_prop_desc), resample_vars=(None, 0),      # (the sampler's list: install_sampler)
                prop_hub=(L.prop_hub.data_ptr(), hubs) if hubs else (None, 0), prop_partial=(L.prop_partial.data_ptr() if hubs else None, 0))
    assert list_fields(s) == want and s.np == L.np_dev.data_ptr() and s.var_lo == s.var_hi == 0
    if hubs:                                                                        # a scratch row of two doubles per slice
        assert tuple(L.prop_partial.shape) == (plan.n_prop_partial, 2) and L.prop_partial.dtype == torch.float64
        assert plan.n_prop_partial == int((L.prop_desc[:, 1] < 0).sum())
    L.install_sampler(s)
    assert (s.resample_vars, s.n_resample_vars) == (L.resample_vars.data_ptr(), pv.size)
    # without its records the proposal kernel walks the graph arrays: no record list, no hub rows; the other kernels keep theirs
    s = _abi.PbpStruct()
    L.install(s, proposal_records=False)
    assert list_fields(s) == dict(want, prop_desc=(None, 0), prop_hub=(None, 0), prop_partial=(None, 0))
    # what the record holds is what the plan built, and a sweep object holds it under these names
    for k, a in plan.host.items():
        t = {'np_dev': L.np_dev, 'resample_vars': L.resample_vars, '_static_idx': L.static_idx, 'prop_desc': L.prop_desc, 'prop_hub': L.prop_hub}.get(k)
        if t is not None:
            np.testing.assert_array_equal(t.numpy(), a)
    named = L.named()
    assert named['v2f_lists'] is L.v2f and named['_fused'] is L.fused and named['np_dev'] is L.np_dev and named['resample_vars'] is L.resample_vars
    assert named['prop_hub'] is L.prop_hub and (named['n_prop_desc'], named['n_prop_hub']) == (plan.n_prop_desc, hubs)
    assert set(named) == {'np_dev', 'resample_vars', 'n_prop_desc', 'prop_hub', 'n_prop_hub', 'v2f_lists', '_fused'}


def test_var_lists_without_v2f_lists_install_none():
    flat = synth.hybrid_mrf_flat(V=120, deg=4, seed=5, frac_discrete=0.0, T=32)     # every variable in the wide class: by range
    plan = var_side_plan(flat, 64, owned=None, opts=OPTS)
    L = plan.on({k: None if a is None else torch.from_numpy(a) for k, a in plan.host.items()}, None)
    s = _abi.PbpStruct()
    L.install(s)
    assert L.v2f is None and L.fused is None and L.prop_hub is None and L.n_prop_desc == int(flat.var_hidden.sum()) < flat.V
    assert list_fields(s) == dict({'v2f_' + k: (None, 0) for k in V2F_CLASSES}, prop_desc=(L.prop_desc.data_ptr(), L.n_prop_desc), prop_hub=(None, 0),
                                  prop_partial=(None, 0), resample_vars=(None, 0))


def test_var_lists_install_the_rest_of_the_fused_pass():
    """the fused pass leaves the rows of more than 64 factors and every discrete variable to the three kernels (lhvi_pbp_var_fused)"""
    plan, L = var_lists('hmln', 16)
    F = L.fused
    assert F.n_prop_rest == plan.n_prop_partial > 0 and F.n_resample_rest == L.n_prop_hub == 2 and F.v2f_rest.n_hub == 2
    full = _abi.PbpStruct()
    L.install(full)
    L.install_sampler(full)
    rest = dict(listed(F.v2f_rest, 'v2f_'), prop_desc=(F.prop_desc_rest.data_ptr(), F.n_prop_rest),
                resample_vars=(F.resample_rest.data_ptr(), F.n_resample_rest))
    kernel_fields = {'v2f': ['v2f_' + k for k in V2F_CLASSES], 'proposal': ['prop_desc'], 'sampler': ['resample_vars']}
    for kernels in (('v2f',), ('proposal',), ('sampler',), ('v2f', 'proposal'), ('v2f', 'proposal', 'sampler')):
        s = _abi.PbpStruct()
        L.install(s)
        L.install_sampler(s)
        for kernel in kernels:
            L.install_rest(s, kernel)
        changed = sum((kernel_fields[k] for k in kernels), [])
        # the named kernels' lists are the rest lists; everything else, the hub rows of the proposal among it, stays
        assert list_fields(s) == dict(list_fields(full), **{k: rest[k] for k in changed}), kernels
        assert s.np == full.np and s.prop_hub == L.prop_hub.data_ptr() and s.n_prop_hub == 2
    # the rest lists name different variables than the full ones
    assert F.v2f_rest.n_mid16 == 0 < L.v2f.n_mid16 and F.n_prop_rest < L.n_prop_desc and F.n_resample_rest < L.n_resample_vars


@pytest.mark.parametrize('lo,hi', [(0, 0), (7, 90), (200, 451)])
def test_var_lists_install_a_range_and_no_list(lo, hi):
    plan, L = var_lists('hmln', 16)
    for filled in (False, True):
        s = _abi.PbpStruct()
        if filled:                                                                  # a range takes every list out again
            L.install(s)
            for kernel in ('v2f', 'proposal', 'sampler'):
                L.install_rest(s, kernel)
        L.install_range(s, lo, hi)
        assert all(v == (None, 0) for v in list_fields(s).values()), list_fields(s)
        assert (s.var_lo, s.var_hi) == (lo, hi) and s.np == L.np_dev.data_ptr()


# ---- the factor side: which described edge goes to which f -> v kernel ---------------------------------------------------------
def words(*rows):
    """descriptor words of hand-built edges: (class, potential kind, nj, np, T, light type, uniform grid)"""
    w = torch.zeros(len(rows), 32, dtype=torch.int32)
    for i, r in enumerate(rows):
        w[i, 4], w[i, 6], w[i, 7], w[i, 8], w[i, 9], w[i, 14], w[i, 15] = r
    return w


LONG_GRID = (1, 1, 64, 64, 128, 0, 1)       # np + T > 128, uniform grid of 128 points, 64 partner particles: the grid recurrence
ROWS = (
    (1, 1, 10, 16, 32, 0, 1),       # both sides at most 16 particles                         -> small16
    (1, 1, 32, 16, 200, 0, 0),      # both at most 32, any number of integral points          -> small32
    (1, 1, 64, 64, 32, 0, 0),       # np + T <= 128, nj <= 64                                 -> heavy list
    (1, 1, 64, 64, 64, 0, 1),       # np + T = 128, uniform grid                              -> heavy list
    LONG_GRID, LONG_GRID,           # heavy list only from long_grid_min_edges such edges on
    (1, 1, 65, 64, 32, 0, 0),       # 65 partner particles                                    -> rest
    (1, 4, 10, 10, 32, 0, 0),       # potential kind 4 is not the heavy kernels'              -> rest
    (1, 4, 10, 10, 32, 1, 0),       # ... marked for the light kernel                         -> light
    (2, 1, 10, 10, 32, 2, 0),       # class 2, marked for the light kernel                    -> light
    (2, 1, 10, 10, 32, 0, 0),       # class 2                                                 -> rest
)


@pytest.mark.parametrize('min_edges', [2, 3])
def test_f2v_split_partitions_the_described_edges(min_edges):
    w = words(*ROWS)
    sp = pbp_plan.f2v_split(w, True, min_edges)
    small = sp.small16 | sp.small32
    lists = torch.stack([sp.heavy & ~small, sp.small16, sp.small32, sp.light, sp.rest]).int()
    assert lists.sum(0).tolist() == [1] * len(ROWS)                                 # every edge in exactly one list
    assert bool((sp.small16 & ~sp.heavy).sum() == 0) and bool((sp.small32 & ~sp.heavy).sum() == 0)
    long_grid = min_edges <= 2                                                      # two such rows: on the list from a threshold of 2
    want = [1, 2, 0, 0] + [0 if long_grid else 4] * 2 + [4, 4, 3, 3, 4]
    assert lists.argmax(0).tolist() == want
    # terms: (np + T) * nj over the heavy class; of those T * nj on a uniform grid (nj >= 24, or any nj in the small lists)
    heavy_rows = [r for r, m in zip(ROWS, sp.heavy.tolist()) if m]
    assert sp.heavy_terms == sum((r[3] + r[4]) * r[2] for r in heavy_rows)
    assert sp.heavy_grid_terms == 32 * 10 + 64 * 64 + (2 * 128 * 64 if long_grid else 0)


def test_f2v_split_without_the_small_lists():
    w = words(*ROWS)
    sp = pbp_plan.f2v_split(w, False, 2)
    assert not sp.small16.any() and not sp.small32.any()
    # the 16-particle edge is an ordinary heavy edge; T = 200 is beyond two rounds and its grid is not uniform
    assert sp.heavy.tolist()[:2] == [True, False] and sp.rest.tolist()[:2] == [False, True]
    assert (sp.heavy.int() + sp.light.int() + sp.rest.int()).tolist() == [1] * len(ROWS)
    assert sp.heavy_grid_terms == 64 * 64 + 2 * 128 * 64                            # the 10-particle edge's grid: not by the recurrence


# ---- the pair records: one per HybridQuadratic(1 discrete, 1 continuous) factor, from the light descriptors ---------------------
NAN = float('nan')


def light_rows(*rows):
    """[k, 128] uint8 light descriptors of hand-built edges (include/lhvi.h, lhvi_pbp_describe): (edge, target, partner, partner's
    canonical edge, nj, np, T, grid base, partner value, type); the six coefficients are 100 * edge + 0 .. 5"""
    out = torch.zeros(len(rows), 128, dtype=torch.uint8)
    w, d = out.view(torch.int32).view(-1, 32), out.view(torch.float64).view(-1, 16)
    for i, (e, target, partner, canon, nj, np_, T, base, value, kind) in enumerate(rows):
        w[i, 0], w[i, 1], w[i, 2], w[i, 3], w[i, 7], w[i, 8], w[i, 9], w[i, 10], w[i, 14] = e, target, partner, canon, nj, np_, T, base, kind
        w[i, 4] = 2 if kind == 2 else 1
        d[i, 6] = value
        d[i, 8:14] = 100.0 * e + torch.arange(6, dtype=torch.float64)
    return out


def record_views(rec):
    assert rec.dtype == torch.uint8 and rec.dim() == 2 and rec.shape[1] == 128 and rec.is_contiguous()
    return rec.view(torch.int32).view(-1, 32).numpy(), rec.view(torch.float64).view(-1, 16).numpy()


def coefficients(e):
    return [100.0 * e + k for k in range(6)]


def test_pair_records_join_the_two_edges_of_a_factor():
    """``lhvi_pbp_t.pair_desc`` (include/lhvi.h): 0 e_c  1 e_d  2 v_c  3 v_d  4 np_c  5 T  6 grid base  7 live states of v_d
    8-9 val_c  10-11 val_d  12-23 coefficients  24 / 25 rows of v2f with the discrete / continuous variable's message"""
    light = light_rows(
        (5, 11, 10, 4, 64, 2, 0, 0, NAN, 2),           # factor A, discrete target 11: its partner 10 is hidden, that one's v -> f row is 4
        (7, 20, 21, 8, 1, 16, 24, 300, 1.0, 1),        # factor B, continuous target 20: its partner 21 is observed at 1.0
        (9, 31, 30, 19, 1, 3, 0, 0, 0.25, 2),          # factor C, discrete target 31 (three live states): partner 30 observed at 0.25
        (4, 10, 11, 5, 2, 64, 32, 200, NAN, 1),        # factor A, continuous target 10: partner 11 hidden, its row 5 is the entry above
    )
    rec, first = pbp_plan.pair_records(light, 40)
    assert first == 0                                                               # no key: no interior part
    w, d = record_views(rec)
    assert w.shape[0] == 3                                                          # B, A (type-1 rows in their order), then what is left: C
    # B: one-sided, the discrete side observed
    assert w[0, :8].tolist() == [7, -1, 20, 21, 16, 24, 300, 1]
    assert np.isnan(d[0, 4]) and d[0, 5] == 1.0 and d[0, 6:12].tolist() == coefficients(7)
    assert w[0, 24] == 8 and w[0, 25] == 0
    # A: both edges, both canonical rows; the coefficients are the continuous target's entry's
    assert w[1, :8].tolist() == [4, 5, 10, 11, 64, 32, 200, 2]
    assert np.isnan(d[1, 4]) and np.isnan(d[1, 5]) and d[1, 6:12].tolist() == coefficients(4)
    assert w[1, 24] == 5 and w[1, 25] == 4
    # C: one-sided, the continuous side observed (one partner "particle": its value)
    assert w[2, :8].tolist() == [-1, 9, 30, 31, 1, 0, 0, 3]
    assert d[2, 4] == 0.25 and np.isnan(d[2, 5]) and d[2, 6:12].tolist() == coefficients(9)
    assert w[2, 24] == 0 and w[2, 25] == 19
    assert not w[:, 26:].any()
    # every input row is consumed exactly once
    used = np.concatenate([w[:, 0][w[:, 0] >= 0], w[:, 1][w[:, 1] >= 0]])
    assert sorted(used.tolist()) == [4, 5, 7, 9]
    for view in (light.view(torch.int32).view(-1, 32), light.view(torch.float64).view(-1, 16)):      # the descriptors' typed views do as well
        assert torch.equal(pbp_plan.pair_records(view, 40)[0], rec)


def test_pair_records_with_an_observed_partner_leave_the_other_entry_alone():
    """a type-1 entry whose partner is observed takes no type-2 entry, whatever its partner's canonical edge names"""
    light = light_rows((4, 10, 11, 5, 1, 64, 32, 200, 2.0, 1), (5, 11, 10, 4, 64, 2, 0, 0, NAN, 2))
    w, d = record_views(pbp_plan.pair_records(light, 8)[0])
    assert w[:, 0].tolist() == [4, -1] and w[:, 1].tolist() == [-1, 5] and d[0, 5] == 2.0 and w[1, 25] == 4


def test_pair_records_put_the_interior_factors_first():
    factors = [(2 * f, 2 * f + 1) for f in range(9)]
    rows, key = [], torch.zeros(18, dtype=torch.int32)
    for f, (ec, ed) in enumerate(factors):
        key[ec] = key[ed] = (1, 0, 1, 1, 0, 0, 1, 0, 1)[f]
        if f % 3 != 2:
            rows.append((ec, 100 + f, 200 + f, ed, 2, 16, 8, 0, NAN if f % 3 == 0 else 1.0, 1))
        if f % 3 != 1:
            rows.append((ed, 200 + f, 100 + f, ec, 16, 2, 0, 0, NAN if f % 3 == 0 else 0.5, 2))
    light = light_rows(*rows)
    plain, zero = pbp_plan.pair_records(light, 18)
    rec, first = pbp_plan.pair_records(light, 18, key)
    assert zero == 0 and plain.shape == rec.shape == (9, 128)
    w = record_views(plain)[0]
    rec_key = key[torch.from_numpy(np.where(w[:, 0] >= 0, w[:, 0], w[:, 1])).long()]
    assert first == int((rec_key == 0).sum()) == 4
    order = [i for i in range(9) if rec_key[i] == 0] + [i for i in range(9) if rec_key[i] == 1]      # stable within a key
    assert torch.equal(rec, plain[order])


def test_pair_records_of_no_light_edge():
    for key in (None, torch.zeros(5, dtype=torch.int32)):
        rec, first = pbp_plan.pair_records(torch.zeros(0, 128, dtype=torch.uint8), 5, key)
        assert rec.shape == (0, 128) and rec.dtype == torch.uint8 and first == 0


# ---- the factor side's lists as one record ---------------------------------------------------------------------------------------
STRIDE = {'heavy': 128, 'small16': 128, 'small32': 128, 'light': 128, 'pair': 128, 'cq': 256}
F2V_PARTS = dict(heavy=(5, 2), small16=(3, 0), small32=(4, 4), light=(6, 1), pair=(2, 1), cq=(3, 2), fast=(4, 3), generic=(5, 0))


def small_lists(counts=F2V_PARTS):
    """an F2vLists of CPU tensors with `counts`: list -> (entries, interior entries)"""
    pad = torch.zeros(1, dtype=torch.int32)
    L = pbp_plan.F2vLists.empty(pad)._asdict()
    for name, nbytes in STRIDE.items():
        k = counts[name][0]
        L[name + '_desc'], L['n_' + name] = (torch.zeros(k * nbytes, dtype=torch.uint8) if name == 'cq' else torch.zeros(k, nbytes, dtype=torch.uint8)), k
    L['fast_edges'], L['generic_edges'] = (torch.arange(counts[name][0], dtype=torch.int32) for name in ('fast', 'generic'))
    L['fast_desc'] = torch.zeros(counts['fast'][0], 128, dtype=torch.uint8)
    L['part_counts'] = {name: first for name, (_, first) in counts.items()}
    L['generic_pts_log2'] = 4
    return pbp_plan.F2vLists(**L)


def test_f2v_lists_install_what_the_sweep_holds():
    L = small_lists()
    assert set(L.part_counts) == set(pbp_plan.F2V_LISTS) == set(F2V_PARTS)
    s = _abi.PbpStruct()
    L.install(s)
    for name in STRIDE:
        assert getattr(s, name + '_desc') == getattr(L, name + '_desc').data_ptr() and getattr(s, 'n_' + name) == F2V_PARTS[name][0]
    assert s.fast_edges == L.fast_edges.data_ptr() and s.n_fast == 4 and s.fast_desc == L.fast_desc.data_ptr()
    assert s.generic_edges == L.generic_edges.data_ptr() and s.n_generic == 5 and s.generic_pts_log2 == 4
    assert L.n_fast == 4 and L.n_generic == 5
    # the light list is the pair list's edges again: not counted
    assert L.n_items == 5 + 3 + 4 + 2 + 3 + 4 + 5 and L.n_interior == 2 + 0 + 4 + 1 + 2 + 3 + 0
    # under the names of the sweep object's attributes, the same tensors
    named = L.named()
    assert named['heavy_desc'] is L.heavy_desc and named['_fast_list'] is L.fast_edges and named['_generic_list'] is L.generic_edges
    assert named['part_counts'] is L.part_counts and named['n_heavy'] == 5 and 'pad' not in named


@pytest.mark.parametrize('part', [0, 1])
def test_f2v_lists_install_a_prefix_or_a_suffix(part):
    L = small_lists()
    s = _abi.PbpStruct()
    L.install(s)
    assert L.install_part(s, part) is s
    for name, (total, first) in F2V_PARTS.items():
        off, cnt = (0, first) if part == 0 else (first, total - first)
        assert getattr(s, 'n_' + name) == cnt, name
        if name in STRIDE:
            assert getattr(s, name + '_desc') == (getattr(L, name + '_desc').data_ptr() + STRIDE[name] * off if cnt else None), name
        elif cnt:
            assert getattr(s, name + '_edges') == getattr(L, name + '_edges').data_ptr() + 4 * off
        else:           # nothing to do, and not "every edge of the graph": the pointer stays
            assert getattr(s, name + '_edges') == getattr(L, name + '_edges').data_ptr()
    assert s.fast_desc == L.fast_desc.data_ptr() + 128 * (0 if part == 0 else 3)


def test_f2v_lists_without_any_list():
    """what a state of the v -> f half alone installs: null descriptors, no entries, edge lists of no entry behind a non-null pointer"""
    pad = torch.zeros(1, dtype=torch.int32)
    L = pbp_plan.F2vLists.empty(pad)
    s = _abi.PbpStruct()
    for part in (None, 0, 1):
        L.install(s)
        if part is not None:
            L.install_part(s, part)
        for name in STRIDE:
            assert getattr(s, name + '_desc') is None and getattr(s, 'n_' + name) == 0
        assert s.fast_edges == pad.data_ptr() and s.generic_edges == pad.data_ptr() and s.n_fast == 0 and s.n_generic == 0
        assert s.fast_desc is None and s.generic_pts_log2 == 6
    assert L.part_counts == dict.fromkeys(pbp_plan.F2V_LISTS, 0) and L.n_items == 0 and L.n_interior == 0
    assert (L.n_heavy_class, L.heavy_terms, L.heavy_grid_terms, L.cq_terms) == (0, 0, 0, 0)
    named = L.named()
    assert named['fast_edges'].numel() == 0 and named['cq_edges'].numel() == 0 and named['_fast_list'] is pad and named['_generic_list'] is pad
    # an empty small or pair list leaves its fields as they are; without pair records there is no pair list
    some = small_lists(dict(F2V_PARTS, small16=(0, 0)))._replace(pair_desc=None, n_pair=0)
    s = _abi.PbpStruct()
    some.install(s)
    assert s.small16_desc is None and s.n_small16 == 0 and s.pair_desc is None and s.n_pair == 0 and s.n_small32 == 4


# f_side_plan over a hand-built graph: edge e belongs to variable e; the described edges are those of ROWS, two more light rows (one
# factor, both sides hidden) and, apart from them, two generic edges, one cq edge and one edge of no list (class 0)
PLAN_ROWS = ROWS + ((1, 4, 2, 10, 32, 1, 0), (2, 1, 10, 2, 0, 2, 0))
N_DESC = len(PLAN_ROWS)
E_GENERIC, E_CQ, E_NONE, E_ALL = (N_DESC, N_DESC + 1), N_DESC + 2, N_DESC + 3, N_DESC + 4


def plan_inputs():
    import types
    cls = torch.tensor([r[0] for r in PLAN_ROWS] + [3, 3, 4, 0], dtype=torch.uint8)
    table = torch.zeros(E_ALL, 128, dtype=torch.uint8)
    w, d = table.view(torch.int32).view(-1, 32), table.view(torch.float64).view(-1, 16)
    w[:N_DESC] = words(*PLAN_ROWS)
    w[:, 0] = torch.arange(E_ALL)
    w[N_DESC - 2, 3], w[N_DESC - 1, 3] = N_DESC - 1, N_DESC - 2           # the last two rows: one factor, each the other's partner
    d[N_DESC - 2:N_DESC, 6] = NAN
    cq = torch.zeros(E_ALL, 64, dtype=torch.int32)                          # lhvi_pbp_describe_cq: 2 type, 3 S, 4 np, 5 T, 9 ny
    cq[E_CQ, 0], cq[E_CQ, 2], cq[E_CQ, 3], cq[E_CQ, 4], cq[E_CQ, 5], cq[E_CQ, 9] = E_CQ, 1, 2, 10, 32, 7
    var_cont = np.ones(E_ALL, dtype=bool)
    var_cont[E_GENERIC[1]] = False
    flat = types.SimpleNamespace(E=E_ALL, edge_var=np.arange(E_ALL), var_cont=var_cont, var_nstates=np.full(E_ALL, 3))
    np_host = np.full(E_ALL, 10, dtype=np.int32)
    calls = []

    def describe(edges):
        calls.append(edges.tolist())
        return table[edges.long()].reshape(-1)

    def describe_cq(edges):
        return cq[edges.long()].contiguous().view(torch.uint8).reshape(-1)
    return cls, flat, np_host, dict(describe=describe, describe_cq=describe_cq, long_grid_min_edges=2), calls


def list_edges(L):
    """list -> its edges, in list order"""
    out = {name: getattr(L, name + '_desc').view(torch.int32).view(-1, 32)[:, 0].tolist() if getattr(L, name + '_desc') is not None else []
           for name in ('heavy', 'small16', 'small32', 'light')}
    out['cq'] = L.cq_desc.view(torch.int32).view(-1, 64)[:, 0].tolist() if L.cq_desc is not None else []
    out['fast'], out['generic'] = L.fast_edges.tolist(), L.generic_edges.tolist()
    return out


def test_f_side_plan_puts_every_edge_on_one_list():
    cls, flat, np_host, kw, calls = plan_inputs()
    L = pbp_plan.f_side_plan(cls, flat, np_host, **kw)
    assert calls == [list(range(N_DESC))]                                           # one describe call, for the edges of class 1 and 2
    got = list_edges(L)
    assert got == {'small16': [0], 'small32': [1], 'heavy': [2, 3, 4, 5], 'fast': [6, 7, 10], 'light': [8, 9, 11, 12],
                   'generic': list(E_GENERIC), 'cq': [E_CQ]}
    assert sorted(sum(got.values(), [])) == [e for e in range(E_ALL) if e != E_NONE]
    for name in ('heavy', 'small16', 'small32', 'light', 'cq'):
        assert getattr(L, 'n_' + name) == len(got[name])
    assert L.cq_edges.tolist() == [E_CQ] and L.cq_edges.dtype == L.fast_edges.dtype == L.generic_edges.dtype == torch.int32
    assert L.fast_desc.view(torch.int32).view(-1, 32)[:, 0].tolist() == got['fast']      # descriptor i is edge i's
    assert L.n_heavy_class == 6                                                     # the heavy class: the heavy list and the two small lists
    sp = pbp_plan.f2v_split(words(*PLAN_ROWS), True, 2)
    assert (L.heavy_terms, L.heavy_grid_terms) == (sp.heavy_terms, sp.heavy_grid_terms)
    assert L.cq_terms == (10 + 32) * 7 * 2                                          # type 1: (np + T) * ny * S
    # generic edges: 10 particles + 3 integral points on the continuous variable, 10 points on the discrete one: 16 lanes
    assert L.generic_pts_log2 == 4
    # the pair list: the light edges again, the two of a factor in one record
    w = record_views(L.pair_desc)[0]
    assert L.n_pair == 3 and w[:, 0].tolist() == [8, 11, -1] and w[:, 1].tolist() == [-1, 12, 9]
    assert L.part_counts == dict.fromkeys(pbp_plan.F2V_LISTS, 0)                    # no key: no interior part
    off = pbp_plan.f_side_plan(cls, flat, np_host, paired_light=False, small_f2v=False, **kw)
    assert off.pair_desc is None and off.n_pair == 0 and off.n_light == 4 and off.small16_desc.shape == (0, 128) and off.n_small16 == 0
    assert list_edges(off)['heavy'] == [0, 2, 3, 4, 5] and list_edges(off)['fast'] == [1, 6, 7, 10]


def test_f_side_plan_without_edges_of_a_kind():
    cls, flat, np_host, kw, calls = plan_inputs()
    L = pbp_plan.f_side_plan(torch.where(cls >= 3, torch.zeros_like(cls), cls), flat, np_host, **kw)
    assert L.cq_desc is None and L.n_cq == 0 and L.cq_terms == 0 and L.generic_edges.numel() == 0 and L.generic_pts_log2 == 6
    L = pbp_plan.f_side_plan(torch.where(cls < 3, torch.zeros_like(cls), cls), flat, np_host, **kw)
    assert len(calls) == 1 and L.fast_edges.numel() == 0 and L.fast_desc is None and L.heavy_desc is None and L.light_desc is None
    assert L.pair_desc is None and L.n_heavy_class == 0 and L.n_cq == 1
    s = _abi.PbpStruct()
    L.install(s)
    assert s.fast_edges == L.pad.data_ptr() and s.n_fast == 0 and s.generic_edges == L.generic_edges.data_ptr() and s.n_generic == 2


def test_f_side_plan_skips_edges_and_puts_interior_entries_first():
    cls, flat, np_host, kw, _ = plan_inputs()
    whole = list_edges(pbp_plan.f_side_plan(cls, flat, np_host, **kw))
    skip = torch.zeros(E_ALL, dtype=torch.bool)
    skip[3] = skip[10] = skip[E_GENERIC[0]] = True
    got = list_edges(pbp_plan.f_side_plan(cls, flat, np_host, skip=skip, **kw))
    assert got == {name: [e for e in es if not skip[e]] for name, es in whole.items()}
    # a key: 1 on every third edge, the two light edges of the one factor alike
    key = (torch.arange(E_ALL) % 3 == 0).to(torch.int32)
    key[N_DESC - 2] = key[N_DESC - 1] = 1
    L = pbp_plan.f_side_plan(cls, flat, np_host, key=key, **kw)
    got = list_edges(L)
    for name, es in got.items():
        assert es == [e for e in whole[name] if key[e] == 0] + [e for e in whole[name] if key[e] == 1], name       # stable
        assert L.part_counts[name] == sum(1 for e in es if key[e] == 0), name
    w = record_views(L.pair_desc)[0]
    rec_key = [int(key[a if a >= 0 else b]) for a, b in zip(w[:, 0].tolist(), w[:, 1].tolist())]
    assert rec_key == sorted(rec_key) and L.part_counts['pair'] == rec_key.count(0) == 1 and L.n_pair == 3
    assert L.fast_desc.view(torch.int32).view(-1, 32)[:, 0].tolist() == got['fast']
    assert L.n_items == sum(len(es) for name, es in got.items() if name != 'light') + L.n_pair
    assert L.n_interior == sum(first for name, first in L.part_counts.items() if name != 'light')
    both = pbp_plan.f_side_plan(cls, flat, np_host, key=key, skip=skip, **kw)
    assert list_edges(both) == {name: [e for e in es if not skip[e]] for name, es in got.items()}


def test_f_side_plan_is_a_function_of_its_arguments():
    cls, flat, np_host, kw, _ = plan_inputs()
    key = (torch.arange(E_ALL) % 2).to(torch.int32)
    key[N_DESC - 2] = key[N_DESC - 1] = 0
    a, b = (pbp_plan.f_side_plan(cls, flat, np_host, key=key, **kw) for _ in range(2))
    assert a._fields == b._fields
    for name, x, y in zip(a._fields, a, b):
        if torch.is_tensor(x):
            assert x.dtype == y.dtype and x.shape == y.shape and x.numpy().tobytes() == y.numpy().tobytes(), name
        else:
            assert x == y, name
