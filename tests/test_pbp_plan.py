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
