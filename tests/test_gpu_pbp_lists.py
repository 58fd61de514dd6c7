"""The f -> v half's work lists as the sweep builds them on the device against ``pbp_plan.f_side_plan`` run on the host: the same
class array, the same descriptors (downloaded), the same key and skip marks -- every list, count, prefix count and term count byte
for byte.  And the two parts a sharded sweep cuts each list into (``F2vLists.install_part``): disjoint, together the list, the
first one the entries with key 0."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STRIDE = {'heavy': 128, 'small16': 128, 'small32': 128, 'light': 128, 'pair': 128, 'cq': 256}
# graph, particles, kind of state, lists that must not be empty for the case to test what it is there for
CASES = {
    'mrf n16': ('mrf', 16, 'single', ('small16', 'pair')),
    'mrf n32': ('mrf', 32, 'single', ('small32', 'pair')),
    'mrf n64': ('mrf', 64, 'single', ('heavy', 'pair')),
    'hmln n16': ('hmln', 16, 'single', ('cq', 'generic')),
    'mrf n80': ('mrf', 80, 'single', ('fast',)),                # more than 64 partner particles: the general kernel's list
    'mrf n64 shard': ('mrf', 64, 'shard', ('heavy', 'pair')),
    'mrf n64 owner': ('mrf', 64, 'owner', ('heavy', 'pair')),
}


@pytest.fixture(scope='module')
def api():
    from lhvi import _abi
    _abi.require_gpu()
    return _abi


def graph(name):
    from lhvi import synth
    if name == 'hmln':
        return synth.paper_popularity_flat(150, 4, seed=2)[0]
    return synth.hybrid_mrf_flat(V=300, deg=4, seed=37, frac_discrete=0.3, T=32)


@functools.lru_cache(maxsize=None)
def state(case):
    """(sweep object after _setup, its _setup arguments edge_key / edge_skip as arrays or None)"""
    from lhvi import dist
    from lhvi.pbp import EPBP
    name, n, kind, _ = CASES[case]
    flat = graph(name)
    bp = EPBP(None, n=n, proposal_approximation='simple', sampler='device', seed=5)
    key = skip = None
    if kind == 'shard':
        plan = dist.ShardPlan(flat, 1, 2)
        key = plan.edge_boundary
        bp._setup(None, flat=plan.flat, edge_key=key)
    elif kind == 'owner':
        plan = dist.OwnerPlan(flat, 1, 2, var_owner=dist.partition_variables(flat, 2))
        plan.flat.edge_canon = plan.ghost_rows(n)[0]           # as OwnerRunner describes its edges
        key, skip = plan.edge_key, plan.edge_skip
        bp._setup(None, flat=plan.flat, edge_key=key, edge_skip=skip, owned=plan.n_owned)
    else:
        bp._setup(None, flat=flat)
    return bp, key, skip


def host_plan(api, bp, key, skip):
    """f_side_plan on CPU copies of what _setup gave it on the device"""
    import torch
    from lhvi import pbp_plan
    E = bp.flat.E
    cls = torch.zeros(max(E, 1), dtype=torch.uint8, device=bp.dg.device)
    api.check(api.lib().lhvi_pbp_classify(bp.dg.g, bp.dg.p, bp._struct(), api.ptr(cls), api.stream_ptr()))
    return pbp_plan.f_side_plan(
        cls[:E].cpu(), bp.flat, bp.np_host, describe=lambda edges: bp._describe(edges.to(bp.dg.device)).cpu(),
        describe_cq=lambda edges: bp._describe(edges.to(bp.dg.device), 'lhvi_pbp_describe_cq', 256).cpu(),
        key=None if key is None else torch.from_numpy(np.ascontiguousarray(key, dtype=np.int32)),
        skip=None if skip is None else torch.from_numpy(np.ascontiguousarray(skip, dtype=bool)),
        paired_light=bp.paired_light, small_f2v=bp.small_f2v, long_grid_min_edges=bp.long_grid_min_edges)


@pytest.mark.parametrize('case', list(CASES))
def test_device_built_lists_equal_the_host_plan(api, case):
    import torch
    bp, key, skip = state(case)
    L, H = bp.f2v_lists, host_plan(api, bp, key, skip)
    counts = {name: getattr(L, 'n_' + name) for name in L.part_counts}
    print(case, counts, L.part_counts, L.generic_pts_log2, L.n_heavy_class, L.heavy_terms, L.heavy_grid_terms, L.cq_terms)
    for name in CASES[case][3]:
        assert counts[name] > 0, name
    for name, dev, host in zip(L._fields, L, H):
        if torch.is_tensor(dev):
            assert dev.is_cuda and not host.is_cuda, name
            assert dev.dtype == host.dtype and dev.shape == host.shape and dev.cpu().numpy().tobytes() == host.numpy().tobytes(), name
        else:
            assert type(dev) is type(host) and dev == host, name
    if key is not None:
        assert sum(L.part_counts.values()) > 0 and any(L.part_counts[name] < counts[name] for name in counts)
    # the sweep object's attributes are the record's fields: the same tensors, not copies
    for name, value in L.named().items():
        assert vars(bp)[name] is value, name
    assert set(bp.part_counts) == {'heavy', 'light', 'fast', 'generic', 'cq', 'pair', 'small16', 'small32'}


def list_keys(L, name, key):
    """the key of every entry of one list, in list order"""
    import torch
    if name in ('fast', 'generic'):
        edges = getattr(L, name + '_edges').cpu().long()
    elif name == 'pair':
        w = L.pair_desc.view(torch.int32).view(-1, 32).cpu().long()
        assert bool((key[w[:, 0].clamp_min(0)] == key[w[:, 1].clamp_min(0)])[(w[:, 0] >= 0) & (w[:, 1] >= 0)].all())
        edges = torch.where(w[:, 0] >= 0, w[:, 0], w[:, 1])
    else:
        edges = getattr(L, name + '_desc').view(torch.int32).view(-1, STRIDE[name] // 4)[:, 0].cpu().long()
    return key[edges]


@pytest.mark.parametrize('case', ['mrf n64', 'hmln n16', 'mrf n64 shard', 'mrf n64 owner'])
def test_the_two_parts_of_every_list_are_disjoint_and_together_the_list(api, case):
    import torch
    bp, key, _ = state(case)
    L = bp.f2v_lists
    key = torch.zeros(max(bp.flat.E, 1), dtype=torch.int64) + 1 if key is None else torch.from_numpy(np.asarray(key)).long()
    spans = {}
    for part in (0, 1):
        s = L.install_part(bp._struct(), part)
        for name in L.part_counts:
            tensor = getattr(L, name + ('_edges' if name in ('fast', 'generic') else '_desc'))
            cnt, p = getattr(s, 'n_' + name), getattr(s, name + ('_edges' if name in ('fast', 'generic') else '_desc'))
            stride = STRIDE.get(name, 4)
            if cnt == 0:
                assert (p is None) == (name in STRIDE), name       # no descriptors: null; no edges: the count says so, never the pointer
                spans[name, part] = None
                continue
            off = p - tensor.data_ptr()
            assert off % stride == 0 and 0 <= off and off + cnt * stride <= tensor.numel() * tensor.element_size(), name
            spans[name, part] = (off // stride, off // stride + cnt)
            if name == 'fast':
                assert s.fast_desc - L.fast_desc.data_ptr() == 128 * (off // 4)
    for name in L.part_counts:
        total, first = getattr(L, 'n_' + name), L.part_counts[name]
        assert spans[name, 0] == ((0, first) if first else None) and spans[name, 1] == ((first, total) if total > first else None), name
        if total:
            k = list_keys(L, name, key)
            assert bool((k[:first] == 0).all()) and bool((k[first:] == 1).all()), name
