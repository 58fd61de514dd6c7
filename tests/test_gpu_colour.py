"""Colour refinement (csrc/color.hip) and the device lifting reductions (``lhvi/lifting.py``) half round by half round against the
pure-Python oracle (``oracle.refine_factors`` / ``refine_rvs`` / ``color_passing``) and NumPy's sequential ``add.at`` /
``minimum.at``.  Every assertion is on integers or on bytes: no tolerance.  The graphs come from tests/colour_models.py;
tests/test_colour_host.py shows on the CPU that the oracle alone satisfies what is relied on here.

Not tested: the collision word (``result[1]``).  It is raised when two items agree on the first 64-bit fingerprint and differ on
the second, which cannot be provoked without a 64-bit collision of the fingerprints; every half round here asserts it is 0."""
import functools

import numpy as np
import pytest

import colour_models as cm
from oracle import oracle
from test_colour_host import RAGGED_SIZES, assert_reductions_equal, check_big_cluster, lift_case

pytestmark = pytest.mark.gpu

METHODS = {'hash': 0, 'sort': 1}              # _abi.COLOR_HASH / COLOR_SORT


@pytest.fixture(scope='module')
def api():
    from lhvi import _abi
    _abi.require_gpu()
    assert (_abi.COLOR_HASH, _abi.COLOR_SORT) == (METHODS['hash'], METHODS['sort'])
    return _abi


class Halves:
    """the two half rounds through the C ABI with the call pattern of ``c2f.FlatRefiner`` -- no fallback to the sort: the result
    words {number of colours, collision, overflow, 0} come back with the colours"""

    def __init__(self, api, flat, sym, g=None):
        import torch
        self.api, self.dg = api, api.DeviceGraph(flat)
        self.g = self.dg.g if g is None else g(self.dg.g)
        self.sym = api.to_dev(np.asarray(sym, dtype=np.uint8))
        self.ws_bytes = int(api.lib().lhvi_color_workspace_bytes(self.g))
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=self.dg.device)

    def _call(self, fn, *args):
        import torch
        api = self.api
        res = torch.full((4,), -7, dtype=torch.int32, device=self.dg.device)
        api.check(fn(self.g, *(api.ptr(a) for a in args), api.ptr(res), api.ptr(self.ws), self.ws_bytes, self.method,
                     api.stream_ptr()))
        return args[-1].cpu().numpy(), res.cpu().numpy().tolist()

    def factors(self, rv_color, f_color, method):
        import torch
        api, self.method = self.api, method
        rvc, fc = api.to_dev(np.asarray(rv_color, dtype=np.int32)), api.to_dev(np.asarray(f_color, dtype=np.int32))
        return self._call(api.lib().lhvi_color_refine_factors, self.sym, rvc, fc, torch.full_like(fc, -1))

    def rvs(self, f_color, rv_color, method):
        import torch
        api, self.method = self.api, method
        rvc, fc = api.to_dev(np.asarray(rv_color, dtype=np.int32)), api.to_dev(np.asarray(f_color, dtype=np.int32))
        return self._call(api.lib().lhvi_color_refine_rvs, fc, rvc, torch.full_like(rvc, -1))


def no_hub_list(g):
    """a copy of the graph struct without the hub list: the hub kernels scan all V variables"""
    from lhvi._abi import GraphStruct
    g2 = GraphStruct.from_buffer_copy(g)
    g2.hub_vars, g2.n_hubs = None, 0
    assert g2.hub_vars is None and g2.V == g.V and g2.var_ptr == g.var_ptr
    return g2


def check_half(run, want, n_want, what):
    """one half round with both methods, twice each, against the oracle's colours `want`; returns the colour array"""
    arrays = {}
    for name, method in METHODS.items():
        got, res = run(method)
        assert res == [n_want, 0, 0, 0], (what, name, res, n_want)
        assert np.array_equal(np.unique(got), np.arange(n_want)), (what, name)          # ids exactly 0 .. n - 1
        assert oracle.canonical_labels(got) == oracle.canonical_labels(want), (what, name)
        again, res2 = run(method)
        assert res2 == res and again.tobytes() == got.tobytes(), (what, name, 'second call')
        arrays[name] = got
    np.testing.assert_array_equal(arrays['hash'], arrays['sort'], err_msg=what)
    return arrays['hash']


@functools.lru_cache(maxsize=None)
def ragged_walk(size, seed, rounds=4):
    """the graph and the oracle's colours before and after every half round: [(side, rv colours in, f colours in, out, n)]"""
    flat, sym, rv, f = cm.ragged(seed, **RAGGED_SIZES[size])
    steps = []
    for _ in range(rounds):
        f2, nf = oracle.refine_factors(flat, sym, rv, f)
        steps.append(('f', rv, f, f2, nf))
        rv2, nr = oracle.refine_rvs(flat, f2, rv)
        steps.append(('rv', rv, f2, rv2, nr))
        rv, f = rv2, f2
    return flat, sym, steps


# ---- 1. single half rounds ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', sorted(RAGGED_SIZES))
@pytest.mark.parametrize('seed', [0, 1])
def test_every_half_round_equals_the_oracle(api, size, seed):
    """four rounds of the oracle on a ragged graph (degrees 0, 1, 63, 64, 65, 127, 128, 129, 300; arities 1 to 6, symmetric and
    not; scopes with a variable twice; every hub with a twin that must keep its colour); every half round starts from the ORACLE's colours, so a split that comes a round late is
    seen at the half round it belongs to, not hidden by the fixed point"""
    flat, sym, steps = ragged_walk(size, seed)
    h = Halves(api, flat, sym)
    splits = 0
    for i, (side, rv, f, want, n) in enumerate(steps):
        run = (lambda m: h.factors(rv, f, m)) if side == 'f' else (lambda m: h.rvs(f, rv, m))
        check_half(run, want, n, '%s half of round %d' % (side, i // 2))
        splits += n > int((f if side == 'f' else rv).max()) + 1
    assert splits >= 4                                    # the walk is not at its fixed point from the start


def test_single_variable_with_one_unary_factor(api):
    flat, sym, rv0, f0 = cm.single()
    h = Halves(api, flat, sym)
    check_half(lambda m: h.factors(rv0, f0, m), [0], 1, 'factor half')
    check_half(lambda m: h.rvs(f0, rv0, m), [0], 1, 'variable half')


# ---- 2. the sort network of the symmetric factors ----------------------------------------------------------------------------
@pytest.mark.parametrize('a', [2, 3, 4, 5, 6])
@pytest.mark.parametrize('symmetric', [True, False])
def test_sort_network(api, a, symmetric):
    """factors of one initial colour whose scopes are every permutation of a multiset of `a` variable colours: one output colour
    per multiset when they are symmetric, one per distinct colour tuple when not.  ('repeated', 'top'): two multisets that differ
    in the largest colour only -- a sort that moves the padding of a scope shorter than LHVI_MAX_ARITY in front of it drops that
    colour and merges them"""
    for multisets in (('distinct',), ('repeated',), ('repeated', 'top')):
        flat, sym, rv0, f0, expected = cm.sort_network_case(a, symmetric, multisets)
        want, n = oracle.refine_factors(flat, sym, rv0, f0)
        assert n == expected
        h = Halves(api, flat, sym)
        check_half(lambda m: h.factors(rv0, f0, m), want, expected, 'arity %d %s' % (a, multisets))


# ---- 3. no hub list ----------------------------------------------------------------------------------------------------------
def test_without_a_hub_list_the_hub_kernels_scan_all_variables(api):
    """``lhvi_graph_t.hub_vars == NULL``: the same colour arrays, bit for bit, as with the list ``DeviceGraph`` always passes"""
    flat, sym, steps = ragged_walk('F_above_V', 0)
    side, rv, f, want, n = steps[1]
    assert side == 'rv'
    with_list, without = Halves(api, flat, sym), Halves(api, flat, sym, g=no_hub_list)
    assert with_list.g.n_hubs == 10 and with_list.g.hub_vars and not without.g.hub_vars and without.g.n_hubs == 0
    a = check_half(lambda m: with_list.rvs(f, rv, m), want, n, 'with the list')
    b = check_half(lambda m: without.rvs(f, rv, m), want, n, 'without the list')
    np.testing.assert_array_equal(a, b)


def test_without_a_hub_list_and_without_hubs(api):
    """largest degree exactly LHVI_HUB_DEGREE: the hub kernels scan all variables and find nothing"""
    flat, sym, rv0, f0 = cm.ragged(3, hubs=(63, 64, 64), n_small=700, n_fac=900)
    assert np.diff(flat.var_ptr).max() == 64
    f1, _ = oracle.refine_factors(flat, sym, rv0, f0)
    want, n = oracle.refine_rvs(flat, f1, rv0)
    with_list, without = Halves(api, flat, sym), Halves(api, flat, sym, g=no_hub_list)
    assert with_list.g.n_hubs == 0
    a = check_half(lambda m: with_list.rvs(f1, rv0, m), want, n, 'with the (empty) list')
    b = check_half(lambda m: without.rvs(f1, rv0, m), want, n, 'without the list')
    np.testing.assert_array_equal(a, b)


# ---- 4. fixed point on permuted copies ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', sorted(RAGGED_SIZES))
def test_fixed_point_on_permuted_copies(api, size):
    from lhvi import lifting
    flat, sym, rv0, f0 = cm.ragged(0, **RAGGED_SIZES[size])
    cflat, csym, crv0, cf0, vperm, fperm = cm.copies(flat, sym, rv0, f0, c=3, seed=5)
    brv, bf = oracle.color_passing(flat, sym, rv0, f0)
    out = {}
    for name, method in METHODS.items():
        st = {}
        rvc, fc = lifting.refine_flat(cflat, csym, crv0, cf0, method=method, stats=st)
        assert st['sorted_half_rounds'] == 0 and st['rounds'] >= 2
        for k in range(1, 3):
            np.testing.assert_array_equal(rvc[vperm[k]], rvc[vperm[0]])
            np.testing.assert_array_equal(fc[fperm[k]], fc[fperm[0]])
        assert oracle.canonical_labels(rvc[vperm[0]]) == oracle.canonical_labels(brv)
        assert oracle.canonical_labels(fc[fperm[0]]) == oracle.canonical_labels(bf)
        assert (np.bincount(rvc) % 3 == 0).all() and (np.bincount(fc) % 3 == 0).all()
        assert np.array_equal(np.unique(rvc), np.arange(int(brv.max()) + 1))
        assert np.array_equal(np.unique(fc), np.arange(int(bf.max()) + 1))
        out[name] = (rvc, fc)
    np.testing.assert_array_equal(out['hash'][0], out['sort'][0])
    np.testing.assert_array_equal(out['hash'][1], out['sort'][1])


# ---- 5. large clusters across the hub threshold ------------------------------------------------------------------------------
@pytest.mark.parametrize('evidence_ratio', [0.2, 0.0])
def test_large_clusters_across_the_hub_threshold(api, evidence_ratio):
    """``synth.rgm_flat(65, 63, n_values=3)``: market degree 64, revenue and recession degree 65; thousands of items share a key, so
    the LDS filter and the table are under same-key contention.
    With ``evidence_ratio=0.2`` (a fifth of the atoms observed at three values) the fixed point is the discrete partition (4 224 /
    8 255 clusters of one, as the oracle says): the large clusters are those of the FIRST round -- 2 555 factors / 1 969 variables
    in the largest -- which is compared half by half.  Without evidence the fixed point itself keeps the 4 095 loss atoms in one
    cluster."""
    from lhvi import lifting, synth
    flat, sym, rv0, f0 = synth.rgm_flat(cm.RGM_C, cm.RGM_B, n_values=3, evidence_ratio=evidence_ratio)
    assert {64, 65} <= set(np.diff(flat.var_ptr).tolist())
    want_rv, want_f = oracle.color_passing(flat, sym, rv0, f0)
    f1, nf1 = oracle.refine_factors(flat, sym, rv0, f0)
    rv1, nrv1 = oracle.refine_rvs(flat, f1, rv0)
    assert np.bincount(f1).max() >= 2000 and np.bincount(rv1).max() >= 1900
    h = Halves(api, flat, sym)
    check_half(lambda m: h.factors(rv0, f0, m), f1, nf1, 'first factor half')
    check_half(lambda m: h.rvs(f1, rv0, m), rv1, nrv1, 'first variable half')
    if evidence_ratio == 0.0:
        assert np.bincount(want_rv).max() == cm.RGM_C * cm.RGM_B and np.bincount(want_f).max() == cm.RGM_C * cm.RGM_B
    out = {}
    for name, method in METHODS.items():
        rvc, fc = lifting.refine_flat(flat, sym, rv0, f0, method=method)
        assert oracle.canonical_labels(rvc) == oracle.canonical_labels(want_rv)
        assert oracle.canonical_labels(fc) == oracle.canonical_labels(want_f)
        out[name] = (rvc, fc)
    np.testing.assert_array_equal(out['hash'][0], out['sort'][0])
    np.testing.assert_array_equal(out['hash'][1], out['sort'][1])


# ---- 6. the table's edge -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('extra', [0, 1])
def test_table_edge(api, extra):
    """MAX_DISTINCT = 524 288 distinct keys fit the hash table, one more overflows and the round is repeated through the sort; the
    partition is the identity either way"""
    from lhvi import lifting
    V = cm.MAX_DISTINCT + extra
    flat, sym, rv0, f0 = cm.all_distinct(V)
    dg = api.DeviceGraph(flat)
    st = {}
    rvc, fc = lifting.refine_flat(flat, sym, rv0, f0, dg=dg, stats=st)
    assert st['rounds'] == 1
    assert (st['sorted_half_rounds'] > 0) == bool(extra), st
    rvs, fs = lifting.refine_flat(flat, sym, rv0, f0, dg=dg, method=api.COLOR_SORT)
    for got, want in ((rvc, rvs), (fc, fs)):
        assert np.array_equal(np.sort(got), np.arange(V))
        np.testing.assert_array_equal(got, want)
    # the half rounds' own result words at the edge
    h = Halves(api, flat, sym)
    for got, res in (h.factors(rv0, f0, api.COLOR_HASH), h.rvs(f0, rv0, api.COLOR_HASH)):
        if extra:
            assert res[1:] == [0, 1, 0]
        else:
            assert res == [V, 0, 0, 0]
            assert np.array_equal(np.sort(got), np.arange(V))


# ---- 7. segment sums and first members at wave-level shapes ------------------------------------------------------------------
def test_segment_sums_with_long_and_short_runs_in_one_wavefront(api):
    import torch
    from lhvi import lifting
    values, lengths = cm.segment_case()
    assert set(lengths.tolist()) == set(cm.SEG_LENGTHS) and lengths.size == 5 * 64 + 37
    for w, (first, last) in enumerate(((256, 1000), (257, 511), (512, 513))):
        seg = lengths[64 * w:64 * w + 64]
        assert (seg[0], seg[63]) == (first, last) and seg[1:63].max() < 256
    assert lengths[256:320].max() < 256 and lengths[-1] == 257
    seg_of = np.repeat(np.arange(lengths.size), lengths)
    want = np.zeros(lengths.size)
    np.add.at(want, seg_of, values)
    tree = np.array([values[seg_of == s].sum() for s in range(lengths.size)])         # (pairwise: another order of additions)
    assert (tree != want).sum() > 20
    got = lifting.segment_sums(torch.from_numpy(values).cuda(), torch.from_numpy(lengths).cuda()).cpu().numpy()
    assert got.tobytes() == want.tobytes(), np.flatnonzero(got != want)


def test_first_members_at_wavefront_shapes(api):
    import torch
    from lhvi import lifting
    for name, col, n_colors in cm.first_member_cases():
        n = col.size
        want = np.full(n_colors, n, dtype=np.int64)
        np.minimum.at(want, col, np.arange(n))
        got = lifting.first_members(torch.from_numpy(col.astype(np.int32)).cuda(), n_colors, n).cpu().numpy()
        np.testing.assert_array_equal(got, want, err_msg=name)
        if name.startswith('straddle'):
            assert (col == 63).sum() == 2 and col[63] == col[64] == 63 and want[63] == 63


# ---- 8. the device lifting reductions at small size --------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['copies', 'rgm'])
def test_device_lifting_reductions_at_small_size(api, monkeypatch, name):
    """``_lift_reduce_device`` below SMALL_LIFT_EDGES, where ``lift_flat`` would use NumPy: field by field the host reductions, the
    evidence values by bytes (a cluster of hundreds of observed members whose running sum passes +-1e16), then the whole lifted
    graph and its count bookkeeping"""
    from lhvi import lifting
    flat, sym, rv0, f0, big, want_rv, want_f = lift_case(name)
    assert flat.E < lifting.SMALL_LIFT_EDGES
    dg = api.DeviceGraph(flat)
    rvc_d, fc_d = lifting.refine_flat(flat, sym, rv0, f0, dg=dg, device_out=True)
    rvc, fc = rvc_d.cpu().numpy(), fc_d.cpu().numpy()
    assert oracle.canonical_labels(rvc) == oracle.canonical_labels(want_rv)
    assert oracle.canonical_labels(fc) == oracle.canonical_labels(want_f)
    check_big_cluster(flat, rv0, big, rvc)
    want = lifting._lift_reduce_host(flat, rvc, fc)
    got = lifting._lift_reduce_device(flat, dg, rvc_d, fc_d)
    assert_reductions_equal(got, want)
    host = lifting.lift_flat(flat, rvc, fc)
    calls = []
    reduce_device = lifting._lift_reduce_device
    monkeypatch.setattr(lifting, '_lift_reduce_device', lambda *a: calls.append(1) or reduce_device(*a))
    monkeypatch.setattr(lifting, 'SMALL_LIFT_EDGES', 0)
    dev = lifting.lift_flat(flat, rvc_d, fc_d, dg=dg)
    assert calls == [1]
    for field in ('fac_ptr', 'edge_var', 'edge_canon', 'var_ptr', 'var_edge', 'edge_count', 'var_dom', 'var_mult', 'fac_mult',
                  'fac_pot'):
        np.testing.assert_array_equal(getattr(dev, field), getattr(host, field), err_msg=field)
    assert dev.var_value.tobytes() == host.var_value.tobytes()
    # count / N bookkeeping: a cluster's counts add up to its representative's ground degree, and over all clusters to E
    n_rv, n_f = int(rvc.max()) + 1, int(fc.max()) + 1
    assert (dev.V, dev.F) == (n_rv, n_f)
    deg = np.diff(flat.var_ptr)
    rep = np.full(n_rv, flat.V, dtype=np.int64)
    np.minimum.at(rep, rvc, np.arange(flat.V))
    owner = np.repeat(np.arange(n_rv), np.diff(dev.var_ptr))
    N = np.bincount(owner, weights=dev.edge_count[dev.var_edge], minlength=n_rv)       # (integers in doubles: exact)
    np.testing.assert_array_equal(N, deg[rep])
    assert float((dev.var_mult * N).sum()) == flat.E and dev.var_mult.sum() == flat.V and dev.fac_mult.sum() == flat.F
    assert (deg == deg[rep][rvc]).all()                           # members of a cluster have the same degree
