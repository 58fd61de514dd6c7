"""CPU tests of the colour-refinement test models (tests/colour_models.py): the pure-Python reference alone satisfies every
condition tests/test_gpu_colour.py relies on, ``build_flat`` refuses what the kernels cannot represent, and the device lifting
reductions, run on CPU tensors, equal the NumPy ones."""
import functools
import math

import numpy as np
import pytest

import colour_models as cm
from oracle import oracle

RAGGED_SIZES = {'F_above_V': dict(n_small=3000, n_fac=4000), 'V_above_F': dict(n_small=5000, n_fac=3000)}


@pytest.mark.parametrize('size', sorted(RAGGED_SIZES))
@pytest.mark.parametrize('seed', [0, 1])
def test_ragged_covers_the_degrees_and_arities(size, seed):
    flat, sym, rv0, f0 = cm.ragged(seed, **RAGGED_SIZES[size])
    deg = np.diff(flat.var_ptr)
    H = len(cm.HUBS)
    np.testing.assert_array_equal(deg[:H], cm.HUBS)
    np.testing.assert_array_equal(deg[H:2 * H], cm.HUBS)        # the hubs' twins
    assert set(deg.tolist()) >= {0, 1, 63, 64, 65, 127, 128, 129, 300}
    assert (deg[-cm.N_ISOLATED:] == 0).all() and (deg[-cm.N_ISOLATED - cm.N_SINGLE:-cm.N_ISOLATED] == 1).all()
    assert deg[2 * H:].max() < 63                                # the hubs alone sit on the threshold
    arity = np.diff(flat.fac_ptr)
    assert set(arity.tolist()) == {1, 2, 3, 4, 5, 6}
    scopes = cm.scopes_of(flat)
    repeated = [s for s in scopes if len(set(s)) < len(s)]
    assert repeated and any(s.count(h) == 2 for s in repeated for h in range(len(cm.HUBS)))
    assert any(len(set(s)) < len(s) and min(s) >= 2 * H for s in scopes)      # ... and among the small variables
    # the workspace is carved for max(V, F): one size each way, neither a multiple of the block
    assert (flat.F > flat.V) == (size == 'F_above_V') and flat.V != flat.F
    assert flat.V % 256 and flat.F % 256
    np.testing.assert_array_equal(sym, f0 % 2)
    assert set(rv0.tolist()) == {0, 1, 2} and set(f0.tolist()) == {0, 1, 2, 3}
    # symmetric factors of every arity the sort network handles, and non-symmetric ones
    assert set(arity[sym == 1].tolist()) == {1, 2, 3, 4, 5, 6} == set(arity[sym == 0].tolist())
    # hub and twin: one colour after every half round of the oracle, from rows that list the same factor colours in another order
    r, f = rv0, f0
    for _ in range(4):
        f, _ = oracle.refine_factors(flat, sym, r, f)
        r, n_rv = oracle.refine_rvs(flat, f, r)
        np.testing.assert_array_equal(r[:H], r[H:2 * H])
        for h in range(H):
            row = lambda v: f[flat.edge_fac[flat.var_edge[flat.var_ptr[v]:flat.var_ptr[v + 1]]]].tolist()
            assert sorted(row(h)) == sorted(row(H + h)) and (row(h) != row(H + h) or len(set(row(h))) == 1)
    assert sum(row(h) != row(H + h) for h in range(H)) >= H - 1
    assert n_rv < flat.V                                         # ... and not because everything is a cluster of one


def test_single_variable_graph():
    flat, sym, rv0, f0 = cm.single()
    assert (flat.V, flat.F, flat.E) == (1, 1, 1)
    rvc, fc = oracle.color_passing(flat, sym, rv0, f0)
    assert rvc.tolist() == [0] and fc.tolist() == [0]


@functools.lru_cache(maxsize=None)
def _copies_case(size):
    base = cm.ragged(0, **RAGGED_SIZES[size])
    return base, cm.copies(*base, c=3, seed=5)


@pytest.mark.parametrize('size', sorted(RAGGED_SIZES))
def test_copies_share_colours_under_the_oracle(size):
    """every copy gets the colours of copy 0 through the permutation tables, and the partition of copy 0 is the base graph's"""
    (flat, sym, rv0, f0), (cflat, csym, crv0, cf0, vperm, fperm) = _copies_case(size)
    assert (cflat.V, cflat.F, cflat.E) == (3 * flat.V, 3 * flat.F, 3 * flat.E)
    assert sorted(vperm.ravel().tolist()) == list(range(cflat.V)) and sorted(fperm.ravel().tolist()) == list(range(cflat.F))
    # the symmetric scopes really were shuffled, the others kept
    base, moved = cm.scopes_of(flat), cm.scopes_of(cflat)
    shuffled = 0
    for f, s in enumerate(base):
        image = vperm[1, s].tolist()
        if sym[f]:
            assert sorted(moved[fperm[1, f]]) == sorted(image)
            shuffled += moved[fperm[1, f]] != image
        else:
            assert moved[fperm[1, f]] == image
    assert shuffled > 100
    rvc, fc = oracle.color_passing(cflat, csym, crv0, cf0)
    brv, bf = oracle.color_passing(flat, sym, rv0, f0)
    for k in range(1, 3):
        np.testing.assert_array_equal(rvc[vperm[k]], rvc[vperm[0]])
        np.testing.assert_array_equal(fc[fperm[k]], fc[fperm[0]])
    assert oracle.canonical_labels(rvc[vperm[0]]) == oracle.canonical_labels(brv)
    assert oracle.canonical_labels(fc[fperm[0]]) == oracle.canonical_labels(bf)
    assert (np.bincount(rvc) % 3 == 0).all() and (np.bincount(fc) % 3 == 0).all()
    # the refinement has something to do: several rounds, and clusters of more than one base member remain
    assert np.unique(brv).size < flat.V and np.unique(bf).size < flat.F


@pytest.mark.parametrize('a', [2, 3, 4, 5, 6])
@pytest.mark.parametrize('symmetric', [True, False])
@pytest.mark.parametrize('multisets', [('distinct',), ('repeated',), ('repeated', 'top')])
def test_sort_network_case_counts(a, symmetric, multisets):
    flat, sym, rv0, f0, expected = cm.sort_network_case(a, symmetric, multisets)
    assert (np.diff(flat.fac_ptr) == a).all()
    ms = cm.sort_multisets(a)
    n_perm = sum(math.factorial(a) // math.prod(math.factorial(ms[m].count(x)) for x in set(ms[m])) for m in multisets)
    assert flat.F == n_perm
    if multisets == ('distinct',):
        assert n_perm == [2, 6, 24, 120, 720][a - 2]
    if multisets == ('repeated',):
        assert n_perm == [1, 3, 12, 60, 360][a - 2]
    assert expected == (len(multisets) if symmetric else n_perm)
    fc, n = oracle.refine_factors(flat, sym, rv0, f0)
    assert n == expected == np.unique(fc).size


def test_build_flat_refuses_arity_above_the_maximum():
    """a 7-ary factor given as arrays: ``factor_sig`` would hash its first LHVI_MAX_ARITY colours only and merge two different
    factors; ``build_flat`` raises like ``flatten`` does"""
    from lhvi import potentials as P
    from lhvi.flat import build_flat
    from lhvi.graph import Domain
    dom = Domain((-1, 1), continuous=True, integral_points=np.linspace(-1, 1, 4))

    def make(arity):
        return build_flat([0, arity, arity + 1], list(range(arity)) + [0], [0, 0], [(P.POT_X2, [1.0, 4.0])], np.full(8, np.nan),
                          np.zeros(8, dtype=np.int32), [dom])
    assert make(P.MAX_ARITY).F == 2
    with pytest.raises(NotImplementedError) as err:
        make(P.MAX_ARITY + 1)
    assert str(err.value) == 'factor arity %d exceeds LHVI_MAX_ARITY=%d' % (P.MAX_ARITY + 1, P.MAX_ARITY)


def _lift_cases():
    return {'copies': cm.copies_lift_case, 'rgm': cm.rgm_lift_case}


@functools.lru_cache(maxsize=None)
def lift_case(name):
    """(flat, sym, rv0, f0, big, oracle rv colours, oracle factor colours)"""
    flat, sym, rv0, f0, big = _lift_cases()[name]()
    rvc, fc = oracle.color_passing(flat, sym, rv0, f0)
    return flat, sym, rv0, f0, big, rvc, fc


def check_big_cluster(flat, rv0, big, rvc):
    """the members of the initial colour `big` are one cluster of at least 300 observed variables whose values include +-1e16"""
    members = np.flatnonzero(rv0 == big)
    assert members.size >= 300 and np.unique(rvc[members]).size == 1
    assert (rvc == rvc[members[0]]).sum() == members.size
    vals = flat.var_value[members]
    assert not np.isnan(vals).any() and (vals == 1e16).any() and (vals == -1e16).any() and (vals == 1.0).any()
    # the order of the additions shows: the running sum differs from the sum of the sorted values
    run = 0.0
    for x in vals.tolist():
        run += x
    back = 0.0
    for x in vals[::-1].tolist():
        back += x
    assert run != back
    return run / members.size


def assert_reductions_equal(got, want):
    assert (got['nV'], got['nF']) == (want['nV'], want['nF'])
    for name in ('rep_v', 'rep_f', 'mult_v', 'mult_f'):
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)
    assert np.asarray(got['val'], dtype=np.float64).tobytes() == np.asarray(want['val'], dtype=np.float64).tobytes()
    for i, name in enumerate(('pair keys', 'first slots', 'pair counts')):
        np.testing.assert_array_equal(got['pairs'][i], want['pairs'][i], err_msg=name)


@pytest.mark.parametrize('name', ['copies', 'rgm'])
def test_lift_reductions_on_cpu_tensors_equal_the_numpy_ones(name):
    import torch
    from lhvi import lifting
    flat, sym, rv0, f0, big, rvc, fc = lift_case(name)
    mean = check_big_cluster(flat, rv0, big, rvc)
    obs = ~np.isnan(flat.var_value)
    assert set(flat.var_value[obs & (rv0 != big)].tolist()) == set(cm.POOL)
    want = lifting._lift_reduce_host(flat, rvc, fc)
    assert want['val'][rvc[np.flatnonzero(rv0 == big)[0]]] == mean
    got = lifting._lift_reduce_device(flat, lifting.TensorGraph(flat), torch.from_numpy(rvc), torch.from_numpy(fc))
    assert_reductions_equal(got, want)
    edges = np.arange(0, flat.E, 7)
    np.testing.assert_array_equal(got['color_of_edge_var'](edges), want['color_of_edge_var'](edges))
    # clusters of one, of a few and of hundreds of observed members in one call
    sizes = np.bincount(rvc[obs])
    assert (sizes == 1).any() and ((sizes > 1) & (sizes < 256)).any() and (sizes >= 300).any()
    # the partition is stable: the lifted graph can be built from it, and its counts add up to the ground degrees
    lf = lifting.lift_flat(flat, rvc, fc)
    owner = np.repeat(np.arange(lf.V), np.diff(lf.var_ptr))
    N = np.bincount(owner, weights=lf.edge_count[lf.var_edge], minlength=lf.V)
    np.testing.assert_array_equal(N, np.diff(flat.var_ptr)[want['rep_v']])
    assert float((lf.var_mult * N).sum()) == flat.E


def test_wave_level_cases():
    """the shapes tests/test_gpu_colour.py feeds to ``segment_sums`` and ``first_members``"""
    values, lengths = cm.segment_case()
    assert set(lengths.tolist()) == set(cm.SEG_LENGTHS) and lengths.size == 5 * 64 + 37 and values.size == lengths.sum()
    for w, (first, last) in enumerate(((256, 1000), (257, 511), (512, 513))):
        seg = lengths[64 * w:64 * w + 64]
        assert (seg[0], seg[63]) == (first, last) and seg[1:63].max() < 256
    mixed = lengths[192:256]
    assert ((mixed >= 256)[1:63]).any() and (mixed < 256).any()
    assert lengths[256:320].max() < 256 and lengths[-1] == 257
    seg_of = np.repeat(np.arange(lengths.size), lengths)
    want = np.zeros(lengths.size)
    np.add.at(want, seg_of, values)
    for s in (0, 63, 64, 127, 128, 191, lengths.size - 1):          # np.add.at is the running sum
        run = 0.0
        for x in values[seg_of == s].tolist():
            run += x
        assert run == want[s]
    tree = np.array([values[seg_of == s].sum() for s in range(lengths.size)])         # (pairwise: another order of additions)
    assert (tree != want).sum() > 20
    names = [name for name, _, _ in cm.first_member_cases()]
    assert len(names) == len(set(names)) == 4 * 3 + 2
    for name, col, n_colors in cm.first_member_cases():
        assert col.min() >= 0 and col.max() < n_colors
        if name.startswith('straddle'):
            assert np.flatnonzero(col == 63).tolist() == [63, 64]
        if name.startswith('distinct64') and col.size >= 64:
            assert np.unique(col[:64]).size == 64


def test_rgm_hub_case_sits_on_the_hub_threshold():
    flat, sym, rv0, f0 = cm.rgm_hub_case()
    deg = np.diff(flat.var_ptr)
    assert {64, 65} <= set(deg.tolist()) and set(deg.tolist()) == {2, 64, 65}
