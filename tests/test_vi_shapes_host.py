"""CPU side of the variational kernels' shape tests (tests/vi_shapes.py): the C oracle that judges the device kernels in
tests/test_gpu_vi_shapes.py is itself held against a plain longdouble NumPy reference at arity 6, K up to 8 and T up to 9, and the
host split ``vi.factor_lists`` is pinned on every constructed threshold and on the random case table."""
import numpy as np
import pytest

import vi_shapes as S


def _distance(got, want):
    """max |got - want| over the quantity, relative to its largest entry (at least 1: g_w is identically zero at K = 1)"""
    got, want = np.asarray(got, dtype=np.longdouble), np.asarray(want, dtype=np.longdouble)
    return float(np.max(np.abs(got - want)) / max(1.0, float(np.max(np.abs(want)))))


# 8 x the largest distance measured over SMALL_CASES when the test was written (see the docstring below)
ORACLE_BOUND = dict(fe=8 * 6.3e-15, g_w=8 * 4.1e-15, g_c=8 * 2.3e-15, g_d=8 * 4.2e-15)


@pytest.mark.parametrize('seed,K,T', S.SMALL_CASES)
def test_oracle_matches_the_longdouble_reference_on_wide_graphs(seed, K, T):
    """``ViOracle.grad()`` (oracle/c/vi_oracle.c, quirks = 0) against ``vi_shapes.reference_grad`` -- the same step in np.longdouble,
    potentials through the host classes -- on small wide graphs (15 variables, 30 factors: arity up to 6, a hidden 8-state
    variable, a Gaussian observation, a scope that names a variable twice) at (K, T) = (4, 6), (8, 2), (1, 9).  This is the
    oracle's footing beyond the fixtures' K <= 3, T = 3; the quirks-on branch stays pinned by the fixtures alone
    (tests/test_oracle_vi.py).

    Distance = max |oracle - reference| / max(1, max |reference|) per quantity.  Measured when written, largest of the three
    cases: fe 6.3e-15, g_w 4.1e-15, g_c 2.3e-15, g_d 4.2e-15 (float64 rounding of sums of a few thousand terms; none near the 1e-10
    that would call the oracle into question).  Each bound is 8 x that."""
    from oracle import oracle
    flat, obs_var, (w_tau, eta_c, tau_d) = S.wide_case(seed, K, T, False, 'large', n_rv=15, n_f=30, n_repeat=1)
    arity = np.diff(flat.fac_ptr)
    scopes = [flat.edge_var[flat.fac_ptr[f]:flat.fac_ptr[f + 1]] for f in range(flat.F)]
    assert arity.max() == 6 and (obs_var > 0).any() and sum(len(set(s)) < len(s) for s in scopes) == 1
    assert (flat.var_hidden & ~flat.var_cont & (flat.var_nstates == 8)).any()
    o = oracle.ViOracle(flat, K, T, quirks=0, obs_var=obs_var)
    o.set_params(w_tau, eta_c, tau_d)
    g_w, g_c, g_d, fe = o.grad()
    r_w, r_c, r_d, r_fe = S.reference_grad(flat, K, T, o.w, o.eta_c, o.eta_d, obs_var)
    assert np.isfinite(fe) and np.abs(g_c).max() > 0.1 and np.abs(g_d).max() > 0.1
    dist = dict(fe=_distance(fe, r_fe), g_w=_distance(g_w, r_w), g_c=_distance(g_c, r_c), g_d=_distance(g_d, r_d))
    print('oracle against the longdouble reference, seed %d K %d T %d: %s' % (seed, K, T, dist))
    for what, d in dist.items():
        assert d <= ORACLE_BOUND[what], (what, d)


def _segments(flat, obs_var, K, T):
    from lhvi.vi import factor_lists
    order, counts, _ = factor_lists(flat, K, T, obs_var, tiny_kernel='always')
    assert sorted(order.tolist()) == list(range(flat.F)) and sum(counts) == flat.F
    return S.segment_of(order, counts), counts


@pytest.mark.parametrize('table_words', ['slim', 'mid'])
def test_factor_lists_on_the_tiny_kernel_thresholds(table_words):
    """``vi.factor_lists`` on vi_shapes.boundary_tiny_graph(): 32 grid nodes against 40, K = 2 against 3, scopes that name a
    variable twice in the tiny, group and thread-per-factor segments, the parameter table on either side of VI_TINY_PAR_SLIM"""
    from lhvi import _abi
    flat, obs_var, names, hubs = S.boundary_tiny_graph(table_words)
    lo, hi = S.TABLE_WORDS[table_words]
    assert lo < S.device_words(flat, obs_var) <= hi and _abi.device_potentials(flat, obs_var)[2] == 0
    assert (lo, hi) == ((0, 1024), (1024, _abi.VI_TINY_PAR))[table_words == 'mid']
    degree = np.diff(flat.var_ptr)
    assert {key: int(degree[v]) for key, v in hubs.items()} == {('d', 64): 64, ('d', 65): 65, ('c', 64): 64, ('c', 65): 65}
    assert int((degree > _abi.HUB_DEGREE).sum()) == 2
    for v in hubs.values():
        assert flat.var_hidden[v]
    seen = set()
    for (K, T), expect in S.BOUNDARY_TINY_EXPECT.items():
        seg, counts = _segments(flat, obs_var, K, T)
        got = {name: int(seg[names[name]]) for name in expect}
        assert got == expect, (K, T, {n: S.SEGMENTS[s] for n, s in got.items()})
        assert counts[S.CC] == 65 and (counts[S.TINY] > 0) == (K <= 2)
        seen |= {(name[:2] == 'r5' or name, S.SEGMENTS[s]) for name, s in got.items() if name.startswith('r')}
    # a repeated variable reaches the tiny, both group and both thread-per-factor segments
    assert {s for _, s in seen} == {'tiny', 'grp3', 'grp6', 'rest3', 'rest6'}


def test_factor_lists_on_the_group_kernel_thresholds():
    """``vi.factor_lists`` on vi_shapes.boundary_group_graph(): S = 24 against 25 at K = 1, K * S = 48 against 51 at K = 3, 48
    against 64 at K = 16, 48 against 72 at K = 24; no tiny segment above VI_TINY_PAR words although some grids have 32 nodes"""
    from lhvi import _abi
    for (K, T), expect in S.BOUNDARY_GROUP_EXPECT.items():
        flat, obs_var, names = S.boundary_group_graph(big=K <= 3)
        assert S.device_words(flat, obs_var) > _abi.VI_TINY_PAR
        seg, counts = _segments(flat, obs_var, K, T)
        got = {name: int(seg[names[name]]) for name in expect}
        assert got == expect, (K, T, {n: S.SEGMENTS[s] for n, s in got.items()})
        assert counts[S.TINY] == 0 and len(expect) == flat.F
    # the same factors on the thresholds of the constants themselves
    assert (_abi.VI_GROUP_SLOTS, _abi.VI_GROUP_COMP, _abi.VI_TINY_NODES, _abi.VI_TINY_K) == (24, 48, 32, 2)


@pytest.mark.parametrize('case,segments', S.WIDE_CASES)
def test_wide_case_table_fills_its_segments_and_the_oracle_is_finite(case, segments):
    """every case of the GPU module's table, on the CPU: the segments it is there for hold factors, and the oracle's outputs are
    finite (an overflowing formula is no valid input: the device kernels never form exp(w * formula))"""
    from oracle import oracle
    seed, K, T, quirks, table_words = case
    flat, obs_var, (w_tau, eta_c, tau_d) = S.wide_case(*case)
    arity = np.diff(flat.fac_ptr)
    assert arity.max() == 6 or table_words == 'slim'            # (slim: most six-argument rows are over the budget of a row)
    assert arity.max() >= 4 and arity.min() == 1
    _, counts = _segments(flat, obs_var, K, T)
    assert ' '.join(name for name, c in zip(S.SEGMENTS, counts) if c) == segments, counts
    o = oracle.ViOracle(flat, K, T, quirks=1 if quirks else 0, obs_var=obs_var)
    o.set_params(w_tau, eta_c, tau_d)
    g_w, g_c, g_d, fe = o.grad()
    assert np.isfinite(fe) and np.isfinite(g_w).all() and np.isfinite(g_c).all() and np.isfinite(g_d).all()


def test_wide_case_table_covers_what_it_is_for():
    """K in {1, 2, 3, 4, 8, 16}, T in {1, 2, 3, 4, 6, 9}, both quirk settings, the three table sizes; every segment in at least two
    cases; the pairwise continuous kernel with a list at T >= 6; the tiny kernel only at K <= 2"""
    cases = [c for c, _ in S.WIDE_CASES]
    assert {c[1] for c in cases} == {1, 2, 3, 4, 8, 16} and {c[2] for c in cases} == {1, 2, 3, 4, 6, 9}
    assert {c[3] for c in cases} == {True, False} and {c[4] for c in cases} == {'slim', 'mid', 'large'}
    for name in S.SEGMENTS:
        assert sum(name in segs.split() for _, segs in S.WIDE_CASES) >= 2, name
    assert any(c[2] >= 6 and 'cc' in segs.split() for c, segs in S.WIDE_CASES)
    assert all(c[1] <= 2 for c, segs in S.WIDE_CASES if 'tiny' in segs.split())
