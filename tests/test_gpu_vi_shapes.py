"""GPU parity: the variational expectation step (``lhvi_vi_grad``, csrc/vi.hip) against the C oracle at the shapes the fixtures and
tests/test_gpu_vi.py's random graphs leave out -- K up to 24, T from 1 to 9, arity up to 6, domains of up to 32 states, every
segment of the host's factor lists and every threshold between two kernels (tests/vi_shapes.py builds the graphs;
tests/test_vi_shapes_host.py anchors the oracle at these shapes and pins the thresholds on the CPU)."""
import numpy as np
import pytest

import vi_shapes as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def api():
    from lhvi import _abi
    _abi.require_gpu()
    return _abi


STAGES = (('tiny', True, 'always'), ('group', True, False), ('thread per factor', False, False))


def _stage(flat, obs_var, K, T, quirks, lists, tiny, **attrs):
    from lhvi import c2fvi
    owner = c2fvi.VarInference.__new__(c2fvi.VarInference)
    owner._init_common(K, T)
    owner.reference_quirks = quirks
    Stage = type('Stage', (c2fvi._DeviceStage,), dict(factor_lists=lists, tiny_kernel=tiny, **attrs))
    return Stage(owner, flat, obs_var)


def check_against_oracle(flat, obs_var, K, T, quirks, params, label=''):
    """gradient and free energy of one case through (a) the lists with the tiny-grid kernel, (b) the lists without it, (c) the
    thread-per-factor kernels without lists, against ``ViOracle.grad()`` and against each other at the bounds of
    test_gpu_vi.py::_random_hybrid_check.  Returns the stages by label; the oracle's outputs must be finite."""
    from oracle import oracle
    w_tau, eta_c, tau_d = params
    o = oracle.ViOracle(flat, K, T, quirks=1 if quirks else 0, obs_var=obs_var)
    o.set_params(w_tau, eta_c, tau_d)
    want = o.grad()
    assert np.isfinite(want[3]) and all(np.isfinite(x).all() for x in want[:3]), 'the oracle overflowed: not a valid case'
    stages, outs = {}, {}
    for name, lists, tiny in STAGES:
        st = stages[name] = _stage(flat, obs_var, K, T, quirks, lists, tiny)
        st._upload_params(w_tau, eta_c, tau_d)
        st._grad()
        outs[name] = [st._dev[k].cpu().numpy().copy() for k in ('g_w', 'g_c', 'g_d', 'fe')]
        if lists:
            print('%s K %d T %d quirks %d %s: cc %d tiny %d grp3 %d grp6 %d rest3 %d rest6 %d' % ((label, K, T, quirks, name) + tuple(st._fac_counts)))
    assert stages['thread per factor']._fac_counts is None and stages['group']._fac_counts[S.TINY] == 0
    cont, disc = flat.var_hidden & flat.var_cont, flat.var_hidden & ~flat.var_cont
    for name, (g_w, g_c, g_d, fe) in outs.items():
        np.testing.assert_allclose(fe[0], want[3], rtol=1e-9, err_msg=name)
        np.testing.assert_allclose(g_w, want[0], rtol=1e-8, atol=1e-8, err_msg=name)
        np.testing.assert_allclose(g_c[cont], want[1][cont], rtol=1e-8, atol=1e-8, err_msg=name)
        np.testing.assert_allclose(g_d[disc], want[2][disc], rtol=1e-8, atol=1e-8, err_msg=name)
    for a, b in (('tiny', 'group'), ('group', 'thread per factor')):
        for x, y, what in zip(outs[a], outs[b], ('g_w', 'g_c', 'g_d', 'fe')):
            np.testing.assert_allclose(x, y, rtol=1e-9, atol=1e-9, err_msg='%s vs %s: %s' % (a, b, what))
    return stages


def _segments_of(stage):
    order = stage._dev['fac_list'].cpu().numpy()
    return S.segment_of(order, stage._fac_counts)


@pytest.mark.parametrize('case,segments', S.WIDE_CASES)
def test_wide_random_graphs_through_every_segment(api, case, segments):
    """the wide random graphs (arity 1-6, domains of up to 8 states, Gaussian observations, scopes that name a variable twice) at K
    up to 16 and T from 1 to 9, both quirk settings, the three sizes of the parameter table: every stage against the C oracle
    and against each other; the segments the case is in the table for hold factors on the device"""
    seed, K, T, quirks, table_words = case
    flat, obs_var, params = S.wide_case(*case)
    stages = check_against_oracle(flat, obs_var, K, T, quirks, params, label='wide seed %d %s' % (seed, table_words))
    counts = stages['tiny']._fac_counts
    assert ' '.join(name for name, c in zip(S.SEGMENTS, counts) if c) == segments, counts
    lo, hi = S.TABLE_WORDS[table_words]
    assert lo < stages['tiny'].dg.pot_param_words <= hi
    if table_words == 'slim':
        assert stages['tiny'].dg.p.interpreted == 0         # the builds without the formula interpreter
    else:
        assert stages['tiny'].dg.p.interpreted > 0
    # (two of the factors name a variable twice)
    scopes = [flat.edge_var[flat.fac_ptr[f]:flat.fac_ptr[f + 1]] for f in range(flat.F)]
    assert sum(len(set(s)) < len(s) for s in scopes) == 2


@pytest.mark.parametrize('table_words', ['slim', 'mid'])
@pytest.mark.parametrize('K,T', sorted(S.BOUNDARY_TINY_EXPECT))
def test_tiny_kernel_thresholds_repeated_variables_and_hubs(api, K, T, table_words):
    """vi_shapes.boundary_tiny_graph(): factors of 32 grid nodes (a unary one over a 32-state variable: Dmax = 32) and of 40, scopes
    that name a hidden continuous or a hidden discrete variable twice, stars around hidden discrete and continuous hubs of
    degree 64 (the thread-per-variable gather) and 65 (the wavefront-per-hub gather), pairwise continuous factors at T = 1, 3, 4,
    5, 6 and 9 -- with the parameter table under VI_TINY_PAR_SLIM and above it"""
    flat, obs_var, names, hubs = S.boundary_tiny_graph(table_words)
    rng = np.random.default_rng(11)
    stages = check_against_oracle(flat, obs_var, K, T, False, S.random_params(rng, flat, K), label='tiny thresholds %s' % table_words)
    st = stages['tiny']
    seg = _segments_of(st)
    assert {name: int(seg[names[name]]) for name in S.BOUNDARY_TINY_EXPECT[K, T]} == S.BOUNDARY_TINY_EXPECT[K, T]
    assert st._fac_counts[S.CC] == 65 and (st._fac_counts[S.TINY] > 0) == (K <= 2)
    assert st.Dmax == 32 and st.dg.p.interpreted == 0
    lo, hi = S.TABLE_WORDS[table_words]
    assert lo < st.dg.pot_param_words <= hi
    assert st.dg.g.n_hubs == 2                               # the hubs of degree 65 only
    degree = np.diff(flat.var_ptr)
    assert sorted(np.flatnonzero(degree > api.HUB_DEGREE).tolist()) == sorted([hubs['d', 65], hubs['c', 65]])


@pytest.mark.parametrize('K,T', sorted(S.BOUNDARY_GROUP_EXPECT))
def test_group_kernel_thresholds(api, K, T):
    """vi_shapes.boundary_group_graph(): S = 24 (six four-state axes, 4096 nodes) against 25, K * S = 48 against 51 / 64 / 72 at
    K = 3, 16, 24 (there without the two six-argument factors); the parameter table is over VI_TINY_PAR, so the 32-node factors stay out of the tiny kernel"""
    flat, obs_var, names = S.boundary_group_graph(big=K <= 3)
    rng = np.random.default_rng(12)
    stages = check_against_oracle(flat, obs_var, K, T, False, S.random_params(rng, flat, K), label='group thresholds')
    st = stages['tiny']
    seg = _segments_of(st)
    assert {name: int(seg[names[name]]) for name in S.BOUNDARY_GROUP_EXPECT[K, T]} == S.BOUNDARY_GROUP_EXPECT[K, T]
    assert st._fac_counts[S.TINY] == 0 and st.dg.pot_param_words > api.VI_TINY_PAR


def test_fused_adam_loop_across_the_list_tails(api):
    """``lhvi_vi_adam_run`` re-enters ``lhvi_vi_grad`` with the caller's lists: five fused updates against the same five through
    the per-array calls on a wide case whose rest3 and rest6 segments hold factors (the fixtures of
    test_gpu_vi.py::test_fused_adam_loop_equals_the_per_array_calls have empty tails); the same bar"""
    case = (0, 4, 6, False, 'large')
    assert dict(S.WIDE_CASES)[case] == 'cc grp3 grp6 rest3 rest6'
    flat, obs_var, (w_tau, eta_c, tau_d) = S.wide_case(*case)
    runs = []
    for fused in (True, False):
        st = _stage(flat, obs_var, case[1], case[2], False, True, 'always', fused_loop=fused)
        assert st._fac_counts[S.REST3] > 0 and st._fac_counts[S.REST6] > 0
        st._upload_params(w_tau, eta_c, tau_d)
        fe = st.adam(5, 0, 0.15)
        assert len(fe) == 5 and np.isfinite(fe).all()
        runs.append((st, fe))
    (a, fa), (b, fb) = runs
    exact = bool(a._uniform_states or not a._has_disc)
    for key in ('w_tau', 'w', 'eta_c', 'tau_d', 'eta_d', 'm_w_tau', 's_w_tau', 'm_eta_c', 's_eta_c', 'm_tau_d', 's_tau_d'):
        x, y = a._dev[key].cpu().numpy(), b._dev[key].cpu().numpy()
        if exact:
            np.testing.assert_array_equal(x, y, err_msg=key)
        else:
            np.testing.assert_allclose(x, y, rtol=1e-11, atol=1e-13, err_msg=key)
    assert fa == fb if exact else np.allclose(fa, fb, rtol=1e-12)
    assert not np.array_equal(a._dev['eta_c'].cpu().numpy()[flat.var_hidden & flat.var_cont], eta_c[flat.var_hidden & flat.var_cont])
