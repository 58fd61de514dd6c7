"""CPU tests of OneShot (lhvi/oneshot.py, csrc/oneshot.hpp and csrc/npvi.hpp through ``lhvi_oneshot_grad_host`` /
``lhvi_oneshot_run_host``): the torch twin of tests/oneshot_models.py has the closed-form mean-field free energy and gradient of a
Gaussian MRF at K = 1 and reaches its optimum, the host twin of the kernels gives the twin's objective, autograd gradients and Adam
trajectory, the lifted solver equals the ground one (which pins the degree of a cluster), argument errors, the interface.
tests/test_gpu_oneshot.py repeats the comparisons on the device."""
import numpy as np
import pytest

import npvi_models as nm
from npvi_models import assert_close, param_diff
import oneshot_models as om
from lhvi import _abi
from lhvi.oneshot import OneShot, LiftedOneShot

GRAD_TOL = 1e-9         # of each array's largest absolute entry: fp64, two summation orders
# the largest parameter difference between 20 updates of lhvi_oneshot_run_host and of the twin's hand-written Adam measured on the
# CPU (test_run_host_follows_the_twins_adam prints it): 8.88e-16; the test asserts 100 times that
RUN_MEASURED = 8.88e-16
RUN_TOL = 100 * RUN_MEASURED

OPTIMUM_SEED = 1        # of the random start of the K = 1 optimum tests (this file and tests/test_gpu_oneshot.py)

GRAPHS = {
    'chain': lambda: (nm.gaussian_chain(), {}),
    'hybrid': lambda: (nm.hybrid_graph(), {}),
    'observed_args': lambda: (nm.hybrid_graph(observe=True), {}),
    'arity3': lambda: (nm.arity3_graph(), {}),
    'observed_factor': lambda: (nm.observed_factor_graph(), {}),
    'counts': lambda: (nm.hybrid_graph(seed=5), 'counts'),
    'interpreted': lambda: (nm.interpreted_graph(), {}),
    'high_arity': lambda: (nm.high_arity_graph(), {}),
    'degree': lambda: (om.degree_graph(), 'counts'),            # kappa = 0 rows next to kappa = -2 c_v
    'isolated': lambda: (om.isolated_graph(), 'counts'),        # kappa = +c_v, no edges
}
CASES = [(name, K, T) for name in GRAPHS for K in (1, 2, 3) for T in (1, 3, 5)] + [('arity3', 16, T) for T in (1, 3, 5)]


def build(name, K, T):
    g, kw = GRAPHS[name]()
    if kw == 'counts':
        rng = np.random.RandomState(7)
        kw = dict(var_count=rng.randint(2, 5, size=len(g.rvs)).astype(float), fac_count=rng.randint(1, 4, size=len(g.factors)).astype(float))
    tw = om.Twin(g, K, T, **kw)
    s = OneShot(g, K, T, **kw)
    return g, tw, s


def compare(got, want, s, tol=GRAD_TOL, nonzero=True):
    """objective and the three gradient arrays; an array that has parameters behind it (g_tau at K > 1, g_c with a hidden continuous
    row, g_rho with a hidden discrete one) must have a non-zero largest entry on both sides, the others are zero on both"""
    assert np.isfinite(want[0]) and np.isfinite(got[0])
    assert abs(got[0] - want[0]) <= tol * max(abs(want[0]), 1.0), ('obj', got[0], want[0])
    live = dict(g_tau=s.K > 1, g_c=bool(s._cont.any()), g_rho=bool(s._disc.any()))
    for name, a, b in zip(('g_tau', 'g_c', 'g_rho'), got[1:], want[1:]):
        if live[name] and nonzero:
            assert np.max(np.abs(b)) > 0.0 and np.max(np.abs(a)) > 0.0, name
        if np.max(np.abs(b)) == 0.0:
            assert np.max(np.abs(a)) == 0.0, name
        else:
            assert_close(a, b, tol, name)


def test_var_coef_is_count_times_one_minus_degree():
    g, tw, s = build('degree', 2, 3)
    deg = np.array([len(rv.nb) for rv in s.flat.rvs], dtype=float)
    assert sorted(deg) == [1, 1, 2, 3, 3]
    np.testing.assert_array_equal(s.var_coef, s.var_count * (1 - deg))
    assert (s.var_coef == 0).sum() == 2
    g, tw, s = build('isolated', 2, 3)
    lone = [v for v, rv in enumerate(s.flat.rvs) if len(rv.nb) == 0]
    assert len(lone) == 2 and np.array_equal(s.var_coef[lone], s.var_count[lone]) and s.var_count[lone].min() >= 2
    s = OneShot(nm.hybrid_graph(observe=True), 2, 3)
    assert np.all(s.var_coef[~s.flat.var_hidden] == 0.0)


def gaussian_closed_form(J, h, Mu, Var):
    """the mean-field free energy of p(x) ~ exp(-x'Jx/2 + h'x) under q = prod N(Mu_v, Var_v), and its gradient in (Mu, log Var)"""
    obj = 0.5 * Mu @ J @ Mu + 0.5 * np.diag(J) @ Var - h @ Mu - np.sum(0.5 * np.log(2 * np.pi * np.e * Var))
    return obj, J @ Mu - h, 0.5 * (np.diag(J) * Var - 1.0)


def test_closed_form_at_k1():
    """K = 1: the Bethe free energy of a product belief is the mean-field free energy, and three Gauss-Hermite nodes are exact for the
    degree-4 integrands of a quadratic energy -- a check of the twin that does not go through the twin's own formulas"""
    g, J, h = nm.dense_gaussian_mrf(4)
    tw, s = om.Twin(g, 1, 3), OneShot(g, 1, 3)
    params = nm.start_params(tw, 5)
    tw.set_params(*params)
    s.set_params(*params)
    Mu, Var = params[1][:, 0], np.exp(params[2][:, 0])
    obj, g_mu, g_lv = gaussian_closed_form(J, h, Mu, Var)
    for got in (tw.obj_and_grads(), s.grad(host=True)):
        assert abs(got[0] - obj) <= 1e-9 * abs(obj)
        np.testing.assert_allclose(got[2][:, 0, 0], g_mu, rtol=1e-9, atol=1e-9 * np.max(np.abs(g_mu)))
        np.testing.assert_allclose(got[2][:, 0, 1], g_lv, rtol=1e-9, atol=1e-9 * np.max(np.abs(g_lv)))


def test_twin_and_host_reach_the_gaussian_optimum():
    g, J, h = nm.dense_gaussian_mrf(4)
    tw = om.Twin(g, 1, 3, Var_bds=[1e-3, 100])
    s = OneShot(g, 1, 3, Var_bds=[1e-3, 100])
    params = nm.start_params(tw, OPTIMUM_SEED)
    tw.set_params(*params)
    s.set_params(*params)
    for _ in range(3000):
        tw.adam_step(0.05, False)
    np.testing.assert_allclose(tw.Mu.detach().numpy()[:, 0], np.linalg.solve(J, h), rtol=0, atol=1e-8)
    np.testing.assert_allclose(np.exp(tw.lVar.detach().numpy()[:, 0]), 1 / np.diag(J), rtol=0, atol=1e-8)
    res = s.run(its=3000, lr=0.05, host=True)
    np.testing.assert_allclose(res['Mu'][:, 0], np.linalg.solve(J, h), rtol=0, atol=1e-8)
    np.testing.assert_allclose(res['Var'][:, 0], 1 / np.diag(J), rtol=0, atol=1e-8)


@pytest.mark.parametrize('name,K,T', CASES, ids=['%s-K%d-T%d' % c for c in CASES])
def test_grad_host_against_the_twin(name, K, T):
    g, tw, s = build(name, K, T)
    params = nm.start_params(tw, 11 + K + T)
    tw.set_params(*params)
    s.set_params(*params)
    compare(s.grad(host=True), tw.obj_and_grads(), s)


def run_case():
    g = nm.hybrid_graph(seed=8)
    tw, s = om.Twin(g, 3, 3), OneShot(g, 3, 3)
    tau, Mu, lVar, Rho = nm.start_params(tw, 3)
    Mu = Mu + 6.0                       # outside the domain [-4, 4]: the clip acts
    return g, tw, s, (tau, Mu, lVar, Rho)


def test_run_host_follows_the_twins_adam():
    g, tw, s, params = run_case()
    tw.set_params(*params)
    s.set_params(*params)
    objs = [tw.adam_step(0.05, it < 5) for it in range(20)]
    res = s.run(its=20, lr=0.05, fix_mix_its=5, host=True)
    d = param_diff(s, tw)
    print('largest parameter difference after 20 updates: %.3g' % d)
    assert float(np.max(np.abs(tw.Mu.detach().numpy()[s._cont]))) <= 4.0 and float(np.max(s._h['theta_c'][s._cont][:, :, 0])) <= 4.0
    assert d <= RUN_TOL
    np.testing.assert_allclose(res['record']['obj'], objs, rtol=1e-9)
    assert np.all(s._h['tau'][:] != 0.0)            # free after the five fixed updates ...
    s2 = OneShot(g, 3, 3)
    s2.set_params(*params)
    s2.run(its=5, lr=0.05, fix_mix_its='all', host=True)
    assert np.all(s2._h['tau'] == 0.0) and np.all(s2._h['m_tau'] != 0.0)        # ... reset while fixed, the moments keep running


def test_lifted_against_ground():
    """the hub's cluster has one edge of count 3 and one of count 1 (ground degree 4), the leaves' cluster two edges of count 1: a
    cluster degree counted in cluster edges (2 for the hub) fails here"""
    g, colors = om.symmetric_rgm()
    K, T = 2, 3
    ground = OneShot(g, K, T)
    from lhvi.lifting import CompressedGraph
    cg = CompressedGraph(g)             # (colour passing itself runs on the device: inject the partition it finds)
    cg.set_colors(*colors)
    lifted = LiftedOneShot(cg, K, T)
    lf, gf = lifted.flat, ground.flat
    assert lf.V < gf.V and lf.lifted
    member = np.array([lifted._var_index(rv) for rv in gf.rvs])          # cluster row of every ground row
    np.testing.assert_array_equal(ground.var_coef, [-3.0, 0.0, -1.0, -1.0, -1.0])
    np.testing.assert_array_equal(lifted.var_coef[member], [-3.0, 0.0, -3.0, -3.0, -3.0])
    rng = np.random.RandomState(4)
    tau, Mu, lVar = rng.randn(K) * 0.3, rng.randn(lf.V, K), np.log(rng.uniform(0.3, 2.0, size=(lf.V, K)))
    lifted.set_params(tau, Mu, lVar)
    ground.set_params(tau, Mu[member], lVar[member])
    ol, gl_tau, gl_c, _ = lifted.grad(host=True)
    og, gg_tau, gg_c, _ = ground.grad(host=True)
    assert abs(ol - og) <= 1e-9 * max(abs(og), 1.0)
    assert_close(gl_tau, gg_tau, 1e-9, 'g_tau')
    summed = np.zeros_like(gl_c)
    np.add.at(summed, member, gg_c)
    assert np.max(np.abs(summed)) > 0
    assert_close(gl_c, summed, 1e-9, 'g_c')
    # the ground solver against the twin on this graph, so that the pair is not merely consistent
    tw = om.Twin(g, K, T)
    tw.set_params(tau, Mu[member], lVar[member], np.zeros((gf.V, K, 1)))
    compare((og, gg_tau, gg_c, np.zeros((gf.V, K, 1))), tw.obj_and_grads(), ground)
    # tied parameters stay tied; Adam's step is invariant to the scale of the gradient only without eps (docs/kernels_npvi.md §4)
    lifted.adam_eps = ground.adam_eps = 0.0
    ground.run(its=10, lr=0.05, host=True)
    lifted.run(its=10, lr=0.05, host=True)          # (last: the members' belief_params are then the cluster's)
    hid = gf.var_hidden
    print('lifted against ground after 10 updates: %.3g' % np.max(np.abs(ground._h['theta_c'][hid] - lifted._h['theta_c'][member][hid])))
    np.testing.assert_allclose(ground._h['theta_c'][hid], lifted._h['theta_c'][member][hid], rtol=0, atol=1e-9)
    np.testing.assert_allclose(ground._h['tau'], lifted._h['tau'], rtol=0, atol=1e-9)
    for rv in np.array(gf.rvs, dtype=object)[hid]:
        np.testing.assert_array_equal(rv.cluster.belief_params['mu'], lifted._h['eta_c'][lifted._var_index(rv), :, 0])
        np.testing.assert_array_equal(rv.belief_params['mu'], lifted._h['eta_c'][lifted._var_index(rv), :, 0])


def test_argument_errors_and_run_shape():
    g = nm.hybrid_graph()
    with pytest.raises(ValueError):
        OneShot(g, 0, 3)
    with pytest.raises(ValueError):
        OneShot(g, _abi.NPVI_MAX_K + 1, 3)
    with pytest.raises(ValueError):
        OneShot(g, 2, 0)
    with pytest.raises(ValueError):
        OneShot(g, 2, 13)               # 1 discrete + 2 continuous arguments: 2 + 26 slots
    with pytest.raises(ValueError):
        OneShot(g, 2, 3, var_count=np.ones(2))
    s = OneShot(g, 2, 3, seed=5)
    l, p = _abi.lib(), s._host_struct()
    out = [np.zeros(1), np.zeros(2), np.zeros((s.flat.V, 2, 2)), np.zeros((s.flat.V, 2, s.Dmax))]
    ptrs = [a.ctypes.data for a in out]
    coef = s.var_coef.ctypes.data
    call = lambda q, ps=ptrs, vc=coef: l.lhvi_oneshot_grad_host(s._hg.g, s._hg.p, q, None, None, vc, *ps)
    assert call(p) == 0
    for field, bad in (('K', 0), ('K', 17), ('T', 0), ('w', None), ('eta_c', None), ('edge_axis', None), ('gh_x', None)):
        q = s._host_struct()
        setattr(q, field, bad)
        assert call(q) == -1, field
    assert call(p, [None] + ptrs[1:]) == -1
    assert call(p, vc=None) == -1                   # var_coef is required
    with pytest.raises(ValueError):
        s.run(its=-1, host=True)
    res = s.run(its=4, lr=0.05, host=True)
    assert sorted(res) == ['Mu', 'Pi', 'Rho', 'Var', 'record', 'w']
    assert len(res['record']['obj']) == 4 and np.all(np.isfinite(res['record']['obj']))
    V = s.flat.V
    assert res['w'].shape == (2,) and res['Mu'].shape == (V, 2) and res['Var'].shape == (V, 2) and res['Pi'].shape == (V, 2, s.Dmax)
    assert abs(res['w'].sum() - 1) < 1e-12
    np.testing.assert_array_equal(OneShot(g, 2, 3, seed=5)._h['theta_c'], OneShot(g, 2, 3, seed=5)._h['theta_c'])
    for v, rv in enumerate(s.flat.rvs):
        if rv.value is None and rv.domain.continuous:
            np.testing.assert_array_equal(rv.belief_params['var'], res['Var'][v])
        elif rv.value is None:
            np.testing.assert_allclose(rv.belief_params['pi'].sum(axis=1), 1.0, rtol=1e-12)
    # the objective that was optimised is the Bethe free energy, not NPVI's bound: on the same parameters the two differ
    from lhvi.npvi import NPVI
    n = NPVI(g, 2, 3, seed=5)
    o = OneShot(g, 2, 3, seed=5)
    assert abs(n.grad(host=True)[0] - o.grad(host=True)[0]) > 1e-3


def test_compat_module_resolves_the_reference_names():
    import importlib
    import os
    import sys
    compat = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'lifted-hybrid-variational-inference_amd', 'compat')
    sys.path.insert(0, compat)
    try:
        mod = importlib.import_module('osi.OneShot')
    finally:
        sys.path.remove(compat)
    assert mod.OneShot is OneShot and mod.LiftedOneShot is LiftedOneShot


def test_belief_is_the_normal_mixture_that_was_fitted():
    """``belief`` / ``map_rows`` / ``map`` evaluate normal densities, and the view handed to the device queries says so"""
    g = nm.hybrid_graph(seed=8)
    s = OneShot(g, 3, 3, seed=4)
    s.run(its=5, lr=0.05, host=True)
    assert s.belief_normaliser == 'gaussian' and s._host_struct().quirks == _abi.VI_GAUSSIAN_PDF
    x = 0.37
    for v in np.flatnonzero(s._cont):
        mu, var = s._h['eta_c'][v, :, 0], s._h['eta_c'][v, :, 1]
        want = float(np.sum(s.w * np.exp(-(x - mu) ** 2 / (2 * var)) / np.sqrt(2 * np.pi * var)))
        assert abs(s.belief(x, s.flat.rvs[v]) - want) <= 1e-9 * want
        xm = s.map_rows()[v]
        f = lambda t: float(np.sum(s.w * np.exp(-(t - mu) ** 2 / (2 * var)) / np.sqrt(2 * np.pi * var)))
        assert f(xm) >= f(xm + 1e-4) and f(xm) >= f(xm - 1e-4)
    a, xr = s.flat.rvs[0], s.flat.rvs[2]
    a.value = 1
    try:
        assert s.map([xr], a) == 1                  # an observed query is its value (OneShot.py:312-326)
    finally:
        a.value = None
