"""CPU tests of nonparametric variational inference (lhvi/npvi.py, csrc/npvi.hpp through ``lhvi_npvi_grad_host`` /
``lhvi_npvi_run_host``): the torch twin of tests/npvi_models.py reaches the analytic optimum of a Gaussian MRF at K = 1, the host
twin of the kernels gives the twin's objective, autograd gradients and Adam trajectory, the lifted solver equals the ground one,
argument errors.  tests/test_gpu_npvi.py repeats the comparisons on the device."""
import numpy as np
import pytest

import npvi_models as nm
from npvi_models import assert_close, param_diff
from lhvi import _abi
from lhvi.npvi import NPVI, LiftedNPVI

GRAD_TOL = 1e-9         # of each array's largest absolute entry: fp64, two summation orders
# the largest parameter difference between 20 updates of lhvi_npvi_run_host and of the twin's hand-written Adam measured on the
# CPU (test_run_host_follows_the_twins_adam prints it): 1.44e-15; the test asserts 100 times that
RUN_MEASURED = 1.44e-15
RUN_TOL = 100 * RUN_MEASURED

OPTIMUM_SEED = 1        # of the random start of the K = 1 optimum tests (this file and tests/test_gpu_npvi.py)

GRAPHS = {
    'chain': lambda: (nm.gaussian_chain(), {}),
    'hybrid': lambda: (nm.hybrid_graph(), {}),
    'observed_args': lambda: (nm.hybrid_graph(observe=True), {}),
    'arity3': lambda: (nm.arity3_graph(), {}),
    'observed_factor': lambda: (nm.observed_factor_graph(), {}),
    'counts': lambda: (nm.hybrid_graph(seed=5), 'counts'),
    'interpreted': lambda: (nm.interpreted_graph(), {}),
    'high_arity': lambda: (nm.high_arity_graph(), {}),
}
# what selects the factor kernel's interpreter / arity-6 build (csrc/npvi.hip): the cases above must reach it
GENERAL_BUILD = {'interpreted': lambda s: s._host_struct() and s._hg.p.interpreted > 0 and s.max_arity == 4,
                 'high_arity': lambda s: s.max_arity == 6}
CASES = [(name, K, T) for name in GRAPHS for K in (1, 2, 3) for T in (1, 3, 5)] + [('arity3', 16, T) for T in (1, 3, 5)]


def build(name, K, T):
    g, kw = GRAPHS[name]()
    if kw == 'counts':
        rng = np.random.RandomState(7)
        kw = dict(var_count=rng.randint(1, 5, size=len(g.rvs)).astype(float), fac_count=rng.randint(1, 4, size=len(g.factors)).astype(float))
    tw = nm.Twin(g, K, T, **kw)
    s = NPVI(g, K, T, **kw)
    return g, tw, s


def compare_grad(s, tw, host, tol=GRAD_TOL):
    want = tw.obj_and_grads()
    got = s.grad(host=host)
    assert np.isfinite(want[0]) and np.isfinite(got[0])
    assert abs(got[0] - want[0]) <= tol * max(abs(want[0]), 1.0), ('obj', got[0], want[0])
    for name, a, b in zip(('g_tau', 'g_c', 'g_rho'), got[1:], want[1:]):
        if np.max(np.abs(b)) == 0.0:
            assert np.max(np.abs(a)) == 0.0, name
        else:
            assert_close(a, b, tol, name)


def test_twin_reaches_the_gaussian_optimum():
    """K = 1 on a dense Gaussian MRF: three-point quadrature is exact for the degree-4 integrands and the Jensen bound differs from
    the Gaussian entropy by a constant, so the optimum is mean J^-1 h, variances 1 / J_ii"""
    g, J, h = nm.dense_gaussian_mrf(4)
    tw = nm.Twin(g, 1, 3, Var_bds=[1e-3, 100])
    tw.set_params(*nm.start_params(tw, OPTIMUM_SEED))
    for _ in range(3000):
        tw.adam_step(0.05, False)
    np.testing.assert_allclose(tw.Mu.detach().numpy()[:, 0], np.linalg.solve(J, h), rtol=0, atol=1e-8)
    np.testing.assert_allclose(np.exp(tw.lVar.detach().numpy()[:, 0]), 1 / np.diag(J), rtol=0, atol=1e-8)


@pytest.mark.parametrize('name,K,T', CASES, ids=['%s-K%d-T%d' % c for c in CASES])
def test_grad_host_against_the_twin(name, K, T):
    g, tw, s = build(name, K, T)
    if name in GENERAL_BUILD:
        assert GENERAL_BUILD[name](s)
    params = nm.start_params(tw, 11 + K + T)
    tw.set_params(*params)
    s.set_params(*params)
    compare_grad(s, tw, host=True)


def run_case():
    g = nm.hybrid_graph(seed=8)
    tw, s = nm.Twin(g, 3, 3), NPVI(g, 3, 3)
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
    s2 = NPVI(g, 3, 3)
    s2.set_params(*params)
    s2.run(its=5, lr=0.05, fix_mix_its='all', host=True)
    assert np.all(s2._h['tau'] == 0.0) and np.all(s2._h['m_tau'] != 0.0)        # ... reset while fixed, the moments keep running


def symmetric_rgm():
    """three exchangeable continuous variables tied to one template variable, one evidence value: colour passing puts the
    three in one cluster"""
    from lhvi.graph import RV, F
    from lhvi.potentials import QuadraticPotential
    dom = nm.cdom()                     # one domain object: colour passing starts from domain identity
    hub, ev = RV(dom), RV(dom, value=0.3)
    leaves = [RV(dom) for _ in range(3)]
    pair = QuadraticPotential(np.array([[-0.5, 0.3], [0.3, -0.6]]), np.array([0.1, -0.2]), 0.0)
    unary = QuadraticPotential(np.array([[-0.4]]), np.array([0.2]), 0.0)
    fs = [F(pair, nb=[hub, x]) for x in leaves] + [F(unary, nb=[x]) for x in leaves] + [F(pair, nb=[ev, hub])]
    return nm._graph([hub, ev] + leaves, fs)


def test_lifted_against_ground():
    g = symmetric_rgm()
    K, T = 2, 3
    ground = NPVI(g, K, T)
    from lhvi.lifting import CompressedGraph
    cg = CompressedGraph(g)             # (colour passing itself runs on the device: inject the partition it finds)
    cg.set_colors([0, 1, 2, 2, 2], [0, 0, 0, 1, 1, 1, 2])
    lifted = LiftedNPVI(cg, K, T)
    lf, gf = lifted.flat, ground.flat
    assert lf.V < gf.V and lf.lifted
    member = np.array([lifted._var_index(rv) for rv in gf.rvs])          # cluster row of every ground row
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
    assert_close(gl_c, summed, 1e-9, 'g_c')
    # tied parameters stay tied.  A cluster's gradient is its members' times the cluster size, and Adam's step m / (sqrt(v) + eps)
    # is invariant to that scale only without eps (with 1e-8 the two runs drift apart by lr eps / |g| per update: 1e-6 here), so
    # the comparison runs with eps = 0
    lifted.adam_eps = ground.adam_eps = 0.0
    lifted.run(its=10, lr=0.05, host=True)
    ground.run(its=10, lr=0.05, host=True)
    hid = gf.var_hidden
    print('lifted against ground after 10 updates: %.3g' % np.max(np.abs(ground._h['theta_c'][hid] - lifted._h['theta_c'][member][hid])))
    np.testing.assert_allclose(ground._h['theta_c'][hid], lifted._h['theta_c'][member][hid], rtol=0, atol=1e-9)
    np.testing.assert_allclose(ground._h['tau'], lifted._h['tau'], rtol=0, atol=1e-9)
    for rv in np.array(gf.rvs, dtype=object)[hid]:
        np.testing.assert_array_equal(rv.cluster.belief_params['mu'], lifted._h['eta_c'][lifted._var_index(rv), :, 0])


def test_argument_errors_and_run_shape():
    g = nm.hybrid_graph()
    with pytest.raises(ValueError):
        NPVI(g, 0, 3)
    with pytest.raises(ValueError):
        NPVI(g, _abi.NPVI_MAX_K + 1, 3)
    with pytest.raises(ValueError):
        NPVI(g, 2, 0)
    with pytest.raises(ValueError):
        NPVI(g, 2, 13)                  # 1 discrete + 2 continuous arguments: 2 + 26 slots
    s = NPVI(g, 2, 3, seed=5)
    l, p = _abi.lib(), s._host_struct()
    out = [np.zeros(1), np.zeros(2), np.zeros((s.flat.V, 2, 2)), np.zeros((s.flat.V, 2, s.Dmax))]
    ptrs = [a.ctypes.data for a in out]
    call = lambda q, ps=ptrs: l.lhvi_npvi_grad_host(s._hg.g, s._hg.p, q, None, None, *ps)
    assert call(p) == 0
    for field, bad in (('K', 0), ('K', 17), ('T', 0), ('w', None), ('eta_c', None), ('edge_axis', None), ('gh_x', None)):
        q = s._host_struct()
        setattr(q, field, bad)
        assert call(q) == -1, field
    assert call(p, [None] + ptrs[1:]) == -1
    res = s.run(its=4, lr=0.05, host=True)
    assert sorted(res) == ['Mu', 'Pi', 'Rho', 'Var', 'record', 'w']
    assert len(res['record']['obj']) == 4 and np.all(np.isfinite(res['record']['obj']))
    V = s.flat.V
    assert res['w'].shape == (2,) and res['Mu'].shape == (V, 2) and res['Var'].shape == (V, 2) and res['Pi'].shape == (V, 2, s.Dmax)
    assert abs(res['w'].sum() - 1) < 1e-12
    same = NPVI(g, 2, 3, seed=5)
    np.testing.assert_array_equal(same._h['theta_c'], NPVI(g, 2, 3, seed=5)._h['theta_c'])
    for v, rv in enumerate(s.flat.rvs):
        if rv.value is None and rv.domain.continuous:
            np.testing.assert_array_equal(rv.belief_params['var'], res['Var'][v])
        elif rv.value is None:
            np.testing.assert_allclose(rv.belief_params['pi'].sum(axis=1), 1.0, rtol=1e-12)


def test_compat_module_resolves_the_reference_names():
    import importlib
    import os
    import sys
    compat = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'lifted-hybrid-variational-inference_amd', 'compat')
    sys.path.insert(0, compat)
    try:
        mod = importlib.import_module('osi.NPVI')
    finally:
        sys.path.remove(compat)
    assert mod.NPVI is NPVI and mod.LiftedNPVI is LiftedNPVI


def test_belief_is_the_normal_mixture_that_was_fitted():
    """``belief`` / ``map_rows`` evaluate normal densities (not ``VarInference.norm_pdf``, which divides by the variance), and the view
    handed to the device queries says so"""
    g = nm.hybrid_graph(seed=8)
    s = NPVI(g, 3, 3, seed=4)
    s.run(its=5, lr=0.05, host=True)
    assert s.belief_normaliser == 'gaussian' and s._host_struct().quirks == _abi.VI_GAUSSIAN_PDF
    x = 0.37
    for v in np.flatnonzero(s._cont):
        mu, var = s._h['eta_c'][v, :, 0], s._h['eta_c'][v, :, 1]
        want = float(np.sum(s.w * np.exp(-(x - mu) ** 2 / (2 * var)) / np.sqrt(2 * np.pi * var)))
        assert abs(s.belief(x, s.flat.rvs[v]) - want) <= 1e-9 * want       # (2.506628274631 for sqrt(2 pi), as the kernels have it)
        xm = s.map_rows()[v]
        f = lambda t: float(np.sum(s.w * np.exp(-(t - mu) ** 2 / (2 * var)) / np.sqrt(2 * np.pi * var)))
        assert f(xm) >= f(xm + 1e-4) and f(xm) >= f(xm - 1e-4)
