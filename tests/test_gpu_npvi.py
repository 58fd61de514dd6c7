"""GPU suite of nonparametric variational inference (csrc/npvi.hip through lhvi/npvi.py): the kernels against their host twin and
against the torch twin of tests/npvi_models.py on the cases and bounds of tests/test_npvi_host.py, two launch-shape cases (a chain
that crosses the block boundary of the entropy reduction, a hub variable for the wavefront gather), the optimiser loop, the
analytic optimum at K = 1, run-to-run bits, and the queries on a fitted model."""
import functools

import numpy as np
import pytest

import npvi_models as nm
import test_npvi_host as th
from lhvi import _abi, mixture
from lhvi.mixture import MixtureBelief
from lhvi.npvi import NPVI, LiftedNPVI

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def shape_case(name):
    """(solver, twin reference) of a launch-shape case, computed once"""
    g = nm.long_chain() if name == 'chain1025' else nm.hub_graph()
    K = 2 if name == 'chain1025' else 3
    tw, s = nm.Twin(g, K, 3), NPVI(g, K, 3)
    params = nm.start_params(tw, 21, spread=0.5)
    tw.set_params(*params)
    s.set_params(*params)
    return s, tw.obj_and_grads()


def compare(got, want, tol=th.GRAD_TOL):
    assert np.isfinite(got[0]) and abs(got[0] - want[0]) <= tol * max(abs(want[0]), 1.0), ('obj', got[0], want[0])
    for name, a, b in zip(('g_tau', 'g_c', 'g_rho'), got[1:], want[1:]):
        if np.max(np.abs(b)) == 0.0:
            assert np.max(np.abs(a)) == 0.0, name
        else:
            th.assert_close(a, b, tol, name)


@pytest.mark.parametrize('name,K,T', th.CASES, ids=['%s-K%d-T%d' % c for c in th.CASES])
def test_grad_against_the_host_twin_and_the_torch_twin(name, K, T):
    g, tw, s = th.build(name, K, T)
    if name in th.GENERAL_BUILD:                # the interpreter / arity-6 build of the factor kernel is the one launched
        assert th.GENERAL_BUILD[name](s)
        s._ensure_dev()
        assert s.dg.p.interpreted > 0 or s.max_arity > 3
    params = nm.start_params(tw, 11 + K + T)
    tw.set_params(*params)
    s.set_params(*params)
    dev = s.grad()
    compare(dev, s.grad(host=True))
    compare(dev, tw.obj_and_grads())


@pytest.mark.parametrize('name', ['chain1025', 'hub70'])
def test_grad_at_the_launch_shape_edges(name):
    s, want = shape_case(name)
    if name == 'hub70':
        assert s.flat.var_ptr[1] - s.flat.var_ptr[0] == 70
    dev = s.grad()
    compare(dev, s.grad(host=True))
    compare(dev, want)


def test_run_against_the_host_run():
    """20 updates with fix_mix_its = 5 and a start outside the domain, against lhvi_npvi_run_host: the bound of
    tests/test_npvi_host.py::test_run_host_follows_the_twins_adam (100 times the difference measured there)"""
    g, tw, s, params = th.run_case()
    host = NPVI(g, 3, 3)
    s.set_params(*params)
    host.set_params(*params)
    rd = s.run(its=20, lr=0.05, fix_mix_its=5)
    rh = host.run(its=20, lr=0.05, fix_mix_its=5, host=True)
    d = max(float(np.max(np.abs(s._h[n] - host._h[n]))) for n in ('tau', 'theta_c', 'rho'))
    print('largest parameter difference between the device and the host run after 20 updates: %.3g' % d)
    assert d <= th.RUN_TOL
    np.testing.assert_allclose(rd['record']['obj'], rh['record']['obj'], rtol=1e-9)


def test_gaussian_optimum_on_the_device():
    g, J, h = nm.dense_gaussian_mrf(4)
    s = NPVI(g, 1, 3, Var_bds=[1e-3, 100])
    tw = nm.Twin(g, 1, 3)
    s.set_params(*nm.start_params(tw, th.OPTIMUM_SEED))
    res = s.run(its=3000, lr=0.05)
    print('mean error %.3g, variance error %.3g' % (np.max(np.abs(res['Mu'][:, 0] - np.linalg.solve(J, h))),
                                                    np.max(np.abs(res['Var'][:, 0] - 1 / np.diag(J)))))
    np.testing.assert_allclose(res['Mu'][:, 0], np.linalg.solve(J, h), rtol=0, atol=1e-8)
    np.testing.assert_allclose(res['Var'][:, 0], 1 / np.diag(J), rtol=0, atol=1e-8)


def test_device_entry_points_refuse_a_short_workspace_before_any_launch():
    """lhvi_npvi_grad and lhvi_npvi_run with ws_bytes one short: LHVI_E_ARG, and no array of the solver has changed"""
    s = NPVI(nm.gaussian_chain(5), 2, 3, seed=3)
    d = s._ensure_dev()
    assert d['ws_bytes'] == _abi.lib().lhvi_npvi_workspace_bytes(s.dg.g, s._struct()) > 0
    before = nm.device_bits(s)
    d['ws_bytes'] -= 1
    with pytest.raises(_abi.LhviError):
        s.grad()
    with pytest.raises(_abi.LhviError):
        s.run(its=2, lr=0.05)
    assert nm.device_bits(s) == before
    d['ws_bytes'] += 1
    assert len(s.run(its=2, lr=0.05)['record']['obj']) == 2 and s.t == 2
    assert nm.device_bits(s) != before


def fitted_hybrid(its=30):
    g = nm.hybrid_graph(seed=8)
    s = NPVI(g, 3, 3, seed=4)
    res = s.run(its=its, lr=0.05, fix_mix_its=3)
    return g, s, res


def test_two_runs_give_the_same_bits():
    _, a, ra = fitted_hybrid()
    _, b, rb = fitted_hybrid()
    assert len(ra['record']['obj']) == 30 and np.all(np.isfinite(ra['record']['obj']))
    assert ra['record']['obj'] == rb['record']['obj']
    for n in ('tau', 'theta_c', 'rho', 'w', 'eta_c', 'eta_d'):
        assert np.array_equal(a._h[n], b._h[n]), n
    s, _ = shape_case('chain1025')
    first = s.grad()
    for x, y in zip(first, s.grad()):
        assert np.array_equal(x, y)


def test_queries_on_a_fitted_model():
    g, s, res = fitted_hybrid()
    flat, K = s.flat, s.K
    belief = MixtureBelief.from_solver(s)
    assert belief.V == flat.V
    assert belief.normaliser == 'gaussian' and s.mixture_belief().normaliser == 'gaussian'
    # the marginal log beliefs of the continuous rows against the fitted mixture -- K normal densities w_k N(x; mu_k, var_k), what
    # the kernels optimised -- evaluated on the host in extended precision; each term is off by a few units of roundoff times its
    # exponent
    crow = np.flatnonzero(s._cont)
    x = np.linspace(-3.0, 3.0, 7)
    got = belief.log_belief_all(np.zeros((1, 0)), [], crow, x)[0]
    LD = np.longdouble
    mu, var, w = s._h['eta_c'][crow, :, 0].astype(LD), s._h['eta_c'][crow, :, 1].astype(LD), s._h['w'].astype(LD)
    expo = -(x[None, None, :].astype(LD) - mu[:, :, None]) ** 2 / (2 * var[:, :, None])
    want = np.log(np.sum(w[None, :, None] * np.exp(expo) / np.sqrt(2 * LD(np.pi) * var[:, :, None]), axis=1))
    bound = 4 * U * (K + 8) * (1 + np.max(np.abs(expo.astype(np.float64)), axis=1))
    assert np.all(np.abs(got - want.astype(np.float64)) <= bound + 4 * U * np.abs(want.astype(np.float64)))
    # conditioning on a discrete row: the device against the module's host side
    a, xr = flat.rvs[0], flat.rvs[2]
    cw_d, lp_d = belief.condition(np.array([[1.0]]), [belief.row(a)])
    cw_h, lp_h = belief.condition(np.array([[1.0]]), [belief.row(a)], host=True)
    np.testing.assert_allclose(cw_d, cw_h, rtol=4 * U * (K + 8), atol=0)
    np.testing.assert_allclose(lp_d, lp_h, rtol=4 * U * (K + 8), atol=0)
    # the variational MAP of every row in one launch against the host path (the bounds of tests/test_gpu_vi_map.py)
    for v in crow:                              # belief() is that mixture too
        rv = flat.rvs[v]
        assert abs(np.log(s.belief(0.5, rv)) - belief.log_belief_all(np.zeros((1, 0)), [], [v], [0.5])[0, 0, 0]) < 1e-12
    xm = s.map_rows_device()
    host = s.map_rows()
    var = s._h['eta_c'][crow, :, 1]
    assert var.max() / var.min() > 1.5          # unequal variances: the two densities have different maximisers
    for v in crow:                              # the answer is a maximum of the normal mixture (a step either way lowers it)
        f = lambda t: s._row_belief(v, t)
        assert f(xm[v]) >= f(xm[v] + 1e-4) and f(xm[v]) >= f(xm[v] - 1e-4)
    hid = flat.var_hidden
    assert np.isnan(xm[~hid]).all()
    np.testing.assert_array_equal(xm[s._disc], host[s._disc])
    np.testing.assert_allclose(xm[s._cont], host[s._cont], rtol=1e-7, atol=1e-7)
    # the reference's convenience query
    a.value = 1
    try:
        got = s.map([a], xr)
        assert got == mixture.marginal_map(np.array([1.0]), [a], xr, s.w) and -4.0 <= got <= 4.0
    finally:
        a.value = None


def test_lifted_solver_on_the_device():
    """colour passing on the device finds the clusters of the symmetric graph; the lifted objective is the ground one and the
    members carry their cluster's parameters after a run"""
    g = th.symmetric_rgm()
    ground, lifted = NPVI(g, 2, 3), LiftedNPVI(g, 2, 3)
    assert lifted.flat.V == 3 and ground.flat.V == 5
    member = np.array([lifted._var_index(rv) for rv in ground.flat.rvs])
    rng = np.random.RandomState(4)
    tau, Mu, lVar = rng.randn(2) * 0.3, rng.randn(3, 2), np.log(rng.uniform(0.3, 2.0, size=(3, 2)))
    lifted.set_params(tau, Mu, lVar)
    ground.set_params(tau, Mu[member], lVar[member])
    ol, gl_tau, gl_c, _ = lifted.grad()
    og, gg_tau, gg_c, _ = ground.grad()
    assert abs(ol - og) <= 1e-9 * max(abs(og), 1.0)
    th.assert_close(gl_tau, gg_tau, 1e-9, 'g_tau')
    summed = np.zeros_like(gl_c)
    np.add.at(summed, member, gg_c)
    th.assert_close(gl_c, summed, 1e-9, 'g_c')
    lifted.adam_eps = ground.adam_eps = 0.0
    ground.run(its=10, lr=0.05)
    lifted.run(its=10, lr=0.05)
    hid = ground.flat.var_hidden
    np.testing.assert_allclose(ground._h['theta_c'][hid], lifted._h['theta_c'][member][hid], rtol=0, atol=1e-9)
    for rv in np.array(ground.flat.rvs, dtype=object)[hid]:
        np.testing.assert_array_equal(rv.belief_params['mu'], lifted._h['eta_c'][lifted._var_index(rv), :, 0])
