"""CPU suite of the block-tridiagonal Gaussian solver: the host twin (lhvi_gauss_chain_host: the device's code with one lane) on
every shape of tests/gauss_chain_models.py and on both relational-Kalman-filter fixtures, ``KalmanFilter.block_tridiagonal``
against the assembled model, and the errors ``ExactGaussianChain`` raises before it reaches a device.

Yardstick: NumPy on the dense J that the helper assembles from ``grounded_flat`` (never the code under test).
Tolerance: tol = 10 N cond(J) 1.1e-16 per model, cond(J) asserted <= 500 (docs/kernels_gauss_chain.md)."""
import numpy as np
import pytest

import gauss_chain_models as cm


def _host(blocks, keep_cov=True):
    from lhvi.gauss_chain import host_solve_block_tridiagonal
    D, O, h = blocks
    return host_solve_block_tridiagonal(D, O if D.shape[-3] > 1 else None, h, keep_cov=keep_cov)


@pytest.mark.parametrize('n,M', cm.SHAPES)
def test_host_twin_on_shapes(n, M):
    from lhvi import _abi, gauss_chain
    ref = cm.shape_case(n, M)
    mu, var, logdet, cov, cross, bad = _host(ref['blocks'])
    assert tuple(bad) == (-1, -1)
    cm.check_solution('host (%d, %d)' % (n, M), ref, ref['sizes'], mu, var, logdet, cov, cross)
    for B in (1, 3):
        assert gauss_chain.ws_doubles(B, M, n) == _abi.lib().lhvi_gauss_chain_ws_doubles(B, M, n)


def test_host_twin_on_ragged_blocks():
    from lhvi.gauss_chain import ExactGaussianChain
    g, rvs, blocks, ref = cm.ragged_chain()
    ex = ExactGaussianChain(g, blocks)
    assert ex.n == 5 and ex.N == 11 and ex.D.shape == (4, 5, 5) and ex.O.shape == (3, 5, 5)
    D, O, h = cm.blocks_of(ref['J'], ref['h'], list(cm.RAGGED))
    np.testing.assert_allclose(ex.D, D, rtol=0, atol=1e-13 * np.abs(D).max())
    np.testing.assert_allclose(ex.O, O, rtol=0, atol=1e-13 * np.abs(D).max())
    np.testing.assert_allclose(ex.h, h, rtol=0, atol=1e-13 * np.abs(h).max())
    mu, var, logdet, cov, cross, bad = _host((ex.D, ex.O, ex.h))
    assert tuple(bad) == (-1, -1)
    cm.check_solution('host ragged', ref, list(cm.RAGGED), mu, var, logdet, cov, cross)


@pytest.mark.parametrize('n,M', cm.SHAPES)
def test_block_tridiagonal_against_assembled_model(n, M):
    """the closed form of the conditioned filter against the joint quadratic of grounded_flat, at 1e-13 of the largest entry"""
    ref = cm.shape_case(n, M)
    D, O, h, const = ref['kf'].block_tridiagonal(ref['T'], ref['data'])
    assert D.shape == (M, n, n) and O.shape == (M - 1, n, n) and h.shape == (M, n)
    wD, wO, wh = ref['blocks']
    top = float(max(np.abs(wD).max(), np.abs(wh).max()))
    for what, got, want in (('D', D, wD), ('O', O, wO), ('h', h, wh)):
        e = float(np.abs(got - want).max()) if want.size else 0.0
        cm.report('block_tridiagonal (%d, %d) %s' % (n, M, what), e, 1e-13 * top)
        assert e <= 1e-13 * top
    assert abs(const - ref['const']) <= 1e-13 * max(1.0, abs(ref['const']))


@pytest.mark.parametrize('which', ['tree', 'cycle'])
def test_fixtures_as_one_batch(which):
    """all five parameter sets of a demo in one call (tree: n = 76, M = 19; cycle: n = 6, M = 19) against dense NumPy; the
    closed-form blocks against the assembled model; ``exact_batch``'s rows and logZ"""
    from lhvi import kalman
    fx = cm.fixture(which)
    n, T = fx['n'], cm.T_FIXTURE
    assert n == (76 if which == 'tree' else 6) and len(fx['filters']) == 5
    parts = [kf.block_tridiagonal(T, fx['data']) for kf in fx['filters']]
    D, O, h = (np.stack([p[i] for p in parts]) for i in range(3))
    assert D.shape == (5, T - 1, n, n)
    mu, var, logdet, cov, cross, bad = _host((D, O, h))
    assert (bad == -1).all()
    bmu, bvar, blogZ = kalman.exact_batch(fx['filters'], T, fx['data'], host=True)
    for k in range(5):
        ref = cm.fixture_reference(which, k)
        wD, wO, wh = cm.blocks_of(ref['J'], ref['h'], [n] * (T - 1))
        top = float(max(np.abs(wD).max(), np.abs(wh).max()))
        assert max(np.abs(D[k] - wD).max(), np.abs(O[k] - wO).max(), np.abs(h[k] - wh).max()) <= 1e-13 * top
        assert abs(parts[k][3] - ref['const']) <= 1e-13 * max(1.0, abs(ref['const']))
        cm.check_solution('host %s set %d' % (which, k), ref, [n] * (T - 1), mu[k], var[k], logdet[k], cov[k], cross[k])
        assert np.array_equal(bmu[k, 1:], mu[k]) and np.array_equal(bvar[k, 1:], var[k])
        assert np.array_equal(bmu[k, 0], fx['data'][:, 0]) and not bvar[k, 0].any()
        e, bnd = cm.report('host %s set %d logZ (rel)' % (which, k), abs(blogZ[k] / ref['logZ'] - 1), cm.tolerance(ref['N'], ref['cond']))
        assert e <= bnd


def test_tree_against_recorded_gabp():
    """on the tree model GaBP is exact: the reference's recorded run agrees with the chain solve at tol"""
    fx = cm.fixture('tree')
    ref = cm.fixture_reference('tree', 0)
    mu, var, logZ = fx['filters'][0].exact(cm.T_FIXTURE, fx['data'], host=True)
    rec = fx['gabp'][ref['state_id'][1:]]                          # [T-1][n][2]
    tol = cm.tolerance(ref['N'], ref['cond'])
    e, bnd = cm.report('tree vs recorded GaBP mu', float(np.abs(mu[1:] - rec[..., 0]).max()), tol * max(1.0, float(np.abs(rec[..., 0]).max())))
    assert e <= bnd
    e, bnd = cm.report('tree vs recorded GaBP var (rel)', float(np.abs(var[1:] / rec[..., 1] - 1).max()), tol)
    assert e <= bnd


def test_cycle_means_near_recorded_gabp():
    """on the cycle model the recorded truth of the demos is loopy BP after 20 sweeps: means within 1e-4 (measured 2.1e-5)"""
    fx = cm.fixture('cycle')
    ref = cm.fixture_reference('cycle', 0)
    mu, var, logZ = fx['filters'][0].exact(cm.T_FIXTURE, fx['data'], host=True)
    rec = fx['gabp'][ref['state_id'][1:]]
    e = float(np.abs(mu[1:] - rec[..., 0]).max())
    cm.report('cycle vs recorded GaBP mu', e, 1e-4)
    cm.report('cycle vs recorded GaBP var (rel, not asserted)', float(np.abs(var[1:] / rec[..., 1] - 1).max()), float('nan'))
    assert e <= 1e-4


def indefinite_batch():
    """three (3, 4) systems; the middle one's block 2 has a negative diagonal entry: (D, O, h, references of systems 0 and 2,
    the expected (block, column))"""
    refs = [cm.shape_case(3, 4), cm.shape_case(3, 4), cm.shape_case(3, 4)]
    D, O, h = (np.stack([r['blocks'][i] for r in refs]).copy() for i in range(3))
    D[1, 2, 1, 1] = -5.0
    J = refs[1]['J'].copy()
    J[2 * 3 + 1, 2 * 3 + 1] = -5.0
    col = cm.first_bad_pivot(J)
    assert col // 3 == 2
    return D, O, h, refs, (col // 3, col % 3)


def test_indefinite_system_in_a_batch():
    from lhvi.gauss_chain import _bad_error
    D, O, h, refs, want = indefinite_batch()
    mu, var, logdet, bad = _host((D, O, h), keep_cov=False)
    assert tuple(bad[1]) == want and tuple(bad[0]) == (-1, -1) and tuple(bad[2]) == (-1, -1)
    for b in (0, 2):
        cm.check_solution('host beside an indefinite system, %d' % b, refs[b], refs[b]['sizes'], mu[b], var[b], logdet[b])
    with pytest.raises(ValueError, match='system 1 .*block %d, column %d' % want):
        raise _bad_error(bad)
    from lhvi.kalman import KalmanFilter
    kf = KalmanFilter(None, np.eye(2), -1.0, np.eye(2), 0.4)                    # a negative transition variance, nothing observed
    data = np.full((2, 3), float(cm.MISSING))
    data[:, 0] = 0.0
    with pytest.raises(ValueError, match='filter 0 .*block 0, column 0'):
        kf.exact(3, data, host=True)


def test_chain_value_errors(monkeypatch):
    """a factor across blocks two apart, a hidden variable in no block or in two, a block wider than 128: ValueError before the
    device is touched"""
    from lhvi import _abi
    from lhvi.gauss_chain import ExactGaussianChain, host_solve_block_tridiagonal, solve_block_tridiagonal
    from lhvi.graph import F, Graph, RV
    from lhvi.potentials import X2Potential, XYPotential

    def no_device(*a, **k):
        raise AssertionError('the device was touched')
    monkeypatch.setattr(_abi, 'require_gpu', no_device)
    monkeypatch.setattr(_abi, 'to_dev', no_device)
    g, rvs, blocks, ref = cm.ragged_chain()
    with pytest.raises(ValueError, match='variable 3 is hidden and in no block'):
        ExactGaussianChain(g, [blocks[0], blocks[2], blocks[3]])
    with pytest.raises(ValueError, match=r'variable 0 is in two blocks \(0 and 1\)'):
        ExactGaussianChain(g, [blocks[0], blocks[1] + blocks[0][:1], blocks[2], blocks[3]])
    with pytest.raises(ValueError, match='variable 11 in block 3 is observed'):
        ExactGaussianChain(g, [blocks[0], blocks[1], blocks[2], blocks[3] + rvs[-1:]])
    d = cm._domain()
    x = [RV(d) for _ in range(3)]
    g2 = Graph()
    g2.rvs = x
    g2.factors = [F(X2Potential(2.0, 1.0), [v]) for v in x] + [F(XYPotential(0.2, 1.0), [x[0], x[1]]), F(XYPotential(0.2, 1.0), [x[2], x[0]])]
    g2.init_nb()
    with pytest.raises(ValueError, match='factor 4 links blocks 0 and 2'):
        ExactGaussianChain(g2, [[x[0]], [x[1]], [x[2]]])
    ExactGaussianChain(g2, [[x[0]], [x[1], x[2]]])
    ExactGaussianChain(g2, [[1], [0], [2]])                                     # by index; 0 in the middle: a chain again
    wide = [RV(d) for _ in range(129)]
    g3 = Graph()
    g3.rvs, g3.factors = wide, [F(X2Potential(2.0, 1.0), [v]) for v in wide]
    g3.init_nb()
    with pytest.raises(ValueError, match='n <= 128'):
        ExactGaussianChain(g3, [wide])
    for solve in (solve_block_tridiagonal, host_solve_block_tridiagonal):
        with pytest.raises(ValueError, match='n <= 128'):
            solve(np.zeros((1, 129, 129)), None, np.zeros((1, 129)))
    assert _abi.lib().lhvi_gauss_chain_host(1, 1, 129, None, None, None, None, None, None, None, None, None, None) == -3
    assert _abi.lib().lhvi_gauss_chain_ws_doubles(1, 1, 129) == 0


def test_chain_class_names_the_variable_of_a_bad_pivot():
    from lhvi.gauss_chain import ExactGaussianChain
    from lhvi.graph import F, Graph, RV
    from lhvi.potentials import QuadraticPotential, X2Potential, XYPotential
    d = cm._domain()
    x = [RV(d), RV(d)]
    g = Graph()
    g.rvs = x
    g.factors = [F(X2Potential(2.0, 1.0), [x[0]]), F(QuadraticPotential(np.array([[1.0]]), np.zeros(1), 0.0), [x[1]]),
                 F(XYPotential(0.2, 1.0), [x[0], x[1]])]
    g.init_nb()
    with pytest.raises(ValueError, match='not positive definite: the pivot of block 1, column 0, variable 1'):
        ExactGaussianChain(g, [[x[0]], [x[1]]]).run(host=True)


def test_empty_inputs_launch_nothing(monkeypatch):
    from lhvi import _abi
    from lhvi.gauss_chain import solve_block_tridiagonal
    monkeypatch.setattr(_abi, 'require_gpu', lambda: (_ for _ in ()).throw(AssertionError('the device was touched')))
    mu, var, logdet = solve_block_tridiagonal(np.zeros((0, 3, 2, 2)), np.zeros((0, 2, 2, 2)), np.zeros((0, 3, 2)))
    assert mu.shape == (0, 3, 2) and var.shape == (0, 3, 2) and logdet.shape == (0,)
    mu, var, logdet, cov, cross, bad = solve_block_tridiagonal(np.zeros((2, 0, 4, 4)), None, np.zeros((2, 0, 4)), keep_cov=True,
                                                                raise_on_bad=False)
    assert mu.shape == (2, 0, 4) and cov.shape == (2, 0, 4, 4) and cross.shape == (2, 0, 4, 4) and bad.shape == (2, 2)


def test_logZ_of_the_chain_class():
    """ExactGaussianChain.logZ (ExactGaussian's convention; the padding of ragged blocks is not counted in N) against
    N/2 log 2 pi - 1/2 slogdet J + 1/2 mu . h + c + const of the dense model, through the host twin"""
    from lhvi.gauss_chain import ExactGaussianChain
    g, rvs, blocks, ref = cm.ragged_chain()
    ex = ExactGaussianChain(g, blocks).run(keep_cov=True, host=True)
    tol = cm.tolerance(ref['N'], ref['cond'])
    e, bnd = cm.report('host ragged logZ (rel)', abs(ex.logZ / ref['logZ'] - 1), tol)
    assert e <= bnd
    mean, var = ex.mu_var
    assert mean[11] == 0.8 and var[11] == 0.0
    assert np.abs(mean[:11] - ref['mu']).max() <= tol * max(1.0, np.abs(ref['mu']).max())
    pick = [blocks[1][0], blocks[2][4], blocks[2][0]]
    at = [3, 8, 4]
    assert np.abs(ex.cov(pick) - ref['Sig'][np.ix_(at, at)]).max() <= tol * max(1.0, np.abs(ref['Sig']).max())
    with pytest.raises(ValueError, match='blocks 0 and 2'):
        ex.cov([blocks[0][0], blocks[2][0]])
    ref5 = cm.shape_case(5, 7)
    ex5 = ExactGaussianChain(ref5['flat'], list(ref5['state_id'][1:])).run(host=True)
    e, bnd = cm.report('host (5, 7) logZ (rel)', abs(ex5.logZ / ref5['logZ'] - 1), cm.tolerance(ref5['N'], ref5['cond']))
    assert e <= bnd


def test_no_cpu_fallback_without_gpu():
    from conftest import has_gpu
    if has_gpu():
        pytest.skip('GPU present')
    from lhvi import _abi
    from lhvi.gauss_chain import ExactGaussianChain, solve_block_tridiagonal
    ref = cm.shape_case(3, 4)
    with pytest.raises(_abi.LhviError):
        solve_block_tridiagonal(*ref['blocks'])
    with pytest.raises(_abi.LhviError):
        ExactGaussianChain(ref['flat'], list(ref['state_id'][1:])).run()
    with pytest.raises(_abi.LhviError):
        ref['kf'].exact(ref['T'], ref['data'])


def test_compat_kalman_filter_reexports():
    import importlib
    import os
    import sys
    compat = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'lifted-hybrid-variational-inference_amd', 'compat')
    sys.path.insert(0, compat)
    try:
        mod = importlib.import_module('KalmanFilter')
    finally:
        sys.path.remove(compat)
    assert callable(mod.exact_batch) and callable(mod.KalmanFilter.exact) and callable(mod.KalmanFilter.block_tridiagonal)
