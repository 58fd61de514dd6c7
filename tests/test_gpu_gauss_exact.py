"""GPU suite of the exact Gaussian solver (lhvi.gauss_exact, csrc/gauss_exact.hip): the blocked fp64 Cholesky against a NumPy
restatement of the reference route and the recorded reference values, at tol = 10 N cond(J) 1.1e-16 per model; host twin
against device at 1e-13.  Shapes: tests/gauss_exact_models.py (one tile of 64, the ragged last tile, two and more panel steps)."""
import numpy as np
import pytest

import gauss_exact_models as gm

pytestmark = pytest.mark.gpu

_runs = {}


def _run(name):
    """ExactGaussian on a shape model, run once with the inverse kept; shared by the tests (never modified)"""
    if name not in _runs:
        from lhvi.gauss_exact import ExactGaussian
        g, rvs = gm.build(name)
        _runs[name] = (ExactGaussian(g).run(keep_inverse=True), gm.reference_route(g, rvs), rvs)
    return _runs[name]


def _cov_check(what, N, cond, got, want):
    tol = gm.tolerance(N, cond)
    e, bnd = gm.report(what + ' cov', float(np.abs(got - want).max()), tol * max(1.0, float(np.abs(want).max())))
    assert e <= bnd


@pytest.mark.parametrize('name', gm.NAMES)
def test_shape_models(name):
    from lhvi import utils
    from lhvi.gauss_exact import host_solve
    ex, ref, rvs = _run(name)
    N, hid = ex.N, ref['hidden']
    assert ref['cond'] <= 500
    mean, var = ex.mu_var
    gm.check_moments('device %s' % name, N, ref['cond'], mean[hid], var[hid], ex.logdet, ref['mu'], np.diag(ref['Sig']), ref['logdet'])
    e, bnd = gm.report('device %s logZ (rel)' % name, abs(ex.logZ / ref['logZ'] - 1), gm.tolerance(N, ref['cond']))
    assert e <= bnd
    rng = np.random.default_rng(5)
    S = rng.choice(N, min(N, 24), replace=False)
    _cov_check('device %s' % name, N, ref['cond'], ex.cov([rvs[hid[s]] for s in S]), ref['Sig'][np.ix_(S, S)])
    # the reference-named call on the dense A, both values of mu_only
    mu1 = utils.get_gaussian_mean_params_from_quadratic_params(ref['A'], ref['b'])
    mu2, Sig = utils.get_gaussian_mean_params_from_quadratic_params(ref['A'], ref['b'], mu_only=False)
    assert np.array_equal(mu1, mu2) and np.array_equal(mu1, mean[hid])
    # diag(Sig) comes from the covariance kernel (lane-strided sums, then a tree), var from the moments' serial column sums:
    # two summation orders, so each is held to the variances' bound against the reference, not to the other's bits
    e, bnd = gm.report('dense %s diag(Sig) (rel)' % name, float(np.abs(np.diag(Sig) / np.diag(ref['Sig']) - 1).max()),
                       gm.tolerance(N, ref['cond']))
    assert e <= bnd
    _cov_check('dense %s' % name, N, ref['cond'], Sig, ref['Sig'])
    # host twin against device
    rc, hmu, hvar, hlogdet, bad = host_solve(-(ref['A'] + ref['A'].T), ref['b'])
    assert rc == 0
    e = max(float(np.abs(hmu - mean[hid]).max()) / max(1.0, float(np.abs(hmu).max())), float(np.abs(hvar / var[hid] - 1).max()),
            abs(hlogdet - ex.logdet) / max(abs(hlogdet), 1.0))
    gm.report('twin vs device %s' % name, e, 1e-13)
    assert e <= 1e-13


@pytest.mark.parametrize('i', range(5))
def test_rgm_fixtures(i):
    """the recorded reference values through ExactGaussian (assembly from the factors) and through the reference-named call on
    the dense A with both values of mu_only (packing, the full covariance at S = N); host twin against device"""
    from lhvi import utils
    from lhvi.gauss_exact import host_solve
    ex, vid, fx = gm.rgm_solver(i)
    ex.run(keep_inverse=True)
    mean, var = ex.mu_var
    N, cond = ex.N, float(fx['cond'])
    tol = gm.tolerance(N, cond)
    gm.check_moments('device rgm%d' % i, N, cond, mean[vid], var[vid], ex.logdet, fx['mu'], fx['var'], float(fx['logdet']))
    used = np.unique(np.concatenate([fx['cov_i'], fx['cov_j']]))
    block = ex.cov([int(vid[k]) for k in used])
    at = {int(k): p for p, k in enumerate(used)}
    got = np.array([block[at[int(a)], at[int(b)]] for a, b in zip(fx['cov_i'], fx['cov_j'])])
    _cov_check('device rgm%d' % i, N, cond, got, fx['cov_v'])
    # dense path: rows of A are the solver's hidden order; `order` is the row of every recorded row
    A, b, c = ex.joint_quadratic()
    pos = np.full(ex.flat.V, -1)
    pos[ex.hidden] = np.arange(N)
    order = pos[vid]
    mu1 = utils.get_gaussian_mean_params_from_quadratic_params(A, b)
    mu2, Sig = utils.get_gaussian_mean_params_from_quadratic_params(A, b, mu_only=False)
    assert np.array_equal(mu1, mu2)
    for what, mu in (('dense rgm%d mu_only' % i, mu1), ('dense rgm%d' % i, mu2)):
        e, bnd = gm.report(what + ' mu', float(np.abs(mu[order] - fx['mu']).max()), tol * max(1.0, float(np.abs(fx['mu']).max())))
        assert e <= bnd
    e, bnd = gm.report('dense rgm%d diag(Sig) (rel)' % i, float(np.abs(np.diag(Sig)[order] / fx['var'] - 1).max()), tol)
    assert e <= bnd
    _cov_check('dense rgm%d' % i, N, cond, Sig[order[fx['cov_i']], order[fx['cov_j']]], fx['cov_v'])
    rc, hmu, hvar, hlogdet, bad = host_solve(-(A + A.T), b)
    e = max(float(np.abs(hmu - mean[ex.hidden]).max()) / max(1.0, float(np.abs(hmu).max())),
            float(np.abs(hvar / var[ex.hidden] - 1).max()), abs(hlogdet - ex.logdet) / abs(hlogdet))
    gm.report('twin vs device rgm%d' % i, e, 1e-13)
    assert rc == 0 and e <= 1e-13


def test_runs_are_bit_identical_and_keep_inverse_changes_nothing():
    from lhvi.gauss_exact import ExactGaussian
    g, rvs = gm.build('n200')
    a = ExactGaussian(g).run(keep_inverse=True)
    b = ExactGaussian(g).run(keep_inverse=True)
    c = ExactGaussian(g).run()
    for other in (b, c):
        assert np.array_equal(a.mu_var[0], other.mu_var[0]) and np.array_equal(a.mu_var[1], other.mu_var[1])
        assert a.logZ == other.logZ and a.logdet == other.logdet
    assert np.array_equal(a.cov(rvs[:40]), b.cov(rvs[:40]))
    with pytest.raises(RuntimeError):
        c.cov(rvs[:2])


@pytest.mark.parametrize('name', ['n1', 'n2', 'n63', 'n64'])
def test_equals_exact_hybrid_gaussian(name):
    """both are Cholesky routes on the same matrix: 1e-12 relative"""
    from lhvi.exact import ExactHybridGaussian
    ex, ref, rvs = _run(name)
    g, _ = gm.build(name)
    hy = ExactHybridGaussian(g).run()
    mean, var = ex.mu_var
    hm, hv = hy.means.reshape(-1), hy.variances.reshape(-1)
    e = max(float(np.abs(mean - hm).max()) / max(1.0, float(np.abs(hm).max())), float(np.abs(var / hv - 1).max()),
            abs(ex.logZ - hy.logZ) / abs(hy.logZ))
    gm.report('vs ExactHybridGaussian %s' % name, e, 1e-12)
    assert e <= 1e-12


def test_gabp_on_a_tree_is_exact():
    from lhvi import synth
    from lhvi.gabp import GaBP
    from lhvi.gauss_exact import ExactGaussian
    g, rvs = synth.gaussian_chain(130)
    bp = GaBP(g)
    bp.run(140)
    ex = ExactGaussian(g).run()
    got = np.array([bp.get_belief_params(rv) for rv in rvs[1:]])
    want = np.array([ex.get_belief_params(rv) for rv in rvs[1:]])
    e = float(np.abs(got - want).max())
    gm.report('GaBP(140) on chain(130)', e, 1e-9)
    assert e <= 1e-9


def test_object_graph_and_ground_flat_give_the_same_bits():
    from lhvi import generators
    from lhvi.gauss_exact import ExactGaussian
    rel = generators.rgm(C=6, B=3)
    data = {('loss', 'c1', 'b2'): 1.5, ('market', 'c3'): -2.0, ('revenue', 'b0'): 4.0, ('loss', 'c4', 'b0'): -7.25}
    rel.ground_graph()
    g, rvs_dict = rel.add_evidence(data)
    flat, keys = generators.rgm(C=6, B=3).ground_flat(data)
    a, b = ExactGaussian(g).run(), ExactGaussian(flat).run()
    assert a.N == b.N == len(rvs_dict) - len(data)
    for key, rv in rvs_dict.items():
        v = keys.var_id(key)
        assert a.map(rv) == b.map(v)
        if key in data:
            assert a.map(rv) == data[key] and b.belief(data[key], v) == 1 and b.belief(data[key] + 1, v) == 0
        else:
            assert a.get_belief_params(rv) == b.get_belief_params(v)
    assert a.logZ == b.logZ


def test_belief_all_and_kl_tables():
    from lhvi import utils
    ex, ref, rvs = _run('ev30')
    mean, var = ex.mu_var
    V, m = len(rvs), 33
    x = np.linspace(-6, 6, m)[None, :] + np.zeros((V, 1))
    obs = [i for i, rv in enumerate(rvs) if rv.value is not None]
    x[obs, 0] = [rvs[i].value for i in obs]
    bel = ex.belief_all(x)
    got = bel.cpu().numpy()
    hid = ref['hidden']
    want = np.exp(-0.5 * (x[hid] - mean[hid, None]) ** 2 / var[hid, None]) / np.sqrt(2 * np.pi * var[hid, None])
    np.testing.assert_allclose(got[hid], want, rtol=1e-12, atol=1e-300)
    assert (got[obs, 0] == 1).all() and (got[obs, 1:] == 0).all()
    kl = utils.kl_tables(bel, bel, np.full(V, -6.0), np.full(V, 6.0))
    assert float(kl.abs().max().item()) == 0.0
    h = rvs[hid[3]]
    assert ex.belief(0.25, h) == pytest.approx(float(np.exp(ex.belief(0.25, h, log_belief=True))), rel=1e-14)
    assert ex.belief(float(x[hid[3], 5]), h) == pytest.approx(want[3, 5], rel=1e-12)
    assert np.array_equal(ex.map_all(), mean)


def test_observed_variable():
    ex, ref, rvs = _run('ev30')
    o = next(rv for rv in rvs if rv.value is not None)
    assert ex.map(o) == o.value
    assert ex.belief(o.value, o) == 1 and ex.belief(o.value + 0.5, o) == 0
    assert ex.belief(o.value, o, log_belief=True) == 0 and ex.belief(o.value + 0.5, o, log_belief=True) == -np.inf
    with pytest.raises(AssertionError):
        ex.get_belief_params(o)
    with pytest.raises(ValueError, match='observed'):
        ex.cov([o])


def test_indefinite_raises_value_error():
    from lhvi import utils
    from lhvi.gauss_exact import ExactGaussian
    g, rvs = gm.build('indefinite')
    ref = gm.reference_route(g, rvs)
    want = gm.first_bad_pivot(ref['J'])
    assert want in (70, 71)
    with pytest.raises(ValueError, match='variable %d' % want):
        ExactGaussian(g).run()
    with pytest.raises(ValueError, match='column %d' % want):
        utils.get_gaussian_mean_params_from_quadratic_params(ref['A'], ref['b'])


def test_device_usable_after_indefinite():
    """runs after test_indefinite_raises_value_error: a definite model on a fresh solver"""
    from lhvi.gauss_exact import ExactGaussian
    g, rvs = gm.build('n130')
    ref = gm.reference_route(g, rvs)
    ex = ExactGaussian(g).run()
    gm.check_moments('after indefinite n130', ex.N, ref['cond'], ex.mu_var[0], ex.mu_var[1], ex.logdet, ref['mu'],
                     np.diag(ref['Sig']), ref['logdet'])


def test_memory_error_before_a_launch(monkeypatch):
    import torch
    from lhvi import _abi, gauss_exact
    free = int(torch.cuda.mem_get_info()[0])
    N = int(np.sqrt(free / 8)) + 4096              # two packed triangles of N^2 / 2 doubles each exceed the free memory
    assert gauss_exact.output_bytes(N, False) > free and gauss_exact.output_bytes(N, True) > free

    def no_launch(*a, **k):
        raise AssertionError('a kernel entry point was reached')
    monkeypatch.setattr(_abi, 'lib', no_launch)
    with pytest.raises(MemoryError, match=str(gauss_exact.output_bytes(N, False))):
        gauss_exact._DeviceSolve(N, lambda Jt, b: None)
    assert int(torch.cuda.mem_get_info()[0]) >= free - (64 << 20)
    # the dense call counts its own A and the full Sig too, and raises before it uploads anything
    assert gauss_exact.dense_bytes(N, False) == gauss_exact.output_bytes(N, True) + 16 * N * N
    monkeypatch.setattr(_abi, 'to_dev', no_launch)

    class Shape:                                    # stands for an N x N array: nothing of that size is allocated
        shape, ndim = (N, N), 2
    with pytest.raises(MemoryError, match=str(gauss_exact.dense_bytes(N, False))):
        gauss_exact.mean_params_from_quadratic(Shape(), np.zeros(N), mu_only=False)


def test_empty_model():
    """every variable observed: N = 0, no launch, logZ is the constant of the observed factors"""
    from lhvi import utils
    from lhvi.gauss_exact import ExactGaussian
    from lhvi.graph import Domain, F, Graph, RV
    from lhvi.potentials import X2Potential
    d = Domain((-5, 5), continuous=True, integral_points=np.linspace(-5, 5, 10))
    x = RV(d, 2.0)
    g = Graph()
    g.rvs, g.factors = [x], [F(X2Potential(3.0, 1.0), [x])]
    g.init_nb()
    ex = ExactGaussian(g).run()
    assert ex.N == 0 and ex.logZ == -0.5 * 3.0 * 4.0 and ex.map(x) == 2.0
    assert utils.get_gaussian_mean_params_from_quadratic_params(np.zeros((0, 0)), np.zeros(0)).size == 0
