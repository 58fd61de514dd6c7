"""CPU suite of the exact Gaussian solver: the host helpers named after osi/utils.py against a NumPy restatement of the reference
route (tests/gauss_exact_models.py), and the blocked Cholesky's host twin (lhvi_gauss_exact_host: the device's tile routines in
the device's panel order) on every shape model and on the five recorded RGM datasets.

Tolerance: tol = 10 N cond(J) 1.1e-16 per model (docs/kernels_gauss_exact.md), with cond(J) asserted <= 500."""
import numpy as np
import pytest

import gauss_exact_models as gm


def _solver(name):
    from lhvi.gauss_exact import ExactGaussian
    g, rvs = gm.build(name)
    return ExactGaussian(g), gm.reference_route(g, rvs)


@pytest.mark.parametrize('name', gm.NAMES)
def test_joint_quadratic_bits(name):
    """A, b, c of the conditioned model: bit-equal to the reference's summation order, through ExactGaussian's own conditioning
    and through get_conditional_mrf + get_quadratic_params_from_factor_graph"""
    from lhvi import utils
    ex, ref = _solver(name)
    A, b, c = ex.joint_quadratic()
    assert np.array_equal(A, ref['A']) and np.array_equal(b, ref['b']) and c == ref['c']
    assert ex.log_const == ref['const']
    g, rvs = gm.build(name)
    evidence = {rv: rv.value for rv in rvs if rv.value is not None}
    cond_g = utils.get_conditional_mrf(g.factors_list, g.rvs_list, evidence)
    (A2, b2, c2), idx = utils.get_quadratic_params_from_factor_graph(cond_g.factors, cond_g.rvs_list)
    assert [idx[rvs[i]] for i in ref['hidden']] == list(range(len(ref['hidden'])))
    assert np.array_equal(A2, ref['A']) and np.array_equal(b2, ref['b']) and c2 == ref['c']


def test_sorted_contributions_sum_to_J():
    """the device's input: summing every entry's two ranges in order reproduces -(A + A^T) and b bit for bit"""
    ex, ref = _solver('ev30')
    ct = ex._contrib
    J = np.zeros_like(ref['A'])
    for e in range(ct['ent_row'].size):
        r, c = int(ct['ent_row'][e]), int(ct['ent_col'][e])
        s1 = s2 = 0.0
        for p in range(ct['ent_ptr'][e], ct['ent_mid'][e]):
            s1 += ct['vals'][p]
        for p in range(ct['ent_mid'][e], ct['ent_ptr'][e + 1]):
            s2 += ct['vals'][p]
        assert r >= c
        J[r, c] = J[c, r] = -(s1 + (s1 if r == c else s2))
    assert np.array_equal(J, -(ref['A'] + ref['A'].T))
    b = np.array([sum(ct['b_vals'][ct['b_ptr'][r]:ct['b_ptr'][r + 1]], 0.0) for r in range(ex.N)])
    assert np.array_equal(b, ref['b'])


def test_conditioning_against_get_conditional_quadratic():
    from lhvi import utils
    g, rvs = gm.build('ev30')
    evidence = {rv: rv.value for rv in rvs if rv.value is not None}
    cond = utils.condition_factors_on_evidence(g.factors_list, evidence)
    assert len(cond) == len(g.factors_list)
    touched = 0
    for f, cf in zip(g.factors_list, cond):
        obs = {i: evidence[rv] for i, rv in enumerate(f.nb) if rv in evidence}
        if not obs:
            assert cf is f
            continue
        touched += 1
        assert cf is not f and cf.uncond_factor is f and list(f.nb) != list(cf.nb)
        if not cf.nb:
            assert cf.potential is None
            continue
        want = utils.get_conditional_quadratic(*f.potential.get_quadratic_params(), obs)
        got = cf.potential.get_quadratic_params()
        for w, h in zip(want, got):
            assert np.array_equal(np.asarray(w), np.asarray(h))
        assert np.array_equal(np.asarray(cf.log_potential_fun.A), np.asarray(want[0]))
    assert touched > 10


def test_condition_rejects_mln():
    from lhvi import utils
    from lhvi.graph import Domain, F, RV
    from lhvi.mln import MLNPotential
    d = Domain((-5, 5), continuous=True, integral_points=np.linspace(-5, 5, 10))
    a, b = RV(d), RV(d)
    f = F(MLNPotential(lambda x: x[0] * x[1], w=0.5), [a, b])
    with pytest.raises(NotImplementedError, match='MLNPotential'):
        utils.condition_factors_on_evidence([f], {a: 1.0})


def test_get_conditional_gaussian_formula():
    from lhvi import utils
    rng = np.random.default_rng(3)
    M = rng.normal(size=(6, 6))
    Sig, mu = M @ M.T + 6 * np.eye(6), rng.normal(size=6)
    obs = {4: 0.3, 1: -1.2}
    cm, cS = utils.get_conditional_gaussian(mu, Sig, obs)
    # the same conditional from the precision form: Sig_a|b = (Lam_aa)^-1, mu_a|b = mu_a - Lam_aa^-1 Lam_ab (x_b - mu_b)
    Lam = np.linalg.inv(Sig)
    a, bi = [0, 2, 3, 5], [4, 1]
    S2 = np.linalg.inv(Lam[np.ix_(a, a)])
    m2 = mu[a] - S2 @ Lam[np.ix_(a, bi)] @ (np.array([0.3, -1.2]) - mu[bi])
    np.testing.assert_allclose(cS, S2, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(cm, m2, rtol=1e-12, atol=1e-14)


def test_prec_mat_from_gaussian_mrf():
    from lhvi import generators, utils
    g, _ = generators.rgm(C=3, B=2).ground_graph()
    rvs = g.rvs_list
    prec, idx = utils.get_prec_mat_from_gaussian_mrf(g.factors_list, rvs)
    (A, b, c), idx2 = utils.get_quadratic_params_from_factor_graph(g.factors_list, rvs)
    assert idx == idx2
    np.testing.assert_allclose(prec, -2 * A, rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize('name', gm.NAMES)
def test_host_twin_on_shape_models(name):
    from lhvi.gauss_exact import host_solve
    ex, ref = _solver(name)
    assert ref['cond'] <= 500
    rc, mu, var, logdet, bad = host_solve(-(ref['A'] + ref['A'].T), ref['b'])
    assert rc == 0 and bad == -1
    gm.check_moments('host %s' % name, ex.N, ref['cond'], mu, var, logdet, ref['mu'], np.diag(ref['Sig']), ref['logdet'])


@pytest.mark.parametrize('i', range(5))
def test_host_twin_on_rgm_fixtures(i):
    """the recorded reference values (np.linalg.inv in the reference's own process) and the restatement's J agree with the twin"""
    from lhvi.gauss_exact import host_solve
    ex, vid, fx = gm.rgm_solver(i)
    assert ex.N == fx['mu'].size and fx['cond'] <= 500
    A, b, c = ex.joint_quadratic()
    J = -(A + A.T)
    eig = np.linalg.eigvalsh(J)
    np.testing.assert_allclose([eig[0], eig[-1]], [fx['eig_min'], fx['eig_max']], rtol=1e-10)
    rc, mu, var, logdet, bad = host_solve(J, b)
    assert rc == 0
    pos = np.full(ex.flat.V, -1)
    pos[ex.hidden] = np.arange(ex.N)
    order = pos[vid]                                    # the twin's row of every recorded row
    assert (order >= 0).all() and np.unique(order).size == ex.N
    gm.check_moments('host rgm%d' % i, ex.N, float(fx['cond']), mu[order], var[order], logdet, fx['mu'], fx['var'], float(fx['logdet']))


def test_host_twin_not_positive_definite():
    from lhvi import _abi
    from lhvi.gauss_exact import host_solve
    ex, ref = _solver('indefinite')
    J = -(ref['A'] + ref['A'].T)
    want = gm.first_bad_pivot(J)
    assert want in (70, 71)
    rc, mu, var, logdet, bad = host_solve(J, ref['b'])
    assert rc == _abi.E_NOT_PD and bad == want


def test_host_twin_empty():
    from lhvi.gauss_exact import host_solve
    rc, mu, var, logdet, bad = host_solve(np.zeros((0, 0)), np.zeros(0))
    assert rc == 0 and mu.size == 0 and var.size == 0 and logdet == 0.0


def test_compat_osi_resolves_demo_names():
    import importlib
    import os
    import sys
    compat = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                          'lifted-hybrid-variational-inference_amd', 'compat')
    sys.path.insert(0, compat)
    try:
        utils = importlib.import_module('osi.utils')
    finally:
        sys.path.remove(compat)
    for name in ('get_conditional_mrf', 'get_quadratic_params_from_factor_graph', 'get_gaussian_mean_params_from_quadratic_params',
                 'get_joint_quadratic_params', 'condition_factors_on_evidence', 'get_conditional_gaussian',
                 'get_prec_mat_from_gaussian_mrf', 'get_conditional_quadratic', 'set_nbrs_idx_in_factors'):
        assert callable(getattr(utils, name)), name


def test_rejects_before_the_device(monkeypatch):
    """a discrete hidden variable or an MLN factor raises in the constructor, before any device call"""
    from lhvi import _abi
    from lhvi.gauss_exact import ExactGaussian
    from lhvi.graph import Domain, F, Graph, RV
    from lhvi.mln import MLNPotential
    from lhvi.potentials import TablePotential, X2Potential

    def no_device(*a, **k):
        raise AssertionError('the device was touched')
    monkeypatch.setattr(_abi, 'require_gpu', no_device)
    monkeypatch.setattr(_abi, 'to_dev', no_device)
    dc = Domain((-5, 5), continuous=True, integral_points=np.linspace(-5, 5, 10))
    dd = Domain((0, 1))
    x, y, z = RV(dc), RV(dc), RV(dd)
    g = Graph()
    g.rvs = [x, z]
    g.factors = [F(X2Potential(1.0, 1.0), [x]), F(TablePotential(np.array([0.4, 0.6])), [z])]
    g.init_nb()
    with pytest.raises(ValueError, match='discrete and hidden'):
        ExactGaussian(g)
    g = Graph()
    g.rvs = [x, y]
    g.factors = [F(X2Potential(1.0, 1.0), [x]), F(X2Potential(1.0, 1.0), [y]), F(MLNPotential(lambda a: a[0] * a[1], w=0.5), [x, y])]
    g.init_nb()
    with pytest.raises(TypeError, match='MLNPotential'):
        ExactGaussian(g)


def test_no_cpu_fallback_without_gpu():
    from conftest import has_gpu
    if has_gpu():
        pytest.skip('GPU present')
    from lhvi import _abi, utils
    ex, ref = _solver('n2')
    with pytest.raises(_abi.LhviError):
        ex.run()
    with pytest.raises(_abi.LhviError):
        utils.get_gaussian_mean_params_from_quadratic_params(ref['A'], ref['b'])


def test_log_quadratic_only_factor():
    """a factor that carries only a LogQuadratic log_potential_fun (no potential), one argument observed: ExactGaussian's
    A, b, c against get_joint_quadratic_params on the hand-conditioned blocks, and the host twin's answer against inv"""
    from lhvi import utils
    from lhvi.gauss_exact import ExactGaussian, host_solve
    from lhvi.graph import Domain, F, Graph, RV
    from lhvi.potentials import LogQuadratic, X2Potential
    d = Domain((-5, 5), continuous=True, integral_points=np.linspace(-5, 5, 10))
    x, y, z = RV(d), RV(d), RV(d, 0.75)
    Aq = np.array([[-1.5, 0.2, 0.1], [0.2, -1.0, -0.3], [0.1, -0.3, -2.0]])
    bq, cq = np.array([0.3, -0.4, 0.9]), 0.25
    g = Graph()
    g.rvs = [x, y, z]
    g.factors = [F(X2Potential(1.0, 2.0), [x]), F(None, [y, z, x], log_potential_fun=LogQuadratic(Aq, bq, cq))]
    g.init_nb()
    ex = ExactGaussian(g)
    assert ex.N == 2 and list(ex.hidden) == [0, 1]
    cond = utils.get_conditional_quadratic(Aq, bq, cq, {1: 0.75})           # over (y, x)
    want = utils.get_joint_quadratic_params([X2Potential(1.0, 2.0).get_quadratic_params(), cond], [(0,), (1, 0)], 2)
    got = ex.joint_quadratic()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    J = -(got[0] + got[0].T)
    rc, mu, var, logdet, bad = host_solve(J, got[1])
    assert rc == 0
    Sig = np.linalg.inv(J)
    np.testing.assert_allclose(mu, Sig @ got[1], rtol=1e-14)
    np.testing.assert_allclose(var, np.diag(Sig), rtol=1e-14)


def test_rejects_lifted_graph():
    """flat arrays marked lifted (cluster multiplicities in edge_count / fac_mult) are refused, not read as a ground graph"""
    import dataclasses
    from lhvi import synth
    from lhvi.flat import flatten
    from lhvi.gauss_exact import ExactGaussian
    g, _ = synth.gaussian_chain(8)
    flat = flatten(g)
    ExactGaussian(flat)
    with pytest.raises(ValueError, match='ground graph'):
        ExactGaussian(dataclasses.replace(flat, lifted=True))
