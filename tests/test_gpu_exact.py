"""GPU suite of the exact hybrid-Gaussian baseline (lhvi/exact.py, csrc/exact.hip) against the reference's recorded results
(tests/golden/exact_*.npz, scripts/capture_exact.py).

Tolerances (docs/kernels_exact.md): log table, logZ, means, variances, covariances rtol 1e-10 (relative to max(1, |value|) for
the log quantities); discrete marginals atol 1e-10; belief_all rtol 1e-10 in log space; continuous marginal MAP: the mixture
log density at the device's answer is not below the one at the reference's by more than 1e-12 max(1, |value|), and
|x - x_ref| <= 1e-4; discrete marginal MAP: equal states."""
import numpy as np
import pytest

import exact_models as em
from lhvi import exact
from lhvi.graph import F, RV, Domain, Graph
from lhvi.potentials import LogHybridQuadratic, LogQuadratic, LogTable

pytestmark = pytest.mark.gpu
RTOL = 1e-10


def bn_of(name):
    """(table, means, covs, logZ, Vd, Vc, Vd_idx, Vc_idx) of a fixture's model: convert_to_bn where the reference's function
    applies (log potentials given, no evidence), the solver class with keep_cov for the evidence model"""
    if name == 'rand_8_8_ev':
        _, s = em.solver(name)
        s.run(keep_cov=True)
        return s.disc_table, s.means, s.covs, s.logZ, s.Vd, s.Vc, s.Vd_idx, s.Vc_idx
    model = em.build(name, **({'hand': True} if name == 'ref_mln0' else {}))
    Vd_idx, Vc_idx = em.set_indices(model)
    out = exact.convert_to_bn(model['factors'], model['Vd'], model['Vc'], return_logZ=True)
    return out + (model['Vd'], model['Vc'], Vd_idx, Vc_idx)


@pytest.fixture(scope='module', params=em.NAMES)
def case(request):
    return request.param, em.load_golden(request.param), bn_of(request.param)


def test_bn_parameters_match_reference(case):
    name, gold, (table, means, covs, logZ, Vd, Vc, _, _) = case
    M, Nc, rows = table.size, len(Vc), gold['cfg']
    assert list(table.shape) == list(gold['dstates']) and means.shape == table.shape + (Nc,) and covs.shape == table.shape + (Nc, Nc)
    em.assert_log_close(logZ, gold['logZ'], RTOL, 'logZ')
    em.assert_log_close(np.log(table.reshape(M)[rows]), np.log(gold['table']), RTOL, 'log table')
    np.testing.assert_allclose(means.reshape(M, Nc)[rows], gold['means'], rtol=RTOL, atol=1e-12)
    var = np.diagonal(covs, axis1=-2, axis2=-1).reshape(M, Nc)
    np.testing.assert_allclose(var[rows], gold['variances'], rtol=RTOL)
    if 'covs_tril' in gold:
        np.testing.assert_allclose(em.tril(covs.reshape(M, Nc, Nc)), gold['covs_tril'], rtol=RTOL, atol=1e-13)
    np.testing.assert_array_equal(covs, np.swapaxes(covs, -1, -2))
    assert abs(table.sum() - 1) <= 1e-12


def test_helpers_match_reference(case):
    name, gold, (table, means, covs, logZ, Vd, Vc, Vd_idx, Vc_idx) = case
    marg = np.concatenate([exact.get_drv_marg(table, i) for i in range(len(Vd))])
    np.testing.assert_allclose(marg, gold['marg'], rtol=0, atol=1e-10)
    for j, rv in enumerate(Vc):
        w, mu, var = exact.get_crv_marg(table, means, covs, j)
        got = exact.get_scalar_gm_log_prob(gold['bel_x'][j], w, mu, var)
        np.testing.assert_allclose(got, gold['bel_logp'][j], rtol=RTOL, atol=0)
    for v, rv in enumerate(list(Vd) + list(Vc)):
        if not gold['maps_recorded'][v]:
            continue
        got = exact.get_rv_marg_map_from_bn_params(table, means, covs, Vd_idx, Vc_idx, rv)
        if rv in Vd_idx:
            assert got == gold['maps'][v] == exact.get_drv_marg_map(table, Vd_idx[rv])
            continue
        w, mu, var = exact.get_crv_marg(table, means, covs, Vc_idx[rv])
        f_got, f_ref = exact.get_scalar_gm_log_prob(np.array([got, gold['maps'][v]]), w, mu, var)
        print('%s rv %d: map %.10g (reference %.10g), log density %.15g (reference %.15g)' % (name, v, got, gold['maps'][v], f_got, f_ref))
        assert f_got >= f_ref - 1e-12 * max(1.0, abs(f_ref))
        assert abs(got - gold['maps'][v]) <= 1e-4


def test_solver_class_equals_convert_to_bn_bit_for_bit(case):
    name, gold, (table, means, covs, logZ, Vd, Vc, _, _) = case
    if name == 'ref_mln0':      # bit for bit on the same log potentials (the hand conversion's table is log(exp(w f)))
        hand = em.build(name, hand=True)
        s = exact.ExactHybridGaussian(factors=hand['factors'], Vd=hand['Vd'], Vc=hand['Vc'])
    else:
        _, s = em.solver(name)
    for keep_cov in (False, True):
        s.run(keep_cov=keep_cov)
        np.testing.assert_array_equal(s.disc_table, table)
        np.testing.assert_array_equal(s.means, means)
        np.testing.assert_array_equal(s.variances, np.diagonal(covs, axis1=-2, axis2=-1))
        assert s.logZ == logZ
        assert (s.covs is None) == (not keep_cov)
        if keep_cov:
            np.testing.assert_array_equal(s.covs, covs)
    if name == 'ref_mln0':      # and the automatic conversion of the MLN potentials against the reference
        _, s = em.solver(name)
        s.run()
        em.assert_log_close(s.logZ, gold['logZ'], RTOL, 'logZ')
        em.assert_log_close(np.log(s.disc_table.ravel()), np.log(gold['table']), RTOL, 'log table')
        np.testing.assert_allclose(s.means.reshape(-1, 2), gold['means'], rtol=RTOL, atol=1e-12)
        np.testing.assert_allclose(s.variances.reshape(-1, 2), gold['variances'], rtol=RTOL)
    # the batched queries: belief_all against the recorded densities, map_all against the recorded MAPs
    x = np.zeros((len(s.rvs), gold['bel_x'].shape[1]))
    crow = [v for v, rv in enumerate(s.rvs) if rv in s.Vc_idx]
    x[crow] = gold['bel_x']
    b = s.belief_all(x).cpu().numpy()
    np.testing.assert_allclose(np.log(b[crow]), gold['bel_logp'], rtol=RTOL, atol=0)
    off = 0
    for v, rv in enumerate(s.rvs):
        if rv in s.Vd_idx:
            np.testing.assert_allclose(b[v, :rv.dstates], gold['marg'][off:off + rv.dstates], rtol=0, atol=1e-10)
            assert s.belief(rv.domain.values[1], rv) == b[v, 1]
            off += rv.dstates
        elif rv.value is not None:
            assert s.map(rv) == rv.value and s.belief(rv.value, rv) == 1 and s.belief(rv.value + 1, rv) == 0
    maps, vals = s.map_all()
    hidden = list(s.Vd) + list(s.Vc)
    for k, rv in enumerate(hidden):
        v = s.rvs.index(rv)
        assert s.map(rv) == maps[v]
        if not gold['maps_recorded'][k]:
            continue
        if rv in s.Vd_idx:
            assert maps[v] == rv.domain.values[int(gold['maps'][k])]
        else:
            f_ref = s.belief(float(gold['maps'][k]), rv, log_belief=True)
            print('%s rv %d: map_all %.10g (reference %.10g), log density %.15g (at the reference value %.15g)'
                  % (name, k, maps[v], gold['maps'][k], vals[v], f_ref))
            assert abs(maps[v] - gold['maps'][k]) <= 1e-4
            assert vals[v] >= f_ref - 1e-12 * max(1.0, abs(f_ref))
            assert abs(s.belief(maps[v], rv, log_belief=True) - vals[v]) <= 1e-12 * max(1.0, abs(vals[v]))


def test_packed_and_one_wavefront_kernels_agree_bit_for_bit():
    _, s = em.solver('rand_8_8')
    runs = [exact._DeviceRun(s.model, keep_cov=True, lanes=lanes) for lanes in (8, 64, 8)]
    assert exact.default_lanes(8) == 8
    for r in runs[1:]:                   # lanes = 64: one wavefront per configuration; the second packed run: the same bits again
        for k in ('logp', 'table', 'logZ', 'means', 'vars', 'covs', 'marg'):
            a, b = getattr(runs[0], k).cpu().numpy(), getattr(r, k).cpu().numpy()
            np.testing.assert_array_equal(a, b, err_msg=k)


def test_device_equals_host_code():
    gold = em.load_golden('rand_12_16')
    _, s = em.solver('rand_12_16')
    r = exact._DeviceRun(s.model, keep_cov=False)
    logp, means, var = r.logp.cpu().numpy(), r.means.cpu().numpy(), r.vars.cpu().numpy()
    for cfg in gold['cfg']:
        lp, mu, v, _ = exact.config_host(s.model, int(cfg))
        assert abs(logp[cfg] - lp) <= 1e-13 * max(1.0, abs(lp))
        np.testing.assert_allclose(means[cfg], mu, rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(var[cfg], v, rtol=1e-13)


def test_no_discrete_variable_equals_gabp_on_a_tree():
    from lhvi import synth
    from lhvi.gabp import GaBP
    g, rvs = synth.gaussian_chain(10)
    bp = GaBP(g)
    bp.run(20)
    s = exact.ExactHybridGaussian(g).run()
    assert s.disc_table.shape == () and s.disc_table == 1.0 and s.means.shape == (9,)
    for rv in rvs[1:]:
        mu, var = bp.get_belief_params(rv)
        assert abs(s.means[s.Vc_idx[rv]] - mu) <= 1e-10 * max(1.0, abs(mu))
        assert abs(s.variances[s.Vc_idx[rv]] - var) <= 1e-10 * var
        assert abs(s.map(rv) - mu) <= 1e-9
    assert s.map(rvs[0]) == rvs[0].value


def test_no_continuous_variable_equals_enumeration():
    rng = np.random.RandomState(5)
    doms = [Domain(tuple(range(d))) for d in (2, 3, 2, 4)]
    Vd = [RV(d) for d in doms]
    scopes = [(0,), (1, 2), (3, 0), (2, 3, 1)]
    factors = [F(nb=tuple(Vd[i] for i in sc), log_potential_fun=LogTable(rng.randn(*[Vd[i].dstates for i in sc]))) for sc in scopes]
    s = exact.ExactHybridGaussian(factors=factors, Vd=Vd, Vc=[]).run(keep_cov=True)
    want = np.zeros([rv.dstates for rv in Vd])
    for idx in np.ndindex(*want.shape):
        want[idx] = sum(f.log_potential_fun(tuple(idx[i] for i in sc)) for f, sc in zip(factors, scopes))
    logZ = np.log(np.exp(want).sum())
    assert abs(s.logZ - logZ) <= RTOL * max(1.0, abs(logZ))
    np.testing.assert_allclose(s.disc_table, np.exp(want - logZ), rtol=RTOL)
    assert s.means.shape == want.shape + (0,) and s.covs.shape == want.shape + (0, 0)
    for i, rv in enumerate(Vd):
        np.testing.assert_allclose(s.disc_marginals[i], exact.get_drv_marg(np.exp(want - logZ), i), rtol=0, atol=1e-10)


def big_model(Nd, Nc, seed=0):
    """Nd binary variables, Nc continuous: a dense diagonally dominant base quadratic, one hybrid factor per discrete variable"""
    rng = np.random.RandomState(seed)
    db, dc = Domain((0, 1)), Domain((-10, 10), continuous=True)
    Vd, Vc = [RV(db) for _ in range(Nd)], [RV(dc) for _ in range(Nc)]
    B = rng.randn(Nc, Nc) / np.sqrt(Nc)
    factors = [F(nb=tuple(Vc), log_potential_fun=LogQuadratic(-0.5 * (B @ B.T + np.eye(Nc)), rng.randn(Nc), 0.))]
    for d in Vd:
        j = int(rng.randint(Nc))
        factors.append(F(nb=(d, Vc[j]), log_potential_fun=LogHybridQuadratic(-0.5 * rng.rand(2, 1, 1), rng.randn(2, 1), 0.1 * rng.randn(2))))
    return factors, Vd, Vc


@pytest.mark.parametrize('Nd,Nc', [(6, 64), (20, 8)])
def test_largest_sizes_run_and_sum_to_one(Nd, Nc):
    """Nc = LHVI_EXACT_MAX_NC, and 2^20 configurations: |sum - 1| <= 1e-9 (a sum of M = 2^20 terms is off by at most M u = 1.2e-10)"""
    factors, Vd, Vc = big_model(Nd, Nc)
    s = exact.ExactHybridGaussian(factors=factors, Vd=Vd, Vc=Vc).run()
    assert s.disc_table.size == 2 ** Nd and s.covs is None
    assert abs(float(s._run.table.sum().item()) - 1) <= 1e-9
    assert np.isfinite(s.means).all() and (s.variances > 0).all()
    for i in range(Nd):
        assert abs(s.disc_marginals[i].sum() - 1) <= 1e-9
    lp, mu, var, _ = exact.config_host(s.model, s.model.M - 1)
    np.testing.assert_allclose(s.means.reshape(-1, Nc)[-1], mu, rtol=1e-12, atol=1e-13)


def test_not_positive_definite_raises_with_the_lowest_configuration():
    from test_exact_host import not_pd_model
    factors, Vd, Vc = not_pd_model()
    with pytest.raises(ValueError, match=r'not positive definite.*\(0, 1\)'):
        exact.ExactHybridGaussian(factors=factors, Vd=Vd, Vc=Vc).run()


def test_kl_of_epbp_against_the_exact_marginals():
    """the use case: kl_tables of a solver's belief_all against the exact belief_all; no threshold on EPBP's quality, only
    finite and better than a uniform belief"""
    import torch
    from lhvi.pbp import EPBP
    from lhvi.utils import kl_tables
    model = em.build('ref_mln0')
    g = Graph()
    g.rvs, g.factors = model['rvs'], model['factors']
    g.init_nb()
    s = exact.ExactHybridGaussian(g).run()
    bp = EPBP(g, n=20, proposal_approximation='simple')
    bp.run(10, log_enable=False)
    assert [rv.id for rv in bp.flat.rvs] == [rv.id for rv in s.rvs]
    m = 20
    x = np.zeros((len(s.rvs), m))
    crow = [v for v, rv in enumerate(s.rvs) if rv.domain.continuous]
    x[crow] = np.linspace(-10, 10, m)
    p, q = s.belief_all(x)[crow], bp.belief_all(x)[crow]
    kl = kl_tables(p, q, -10., 10.).cpu().numpy()
    kl_uniform = kl_tables(p, torch.full_like(p, 1 / 20.), -10., 10.).cpu().numpy()
    print('KL(exact || EPBP) = %s, KL(exact || uniform) = %s' % (kl, kl_uniform))
    assert np.isfinite(kl).all() and (kl < kl_uniform).all()
    for v in range(2):
        np.testing.assert_allclose(s.belief_all(x)[v, :2].cpu().numpy(), s.disc_marginals[v])
