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


# ---- shapes the fixtures lack (exact_models.SHAPE_SPECS; each proven on the CPU in tests/test_exact_host.py) --------------------------
OUTPUTS = ('logp', 'table', 'logZ', 'means', 'vars', 'covs', 'marg')


def allowed_lanes(Nc, Nd):
    from lhvi import _abi
    return [l for l in (1, 2, 4, 8, 16, 32, 64) if _abi.lib().lhvi_exact_lds_bytes(Nc, Nd, l) <= 64 * 1024]


def outputs_of(run):
    return {k: getattr(run, k).cpu().numpy() for k in OUTPUTS}


@pytest.fixture(scope='module', params=em.SHAPES)
def shape(request):
    """(name, flat model, numpy_config over every configuration, the run at the first allowed lane count)"""
    model = em.build(request.param)
    em.set_indices(model)
    dstates = [rv.dstates for rv in model['Vd']]
    m = exact.flatten_factors(model['factors'], dstates, len(model['Vc']))
    lanes = allowed_lanes(m.Nc, m.Nd)
    return request.param, m, em.enumerate_numpy(model), lanes, outputs_of(exact._DeviceRun(m, keep_cov=True, lanes=lanes[0]))


def test_shape_configurations_equal_numpy_and_host_code(shape):
    """every configuration: log p~, means and full covariances against numpy_config at RTOL (c n cond(J) u: 64 * 500 * 1.1e-16
    = 4e-12 at the largest matrix), and against the host run of the same code at the 1e-13 of test_device_equals_host_code"""
    name, m, (want_lp, want_mu, want_sig, cond), lanes, got = shape
    assert cond <= 500
    em.assert_log_close(got['logp'], want_lp, RTOL, 'log p~')
    np.testing.assert_allclose(got['means'], want_mu, rtol=RTOL, atol=1e-12)
    np.testing.assert_allclose(got['covs'], want_sig, rtol=RTOL, atol=1e-12)
    np.testing.assert_array_equal(got['vars'], np.diagonal(got['covs'], axis1=1, axis2=2))
    np.testing.assert_array_equal(got['covs'], np.swapaxes(got['covs'], 1, 2))
    err = 0.0
    for cfg in range(m.M):
        lp, mu, v, cov = exact.config_host(m, cfg, cov=True)
        assert abs(got['logp'][cfg] - lp) <= 1e-13 * max(1.0, abs(lp))
        np.testing.assert_allclose(got['means'][cfg], mu, rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(got['vars'][cfg], v, rtol=1e-13)
        np.testing.assert_allclose(got['covs'][cfg], cov, rtol=1e-13, atol=1e-13)
        err = max(err, np.abs(got['means'][cfg] - mu).max() if m.Nc else 0.0)
    print('%s: lanes %s, max cond(J) %.3g, max |log p~ - numpy| %.3g, max |mean - host| %.3g'
          % (name, lanes, cond, np.abs(got['logp'] - want_lp).max(), err))


def test_shape_lane_counts_agree_bit_for_bit(shape):
    """every power-of-two lane count whose workgroup fits 64 KiB: idle lanes (lanes > Nc), ragged row ownership (lanes does not
    divide Nc), one lane"""
    name, m, _, lanes, base = shape
    if name in ('wide_states', 'deep_scope', 'nc1', 'nc7'):
        assert lanes == [1, 2, 4, 8, 16, 32, 64]
    for l in lanes[1:]:
        other = outputs_of(exact._DeviceRun(m, keep_cov=True, lanes=l))
        for k in OUTPUTS:
            np.testing.assert_array_equal(base[k], other[k], err_msg='%s, lanes %d against %d' % (k, l, lanes[0]))


def test_nc64_fills_the_lds_and_half_a_wavefront_is_refused(shape):
    from lhvi import _abi
    name, m, _, lanes, _ = shape
    if name != 'nc64':
        return
    assert lanes == [64] and _abi.lib().lhvi_exact_lds_bytes(64, 2, 32) > 64 * 1024
    # refused by the entry point's own check of the LDS size, before the launch
    with pytest.raises(_abi.LhviError, match='unsupported configuration'):
        exact._DeviceRun(m, keep_cov=True, lanes=32)


@pytest.mark.parametrize('name', ['deep_scope', 'wide_states'])
def test_chunked_launches_equal_one_launch_bit_for_bit(name):
    """chunks of 7 configurations at 8 lanes (8 groups a workgroup): cfg_begin > 0, a count below one workgroup with a padding
    group in every launch, a short last chunk"""
    model = em.build(name)
    em.set_indices(model)
    m = exact.flatten_factors(model['factors'], [rv.dstates for rv in model['Vd']], len(model['Vc']))
    assert m.M % 7 and m.M > 21
    one, many = outputs_of(exact._DeviceRun(m, keep_cov=True, lanes=8)), outputs_of(exact._DeviceRun(m, keep_cov=True, lanes=8, chunk=7))
    for k in OUTPUTS:
        np.testing.assert_array_equal(one[k], many[k], err_msg=k)


# ---- reductions at the M where their geometry changes (exact_models.reduction_model, Nc = 1) -------------------------------------
def reduction_run(M):
    from test_exact_host import REDUCTION_DSTATES
    dstates = list(REDUCTION_DSTATES[M])
    model = em.reduction_model(em.local_ns(), dstates)
    em.set_indices(model)
    m = exact.flatten_factors(model['factors'], dstates, 1)
    return m, exact._DeviceRun(m, keep_cov=False)


@pytest.mark.parametrize('M', [243, 256, 288, 177147, 262144, 531441])
def test_reductions_against_exactly_rounded_sums(M):
    """logZ, the table and every marginal recomputed on the host from the device's log p~: math.fsum for logZ, np.longdouble for
    the marginals.  Bounds from the kernels' fixed order of additions (docs/kernels_exact.md, "Tests"):
    logZ: the longest chain is ceil(per / 256) + 8 + 4 + 8 additions of positive terms, one exp each: <= 1e-13, more than ten
    times chain * 2^-53; a marginal of a d-state variable: chain M / (256 d) + 8, atol (M / (256 d) + 64) * 2.3e-16 (the 64
    covers the few-ulp error of a table entry at |log p~ - logZ| <= 60); a table entry: its exponent is off by the error of
    logZ (1e-13) and one rounding of the difference (ulp(64) / 2 = 7e-15), the exp by an ulp: rtol 2e-13."""
    import math
    m, r = reduction_run(M)
    assert m.M == M
    logp = r.logp.cpu().numpy()
    assert logp.max() - logp.min() >= 60
    mx = float(logp.max())
    logZ = mx + math.log(math.fsum(np.exp(logp - mx)))
    got_logZ = float(r.logZ.item())
    table = np.exp(logp - logZ)
    got_table = r.table.cpu().numpy()
    rel = np.abs(got_table - table) / table
    marg, off, worst = r.marg.cpu().numpy(), 0, 0.0
    joint = table.reshape(tuple(m.dstates)).astype(np.longdouble)
    for i, d in enumerate(m.dstates):
        want = joint.sum(axis=tuple(a for a in range(m.Nd) if a != i), dtype=np.longdouble)
        err = float(np.abs(marg[off:off + d] - want).max())
        atol = (M / (256. * d) + 64) * 2.3e-16
        worst = max(worst, err / atol)
        assert err <= atol, 'marginal of variable %d: error %.3g, bound %.3g' % (i, err, atol)
        off += d
    print('M = %d: |logZ - fsum| = %.3g (bound 1e-13), table rel %.3g (bound 2e-13), marginals at most %.3g of their bound'
          % (M, abs(got_logZ - logZ), rel.max(), worst))
    assert abs(got_logZ - logZ) <= 1e-13
    assert rel.max() <= 2e-13
    # log p~ itself against the host run of the same code: the ends, both sides of every launch boundary, 32 seeded ones
    cfgs = {0, M - 1} | set(int(c) for c in np.random.RandomState(M % 1000).randint(M, size=32))
    for b in range(exact.CHUNK, M, exact.CHUNK):
        cfgs |= {b - 1, b}
    means, var = r.means.cpu().numpy(), r.vars.cpu().numpy()
    for cfg in sorted(cfgs):
        lp, mu, v, _ = exact.config_host(m, cfg)
        assert abs(logp[cfg] - lp) <= 1e-13 * max(1.0, abs(lp)), cfg
        np.testing.assert_allclose(means[cfg], mu, rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(var[cfg], v, rtol=1e-13)


# ---- the mixture and polish kernels against a longdouble mixture --------------------------------------------------------------------
MIX_DOMAIN = (-42, 42)      # every mean is within 3.6 of the origin, every variance <= 1: at the ends every exponent is below -700


def mixture_ref(w, mu, var, x, keep=None):
    """log density, first and second derivative of sum_k w_k N(x; mu_k, var_k) in np.longdouble at the points x, and the two
    sums over absolute values that bound the derivatives' errors: (f [m], g [m], h [m], G [m], H [m], largest exponent [m])"""
    ld = np.longdouble
    w, mu, var = (np.asarray(a, dtype=ld) for a in (w, mu, var))
    if keep is not None:
        w, mu, var = w[keep], mu[keep], var[keep]
    out = []
    for xi in np.asarray(x, dtype=ld):
        a = (mu - xi) / var
        t = np.log(w) - ld(0.5) * np.log(2 * ld(np.pi) * var) - ld(0.5) * (mu - xi) * a
        mx = t.max()
        p = np.exp(t - mx)
        s0 = p.sum()
        g = (p * a).sum() / s0
        out.append((mx + np.log(s0), g, (p * (a * a - 1 / var)).sum() / s0 - g * g, (p * np.abs(a)).sum() / s0,
                    (p * np.abs(a * a - 1 / var)).sum() / s0, mx))
    return tuple(np.array(c, dtype=ld) for c in zip(*out))


def assert_mixture(got, ref, what):
    """log density: 1e-10 relative to max(1, |value|).  Derivatives: each is a quotient of signed sums, (log f)' = S1 / S0 and
    (log f)'' = S2 / S0 - (S1 / S0)^2 with S1 = sum p_k a_k, S2 = sum p_k (a_k^2 - 1 / var_k), a_k = (mu_k - x) / var_k; the
    bound is 1e-12 times the same sums over absolute values, G = sum p_k |a_k| / S0 for the first and
    H + G^2 = sum p_k |a_k^2 - 1 / var_k| / S0 + G^2 for the second, computed in the reference"""
    f, g, h, G, H, _ = ref
    e0 = np.abs(got[:, 0] - f) / np.maximum(1, np.abs(f))
    e1, e2 = np.abs(got[:, 1] - g) / G, np.abs(got[:, 2] - h) / (H + G * G)
    print('%s: log density %.3g (bound 1e-10), first derivative %.3g, second %.3g of the absolute sums (bound 1e-12)'
          % (what, e0.max(), e1.max(), e2.max()))
    assert e0.max() <= 1e-10 and e1.max() <= 1e-12 and e2.max() <= 1e-12


def mixture_case(run, j=0):
    w, mu, var = run.table.cpu().numpy(), run.means.cpu().numpy()[:, j], run.vars.cpu().numpy()[:, j]
    top = np.argsort(w)[::-1][:3]
    x = np.array(list(mu[top]) + [0.5 * (mu[top[0]] + mu[top[1]]), 0.5 * (mu.min() + mu.max()), mu.max() + 2.5, mu.min() - 4.0,
                                  MIX_DOMAIN[0], MIX_DOMAIN[1]])
    return w, mu, var, x


@pytest.mark.parametrize('M', [90, 531441])
def test_mixture_value_and_derivatives_against_longdouble(M):
    """M = 90: fewer components than threads (idle threads merge an empty accumulator); M = 531441: 2076 components a thread"""
    import torch
    if M == 90:
        model = em.build('wide_states', cdom=MIX_DOMAIN)
        em.set_indices(model)
        run = exact._DeviceRun(exact.flatten_factors(model['factors'], [9, 5, 2], 3), keep_cov=False)
    else:
        run = reduction_run(M)[1]
    Nc = run.model.Nc
    cases = [mixture_case(run, j) for j in range(Nc)]
    x = torch.from_numpy(np.stack([c[3] for c in cases])).to(run.logp.device)
    got = run.mixture(x).cpu().numpy()
    for j, (w, mu, var, xj) in enumerate(cases):
        assert np.abs(mu).max() <= 3.6 and var.max() <= 1.0
        ref = mixture_ref(w, mu, var, xj)
        assert (ref[5][-2:] < -700).all() and (ref[5][:5] > -100).all()        # the running maximum rescales from below -700
        assert_mixture(got[j], ref, 'M = %d, variable %d' % (M, j))


def test_mixture_skips_components_of_weight_zero():
    """the 9 x 5 table's entry (4, 2) at -800: the two configurations over it have exp(log p~ - logZ) == 0.0 in fp64 (not in
    longdouble, so the reference drops them by hand); the density stays finite, also at those components' own means"""
    import torch
    model = em.build('wide_states', cdom=MIX_DOMAIN)
    em.set_indices(model)
    pair = [f for f in model['factors'] if f.disc_nb_idx == (0, 1)][0]
    pair.log_potential_fun.table[4, 2] = -800.
    run = exact._DeviceRun(exact.flatten_factors(model['factors'], [9, 5, 2], 3), keep_cov=False)
    logp, w = run.logp.cpu().numpy(), run.table.cpu().numpy()
    zero = [int(np.ravel_multi_index((4, 2, k), (9, 5, 2))) for k in range(2)]
    assert (np.exp(logp - float(run.logZ.item()))[zero] == 0.0).all() and (w[zero] == 0.0).all() and np.count_nonzero(w) == 88
    keep = np.setdiff1d(np.arange(90), zero)
    for j in range(3):
        _, mu, var, x = mixture_case(run, j)
        x[:2] = mu[zero]
        got = run.mixture(torch.from_numpy(np.tile(x, (3, 1))).to(run.logp.device)).cpu().numpy()[j]
        assert np.isfinite(got).all()
        assert_mixture(got, mixture_ref(w, mu, var, x, keep), 'weight 0, variable %d' % j)


def test_map_on_the_domain_bound():
    """every component mean of x lies beyond the upper domain value: the marginal MAP is the bound itself"""
    db, dc = Domain((0, 1, 2)), Domain((-10, 10), continuous=True)
    d, x, y = RV(db), RV(dc), RV(dc)
    factors = [F(nb=(x,), log_potential_fun=LogQuadratic(-0.5 * np.ones((1, 1)), np.array([14.]), 0.)),
               F(nb=(y,), log_potential_fun=LogQuadratic(-0.5 * np.ones((1, 1)), np.array([1.]), 0.)),
               F(nb=(d, x, y), log_potential_fun=LogHybridQuadratic(-0.5 * np.array([0.1, 0.2, 0.3])[:, None, None] * np.eye(2),
                                                                    np.array([[1., -1.], [2., 0.5], [0., 3.]]), np.zeros(3))),
               F(nb=(d,), log_potential_fun=LogTable(np.array([0.3, -0.2, 0.1])))]
    s = exact.ExactHybridGaussian(factors=factors, Vd=[d], Vc=[x, y]).run()
    assert s.means[:, 0].min() > 10 and np.abs(s.means[:, 1]).max() < 10
    assert s.map(x) == 10.0
    assert -10 < s.map(y) < 10
    maps, vals = s.map_all()
    assert maps[1] == 10.0 and abs(vals[1] - s.belief(10.0, x, log_belief=True)) <= 1e-12 * max(1.0, abs(vals[1]))


def test_map_from_the_top_candidates_against_a_host_grid():
    """M = 2^17, the smallest all-binary M above MAX_CANDIDATES: cont_map starts from the 2^16 components of largest peak
    density.  Reference: the mixture in np.longdouble on a grid of 31 points over the domain, then a golden-section search in
    the two cells around the best point.  The grid values must have one local maximum, so that the bracket holds the global
    one (the components' standard deviations are 0.9 or more, the cells 0.67 wide).  Criterion of this file: the log density at the device's answer is not below
    the reference's by more than 1e-12 max(1, |f|), and |x - x_ref| <= 1e-4."""
    M = 1 << 17
    assert exact.MAX_CANDIDATES < M <= 2 * exact.MAX_CANDIDATES
    m, run = reduction_run(M)
    x_dev, f_dev = (t.cpu().numpy() for t in run.cont_map([-10.], [10.]))
    w, mu, var = run.table.cpu().numpy(), run.means.cpu().numpy()[:, 0], run.vars.cpu().numpy()[:, 0]
    live = w > 0
    f = lambda x: mixture_ref(w, mu, var, np.atleast_1d(x), live)[0]                   # noqa: E731
    grid = np.linspace(-10, 10, 31)
    fg = f(grid)
    k = int(np.argmax(fg))
    assert 0 < k < 30 and np.count_nonzero((fg[1:-1] > fg[:-2]) & (fg[1:-1] > fg[2:])) == 1
    a, b = np.longdouble(grid[k - 1]), np.longdouble(grid[k + 1])
    inv = (np.sqrt(np.longdouble(5)) - 1) / 2
    c, d = b - inv * (b - a), a + inv * (b - a)
    fc, fd = f(c)[0], f(d)[0]
    for _ in range(36):                     # the bracket shrinks to 4e-8: the density there is flat to 1e-15
        if fc > fd:
            b, d, fd = d, c, fc
            c = b - inv * (b - a)
            fc = f(c)[0]
        else:
            a, c, fc = c, d, fd
            d = a + inv * (b - a)
            fd = f(d)[0]
    x_ref = float((a + b) / 2)
    f_at = f(np.array([x_dev[0], x_ref]))
    print('M = 2^17: map %.10g (host grid %.10g), log density %.17g (at the host value %.17g)'
          % (x_dev[0], x_ref, float(f_at[0]), float(f_at[1])))
    assert f_at[0] >= f_at[1] - 1e-12 * max(1.0, abs(float(f_at[1])))
    assert abs(x_dev[0] - x_ref) <= 1e-4
    assert abs(f_dev[0] - float(f_at[0])) <= 1e-10 * max(1.0, abs(f_dev[0]))
