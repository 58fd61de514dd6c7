"""CPU suite of the annealed importance sampler (lhvi/ais.py, docs/kernels_ais.md): the device's per-chain code run on the host
(lhvi_ais_chain_host) against the NumPy restatement of one annealing run (tests/ais_models.py), the split of a run over calls,
the telescoping and one-step identities, the beta = 1 end against the block Gibbs sampler, the Philox stream against its written
counter layout, the estimates and the errors.

Tolerances: final x_d equal; logw within 1e-9 relative to max(1, |logw|) (the deterministic Gibbs test's tolerance:
cond(J_beta) <= max(cond J, 1) <= 500 is asserted by the restatement); the telescoping sum within 2 T x 1e-10 x max(1, |log m|)
(2 T collapsed masses, each at the exact baseline's stated tolerance)."""
import math

import numpy as np
import pytest

import ais_models as am
import exact_models as em
import gibbs_models as gmod
from lhvi import ais, exact, gibbs

T = len(am.BETAS) - 1


def host_run(model, x0, z, u, chains=am.CHAINS, **kw):
    mu0 = am.mu0_of(len(model['Vc']))
    out = [ais.chain_host(model['gm'], x0[c], am.BETAS, am.TAU0, mu0, am.SWEEPS, z=z[:, c], u=u[:, c], **kw) for c in range(chains)]
    return np.array([r.x_d for r in out]).reshape(chains, -1), np.array([r.logw for r in out])


@pytest.mark.parametrize('name', am.DET_HOST)
def test_host_chain_equals_numpy_restatement(name):
    model, x0, z, u, _, want_lw = am.restated(name)
    x_d, logw = host_run(model, x0, z, u)
    print('%s: logw %s' % (name, np.array2string(want_lw, precision=4)))
    am.assert_matches(name, x_d, logw, 'host')


def test_run_split_over_calls_equals_one_call():
    model, x0, z, u, _, _ = am.restated('rand_8_8')
    mu0 = am.mu0_of(8)
    for c in range(am.CHAINS):
        one = ais.chain_host(model['gm'], x0[c], am.BETAS, am.TAU0, mu0, am.SWEEPS, z=z[:, c], u=u[:, c])
        a = ais.chain_host(model['gm'], x0[c], am.BETAS, am.TAU0, mu0, am.SWEEPS, z=z[:, c], u=u[:, c], t_end=2)
        b = ais.chain_host(model['gm'], a.x_d, am.BETAS, am.TAU0, mu0, am.SWEEPS, z=z[:, c], u=u[:, c], t_begin=2, logw=a.logw)
        assert b.logw == one.logw and np.array_equal(b.x_d, one.x_d)


def test_without_discrete_variables_the_weights_telescope_to_log_z():
    """Nd = 0: every chain's logw is the same number, log Z0 + logw is the exact log Z, the standard errors are 0"""
    model = gmod.build('no_disc')
    Nc = 5
    mu0 = am.mu0_of(Nc)
    rng = np.random.RandomState(3)
    logw = np.array([ais.chain_host(model['gm'], [], am.BETAS, am.TAU0, mu0, am.SWEEPS, z=rng.randn(T, Nc)).logw for _ in range(4)])
    assert (logw == logw[0]).all()
    want = em.numpy_config(model['factors'], [], Nc, ())[0]
    scale = max(1.0, max(abs(am.collapsed_mass(model, [], b, am.TAU0, mu0)[0]) for b in am.BETAS))
    logZ0 = ais.log_z0([], Nc, am.TAU0)
    assert logZ0 == 0.5 * Nc * math.log(2 * math.pi / am.TAU0)
    print('no_disc: log Z0 + logw - log Z = %.3g (bound %.3g)' % (logZ0 + logw[0] - want, 2 * T * 1e-10 * scale))
    assert abs(logZ0 + logw[0] - want) <= 2 * T * 1e-10 * scale
    est = ais.estimates(ais.reduce_numpy(logw), len(logw), logZ0)
    assert est.stderr == 0.0 and est.lower_stderr == 0.0 and est.ess == 1.0 and est.obj == -est.logZ
    assert abs(est.logZ - want) <= 2 * T * 1e-10 * scale and abs(est.lower - want) <= 2 * T * 1e-10 * scale


@pytest.mark.parametrize('name', ['rand_3_2', 'wide_states', 'pure_disc'])
def test_one_step_weighs_the_initial_state_by_its_collapsed_mass(name):
    """betas = [0, 1]: log Z0 + logw = sum log dstates + log p~(x_d) of the exact baseline at the chain's initial state"""
    model = gmod.build(name)
    gm = model['gm']
    Nc, dstates = gm.ex.Nc, model['dstates']
    mu0 = am.mu0_of(Nc)
    x0 = gmod.philox_init(11, 6, dstates)
    for c in range(6):
        r = ais.chain_host(gm, x0[c], [0., 1.], am.TAU0, mu0, 1, seed=11, chain=c)
        assert np.array_equal(r.x_d, x0[c])
        want = sum(math.log(d) for d in dstates) + exact.config_at_host(gm.ex, x0[c])[0]
        em.assert_log_close(ais.log_z0(dstates, Nc, am.TAU0) + r.logw, want, 1e-10, '%s chain %d' % (name, c))


@pytest.mark.parametrize('name', ['rand_8_8', 'deep_scope', 'pure_disc'])
def test_the_end_of_the_path_is_the_block_gibbs_sampler(name):
    """betas = [0, 1, 1, 1]: the increments of steps 1 and 2 are exactly 0.0 and the two transitions are two iterations of
    gibbs.chain_host from the same state with the same draws (a product with 1 and a sum with 0 are exact)"""
    model = gmod.build(name)
    gm = model['gm']
    Nc = gm.ex.Nc
    mu0 = am.mu0_of(Nc)
    x0, z, u = am.draws(model, T=3)
    betas = [0., 1., 1., 1.]
    for c in range(am.CHAINS):
        a = ais.chain_host(gm, x0[c], betas, am.TAU0, mu0, am.SWEEPS, z=z[:, c], u=u[:, c], t_end=1)
        b = ais.chain_host(gm, a.x_d, betas, am.TAU0, mu0, am.SWEEPS, z=z[:, c], u=u[:, c], t_begin=1, t_end=2)
        d = ais.chain_host(gm, b.x_d, betas, am.TAU0, mu0, am.SWEEPS, z=z[:, c], u=u[:, c], t_begin=2)
        assert b.logw == 0.0 and d.logw == 0.0 and a.logw != 0.0
        assert np.array_equal(d.x_d, b.x_d)                      # the last step makes no transition
        want = gibbs.chain_host(gm, x0[c], z[:2, c], u[:2, c], am.SWEEPS, 0, 2)
        assert np.array_equal(b.x_d, want.x_d)


@pytest.mark.parametrize('name', ['rand_8_8', 'wide_states'])
def test_host_generator_equals_its_specification(name):
    """z and u restated in NumPy from the counters of docs/kernels_ais.md, injected, against the host twin drawing for itself"""
    model = gmod.build(name)
    gm = model['gm']
    Nc, Nd, seed, chains = gm.ex.Nc, gm.ex.Nd, 20261021, 5
    z, u = am.philox_normals(seed, chains, T, Nc), am.philox_uniforms(seed, chains, T, am.SWEEPS, Nd)
    assert np.abs(z).max() < 6 and 0 <= u.min() and u.max() < 1
    x0 = gmod.philox_init(seed, chains, model['dstates'])
    mu0 = am.mu0_of(Nc)
    for c in range(chains):
        a = ais.chain_host(gm, x0[c], am.BETAS, am.TAU0, mu0, am.SWEEPS, seed=seed, chain=c)
        b = ais.chain_host(gm, x0[c], am.BETAS, am.TAU0, mu0, am.SWEEPS, z=z[:, c], u=u[:, c])
        assert np.array_equal(a.x_d, b.x_d)
        assert abs(a.logw - b.logw) <= 1e-9 * max(1.0, abs(b.logw))     # sin / cos / log of the two libraries


def test_estimates_from_the_sums():
    rng = np.random.RandomState(5)
    lw = 300.0 + 0.4 * rng.randn(1000)
    est = ais.estimates(ais.reduce_numpy(lw), lw.size, 2.5, log_const=-1.0)
    w = np.exp(lw - lw.max())
    assert abs(est.logZ - (1.5 + lw.max() + np.log(w.mean()))) < 1e-12 * 300
    assert abs(est.stderr - (w / w.mean()).std() / np.sqrt(lw.size)) < 1e-12
    assert abs(est.ess - w.sum() ** 2 / (lw.size * (w * w).sum())) < 1e-12
    assert abs(est.lower - (1.5 + lw.mean())) < 1e-12 * 300
    assert abs(est.lower_stderr - lw.std(ddof=1) / np.sqrt(lw.size)) < 1e-12
    assert est.lower <= est.logZ


def test_schedule_and_base_errors():
    gm = gmod.build('rand_3_2')['gm']
    for bad in ([0., .6, .5, 1.], [0., .5], [.1, .5, 1.], [0., float('nan'), 1.], [1.]):
        with pytest.raises(ValueError, match='betas'):
            ais.schedule(betas=bad)
        with pytest.raises(ValueError, match='betas'):
            ais.chain_host(gm, [0, 0, 0], bad, 1.0, None)
    with pytest.raises(ValueError, match='steps'):
        ais.schedule(0)
    assert np.array_equal(ais.schedule(4), [0., .25, .5, .75, 1.])
    with pytest.raises(ValueError, match='base_prec'):
        ais.base(2, None, 0.0)
    with pytest.raises(ValueError, match='base_mean'):
        ais.base(2, [0., 1., 2.], 1.0)
    with pytest.raises(ValueError, match='outside'):
        ais.chain_host(gm, [0, 5, 0], [0., 1.], 1.0, None)


def test_not_positive_definite_raises_the_samplers_error():
    gm = gmod.build('not_pd')['gm']
    with pytest.raises(ValueError, match=r'not positive definite at the discrete state \(0, 1\)'):
        ais.chain_host(gm, [0, 1], [0., .5, 1.], 1.0, None, 0, z=np.zeros((2, 2)))
    assert math.isfinite(ais.chain_host(gm, [1, 0], [0., .5, 1.], 1.0, None, 0, z=np.zeros((2, 2))).logw)


def test_public_entry_points_exist():
    import inspect
    import importlib
    import os
    import sys
    sig = inspect.signature(gibbs.GibbsHybridGaussian.log_partition)
    want = dict(chains=4096, steps=256, betas=None, disc_block_its=1, seed=0, base_mean=None, base_prec=None, lanes=None,
                steps_per_launch=None)
    for fn in (gibbs.GibbsHybridGaussian.log_partition, gibbs.HybridGaussianSampler.log_partition, gibbs.ais_log_partition):
        sig = inspect.signature(fn)
        assert {k: sig.parameters[k].default for k in want} == want
        assert 'never biases' in fn.__doc__
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                    'lifted-hybrid-variational-inference_amd', 'compat'))
    try:
        compat = importlib.import_module('hybrid_gaussian_mrf')
    finally:
        sys.path.pop(0)
    assert compat.ais_log_partition is gibbs.ais_log_partition
    assert compat.HybridGaussianSampler.log_partition is gibbs.HybridGaussianSampler.log_partition
