"""GPU suite of the annealed importance sampler (csrc/ais.hip, lhvi/ais.py, docs/kernels_ais.md): the kernel against the NumPy
restatement of one annealing run at every allowed lane count, bit equality across lanes / launches / chain counts / table
placement, the telescoping, one-step and beta = 1 identities, the reduction kernel, and the estimator against the exact
log Z of the enumerable models.

Deterministic tolerances are those of tests/test_ais_host.py.  Statistical bounds: with w~ = exp(logw + log Z0 - log Z),
|mean(w~) - 1| <= 4.5 std(w~) / sqrt(C) (the sampler tests' bound) and lower - log Z <= 4.5 lower_stderr (Jensen); the steps
per model were chosen ahead on the CPU by the protocol of docs/kernels_ais.md (ais_models.STAT_STEPS)."""
import math

import numpy as np
import pytest

import ais_models as am
import exact_models as em
import gibbs_models as gmod
from lhvi import _abi, ais, exact, gibbs

pytestmark = pytest.mark.gpu
SEED = 20261021
T = len(am.BETAS) - 1


def allowed_lanes(gm, in_lds=True):
    """every power-of-two lane count at which a workgroup's chains fit 64 KiB of LDS"""
    Nc, Nd, disc = gm.ex.Nc, gm.ex.Nd, gm.max_states + (gm.table_doubles if in_lds else 0)
    return [l for l in (1, 2, 4, 8, 16, 32, 64) if 0 < _abi.lib().lhvi_ais_lds_bytes(Nc, Nd, disc, l) <= gibbs.LDS_LIMIT]


def chains_of(gm, chains=am.CHAINS, betas=am.BETAS, lanes=None, split=None, seed=SEED, its=am.SWEEPS, **kw):
    r = ais._AisChains(gm, chains, np.asarray(betas, dtype=np.float64), am.TAU0, am.mu0_of(gm.ex.Nc), its, seed, lanes=lanes, **kw)
    return r.run(split)


def state(r):
    return r.x_d.cpu().numpy(), r.logw.cpu().numpy()


def assert_same(a, b, rows=slice(None)):
    (ax, al), (bx, bl) = state(a), state(b)
    np.testing.assert_array_equal(ax[rows], bx)
    np.testing.assert_array_equal(al[rows], bl)


# ---- injected draws ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', am.DET_HOST + am.DET_SHAPES)
def test_kernel_equals_numpy_restatement(name):
    """every allowed lane count: fewer lanes than states, idle lanes, lanes that do not divide Nc, the one lane count left at
    Nc = 64; x_d and logw bit-identical across them"""
    model, x0, z, u, _, _ = am.restated(name)
    lanes = allowed_lanes(model['gm'])
    assert 64 in lanes and (name not in ('wide_states', 'deep_scope', 'nc1') or lanes == [1, 2, 4, 8, 16, 32, 64])
    assert name != 'nc64' or lanes == [64]
    got = {l: state(chains_of(model['gm'], lanes=l, init_x_d=x0, z=z, u=u)) for l in lanes}
    for l in lanes[1:]:
        np.testing.assert_array_equal(got[lanes[0]][0], got[l][0], err_msg='lanes %d' % l)
        np.testing.assert_array_equal(got[lanes[0]][1], got[l][1], err_msg='lanes %d' % l)
    am.assert_matches(name, *got[lanes[0]], what='kernel')


def test_reduced_tables_in_global_scratch_equal_tables_in_lds():
    """scratch_tables: 630 doubles of reduced tables a chain.  At the default 4 lanes they do not fit and go to global scratch;
    at 8 lanes they fit: the forced-LDS run gives the same bits, with injected draws and with the device generator, and both
    equal the host twin"""
    model = gmod.build('scratch_tables')
    gm = model['gm']
    x0, z, u = am.draws(model)
    a = chains_of(gm, init_x_d=x0, z=z, u=u)
    assert a.lanes == 4 and not a.in_lds and a.scratch.shape == (64, 630)
    b = chains_of(gm, lanes=8, tables='lds', init_x_d=x0, z=z, u=u)
    assert b.in_lds and b.scratch is None
    with pytest.raises(ValueError, match='bytes of LDS'):
        chains_of(gm, lanes=4, tables='lds')
    assert_same(a, b)
    assert_same(chains_of(gm, chains=70), chains_of(gm, chains=70, lanes=8, tables='lds'))
    x_d, logw = state(a)
    for c in range(am.CHAINS):
        h = ais.chain_host(gm, x0[c], am.BETAS, am.TAU0, am.mu0_of(2), am.SWEEPS, z=z[:, c], u=u[:, c])
        assert np.array_equal(h.x_d, x_d[c]) and abs(h.logw - logw[c]) <= 1e-9 * max(1.0, abs(h.logw))


# ---- the device generator ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def rand88():
    gm = gmod.build('rand_8_8')['gm']
    betas = np.linspace(0, 1, 8)
    return gm, betas, chains_of(gm, 64, betas, lanes=8)


def test_device_generator_equals_its_specification(rand88):
    """z, u (ais_models.philox_*) and the initial state (gibbs_models.philox_init) restated from the written counter layouts and
    injected, against the kernel drawing for itself"""
    gm, betas, ref = rand88
    z, u = am.philox_normals(SEED, 64, 7, 8), am.philox_uniforms(SEED, 64, 7, am.SWEEPS, 8)
    x0 = gmod.philox_init(SEED, 64, gm.ex.dstates)
    inj = chains_of(gm, 64, betas, lanes=8, init_x_d=x0, z=z, u=u)
    (ax, al), (bx, bl) = state(ref), state(inj)
    np.testing.assert_array_equal(ax, bx)
    np.testing.assert_allclose(al, bl, rtol=1e-9, atol=1e-9)        # sin / cos / log of the two libraries


def test_lanes_launches_and_chain_counts_give_identical_bits(rand88):
    gm, betas, ref = rand88
    for lanes in (4, 16, 64):
        assert_same(ref, chains_of(gm, 64, betas, lanes=lanes))
    r = ais._AisChains(gm, 64, betas, am.TAU0, am.mu0_of(8), am.SWEEPS, SEED, lanes=8)
    r.advance(3)
    r.advance(7)                                                    # 7 steps run as 3 + 4
    assert_same(ref, r)
    assert_same(ref, chains_of(gm, 16, betas, lanes=8), rows=slice(0, 16))
    assert_same(ref, chains_of(gm, 64, betas, lanes=8))             # two runs
    other = chains_of(gm, 64, betas, lanes=8, seed=SEED + 1)
    assert not np.array_equal(state(other)[1], state(ref)[1])


def test_solver_class_equals_functional_form():
    model = em.build('rand_8_8')
    em.set_indices(model)
    kw = dict(chains=256, steps=16, disc_block_its=2, seed=SEED, base_mean=am.mu0_of(8), base_prec=am.TAU0)
    a = gibbs.GibbsHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc']).log_partition(**kw)
    b = gibbs.ais_log_partition(model['factors'], model['Vd'], model['Vc'], **kw)
    c = gibbs.HybridGaussianSampler(model['factors'], model['Vd'], model['Vc'], None, None).log_partition(steps_per_launch=5, **kw)
    for other in (b, c):
        np.testing.assert_array_equal(a.log_weights.cpu().numpy(), other.log_weights.cpu().numpy())
        np.testing.assert_array_equal(a.x_d.cpu().numpy(), other.x_d.cpu().numpy())
        assert (a.logZ, a.stderr, a.ess, a.lower, a.lower_stderr) == (other.logZ, other.stderr, other.ess, other.lower, other.lower_stderr)
    assert a.obj == -a.logZ and a.log_weights.shape == (256,) and a.x_d.shape == (256, 8) and a.steps == 16


# ---- identities ---------------------------------------------------------------------------------------------------------------
def test_without_discrete_variables_the_weights_telescope_to_log_z():
    model = gmod.build('no_disc')
    mu0 = am.mu0_of(5)
    r = ais.log_partition(model['gm'], chains=70, betas=am.BETAS, base_mean=mu0, base_prec=am.TAU0, seed=SEED)
    logw = r.log_weights.cpu().numpy()
    assert (logw == logw[0]).all()
    want = em.numpy_config(model['factors'], [], 5, ())[0]
    bound = 2 * T * 1e-10 * max(1.0, max(abs(am.collapsed_mass(model, [], b, am.TAU0, mu0)[0]) for b in am.BETAS))
    print('no_disc: log Z0 + logw - log Z = %.3g, logZ - log Z = %.3g (bound %.3g)' % (r.logZ0 + logw[0] - want, r.logZ - want, bound))
    assert abs(r.logZ0 + logw[0] - want) <= bound and abs(r.logZ - want) <= bound and abs(r.lower - want) <= bound
    assert r.stderr <= bound and r.lower_stderr <= bound and abs(r.ess - 1.0) <= bound


@pytest.mark.parametrize('name', ['rand_8_8', 'wide_states', 'pure_disc'])
def test_one_step_weighs_the_initial_state_by_its_collapsed_mass(name):
    """betas = [0, 1]: log Z0 + logw[c] = sum log dstates + logp of lhvi_exact_configs_at at chain c's initial state, and the
    initial states are those of gibbs_models.philox_init"""
    model = gmod.build(name)
    gm = model['gm']
    r = ais.log_partition(gm, chains=100, betas=[0., 1.], base_mean=am.mu0_of(gm.ex.Nc), base_prec=am.TAU0, seed=SEED)
    x_d = r.x_d.cpu().numpy()
    np.testing.assert_array_equal(x_d, gmod.philox_init(SEED, 100, model['dstates']))
    logp = exact.configs_at(gm.ex, r.run.s.ex, r.x_d)[0].cpu().numpy()
    want = sum(math.log(d) for d in model['dstates']) + logp
    em.assert_log_close(r.logZ0 + r.log_weights.cpu().numpy(), want, 1e-10, name)


@pytest.mark.parametrize('name', ['rand_8_8', 'deep_scope', 'pure_disc'])
def test_the_end_of_the_path_is_the_block_gibbs_sampler(name):
    """betas = [0, 1, 1, 1] with injected draws: steps 1 and 2 add exactly 0.0, and x_d after the two transitions is that of
    two iterations of gibbs.chain_host from the same state with the same draws"""
    model = gmod.build(name)
    gm = model['gm']
    x0, z, u = am.draws(model, T=3)
    r = ais._AisChains(gm, am.CHAINS, np.array([0., 1., 1., 1.]), am.TAU0, am.mu0_of(gm.ex.Nc), am.SWEEPS, 0, init_x_d=x0, z=z, u=u)
    r.advance(1)
    first = r.logw.cpu().numpy().copy()
    assert (first != 0.0).all()
    r.advance(2)
    np.testing.assert_array_equal(r.logw.cpu().numpy(), first)
    x2 = r.x_d.cpu().numpy().copy()
    r.advance(3)
    np.testing.assert_array_equal(r.logw.cpu().numpy(), first)
    np.testing.assert_array_equal(r.x_d.cpu().numpy(), x2)
    r.check()
    for c in range(am.CHAINS):
        np.testing.assert_array_equal(x2[c], gibbs.chain_host(gm, x0[c], z[:2, c], u[:2, c], am.SWEEPS, 0, 2).x_d)


@pytest.mark.parametrize('chains', [1, 257, 300000])
def test_reduction_kernel_against_numpy(chains):
    """one chain, more than one workgroup with a ragged tail, more chains than one pass of the partial sums holds"""
    torch = _abi._torch()
    lw = 250.0 + 0.7 * np.random.RandomState(chains).randn(chains)
    t = _abi.to_dev(lw)
    got, again, want = ais.reduce(t), ais.reduce(t), ais.reduce_numpy(lw)
    np.testing.assert_array_equal(got, again)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-9)
    assert got[4] == lw.max()
    assert torch.equal(t, _abi.to_dev(lw))


# ---- errors -------------------------------------------------------------------------------------------------------------------
def test_errors():
    gm = gmod.build('rand_3_2')['gm']
    for bad in ([0., .6, .5, 1.], [0., .5], [.1, 1.]):
        with pytest.raises(ValueError, match='betas'):
            ais.log_partition(gm, chains=8, betas=bad)
    with pytest.raises(ValueError, match=r'not positive definite at the discrete state \(\d, 1\)'):
        ais.log_partition(gmod.build('not_pd')['gm'], chains=64, steps=4)
    with pytest.raises(ValueError, match='lanes'):
        ais.log_partition(gm, chains=8, steps=2, lanes=3)


# ---- statistical ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(am.STAT_STEPS))
def test_estimate_matches_the_exact_log_partition(name):
    s, logZ = am.stat_solver(name)
    r = s.log_partition(chains=am.STAT_CHAINS, steps=am.STAT_STEPS[name], seed=SEED)
    logw = r.log_weights.cpu().numpy()
    z = am.z_score(logw, r.logZ0 + s.log_const, logZ)
    print('%s: T = %d, std(logw) %.3f, z %+.2f, logZ %.4f +- %.4f (exact %.4f), ess %.3f, lower - logZ %+.4f (se %.4f)'
          % (name, r.steps, logw.std(ddof=1), z, r.logZ, r.stderr, logZ, r.ess, r.lower - logZ, r.lower_stderr))
    assert abs(z) <= 4.5
    assert r.lower - logZ <= 4.5 * r.lower_stderr
    assert r.lower <= r.logZ and 0.0 < r.ess <= 1.0
    assert abs(r.logZ - (r.logZ0 + s.log_const + np.log(np.exp(logw - logw.max()).mean()) + logw.max())) <= 1e-9


def test_forty_discrete_variables_agree_between_seeds_and_bound_the_visited_mass():
    """rand_model(40, 8, 5) has no exact value: two seeds agree within 4.5 combined standard errors, and logZ + 4.5 stderr is at
    least the log-sum-exp of the exact log p~ over the distinct final states, a deterministic lower bound of log Z"""
    torch = _abi._torch()
    s = am.beyond_solver()
    a = s.log_partition(chains=am.STAT_CHAINS, steps=am.BEYOND_STEPS, seed=SEED)
    b = s.log_partition(chains=am.STAT_CHAINS, steps=am.BEYOND_STEPS, seed=SEED + 1)
    rows = torch.unique(torch.cat([a.x_d, b.x_d]), dim=0).to(torch.int32).contiguous()
    logp = exact.configs_at(s.model.ex, a.run.s.ex, rows)[0].cpu().numpy()
    visited = float(logp.max() + np.log(np.exp(logp - logp.max()).sum())) + s.log_const
    print('Nd = 40: logZ %.4f +- %.4f / %.4f +- %.4f, std(logw) %.3f / %.3f, %d distinct final states hold log mass %.4f'
          % (a.logZ, a.stderr, b.logZ, b.stderr, a.log_weights.std().item(), b.log_weights.std().item(), len(rows), visited))
    assert abs(a.logZ - b.logZ) <= 4.5 * math.hypot(a.stderr, b.stderr)
    for r in (a, b):
        assert r.logZ + 4.5 * r.stderr >= visited


def test_base_defaults_come_from_the_moments_of_a_run():
    s, logZ = am.stat_solver('rand_8_8_ev')
    before = s.log_partition(chains=64, steps=2, seed=SEED)
    assert before.base_prec == 1.0 and not before.base_mean.any()
    s.run(chains=256, num_burnin=20, num_samples=20, disc_block_its=2, seed=SEED)
    mo = s.moments()
    r = s.log_partition(chains=am.STAT_CHAINS, steps=am.STAT_STEPS['rand_8_8_ev'], seed=SEED)
    np.testing.assert_array_equal(r.base_mean, mo.mean)
    assert r.base_prec == 1.0 / np.diag(mo.cov).mean()
    print('rand_8_8_ev with the base of a run: std(logw) %.3f against %.3f with the default base, logZ %.4f +- %.4f (exact %.4f)'
          % (r.log_weights.std().item(), s.log_partition(chains=am.STAT_CHAINS, steps=r.steps, seed=SEED, base_mean=np.zeros(6),
                                                          base_prec=1.0).log_weights.std().item(), r.logZ, r.stderr, logZ))
    assert r.logZ0 == ais.log_z0(s.dstates, 6, r.base_prec)
