"""GPU suite of the block Gibbs sampler (lhvi/gibbs.py, csrc/gibbs.hip).

Deterministic: the kernel with injected draws against the NumPy restatement of the reference's loop (tests/gibbs_models.py):
discrete samples equal, continuous samples rtol 1e-9 / atol 1e-12 (cond(J) <= 500, the Cholesky bound of docs/kernels_exact.md).
Bit equality with the device generator over lanes, launch splits, number of chains, where the reduced tables live, and runs.
Statistical: against the reference's recorded exact results (tests/golden/exact_*.npz): per quantity
z = |grand mean - expected| / (std of the per-chain means / sqrt(chains)) <= 4.5 over every discrete marginal, every E[x_i] and
every E[x_i x_j], 4096 chains, burn-in 50, 50 kept, 10 sweeps (docs/kernels_gibbs.md records what the host code gave at these
settings)."""
import numpy as np
import pytest

import exact_models as em
import gibbs_models as gmod
from lhvi import exact, gibbs
from lhvi.graph import F, RV, Domain
from lhvi.potentials import LogQuadratic

pytestmark = pytest.mark.gpu
SEED = 20261017


# ---- injected draws ----------------------------------------------------------------------------------------------------------------
def allowed_lanes(gm):
    """every power-of-two lane count at which a workgroup's chains, reduced tables included, fit 64 KiB of LDS"""
    from lhvi import _abi
    Nc, Nd, disc = gm.ex.Nc, gm.ex.Nd, gm.max_states + gm.table_doubles
    return [l for l in (1, 2, 4, 8, 16, 32, 64) if _abi.lib().lhvi_gibbs_lds_bytes(Nc, Nd, disc, l) <= gibbs.LDS_LIMIT]


def injected_run(gm, lanes, x0, z, u):
    r = gibbs._Chains(gm, gmod.CHAINS, gmod.BURNIN, gmod.ITERS - gmod.BURNIN, gmod.ITS, 0, keep_samples=True, lanes=lanes,
                      init_x_d=x0, z=z, u=u).run()
    return r.disc.cpu().numpy(), r.cont.cpu().numpy()


@pytest.mark.parametrize('name', gmod.DET_MODELS)
def test_kernel_equals_numpy_restatement(name):
    """every allowed lane count: fewer lanes than states (wide_states has 9 states, deep_scope 12 local states of a hybrid
    factor), idle lanes, lanes that do not divide Nc, the one lane count left at Nc = 64"""
    model = gmod.build(name)
    x0, z, u = gmod.draws(model)
    lanes = allowed_lanes(model['gm'])
    assert 64 in lanes and (name not in ('wide_states', 'deep_scope', 'nc1') or lanes == [1, 2, 4, 8, 16, 32, 64])
    assert name != 'nc64' or lanes == [64]
    got = {l: injected_run(model['gm'], l, x0, z, u) for l in lanes}
    for l in lanes[1:]:
        np.testing.assert_array_equal(got[lanes[0]][0], got[l][0], err_msg='lanes %d' % l)
        np.testing.assert_array_equal(got[lanes[0]][1], got[l][1], err_msg='lanes %d' % l)
    for c in range(gmod.CHAINS):
        disc, cont, closest = gmod.restate(model, x0[c], z[:, c], u[:, c], gmod.BURNIN)
        assert closest >= gmod.MARGIN
        np.testing.assert_array_equal(got[lanes[0]][0][c], disc)
        np.testing.assert_allclose(got[lanes[0]][1][c], cont, rtol=1e-9, atol=1e-12)


def test_reduced_tables_too_large_for_lds_go_to_global_scratch():
    """scratch_tables: 625 + 5 doubles of reduced tables a chain.  At the default 4 lanes a workgroup holds 16 chains and the
    tables do not fit: the default choice puts them in global scratch.  At 8 lanes they fit; the forced-LDS run there gives the
    same samples and accumulators bit for bit, and both equal the restatement"""
    model = gmod.build('scratch_tables')
    gm = model['gm']
    assert gm.table_doubles == 630 and gibbs.default_lanes(2) == 4
    x0, z, u = gmod.draws(model)
    kept = gmod.ITERS - gmod.BURNIN
    a = gibbs._Chains(gm, gmod.CHAINS, gmod.BURNIN, kept, gmod.ITS, 0, keep_samples=True, init_x_d=x0, z=z, u=u)
    assert a.lanes == 4 and not a.in_lds and a.scratch is not None and a.scratch.shape == (64, 630)
    b = gibbs._Chains(gm, gmod.CHAINS, gmod.BURNIN, kept, gmod.ITS, 0, keep_samples=True, lanes=8, tables='lds', init_x_d=x0, z=z, u=u)
    assert b.in_lds and b.scratch is None
    with pytest.raises(ValueError, match='bytes of LDS'):
        gibbs._Chains(gm, gmod.CHAINS, gmod.BURNIN, kept, gmod.ITS, 0, lanes=4, tables='lds')
    a.run(), b.run()
    for k in ('disc', 'cont', 'counts', 'sum1', 'sum2', 'x_d'):
        np.testing.assert_array_equal(getattr(a, k).cpu().numpy(), getattr(b, k).cpu().numpy(), err_msg=k)
    got_d, got_c = a.disc.cpu().numpy(), a.cont.cpu().numpy()
    for c in range(gmod.CHAINS):
        disc, cont, closest = gmod.restate(model, x0[c], z[:, c], u[:, c], gmod.BURNIN)
        np.testing.assert_array_equal(got_d[c], disc)
        np.testing.assert_allclose(got_c[c], cont, rtol=1e-9, atol=1e-12)
    assert_same(chains_of(gm, lanes=None), chains_of(gm, lanes=8, tables='lds'))       # and with the device generator


# ---- the device generator against its written specification -----------------------------------------------------------------------
@pytest.mark.parametrize('name', ['rand_8_8', 'wide_states'])
def test_device_generator_equals_its_specification(name):
    """z, u and the initial state restated in NumPy from the counters of docs/kernels_gibbs.md (gibbs_models.philox_*), injected
    into the kernel, against the kernel drawing for itself on the same seed: discrete samples equal, continuous within rtol 1e-9
    (libm and the device's log / sin / cos differ by ulps; the restatement's margin check holds for the injected side, so an ulp
    cannot move a state).  An off-by-one in a draw index, a swapped sine and cosine or a swapped pair of uniforms gives other
    samples altogether."""
    model = gmod.build(name)
    gm, Nd, Nc = model['gm'], len(model['Vd']), len(model['Vc'])
    chains, iters, its = 8, 6, 3                        # 3 sweeps of an odd Nd (wide_states): draw indices of both parities
    z = gmod.philox_normals(SEED, chains, iters, Nc)
    u = gmod.philox_uniforms(SEED, chains, iters, its, Nd)
    x0 = gmod.philox_init(SEED, chains, model['dstates'])
    dev = gibbs._Chains(gm, chains, 0, iters, its, SEED, keep_samples=True)
    np.testing.assert_array_equal(dev.x_d.cpu().numpy(), x0)                     # gibbs_init_kernel, before any iteration
    dev.run()
    inj = gibbs._Chains(gm, chains, 0, iters, its, SEED + 1, keep_samples=True, init_x_d=x0, z=z, u=u).run()
    np.testing.assert_array_equal(dev.disc.cpu().numpy(), inj.disc.cpu().numpy())
    np.testing.assert_allclose(dev.cont.cpu().numpy(), inj.cont.cpu().numpy(), rtol=1e-9, atol=0)
    for c in range(chains):
        disc, cont, closest = gmod.restate(model, x0[c], z[:, c], u[:, c])
        assert closest >= gmod.MARGIN
        np.testing.assert_array_equal(inj.disc.cpu().numpy()[c], disc)
        np.testing.assert_allclose(inj.cont.cpu().numpy()[c], cont, rtol=1e-9, atol=1e-12)


# ---- bit equality, device generator ----------------------------------------------------------------------------------------------
def chains_of(gm, chains=64, iters=20, burnin=5, lanes=8, tables=None, split=None, seed=SEED):
    r = gibbs._Chains(gm, chains, burnin, iters - burnin, 4, seed, keep_samples=True, lanes=lanes, tables=tables)
    for end in (split or []):
        r.advance(end)
    r.run()
    return {k: getattr(r, k).cpu().numpy() for k in ('disc', 'cont', 'counts', 'sum1', 'sum2', 'x_d')}


def assert_same(a, b, rows=slice(None)):
    for k in a:
        np.testing.assert_array_equal(a[k][rows], b[k][rows], err_msg=k)


@pytest.fixture(scope='module')
def rand88():
    gm = gmod.build('rand_8_8')['gm']
    return gm, chains_of(gm)


def test_lanes_give_identical_samples_and_accumulators(rand88):
    gm, base = rand88
    for lanes in (16, 64):
        assert_same(base, chains_of(gm, lanes=lanes))


def test_split_launches_equal_one(rand88):
    gm, base = rand88
    assert_same(base, chains_of(gm, split=[7]))


def test_fewer_chains_are_a_prefix(rand88):
    gm, base = rand88
    assert_same(chains_of(gm, chains=16), base, rows=slice(0, 16))


def test_tables_in_global_scratch_equal_tables_in_lds(rand88):
    gm, base = rand88
    assert gm.table_doubles > 0
    assert_same(base, chains_of(gm, tables='lds'))
    assert_same(base, chains_of(gm, tables='global'))
    assert_same(base, chains_of(gm, tables='global', chains=61, lanes=16), rows=slice(0, 61))      # padding groups


def test_accumulators_are_the_sums_of_the_kept_samples(rand88):
    gm, base = rand88
    dstates = gm.ex.dstates
    for c in range(64):
        counts = np.concatenate([np.bincount(base['disc'][c, :, n], minlength=dstates[n]) for n in range(gm.ex.Nd)])
        np.testing.assert_array_equal(base['counts'][c], counts)
    i, j = np.tril_indices(gm.ex.Nc)
    s1, s2 = np.zeros_like(base['sum1']), np.zeros_like(base['sum2'])
    for s in range(base['cont'].shape[1]):                  # the kernel's order of additions
        s1 += base['cont'][:, s]
        s2 += base['cont'][:, s][:, i] * base['cont'][:, s][:, j]
    np.testing.assert_allclose(base['sum1'], s1, rtol=1e-13)
    np.testing.assert_allclose(base['sum2'], s2, rtol=1e-13)


def test_two_runs_are_identical_and_seeds_differ(rand88):
    gm, base = rand88
    assert_same(base, chains_of(gm))
    other = chains_of(gm, seed=SEED + 1)
    assert (other['cont'] != base['cont']).all() and (other['disc'] != base['disc']).any()
    # the initial state is uniform over each variable's states: 64 chains x 8 variables, every state of every variable occurs
    r = gibbs._Chains(gm, 4096, 0, 0, 1, SEED)
    x = r.x_d.cpu().numpy()
    for n, d in enumerate(gm.ex.dstates):
        freq = np.bincount(x[:, n], minlength=d) / 4096.
        assert np.abs(freq - 1. / d).max() <= 4.5 * np.sqrt((1. / d) * (1 - 1. / d) / 4096)


def test_reference_function_equals_solver_class():
    model = gmod.build('rand_8_8')
    disc, cont = gibbs.block_gibbs_sample(model['factors'], model['Vd'], model['Vc'], 5, 6, disc_block_its=4, seed=SEED, chains=16)
    assert disc.shape == (96, 8) and cont.shape == (96, 8) and disc.dtype.kind == 'i'
    s = gibbs.GibbsHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc'])
    s.run(chains=16, num_burnin=5, num_samples=6, disc_block_its=4, seed=SEED, keep_samples=True, its_per_launch=4)
    np.testing.assert_array_equal(disc, s.disc_samples.reshape(96, 8))
    np.testing.assert_array_equal(cont, s.cont_samples.reshape(96, 8))
    one = gibbs.block_gibbs_sample(model['factors'], model['Vd'], model['Vc'], 5, 6, disc_block_its=4, seed=SEED)
    np.testing.assert_array_equal(one[0], disc[:6])
    np.testing.assert_array_equal(one[1], cont[:6])
    # the sampler class of the reference on the same stream
    Vd_idx, Vc_idx = ({rv: i for i, rv in enumerate(model[k])} for k in ('Vd', 'Vc'))
    h = gibbs.HybridGaussianSampler(model['factors'], model['Vd'], model['Vc'], Vd_idx, Vc_idx)
    h.block_gibbs_sample(5, 6, disc_block_its=4, seed=SEED, chains=16)
    np.testing.assert_array_equal(h.cont_samples, cont)
    assert abs(h.sampled_disc_marginal_table.sum() - 1) <= 1e-12
    for n, rv in enumerate(model['Vd']):
        marg = exact.get_drv_marg(h.sampled_disc_marginal_table, n)
        np.testing.assert_allclose(marg, np.bincount(disc[:, n], minlength=rv.dstates) / 96., rtol=1e-12)
        assert h.map(rv) == np.argmax(marg)
    assert h.map(model['Vc'][0]) == float(np.clip(cont[:, 0].mean(), -10, 10))
    two = h.map(model['Vc'][0], num_gm_components_for_crv=2)
    assert -10 <= two <= 10


# ---- statistical -------------------------------------------------------------------------------------------------------------------
def expected_of(name):
    """(discrete marginals, E[x_c], E[x_i x_j] lower triangle by rows) from the reference's recorded exact results"""
    g = em.load_golden(name)
    t, mu = g['table'], g['means']
    i, j = np.tril_indices(mu.shape[1])
    return g['marg'], t @ mu, t @ (g['covs_tril'] + mu[:, i] * mu[:, j])


@pytest.mark.parametrize('name', ['ref_hybrid2', 'ref_mln0', 'rand_3_2', 'rand_8_8', 'rand_8_8_ev'])
def test_sampled_moments_match_the_reference_exact_results(name):
    model = em.build(name)                      # ref_mln0 with its MLN potentials, through the conversion
    for p, v in model['evidence'].items():
        model['rvs'][p].value = v
    s = gibbs.GibbsHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc'])
    s.run(chains=4096, num_burnin=50, num_samples=50, disc_block_its=10, seed=SEED)
    marg, m1, m2 = expected_of(name)
    got = np.concatenate([s.counts, s.sum1, s.sum2], axis=1) / 50.
    want = np.concatenate([marg, m1, m2])
    assert got.shape == (4096, want.size)
    z = np.abs(got.mean(axis=0) - want) / (got.std(axis=0, ddof=1) / np.sqrt(4096))
    print('%s: %d quantities, max z = %.2f' % (name, want.size, z.max()))
    assert z.max() <= 4.5
    # the class's own summaries are these numbers
    dm = s.disc_marginals()
    np.testing.assert_allclose(np.concatenate([m for m, _ in dm]), got.mean(axis=0)[:marg.size], rtol=1e-12)
    mom = s.moments()
    np.testing.assert_allclose(mom.mean, got.mean(axis=0)[marg.size:marg.size + m1.size], rtol=1e-12, atol=1e-15)
    i, j = np.tril_indices(m1.size)
    np.testing.assert_allclose(mom.second[i, j], got.mean(axis=0)[marg.size + m1.size:], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(mom.cov, mom.second - np.outer(mom.mean, mom.mean))
    assert np.isfinite(s.rhat().cont).all()
    for n, rv in enumerate(s.Vd):
        assert s.map(rv) == rv.domain.values[int(np.argmax(dm[n][0]))]
        assert s.belief(rv.domain.values[0], rv) == dm[n][0][0]
    for p, v in model['evidence'].items():          # an observed variable's map is its value
        assert s.map(model['rvs'][p]) == v
    assert s.map_all().shape == (len(model['rvs']),)


def test_sampled_moments_of_wide_states_match_the_host_enumeration():
    """a 9-state and a 5-state variable, which the recorded models lack: marginals, E[x_i] and E[x_i x_j] enumerated on the host
    with numpy_config (M = 90), not with the device's exact solver; the settings and the bound of the test above
    (docs/kernels_gibbs.md records what the host code gave on three seeds)"""
    model = em.build('wide_states')
    em.set_indices(model)
    logp, mu, sig, _ = em.enumerate_numpy(model)
    t = np.exp(logp - logp.max())
    t /= t.sum()
    joint = t.reshape(9, 5, 2)
    marg = np.concatenate([joint.sum(axis=(1, 2)), joint.sum(axis=(0, 2)), joint.sum(axis=(0, 1))])
    i, j = np.tril_indices(3)
    want = np.concatenate([marg, t @ mu, t @ (sig[:, i, j] + mu[:, i] * mu[:, j])])
    s = gibbs.GibbsHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc'])
    s.run(chains=4096, num_burnin=50, num_samples=50, disc_block_its=10, seed=SEED)
    got = np.concatenate([s.counts, s.sum1, s.sum2], axis=1) / 50.
    assert got.shape == (4096, want.size) and want.size == 16 + 3 + 6
    z = np.abs(got.mean(axis=0) - want) / (got.std(axis=0, ddof=1) / np.sqrt(4096))
    print('wide_states: %d quantities, max z = %.2f' % (want.size, z.max()))
    assert z.max() <= 4.5


def test_forty_discrete_variables_mix_and_agree_between_seeds():
    """Nd = 40: enumeration is impossible.  R-hat <= 1.1, and two seeds agree within 4.5 combined standard errors.

    Run length: 100 burn-in, 200 kept.  The block sampler alternates x_c | x_d and x_d | x_c, so a continuous variable tied to
    a discrete one by a strong hybrid factor decorrelates over outer iterations, however many sweeps the discrete block makes.
    The host code (lhvi_gibbs_chain_host, NumPy draws, 2048 chains) at 50 kept iterations gave R-hat 1.11 on the slowest
    continuous variable of this model, i.e. the between-chain variance of the means is a quarter of the within-chain variance:
    about 4 effective samples in 50, an autocorrelation time near 12 iterations.  R-hat then reads "run longer": with 200
    kept, sqrt(199 / 200 + 0.25 * 50 / 200) = 1.03, and the host code gave 1.028 on two seeds (max z between them 1.9)."""
    model = em.rand_model(em.local_ns(), 40, 8, 5)
    runs = []
    for seed in (SEED, SEED + 7):
        s = gibbs.GibbsHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc'])
        s.run(chains=2048, num_burnin=100, num_samples=200, disc_block_its=10, seed=seed)
        rh = s.rhat()
        print('Nd = 40, seed %d: R-hat max %.4f' % (seed, rh.max))
        assert rh.max <= 1.1
        per = np.concatenate([s.counts, s.sum1, s.sum2], axis=1) / 200.
        runs.append((per.mean(axis=0), per.std(axis=0, ddof=1) / np.sqrt(2048)))
    (a, sa), (b, sb) = runs
    z = np.abs(a - b) / np.sqrt(sa * sa + sb * sb)
    print('Nd = 40: %d quantities, max z between seeds = %.2f' % (z.size, z.max()))
    assert z.max() <= 4.5


# ---- errors and edges --------------------------------------------------------------------------------------------------------------
def test_not_positive_definite_raises_with_the_discrete_state():
    model = gmod.build('not_pd')
    with pytest.raises(ValueError, match=r'not positive definite at the discrete state \([01], 1\)'):
        gibbs.block_gibbs_sample(model['factors'], model['Vd'], model['Vc'], 2, 2, disc_block_its=2, seed=1, chains=64)
    with pytest.raises(ValueError, match=r'not positive definite at the discrete state \(0, 1\).*chain 0, iteration 0'):
        gibbs.block_gibbs_sample(model['factors'], model['Vd'], model['Vc'], 2, 2, init_x_d=[0, 1], seed=1)


def test_too_many_continuous_variables_raise_before_any_launch():
    dc = Domain((-10, 10), continuous=True)
    Vc = [RV(dc) for _ in range(exact.MAX_NC + 1)]
    factors = [F(nb=(rv,), log_potential_fun=LogQuadratic(-np.ones((1, 1)), np.zeros(1), 0.)) for rv in Vc]
    for f in factors:
        f.disc_nb_idx, f.cont_nb_idx = (), (Vc.index(f.nb[0]),)
    with pytest.raises(ValueError, match='LHVI_EXACT_MAX_NC'):
        gibbs.block_gibbs_sample(factors, [], Vc, 1, 1, seed=1)
    with pytest.raises(MemoryError, match='bytes of device memory'):
        gibbs.GibbsHybridGaussian(factors=factors[:2], Vd=[], Vc=Vc[:2]).run(chains=1 << 24, num_samples=1 << 20,
                                                                             keep_samples=True)


def test_one_discrete_variable_and_init_state():
    """Nd = 1 runs one sweep whatever disc_block_its says: the same samples for 1 and for 100.  init_x_d is honoured: with no
    iteration run the state is the given one, and a run from it differs from the default start only through it"""
    model = em.rand_model(em.local_ns(), 1, 3, 7)
    em.set_indices(model)
    a = gibbs.block_gibbs_sample(model['factors'], model['Vd'], model['Vc'], 3, 5, disc_block_its=100, seed=5, chains=8)
    b = gibbs.block_gibbs_sample(model['factors'], model['Vd'], model['Vc'], 3, 5, disc_block_its=1, seed=5, chains=8)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    gm = gmod.build('rand_8_8')['gm']
    init = np.array([1, 0, 1, 0, 1, 0, 1, 0])
    r = gibbs._Chains(gm, 4, 0, 0, 3, SEED, init_x_d=init).run()
    np.testing.assert_array_equal(r.x_d.cpu().numpy(), np.tile(init, (4, 1)))
    # the first x_c depends on the start alone (same z): two chains given the same start and different ones otherwise
    base = gibbs._Chains(gm, 4, 0, 1, 0, SEED, keep_samples=True).run()
    same = gibbs._Chains(gm, 4, 0, 1, 0, SEED, keep_samples=True, init_x_d=base.x_d.cpu().numpy()).run()
    np.testing.assert_array_equal(base.cont.cpu().numpy(), same.cont.cpu().numpy())
    with pytest.raises(ValueError, match='outside'):
        gibbs._Chains(gm, 4, 0, 1, 3, SEED, init_x_d=[2] * 8)


def test_pure_discrete_sampler_matches_enumeration():
    """disc_mrf.gibbs_sample over the same kernel: marginals within 4.5 standard errors of the enumerated ones"""
    model = gmod.build('pure_disc')
    tables = [f.log_potential_fun.table for f in model['factors']]
    scopes = [f.disc_nb_idx for f in model['factors']]
    dstates = model['dstates']
    nbrs = [[j for j, sc in enumerate(scopes) if n in sc] for n in range(len(dstates))]
    joint = np.zeros(dstates)
    for t, sc in zip(tables, scopes):
        joint += np.transpose(t, np.argsort(sc)).reshape([dstates[i] if i in sc else 1 for i in range(len(dstates))])
    joint = np.exp(joint - joint.max())
    joint /= joint.sum()
    x = np.zeros(len(dstates), dtype=np.int64)
    samples = gibbs.gibbs_sample(tables, scopes, nbrs, dstates, x, 30, 20, seed=SEED, chains=2048)
    assert samples.shape == (2048 * 20, len(dstates))
    per = samples.reshape(2048, 20, -1)
    for n, d in enumerate(dstates):
        want = joint.sum(axis=tuple(a for a in range(len(dstates)) if a != n))
        freq = np.stack([(per[:, :, n] == k).mean(axis=1) for k in range(d)], axis=1)
        z = np.abs(freq.mean(axis=0) - want) / (freq.std(axis=0, ddof=1) / np.sqrt(2048))
        assert z.max() <= 4.5, (n, z)
    one = gibbs.gibbs_sample(tables, scopes, nbrs, dstates, x, 3, 4, seed=SEED)
    assert one.shape == (4, len(dstates)) and (x == one[-1]).all()
