"""GPU suite of the Rao-Blackwellised marginals of the block Gibbs sampler (lhvi/gibbs.py, csrc/gibbs_rb.hip;
docs/kernels_gibbs_rb.md).

Deterministic: lhvi_exact_configs_at against lhvi_exact_configs bit for bit over every lane count; lhvi_gibbs_rb_disc against the
NumPy restatement (tests/gibbs_rb_models.py) at rtol 1e-9 / atol 1e-12 and bit-identical over lanes, launch splits, number of
chains and where the reduced tables live; the class against its parts; the data-processing inequality
KL(exact_i || rb_i) <= KL(table || counts / S), which holds exactly when every configuration occurs among the samples.
Statistical: the sampler's settings and bound (4096 chains, burn-in 50, 50 kept, 10 sweeps, z <= 4.5 standard errors over chains;
docs/kernels_gibbs_rb.md records what the host code gave on three seeds)."""
import numpy as np
import pytest

import exact_models as em
import gibbs_models as gmod
import gibbs_rb_models as rbm
from lhvi import _abi, exact, gibbs

pytestmark = pytest.mark.gpu
SEED = 20261017
STAT = dict(chains=4096, num_burnin=50, num_samples=50, disc_block_its=10, seed=SEED, keep_samples=True)


def torch():
    return _abi._torch()


# ---- configs_at ----------------------------------------------------------------------------------------------------------------------
def exact_lanes(ex):
    return [l for l in (1, 2, 4, 8, 16, 32, 64) if _abi.lib().lhvi_exact_lds_bytes(ex.Nc, ex.Nd, l) <= 64 * 1024]


def dev_struct(ex):
    """(tensors, lhvi_exact_t over them) of a flat model on the device"""
    t = _abi.upload({n: (a if a.size else np.zeros(1, dtype=a.dtype)) for n, a in ((n, getattr(ex, n)) for n in exact.ExactModel.FIELDS)})
    return t, ex.struct(lambda n: _abi.ptr(t[n]))


def assert_rows_equal(got, run, cfg, what):
    idx = torch().from_numpy(np.asarray(cfg, dtype=np.int64)).to(run.logp.device)
    for g, w, k in zip(got, (run.logp, run.means, run.vars), ('logp', 'means', 'vars')):
        np.testing.assert_array_equal(g.cpu().numpy(), w[idx].cpu().numpy(), err_msg='%s: %s' % (what, k))


@pytest.mark.parametrize('name', rbm.ENUMERABLE)
def test_configs_at_equals_configs_bit_for_bit(name):
    """all configurations in a seeded shuffle, the first three repeated, at every lane count whose workgroup fits 64 KiB; S = 1,
    an S that leaves the last wavefront partly filled, and a launch per chunk of 5 rows"""
    ex = gmod.build(name)['gm'].ex
    run = exact._DeviceRun(ex, keep_cov=False)
    cfg, rows = rbm.shuffled_rows(ex.dstates)
    dev_rows = _abi.to_dev(rows)
    lanes = exact_lanes(ex)
    assert 64 in lanes and (name != 'nc64' or lanes == [64])
    S = len(cfg)
    assert lanes == [64] or any(S % (64 // l) for l in lanes), 'S fills the last wavefront at every lane count'
    for l in lanes:
        assert_rows_equal(exact.configs_at(ex, run.s, dev_rows, lanes=l), run, cfg, '%s, %d lanes' % (name, l))
    assert_rows_equal(exact.configs_at(ex, run.s, dev_rows[:1], lanes=lanes[0]), run, cfg[:1], '%s, S = 1' % name)
    assert_rows_equal(exact.configs_at(ex, run.s, dev_rows, chunk=5), run, cfg, '%s, chunks of 5' % name)


def test_configs_at_serves_a_model_whose_configurations_cannot_be_numbered():
    """Nd = 40: 64 seeded rows against numpy_config at rtol 1e-10 (docs/kernels_exact.md; cond(J) <= 500 asserted for each row),
    through a struct with M = 0 and no dstride"""
    model = rbm.m0_model()
    ex = model['gm'].ex
    rows = rbm.m0_rows(model)
    t, s = dev_struct(ex)
    s.M, s.dstride = 0, None
    logp, means, vars_ = (a.cpu().numpy() for a in exact.configs_at(ex, s, _abi.to_dev(rows)))
    for i, row in enumerate(rows):
        want_lp, want_mu, want_sig = em.numpy_config(model['factors'], model['dstates'], ex.Nc, tuple(int(k) for k in row))
        assert np.linalg.cond(want_sig) <= 500
        em.assert_log_close(logp[i], want_lp, 1e-10, 'log p~ of row %d' % i)
        np.testing.assert_allclose(means[i], want_mu, rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(vars_[i], np.diagonal(want_sig), rtol=1e-10, atol=1e-12)


def test_configs_at_not_positive_definite_names_the_state():
    ex = gmod.build('not_pd')['gm'].ex
    t, s = dev_struct(ex)
    with pytest.raises(ValueError, match=r'not positive definite at the discrete state \(0, 1\)'):
        exact.configs_at(ex, s, _abi.to_dev(np.array([[0, 0], [0, 1]], dtype=np.int32)))
    logp, means, vars_ = exact.configs_at(ex, s, _abi.to_dev(np.array([[0, 0]], dtype=np.int32)))
    assert np.isfinite(logp.cpu().numpy()).all() and (vars_.cpu().numpy() > 0).all()
    with pytest.raises(ValueError, match='outside'):
        exact.configs_at(ex, s, _abi.to_dev(np.array([[0, 2]], dtype=np.int32)))
    # outputs that do not fit raise with the byte count before anything is allocated or launched: 2^40 rows as a view of one
    many = _abi.to_dev(np.zeros((1, 2), dtype=np.int32)).expand(1 << 40, 2)
    with pytest.raises(MemoryError, match='%d bytes of device memory' % (8 * (1 << 40) * 5)):
        exact.configs_at(ex, s, many)


# ---- rb_disc -------------------------------------------------------------------------------------------------------------------------
def fed(gm, disc, cont, lanes=None, tables=None):
    """a _Chains that holds the given kept samples (nothing is run): what lhvi_gibbs_rb_disc reads"""
    r = gibbs._Chains(gm, disc.shape[0], 0, disc.shape[1], gmod.ITS, 0, keep_samples=True, lanes=lanes, tables=tables)
    r.disc.copy_(_abi.to_dev(np.ascontiguousarray(disc, dtype=np.int32)))
    if cont.size:
        r.cont.copy_(_abi.to_dev(np.ascontiguousarray(cont)))
    return r


def gibbs_lanes(gm):
    Nc, Nd, disc = gm.ex.Nc, gm.ex.Nd, gm.max_states + gm.table_doubles
    return [l for l in (1, 2, 4, 8, 16, 32, 64) if _abi.lib().lhvi_gibbs_lds_bytes(Nc, Nd, disc, l) <= gibbs.LDS_LIMIT]


@pytest.mark.parametrize('name', rbm.DISC_MODELS + ('nd1',))
def test_rb_disc_equals_numpy_restatement_and_is_bit_identical(name):
    """the kept samples of the deterministic run (8 chains, 4 kept) fed back.  Against the restatement at the tolerance of the
    sampler's deterministic tests; the states of a variable sum to num_samples; the same bits at every lane count, for [0, 4)
    against [0, 1) + [1, 4), and for 8 chains against the first 8 of 16"""
    model = rbm.build(name)
    gm = model['gm']
    disc, cont = rbm.kept_samples(model)
    kept = disc.shape[1]
    lanes = gibbs_lanes(gm)
    assert 64 in lanes
    got = {l: fed(gm, disc, cont, lanes=l, tables='lds').rb_disc().cpu().numpy() for l in lanes}
    base = got[lanes[0]]
    for l in lanes[1:]:
        np.testing.assert_array_equal(base, got[l], err_msg='lanes %d' % l)
    for c in range(gmod.CHAINS):
        np.testing.assert_allclose(base[c], rbm.prob_sum(model, disc[c], cont[c]), rtol=1e-9, atol=1e-12)
        for n, d in enumerate(model['dstates']):
            total = base[c, gm.dstate_off[n]:gm.dstate_off[n + 1]].sum()
            assert abs(total - kept) <= kept * 4e-16 * d, (name, c, n, total)
    r = fed(gm, disc, cont)
    np.testing.assert_array_equal(base, r.rb_disc().cpu().numpy())              # the default lanes and place of the tables
    split = r.rb_disc(1, 4, prob_sum=r.rb_disc(0, 1))
    np.testing.assert_array_equal(base, split.cpu().numpy())
    twice = fed(gm, np.concatenate([disc, disc[::-1]]), np.concatenate([cont, cont[::-1]]), lanes=lanes[-1])
    assert twice.chains == 16
    np.testing.assert_array_equal(base, twice.rb_disc().cpu().numpy()[:8])
    odd = fed(gm, disc[:5], cont[:5], lanes=lanes[0])                             # padding groups
    np.testing.assert_array_equal(base[:5], odd.rb_disc().cpu().numpy())


def test_rb_disc_tables_in_global_scratch_equal_tables_in_lds():
    """scratch_tables: 630 doubles of reduced tables a chain, in global scratch at the default 4 lanes, in LDS at 8"""
    model = gmod.build('scratch_tables')
    gm = model['gm']
    disc, cont = rbm.kept_samples(model)
    a = fed(gm, disc, cont)
    assert a.lanes == 4 and not a.in_lds and a.scratch is not None
    b = fed(gm, disc, cont, lanes=8, tables='lds')
    assert b.in_lds and b.scratch is None
    c = fed(gm, disc, cont, lanes=8, tables='global')
    pa, pb, pc = (r.rb_disc().cpu().numpy() for r in (a, b, c))
    np.testing.assert_array_equal(pa, pb)
    np.testing.assert_array_equal(pa, pc)
    for ch in range(gmod.CHAINS):
        np.testing.assert_allclose(pa[ch], rbm.prob_sum(model, disc[ch], cont[ch]), rtol=1e-9, atol=1e-12)
    with pytest.raises(_abi.LhviError):                                         # 16 chains of LDS tables do not fit a workgroup
        b.rb_disc(lanes=4)


# ---- the class against its parts -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def rand88():
    model = gmod.build('rand_8_8')
    s = gibbs.GibbsHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc'])
    s.run(chains=64, num_burnin=5, num_samples=20, disc_block_its=4, seed=SEED, keep_samples=True)
    ex = exact.ExactHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc']).run()
    return model, s, ex


def test_class_rows_counts_and_components(rand88):
    model, s, ex = rand88
    before_map, before_disc = s.map_all(), [s.belief(0, rv) for rv in s.Vd]
    mix = s.rb_marginals()
    rows, inverse, counts = np.unique(s.disc_samples.reshape(-1, 8), axis=0, return_inverse=True, return_counts=True)
    rb = s.rb
    np.testing.assert_array_equal(rb.rows.cpu().numpy(), rows)
    np.testing.assert_array_equal(rb.counts.cpu().numpy(), counts)
    np.testing.assert_array_equal(rb.inverse.cpu().numpy(), inverse.reshape(64, 20))
    U = len(rows)
    assert (mix.R, mix.K) == (8, U) and 1 < U <= 64 * 20
    cfg = np.ravel_multi_index(tuple(rows.T), tuple(model['dstates']))
    np.testing.assert_array_equal(rb.means.cpu().numpy(), ex._run.means.cpu().numpy()[cfg])
    np.testing.assert_array_equal(rb.vars.cpu().numpy(), ex._run.vars.cpu().numpy()[cfg])
    # the device divides by a scalar as a multiplication by its reciprocal: an ulp from NumPy's quotient
    np.testing.assert_allclose(mix.w.cpu().numpy(), np.tile(counts / 1280., (8, 1)), rtol=4e-16, atol=0)
    assert mix.w.stride(0) == 0                              # one row of weights shared by the variables
    np.testing.assert_array_equal(mix.mu.cpu().numpy(), rb.means.cpu().numpy().T)
    assert abs(mix.w[0].sum().item() - 1) <= 1e-12
    mom = s.rb_moments()
    means = rb.means.cpu().numpy()[inverse].reshape(64, 20, 8)
    np.testing.assert_allclose(mom.mean, means.mean(axis=(0, 1)), rtol=1e-12)
    second = (rb.vars.cpu().numpy() + rb.means.cpu().numpy() ** 2)[inverse].reshape(64, 20, 8)
    np.testing.assert_allclose(mom.second_diag, second.mean(axis=(0, 1)), rtol=1e-12)
    np.testing.assert_allclose(mom.mean_se, means.mean(axis=1).std(axis=0, ddof=1) / 8., rtol=1e-10)
    # the defaults of map / belief are what they were before rb_marginals()
    np.testing.assert_array_equal(s.map_all(), before_map)
    assert [s.belief(0, rv) for rv in s.Vd] == before_disc and s.marginals is None
    with pytest.raises(NotImplementedError):
        s.belief(0.0, s.Vc[0])


def test_class_disc_marginals_map_and_belief(rand88):
    model, s, ex = rand88
    r = s._run
    prob = r.rb_disc().cpu().numpy() / 20.
    dm = s.rb_disc_marginals()
    off = s.model.dstate_off
    for n, rv in enumerate(s.Vd):
        np.testing.assert_allclose(dm[n][0], prob.mean(axis=0)[off[n]:off[n + 1]], rtol=1e-12)
        np.testing.assert_allclose(dm[n][1], prob.std(axis=0, ddof=1)[off[n]:off[n + 1]] / 8., rtol=1e-10)
        assert abs(dm[n][0].sum() - 1) <= 1e-13
        assert s.map(rv, rao_blackwell=True) == rv.domain.values[int(np.argmax(dm[n][0]))]
        assert s.belief(rv.domain.values[1], rv, rao_blackwell=True) == dm[n][0][1]
    # continuous: the mode and the density of the RB mixture through the exact baseline's mixture kernels, against the mixture
    # written out in NumPy
    w = s.rb.counts.cpu().numpy() / 1280.
    mu, var = s.rb.means.cpu().numpy(), s.rb.vars.cpu().numpy()

    def density(i, x):
        x = np.asarray(x, dtype=np.float64)
        return (w * np.exp(-0.5 * (x[..., None] - mu[:, i]) ** 2 / var[:, i]) / np.sqrt(2 * np.pi * var[:, i])).sum(axis=-1)
    full = s.map_all(rao_blackwell=True)
    for i, rv in enumerate(s.Vc):
        pts = em.query_points(rv, 5)
        np.testing.assert_allclose(s.belief(pts, rv, rao_blackwell=True), density(i, pts), rtol=1e-10)
        x = s.map(rv, rao_blackwell=True)
        assert rv.domain.values[0] <= x <= rv.domain.values[1] and full[s.rvs.index(rv)] == x
        grid = np.linspace(rv.domain.values[0], rv.domain.values[1], 4001)
        assert density(i, x) >= density(i, grid).max() * (1 - 1e-12)
        assert abs(s.belief(x, rv, rao_blackwell=True) - density(i, x)) <= 1e-10 * density(i, x)


def test_class_errors():
    model = gmod.build('ref_hybrid2')
    s = gibbs.GibbsHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc'])
    s.run(chains=8, num_burnin=2, num_samples=3, disc_block_its=2, seed=1)
    for call in (s.rb_marginals, s.rb_disc_marginals, s.rb_moments, lambda: s.map(s.Vc[0], rao_blackwell=True),
                 lambda: s.belief(0, s.Vd[0], rao_blackwell=True)):
        with pytest.raises(RuntimeError, match=r'needs the kept samples: call run\(keep_samples=True\)'):
            call()
    assert s.map(s.Vd[0]) in (0, 1, 2)                      # the defaults need no samples
    pd = gmod.build('pure_disc')
    s = gibbs.GibbsHybridGaussian(factors=pd['factors'], Vd=pd['Vd'], Vc=pd['Vc'])
    s.run(chains=8, num_burnin=2, num_samples=3, disc_block_its=2, seed=1, keep_samples=True)
    with pytest.raises(ValueError, match='no continuous variable'):
        s.rb_marginals()
    assert len(s.rb_disc_marginals()) == 5                  # Nc = 0 has discrete marginals
    nd = gmod.build('no_disc')
    s = gibbs.GibbsHybridGaussian(factors=nd['factors'], Vd=nd['Vd'], Vc=nd['Vc'])
    s.run(chains=8, num_burnin=2, num_samples=3, seed=1, keep_samples=True)
    mix = s.rb_marginals()                                  # Nd = 0: one component, the Gaussian itself
    assert (mix.R, mix.K) == (5, 1) and s.rb.counts.item() == 24 and s.rb_disc_marginals() == []
    lp, mu, var = exact.config_at_host(s.model.ex, [])
    np.testing.assert_array_equal(s.rb.means.cpu().numpy()[0], mu)
    np.testing.assert_allclose(s.rb_moments().mean, mu, rtol=1e-15)


# ---- an inequality that holds exactly ------------------------------------------------------------------------------------------------
EPSABS = 1e-9


@pytest.mark.parametrize('name', ['ref_hybrid2', 'rand_3_2', 'wide_states'])
def test_kl_of_rb_marginals_is_bounded_by_the_kl_of_the_sampled_table(name):
    """The RB mixture's components are the exact mixture's own, so x_i is the same channel applied to the configuration under
    both: by the data-processing inequality KL(exact_i || rb_i) <= KL(table || counts / S) for every continuous variable,
    whenever every configuration occurs among the kept samples (asserted).  On top of the bound: the KL call's epsabs and 1e-12."""
    model = em.build(name)
    s = gibbs.GibbsHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc']).run(**STAT)
    ex = exact.ExactHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc']).run()
    mix = s.rb_marginals()
    M = ex.model.M
    assert mix.K == M, 'only %d of the %d configurations occur among the kept samples' % (mix.K, M)
    table = ex.disc_table.reshape(-1)
    q = s.rb.counts.cpu().numpy() / float(4096 * 50)
    bound = float((table * np.log(table / q)).sum())
    kl, info = ex.marginals().kl(mix, epsabs=EPSABS, epsrel=0.0, info=True)
    kl = kl.cpu().numpy()
    print('%s: KL(table || counts / S) = %.3e, KL(exact_i || rb_i) = %s, status %s' % (name, bound, kl, info['status'].cpu().numpy()))
    assert (info['status'].cpu().numpy() == 0).all()
    assert (kl <= bound + EPSABS + 1e-12).all()


# ---- statistical ---------------------------------------------------------------------------------------------------------------------
def expected_of(name):
    """(discrete marginals, E[x_i], E[x_i^2]) from the reference's recorded exact results"""
    g = em.load_golden(name)
    t, mu = g['table'], g['means']
    i, j = np.tril_indices(mu.shape[1])
    diag = g['covs_tril'][:, i == j]
    return g['marg'], t @ mu, t @ (diag + mu * mu)


def assert_within(got, se, want, what):
    """z <= 4.5 standard errors over chains.  A quantity whose conditional does not depend on the sample has a standard error of
    rounding size: the recorded results agree with this package at rtol 1e-10 (docs/kernels_exact.md), which is allowed on top"""
    diff = np.abs(got - want)
    z = diff / np.maximum(se, 1e-300)
    print('%s: %d quantities, max z = %.2f' % (what, want.size, z[se > 1e-9].max() if (se > 1e-9).any() else 0.0))
    assert (diff <= 4.5 * se + 1e-10 * np.maximum(1.0, np.abs(want))).all(), (what, z)


def check_statistics(s, marg, m1, m2d, name):
    dm = s.rb_disc_marginals()
    got = np.concatenate([m for m, _ in dm]) if dm else np.zeros(0)
    se = np.concatenate([e for _, e in dm]) if dm else np.zeros(0)
    assert_within(got, se, marg, name + ' rb_disc_marginals')
    mom = s.rb_moments()
    assert_within(mom.mean, mom.mean_se, m1, name + ' rb_moments.mean')
    assert_within(mom.second_diag, mom.second_diag_se, m2d, name + ' rb_moments.second_diag')
    # recorded, not asserted: Rao-Blackwell's variance guarantee is for independent draws, not for every chain
    plain = np.concatenate([e for _, e in s.disc_marginals()]) if dm else np.zeros(0)
    pm = s.moments()
    with np.errstate(divide='ignore', invalid='ignore'):
        print('%s: RB / plain standard errors: discrete median %.3f max %.3f, mean median %.3f max %.3f, second median %.3f max %.3f'
              % ((name,) + tuple(f(r) for r in (se / plain, mom.mean_se / pm.mean_se, mom.second_diag_se / np.diagonal(pm.second_se))
                                 for f in (np.nanmedian, np.nanmax))))


@pytest.mark.parametrize('name', ['ref_hybrid2', 'ref_mln0', 'rand_3_2', 'rand_8_8', 'rand_8_8_ev'])
def test_rb_marginals_and_moments_match_the_reference_exact_results(name):
    model = em.build(name)
    for p, v in model['evidence'].items():
        model['rvs'][p].value = v
    s = gibbs.GibbsHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc']).run(**STAT)
    check_statistics(s, *expected_of(name), name)


def test_rb_marginals_and_moments_of_wide_states_match_the_host_enumeration():
    model = em.build('wide_states')
    em.set_indices(model)
    logp, mu, sig, _ = em.enumerate_numpy(model)
    t = np.exp(logp - logp.max())
    t /= t.sum()
    joint = t.reshape(9, 5, 2)
    marg = np.concatenate([joint.sum(axis=(1, 2)), joint.sum(axis=(0, 2)), joint.sum(axis=(0, 1))])
    d = np.arange(3)
    s = gibbs.GibbsHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc']).run(**STAT)
    check_statistics(s, marg, t @ mu, t @ (sig[:, d, d] + mu * mu), 'wide_states')


def test_rb_density_of_rand_8_8_matches_the_exact_marginals():
    """per chain the RB density of every continuous variable at five points, computed here from rb.means, rb.vars and
    rb.inverse, against ExactHybridGaussian.belief_all; only points where the exact density is at least 1e-3 of its maximum
    for the variable (the density at its marginal MAP), at least three a variable (asserted).

    The five points are the exact marginal's mean and mean +- 1 and 2 standard deviations.  em.query_points spreads its points
    over the domain (-10, 10), where these marginals (standard deviation about 1) leave one or two of them above the threshold
    (one of five, at most two of nine, for every variable), so the three points the test needs cannot come from it."""
    model = em.build('rand_8_8')
    s = gibbs.GibbsHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc']).run(**STAT)
    ex = exact.ExactHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc']).run()
    s.rb_marginals()
    t = torch()
    pts = np.zeros((len(ex.rvs), 5))
    table, mu, var = ex.disc_table.reshape(-1), ex.means.reshape(-1, 8), ex.variances.reshape(-1, 8)
    m1, m2 = table @ mu, table @ (var + mu * mu)
    for i, rv in enumerate(ex.Vc):
        pts[ex.rvs.index(rv)] = m1[i] + np.sqrt(m2[i] - m1[i] ** 2) * np.linspace(-2, 2, 5)
        assert rv.domain.values[0] < pts[ex.rvs.index(rv)].min() and pts[ex.rvs.index(rv)].max() < rv.domain.values[1]
    want = ex.belief_all(pts).cpu().numpy()
    x_map, log_peak = ex.map_all()
    rb = s.rb
    worst = 0.0
    for i, rv in enumerate(s.Vc):
        v = ex.rvs.index(rv)
        x = _abi.to_dev(pts[v])
        mu, var = rb.means[:, i][rb.inverse], rb.vars[:, i][rb.inverse]                            # [chains, kept]
        dens = (t.exp(-0.5 * (x[None, None, :] - mu[..., None]) ** 2 / var[..., None]) / t.sqrt(2 * np.pi * var[..., None])).mean(dim=1)
        dens = dens.cpu().numpy()                                                                   # [chains, 5]
        keep = want[v] >= 1e-3 * np.exp(log_peak[v])
        assert keep.sum() >= 3, (i, want[v], np.exp(log_peak[v]))
        z = np.abs(dens.mean(axis=0) - want[v]) / (dens.std(axis=0, ddof=1) / np.sqrt(dens.shape[0]))
        worst = max(worst, z[keep].max())
    print('rand_8_8: RB density, max z = %.2f' % worst)
    assert worst <= 4.5


def test_forty_discrete_variables():
    """Nd = 40 at the settings of the sampler's test (2048 chains, burn-in 100, 200 kept, two seeds): rb_marginals() runs, its
    weights sum to 1, and the two seeds' RB means and discrete marginals agree within 4.5 combined standard errors"""
    model = em.rand_model(em.local_ns(), 40, 8, 5)
    runs = []
    for seed in (SEED, SEED + 7):
        s = gibbs.GibbsHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc'])
        s.run(chains=2048, num_burnin=100, num_samples=200, disc_block_its=10, seed=seed, keep_samples=True)
        mix = s.rb_marginals()
        assert abs(mix.w[0].sum().item() - 1) <= 1e-12 and mix.R == 8
        print('Nd = 40, seed %d: U = %d distinct discrete states among %d samples' % (seed, mix.K, 2048 * 200))
        mom, dm = s.rb_moments(), s.rb_disc_marginals()
        runs.append((np.concatenate([mom.mean] + [m for m, _ in dm]), np.concatenate([mom.mean_se] + [e for _, e in dm])))
    (a, sa), (b, sb) = runs
    z = np.abs(a - b) / np.sqrt(sa * sa + sb * sb)
    print('Nd = 40: %d quantities, max z between seeds = %.2f' % (z.size, z.max()))
    assert z.max() <= 4.5
