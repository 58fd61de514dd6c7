"""GPU suite of the tempered block Gibbs sampler (csrc/pt.hip, lhvi/pt.py, docs/kernels_pt.md): the kernel against the NumPy
restatement of one ladder (tests/pt_models.py) at every ladder shape, bit equality across lanes / workgroup packing / launches /
ladder counts / table placement, a ladder without swaps against the plain sampler, equal temperatures, the device generator
against its written counter layout, the errors, and the sampled moments against enumeration.

Deterministic tolerances are those of tests/test_pt_host.py.  Statistical bound: per quantity
z = |grand mean - expected| / (std of the per-ladder means / sqrt(ladders)) <= 4.5 (the sampler tests' bound); the models and
quantities were qualified ahead on the CPU by the protocol of docs/kernels_pt.md (scripts/pt_protocol.py)."""
import numpy as np
import pytest

import gibbs_models as gmod
import pt_models as pm
from lhvi import _abi, gibbs, pt

pytestmark = pytest.mark.gpu
SEED = 20261021
KEPT = pm.ITERS - pm.BURNIN
FIELDS = pm.FIELDS_EQUAL + pm.FIELDS_CLOSE


def allowed_lanes(gm, R, in_lds=True):
    """every power-of-two lane count at which a workgroup's ladders fit 256 threads and 64 KiB of LDS"""
    Nc, Nd, disc = gm.ex.Nc, gm.ex.Nd, gm.max_states + (gm.table_doubles if in_lds else 0)
    return [l for l in (1, 2, 4, 8, 16, 32, 64) if 0 < _abi.lib().lhvi_pt_lds_bytes(Nc, Nd, disc, R, l) <= gibbs.LDS_LIMIT]


def ladders_of(gm, R, ladders=pm.LADDERS, betas=None, lanes=None, split=None, seed=SEED, swap_every=1, **kw):
    b = np.asarray(pm.LADDER_BETAS[R] if betas is None else betas, dtype=np.float64)
    r = pt._Ladders(gm, ladders, b, pm.TAU0, pm.mu0_of(gm.ex.Nc), pm.BURNIN, KEPT, pm.SWEEPS, swap_every, seed, keep_samples=True,
                    lanes=lanes, **kw)
    return r.run(split)


def state(r):
    return {k: getattr(r, k).cpu().numpy() for k in FIELDS}


def assert_same(a, b, rows=slice(None)):
    a, b = state(a), state(b)
    for k in FIELDS:
        np.testing.assert_array_equal(a[k][rows], b[k], err_msg=k)


def assert_restated(want, got, what=''):
    for l, w in enumerate(want):
        pm.assert_matches(w, {k: v[l] for k, v in got.items()}, '%s ladder %d' % (what, l))


# ---- injected draws ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R', sorted(pm.LADDER_BETAS))
@pytest.mark.parametrize('name', pm.DET_MODELS)
def test_kernel_equals_numpy_restatement(name, R):
    """R = 1, 2, 3 (an end replica unpaired in each parity), 5 and 8 at swap_every 1 and 2, the default lanes: several ladders
    in one wavefront with padding groups (R = 3, 5), exactly filled (R = 1, 2, 8 at 4 lanes)"""
    for swap_every in pm.SWAP_EVERY:
        model, x0, z, u, usw, want = pm.restated(name, R, swap_every)
        got = state(ladders_of(model['gm'], R, swap_every=swap_every, init_x_d=x0, z=z, u=u, usw=usw))
        assert_restated(want, got, '%s R = %d swap_every = %d' % (name, R, swap_every))


@pytest.mark.parametrize('name', pm.DET_SHAPES)
def test_every_lane_count_gives_the_restatement_and_identical_bits(name):
    """R = 3 on the shapes the fixtures lack, at every allowed lane count: fewer lanes than states, idle lanes, lanes that do not
    divide Nc; 1 - 21 ladders a wavefront and, from 32 lanes on, a ladder over two and three wavefronts"""
    model, x0, z, u, usw, want = pm.restated(name, 3)
    gm = model['gm']
    lanes = allowed_lanes(gm, 3, name != 'scratch_tables')
    assert lanes[-1] == 64 and (name not in ('wide_states', 'deep_scope', 'nc1', 'nc7') or lanes == [1, 2, 4, 8, 16, 32, 64])
    got = {l: state(ladders_of(gm, 3, lanes=l, init_x_d=x0, z=z, u=u, usw=usw)) for l in lanes}
    for l in lanes[1:]:
        for k in FIELDS:
            np.testing.assert_array_equal(got[lanes[0]][k], got[l][k], err_msg='lanes %d: %s' % (l, k))
    assert_restated(want, got[lanes[0]], name)


def test_eight_replicas_over_half_one_and_two_wavefronts():
    """rand_8_8 at R = 8: 4 lanes (two ladders share a wavefront), 8 lanes (exactly one wavefront), 16 lanes (two wavefronts,
    the pair (3, 4) straddles them): identical bits, and the restatement"""
    model, x0, z, u, usw, want = pm.restated('rand_8_8', 8)
    got = {l: state(ladders_of(model['gm'], 8, lanes=l, init_x_d=x0, z=z, u=u, usw=usw)) for l in (4, 8, 16)}
    for l in (8, 16):
        for k in FIELDS:
            np.testing.assert_array_equal(got[4][k], got[l][k], err_msg='lanes %d: %s' % (l, k))
    assert_restated(want, got[4], 'rand_8_8 R = 8')
    assert sum(w['swap_acc'].sum() for w in want) > 0 and sum((w['swap_try'] - w['swap_acc']).sum() for w in want) > 0


def test_reduced_tables_in_global_scratch_equal_tables_in_lds():
    """scratch_tables at R = 3: 630 doubles of reduced tables a replica.  At 4 lanes five ladders share a wavefront and the tables
    do not fit; at 16 lanes a workgroup holds one ladder and they do: the same bits, with injected draws and with the device
    generator"""
    model, x0, z, u, usw, want = pm.restated('scratch_tables', 3)
    gm = model['gm']
    a = ladders_of(gm, 3, lanes=4, init_x_d=x0, z=z, u=u, usw=usw)
    assert not a.in_lds and a.scratch.shape == (64, 630)
    b = ladders_of(gm, 3, lanes=16, tables='lds', init_x_d=x0, z=z, u=u, usw=usw)
    assert b.in_lds and b.scratch is None
    with pytest.raises(ValueError, match=r'needs \d+ bytes of LDS'):
        ladders_of(gm, 3, lanes=4, tables='lds')
    assert_same(a, b)
    assert_restated(want, state(a), 'scratch_tables')
    assert_same(ladders_of(gm, 3, ladders=23, lanes=4), ladders_of(gm, 3, ladders=23, lanes=16, tables='lds'))


@pytest.mark.parametrize('name,R,swap_every', [('rand_8_8', 3, 0), ('two_wells', 8, 0), ('pure_disc', 3, 0), ('rand_8_8', 1, 1)])
def test_without_swaps_the_last_replica_is_the_plain_sampler(name, R, swap_every):
    """replica R - 1 of the kernel against gibbs.chain_host fed the same rows: x_d equal, x_c and the accumulators rtol 1e-9"""
    model, x0, z, u, usw, want = pm.restated(name, R, swap_every)
    Nc = len(model['Vc'])
    got = state(ladders_of(model['gm'], R, swap_every=swap_every, init_x_d=x0, z=z, u=u, usw=usw))
    assert_restated(want, got, name)
    assert not got['swap_try'].any()
    z4, u4 = z.reshape(pm.ITERS, pm.LADDERS, R, Nc), u.reshape(pm.ITERS, pm.LADDERS, R, u.shape[2], -1)
    for l in range(pm.LADDERS):
        plain = gibbs.chain_host(model['gm'], x0[l, R - 1], z4[:, l, R - 1], u4[:, l, R - 1], pm.SWEEPS, pm.BURNIN, KEPT)
        np.testing.assert_array_equal(got['x_d'][l, R - 1], plain.x_d)
        np.testing.assert_array_equal(got['disc'][l], plain.disc)
        np.testing.assert_array_equal(got['counts'][l], plain.counts)
        for k in pm.FIELDS_CLOSE:
            np.testing.assert_allclose(got[k][l], getattr(plain, k), rtol=1e-9, atol=1e-12, err_msg=k)


def test_equal_temperatures_always_swap():
    """betas = [1, 1, 1, 1] on two_wells: every la of the restatement is exactly 0.0, swap_acc == swap_try, and the states follow
    its even / odd permutation (tests/test_pt_host.py says what "exactly" rests on)"""
    betas = (1., 1., 1., 1.)
    model, x0, z, u, usw, want = pm.restated('two_wells', 4, 1, betas=betas)
    assert all(la == 0.0 for w in want for la in w['la'])
    got = state(ladders_of(model['gm'], 4, betas=betas, init_x_d=x0, z=z, u=u, usw=usw))
    assert np.array_equal(got['swap_try'], [[4, 3, 4]] * pm.LADDERS) and np.array_equal(got['swap_acc'], got['swap_try'])
    assert_restated(want, got, 'equal temperatures')


# ---- the device generator ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def rand88():
    gm = pm.build('rand_8_8')['gm']
    return gm, ladders_of(gm, 5, ladders=16, lanes=4)


def test_device_generator_equals_its_specification(rand88):
    """z, u, usw (pt_models.philox_*) and the initial state (gibbs_models.philox_init over ladders * R rows) restated from the
    written counter layouts and injected, against the kernel drawing for itself"""
    gm, ref = rand88
    z, u = pm.philox_normals(SEED, 16, 5, pm.ITERS, 8), pm.philox_uniforms(SEED, 16, 5, pm.ITERS, pm.SWEEPS, 8)
    usw = pm.philox_swaps(SEED, 16, 5, pm.ITERS)
    x0 = gmod.philox_init(SEED, 16 * 5, gm.ex.dstates)
    a, b = state(ref), state(ladders_of(gm, 5, ladders=16, lanes=4, init_x_d=x0, z=z, u=u, usw=usw))
    for k in pm.FIELDS_EQUAL:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for k in pm.FIELDS_CLOSE:                                       # sin / cos / log of the two libraries
        np.testing.assert_allclose(a[k], b[k], rtol=1e-9, atol=1e-9, err_msg=k)
    assert a['swap_acc'].sum() > 0


def test_launches_ladder_counts_and_runs_give_identical_bits(rand88):
    gm, ref = rand88
    b = np.asarray(pm.LADDER_BETAS[5])
    r = pt._Ladders(gm, 16, b, pm.TAU0, pm.mu0_of(8), pm.BURNIN, KEPT, pm.SWEEPS, 1, SEED, keep_samples=True, lanes=4)
    r.advance(3)
    r.advance(7)                                                    # 7 iterations run as 3 + 4
    assert_same(ref, r)
    assert_same(ref, ladders_of(gm, 5, ladders=4, lanes=4), rows=slice(0, 4))      # 4 ladders against the first 4 of 16
    assert_same(ref, ladders_of(gm, 5, ladders=16, lanes=4))                        # two runs
    assert_same(ref, ladders_of(gm, 5, ladders=16, lanes=16))
    other = state(ladders_of(gm, 5, ladders=16, lanes=4, seed=SEED + 1))
    assert not np.array_equal(other['cont'], state(ref)['cont'])


def test_accumulators_are_the_sums_of_the_kept_samples(rand88):
    gm, ref = rand88
    s = state(ref)
    off = gm.dstate_off
    i, j = np.tril_indices(8)
    for l in range(16):
        counts = np.concatenate([np.bincount(s['disc'][l][:, n], minlength=off[n + 1] - off[n]) for n in range(8)])
        np.testing.assert_array_equal(s['counts'][l], counts)
        s1, s2 = np.zeros(8), np.zeros(36)
        for x in s['cont'][l]:
            s1, s2 = s1 + x, s2 + x[i] * x[j]
        np.testing.assert_array_equal(s['sum1'][l], s1)
        np.testing.assert_array_equal(s['sum2'][l], s2)


def test_solver_class_equals_functional_form_and_keeps_the_read_outs():
    model = pm.build('rand_8_8')
    kw = dict(replicas=4, num_burnin=5, num_samples=6, disc_block_its=2, swap_every=2, seed=SEED, base_mean=pm.mu0_of(8), base_prec=pm.TAU0)
    s = gibbs.GibbsHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc'])
    assert s.run_tempered(ladders=64, keep_samples=True, its_per_launch=4, **kw) is s
    disc, cont = gibbs.tempered_gibbs_sample(model['factors'], model['Vd'], model['Vc'], 5, 6, ladders=64,
                                             **{k: v for k, v in kw.items() if k not in ('num_burnin', 'num_samples')})
    assert disc.shape == (64 * 6, 8) and cont.shape == (64 * 6, 8) and disc.dtype.kind == 'i'
    np.testing.assert_array_equal(s.disc_samples.reshape(-1, 8), disc)
    np.testing.assert_array_equal(s.cont_samples.reshape(-1, 8), cont)
    smp = gibbs.HybridGaussianSampler(model['factors'], model['Vd'], model['Vc'], None, None)
    smp.tempered_gibbs_sample(5, 6, ladders=64, **{k: v for k, v in kw.items() if k not in ('num_burnin', 'num_samples')})
    np.testing.assert_array_equal(smp.cont_samples, cont)
    assert abs(smp.sampled_disc_marginal_table.sum() - 1.0) < 1e-12
    # the state run() leaves, chains = ladders
    assert s.chains == 64 and s.num_samples == 6 and s.counts.shape == (64, s.model.n_states)
    dm = s.disc_marginals()
    assert len(dm) == 8 and all(abs(m.sum() - 1.0) < 1e-12 for m, _ in dm)
    mo = s.moments()
    np.testing.assert_allclose(mo.mean, s.cont_samples.mean(axis=(0, 1)), rtol=1e-12, atol=1e-14)
    assert np.isfinite(s.rhat().cont).all()
    assert tuple(s.fit_marginals(2).w.shape) == (8, 2)
    rb = s.rb_disc_marginals()
    assert len(rb) == 8 and all(abs(m.sum() - 1.0) < 1e-9 for m, _ in rb)
    assert s.rb_marginals().w.shape[0] == 8 and s.rb_moments().mean.shape == (8,)
    assert tuple(s.sample_energies().shape) == (64, 6)
    jm = s.joint_map()
    assert jm['energy'] == float(s.sample_energies().max().item()) and 0 <= jm['chain'] < 64
    assert s.map_all().shape == (16,) and 0.0 <= s.belief(model['Vd'][0].domain.values[0], model['Vd'][0]) <= 1.0
    tried, acc = s.swap_counts()
    assert np.array_equal(tried, [64 * 3, 64 * 2, 64 * 3]) and (acc <= tried).all()       # rounds at it = 1, 3, .., 9: 3 even, 2 odd
    np.testing.assert_array_equal(s.swap_rates(), acc / tried)
    with pytest.raises(RuntimeError, match='run_tempered'):
        s.run(chains=8, num_burnin=1, num_samples=2, disc_block_its=1).swap_counts()


# ---- errors ----------------------------------------------------------------------------------------------------------------------
def test_schedule_errors_raise():
    model = pm.build('rand_3_2')
    s = gibbs.GibbsHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc'])
    for kw, what in ((dict(betas=[0., .6, .5, 1.]), 'decrease'), (dict(betas=[0., .5]), 'end at 1'), (dict(betas=[-.1, 1.]), 'negative'),
                     (dict(swap_every=-1), 'swap_every')):
        with pytest.raises(ValueError, match=what):
            s.run_tempered(ladders=4, num_burnin=1, num_samples=1, **kw)
        with pytest.raises(ValueError, match=what):
            gibbs.tempered_gibbs_sample(model['factors'], model['Vd'], model['Vc'], 1, 1, **kw)


def test_not_positive_definite_raises_the_samplers_error():
    gm = gmod.build('not_pd')['gm']
    b = np.array([.5, 1.])
    with pytest.raises(ValueError, match=r'not positive definite at the discrete state \([01], 1\).*ladder \d+, iteration \d'):
        pt._Ladders(gm, 64, b, 1.0, np.zeros(2), 2, 2, 2, 1, 1).run()
    with pytest.raises(ValueError, match=r'not positive definite at the discrete state \(0, 1\).*ladder 0, iteration 0'):
        pt._Ladders(gm, 1, b, 1.0, np.zeros(2), 2, 2, 0, 1, 1, init_x_d=[[1, 0], [0, 1]]).run()
    # a dead ladder stores, counts and swaps nothing; its neighbours in the wavefront go on
    r = pt._Ladders(gm, 3, b, 1.0, np.zeros(2), 0, 2, 0, 1, 1, init_x_d=[[1, 0], [0, 0], [1, 0], [0, 1], [0, 0], [1, 0]])
    r.advance(2)
    assert int(r.bad.item()) == (1 << 32)
    assert r.counts.cpu().numpy().sum(axis=1).tolist() == [4, 0, 4] and r.swap_try.cpu().numpy().ravel().tolist() == [1, 0, 1]
    assert r.x_d.cpu().numpy()[1].tolist() == [[1, 0], [0, 1]]


def test_an_oversize_workgroup_raises_with_its_byte_count():
    gm = pm.build('nc33')['gm']
    with pytest.raises(ValueError, match=r'8 replicas needs \d+ bytes of LDS, more than 65536'):
        ladders_of(gm, 8)
    with pytest.raises(ValueError, match='threads of a workgroup'):
        ladders_of(gm, 8, lanes=64)
    assert allowed_lanes(gm, 8) == [] and allowed_lanes(gm, 3) != []


# ---- statistical -----------------------------------------------------------------------------------------------------------------
def test_tempering_samples_the_two_wells_where_the_plain_sampler_stands_still():
    """two_wells: every discrete marginal, E[x_i] and E[x_i x_j] of the tempered run within 4.5 standard errors of the enumeration;
    plain block Gibbs on the same model is at least 6 of its own standard errors off on a discrete marginal (each chain keeps
    the wells it started in: that half says what the feature is for)"""
    model = pm.build('two_wells')
    want = pm.expected_of('two_wells')
    s = gibbs.GibbsHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc'])
    s.run_tempered(replicas=8, seed=SEED, base_prec=0.1, base_mean=np.zeros(3), **pm.STAT)
    z = pm.z_scores(s.counts, s.sum1, s.sum2, 100, want)
    rates = s.swap_rates()
    print('two_wells tempered: %d quantities, max z = %.2f (discrete %.2f); swap rates %s'
          % (z.size, z.max(), z[:6].max(), np.array2string(rates, precision=3)))
    assert z.size == 6 + 3 + 6 and z.max() <= pm.Z_BOUND
    assert (rates > 0).all() and rates.shape == (7,)
    p = gibbs.GibbsHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc'])
    p.run(chains=1024, num_burnin=100, num_samples=100, disc_block_its=10, seed=SEED)
    zp = pm.z_scores(p.counts, p.sum1, p.sum2, 100, want)
    print('two_wells plain: max discrete z = %.2f, R-hat max %.3f' % (zp[:6].max(), p.rhat().max))
    assert zp[:6].max() >= 6.0


@pytest.mark.parametrize('name', pm.STAT_FIXTURES)
def test_tempering_does_not_bias_an_easy_model(name):
    """4 replicas against the reference's recorded exact results (tests/golden/exact_*.npz)"""
    import exact_models as em
    model = em.build(name)
    s = gibbs.GibbsHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc'])
    s.run_tempered(replicas=4, seed=SEED, **pm.STAT)
    z = pm.z_scores(s.counts, s.sum1, s.sum2, 100, pm.expected_of(name))
    print('%s tempered: %d quantities, max z = %.2f; swap rates %s' % (name, z.size, z.max(), np.array2string(s.swap_rates(), precision=3)))
    assert z.max() <= pm.Z_BOUND and (s.swap_rates() > 0).all()
