"""GPU suite of the joint energies and the joint MAP of the exact and Gibbs baselines (lhvi/hg_energy.py, lhvi/exact.py,
lhvi/gibbs.py, csrc/hg_energy.hip).  The models and references are tests/hg_energy_models.py's, proven on the CPU by
tests/test_hg_energy_host.py.

Energies: ``|e - e_ref| <= 2 n_terms * 1.1e-16 * sum |term|`` against the np.longdouble restatement and, with the same bound,
against the host twin (contraction may differ); device against device bit-equal (one call against two, implicit against
explicit addressing, repeated runs).  The arg-max: exactly its definition.  The exact joint MAP against the reference's
recorded results: the index, xc at rtol 1e-10, the energy at 1e-10 of max(1, |e|)."""
import numpy as np
import pytest
import torch

import exact_models as em
import hg_energy_models as hm
from lhvi import _abi, exact, gibbs, hg_energy

pytestmark = pytest.mark.gpu
RTOL = 1e-10


class Device:
    """a flat model on the device"""

    def __init__(self, flat):
        self.t = _abi.upload({n: (a if a.size else np.zeros(1, dtype=a.dtype)) for n, a in
                              ((n, getattr(flat, n)) for n in exact.ExactModel.FIELDS)})
        self.s = flat.struct(lambda n: _abi.ptr(self.t[n]))

    def energies(self, x_d=None, cfg_range=None, x_c=None):
        """through a buffer 64 entries longer, prefilled with a sentinel that must survive"""
        S = cfg_range[1] if x_d is None else len(x_d)
        buf = torch.full((S + 64,), hm.SENTINEL, dtype=torch.float64, device='cuda')
        out = hg_energy.energies(self.s, x_d=None if x_d is None else _abi.to_dev(x_d), cfg_range=cfg_range,
                                 x_c=None if x_c is None else _abi.to_dev(x_c), out=buf[:S])
        assert out.data_ptr() == buf.data_ptr()
        host = buf.cpu().numpy()
        assert (host[S:] == hm.SENTINEL).all(), 'the kernel stored past S'
        return host[:S].copy()


@pytest.mark.parametrize('name', hm.ENERGY_MODELS)
def test_device_energies_within_the_derived_bound(name):
    model, flat = hm.build(name)
    dev = Device(flat)
    for S in hm.S_LIST:
        _, x_d, x_c = hm.rows(model, flat, S, seed=S)
        xc = x_c if flat.Nc else None
        got = dev.energies(x_d=x_d, x_c=xc)
        hm.assert_within_bound(got, model['factors'], x_d, x_c, '%s, S = %d, device' % (name, S))
        twin = hg_energy.energies(flat.host_struct(), x_d=x_d, x_c=x_c, host=True)
        _, T, n_terms = hm.numpy_energy(model['factors'], x_d, x_c)
        assert (np.abs(got - twin) <= hm.bound(T, n_terms)).all(), 'device against host twin'
        np.testing.assert_array_equal(dev.energies(x_d=x_d, x_c=xc), got)                          # a repeated run
        if S > 1:       # the same rows over two calls: other lanes, other workgroups, the same bits
            k = S // 2 + 1
            two = np.concatenate([dev.energies(x_d=x_d[:k], x_c=None if xc is None else xc[:k]),
                                  dev.energies(x_d=x_d[k:], x_c=None if xc is None else xc[k:])])
            np.testing.assert_array_equal(two, got)


def test_device_implicit_addressing_equals_explicit_digits():
    model, flat = hm.build('wide_states')
    dev = Device(flat)
    _, x_d, x_c = hm.rows(model, flat, 83, seed=7, cfg_begin=7)
    a = dev.energies(cfg_range=(7, 83), x_c=x_c)
    np.testing.assert_array_equal(a, dev.energies(x_d=x_d, x_c=x_c))
    hm.assert_within_bound(a, model['factors'], x_d, x_c, 'wide_states, configurations 7 .. 89, device')
    assert hg_energy.energies(dev.s, cfg_range=(0, 0), x_c=_abi.to_dev(np.zeros((0, 3)))).shape == (0,)


@pytest.mark.parametrize('n', hm.ARGMAX_N)
def test_device_argmax_first_is_the_definition(n):
    for pattern, v in hm.argmax_cases(n).items():
        want_i, want_v = hm.argmax_definition(v)
        index, value = hg_energy.argmax_first(_abi.to_dev(v))
        got_i, got_v = int(index.item()), value.cpu().numpy()[0]
        assert got_i == want_i, (n, pattern, got_i, want_i)
        if want_i < 0:
            assert got_v != got_v
        else:
            assert got_v.tobytes() == np.float64(v[want_i]).tobytes(), (n, pattern)
    index, value = hg_energy.argmax_first(torch.empty(0, dtype=torch.float64, device='cuda'))
    assert int(index.item()) == -1 and np.isnan(value.item())


@pytest.mark.parametrize('name', sorted(hm.FIXTURES))
def test_exact_joint_map_matches_the_recorded_results(name):
    gold = em.load_golden(name)
    _, s = em.solver(name)
    s.run()
    want = hm.golden_energies(gold)
    e = s.config_energies()
    assert e.shape == s.disc_table.shape and s.config_energies() is e
    em.assert_log_close(e.reshape(-1), want, RTOL, 'energy of every configuration')
    jm = s.joint_map()
    index = hm.FIXTURES[name]
    print('%s: joint MAP configuration %d, energy %.15g (recorded %.15g)' % (name, jm['index'], jm['energy'], want[index]))
    assert jm['index'] == index and jm['config'] == tuple(int(k) for k in np.unravel_index(index, s.disc_table.shape))
    assert jm['xd'] == tuple(rv.domain.values[k] for rv, k in zip(s.Vd, jm['config']))
    np.testing.assert_allclose(jm['xc'], gold['means'][index], rtol=RTOL, atol=1e-12)
    np.testing.assert_array_equal(jm['xc'], s.means.reshape(-1, len(s.Vc))[index])
    assert abs(jm['energy'] - want[index]) <= RTOL * max(1.0, abs(want[index])) and jm['energy'] == e.reshape(-1)[index]
    assert jm['inside'] is True
    assert list(jm['assignment']) == list(s.rvs)
    for rv in s.rvs:
        if rv.value is not None:
            assert jm['assignment'][rv] == rv.value
    # energy() of the joint MAP's own assignment is its energy, up to the bound of the evaluation
    X = np.array([[float(jm['assignment'][rv]) for rv in s.rvs]])
    x_d, x_c = exact.states_of(s, X)
    got = s.energy(X)
    np.testing.assert_array_equal(got, [jm['energy']])
    hm.assert_within_bound(got, s.factors, x_d, x_c, '%s: energy() at the joint MAP' % name, offset=s.log_const)


def test_joint_map_from_bn_is_the_drivers_block():
    model, _ = hm.build('ref_hybrid2')
    energy, config, xc = exact.joint_map_from_bn(model['factors'], model['Vd'], model['Vc'])
    _, s = em.solver('ref_hybrid2')
    jm = s.run().joint_map()
    assert config == jm['config'] == (1, 1) and energy == jm['energy']
    np.testing.assert_array_equal(xc, jm['xc'])
    # the driver's own loop at that configuration, on the host
    from lhvi.utils import eval_joint_assignment_energy
    vals = dict(zip(model['Vd'], config))
    vals.update(zip(model['Vc'], xc))
    assert abs(eval_joint_assignment_energy(model['factors'], vals) - energy) <= 1e-13


@pytest.mark.parametrize('name', ['peak_vs_mass', 'peak_vs_mass2'])
def test_joint_map_is_not_the_most_probable_configuration(name):
    _, s = hm.solver(name)
    jm = s.run().joint_map()
    peak = int(np.argmax(s.disc_table))
    print('%s: joint MAP configuration %d, argmax(disc_table) %d' % (name, jm['index'], peak))
    assert jm['index'] != peak and jm['config'][0] == 0 and np.unravel_index(peak, s.disc_table.shape)[0] == 1
    e = s.config_energies().reshape(-1)
    assert jm['index'] == hm.argmax_definition(e)[0] and np.sort(e)[-1] - np.sort(e)[-2] >= 0.1
    if name == 'peak_vs_mass':
        np.testing.assert_array_equal(e, [0.0, -1.0])


def test_ties_go_to_the_first_configuration():
    _, s = hm.solver('tie_model')
    jm = s.run().joint_map()
    e = s.config_energies().reshape(-1)
    assert e[0].tobytes() == e[1].tobytes() and e[2].tobytes() == e[3].tobytes()
    assert jm['config'] == (1, 0) and jm['config'][1] == 0 and jm['index'] == 2


@pytest.mark.parametrize('M', sorted(hm.REDUCTION))
def test_joint_map_at_large_M(M):
    """531 441 configurations are three launches of the 2^18 chunk"""
    model, s = hm.solver(M)
    s.run()
    assert s.model.M == M
    e = s.config_energies().reshape(-1)
    jm = s.joint_map()
    assert jm['index'] == hm.argmax_definition(e)[0] and jm['energy'] == e[jm['index']]
    x_d = hm.digits(s.model, np.arange(M))
    hm.assert_within_bound(e, model['factors'], x_d, s.means.reshape(M, 1), 'reduction_model, M = %d' % M)
    np.testing.assert_array_equal(jm['xc'], s.means.reshape(M, 1)[jm['index']])


# ---- Gibbs -----------------------------------------------------------------------------------------------------------------------
def gibbs_of(name):
    model, s = hm.solver(name)
    em.set_indices(model)                   # (no evidence in these models: Vd / Vc are the hidden variables)
    return model, s, gibbs.GibbsHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc'])


@pytest.mark.parametrize('name', ['deep_scope', 'wide_states'])
def test_gibbs_sample_energies_and_joint_map(name):
    model, _, g = gibbs_of(name)
    g.run(chains=8, num_burnin=5, num_samples=5, disc_block_its=3, seed=4, keep_samples=True)
    e = g.sample_energies()
    assert torch.is_tensor(e) and tuple(e.shape) == (8, 5) and g.sample_energies() is e
    e = e.cpu().numpy()
    Nd, Nc = len(g.Vd), len(g.Vc)
    hm.assert_within_bound(e.reshape(-1), model['factors'], g.disc_samples.reshape(40, Nd), g.cont_samples.reshape(40, Nc),
                           '%s: 8 chains x 5 samples' % name)
    jm = g.joint_map()
    row = hm.argmax_definition(e.reshape(-1))[0]
    assert (jm['chain'], jm['sample']) == divmod(row, 5) and jm['energy'] == e.reshape(-1)[row]
    assert jm['config'] == tuple(int(k) for k in g.disc_samples[jm['chain'], jm['sample']])
    assert jm['xd'] == tuple(rv.domain.values[k] for rv, k in zip(g.Vd, jm['config']))
    np.testing.assert_array_equal(jm['xc'], g.cont_samples[jm['chain'], jm['sample']])
    assert jm['index'] == int(np.ravel_multi_index(jm['config'], g.dstates))
    # the reference-shaped sampler on the same samples (as host arrays)
    hs = gibbs.HybridGaussianSampler(model['factors'], model['Vd'], model['Vc'], g.Vd_idx, g.Vc_idx)
    hs.disc_samples, hs.cont_samples = g.disc_samples.reshape(40, Nd).astype(np.int64), g.cont_samples.reshape(40, Nc)
    hj = hs.joint_map()
    assert hj['sample'] == row and hj['config'] == jm['config'] and hj['energy'] == jm['energy']


@pytest.mark.parametrize('name', ['ref_hybrid2', 'peak_vs_mass'])
def test_gibbs_joint_map_reaches_the_exact_one(name):
    """E_exact - 0.05 <= E_gibbs <= E_exact + bound: the upper inequality is mathematical; the lower one needs one of 409 600
    samples in the MAP configuration within chi^2 / 2 < 0.05 of its mode (probability 0.049 / 0.25 per sample there, over
    10 000 such samples: a miss is below 1e-200), and 0.05 is under the models' 0.1 gap, so it decides xd too"""
    model, s, g = gibbs_of(name)
    exact_jm = s.run().joint_map()
    g.run(chains=4096, num_burnin=20, num_samples=100, disc_block_its=10, seed=5, keep_samples=True)
    jm = g.joint_map()
    x_d = np.array([jm['config']], dtype=np.int32)
    _, T, n_terms = hm.numpy_energy(model['factors'], x_d, jm['xc'][None, :])
    print('%s: exact %.12g at %s, Gibbs %.12g at %s (chain %d, sample %d)' % (name, exact_jm['energy'], exact_jm['xd'], jm['energy'],
                                                                             jm['xd'], jm['chain'], jm['sample']))
    assert jm['xd'] == exact_jm['xd'] and jm['config'] == exact_jm['config'] and jm['index'] == exact_jm['index']
    assert exact_jm['energy'] - 0.05 <= jm['energy'] <= exact_jm['energy'] + float(hm.bound(T, n_terms)[0])


def test_gibbs_needs_the_kept_samples():
    _, _, g = gibbs_of('peak_vs_mass')
    g.run(chains=4, num_burnin=2, num_samples=3, seed=1, keep_samples=False)
    with pytest.raises(RuntimeError, match='keep_samples'):
        g.sample_energies()
    with pytest.raises(RuntimeError, match='keep_samples'):
        g.joint_map()


def test_gibbs_carries_log_const():
    """evidence: the sampler's energies include the constants of the fully observed factors, like the exact solver's"""
    _, s = em.solver('rand_8_8_ev')
    model = em.build('rand_8_8_ev')
    for p, v in model['evidence'].items():
        model['rvs'][p].value = v
    g = gibbs.GibbsHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc'])
    assert g.log_const == s.log_const
    g.run(chains=4, num_burnin=3, num_samples=2, disc_block_its=2, seed=2, keep_samples=True)
    Nd, Nc = len(g.Vd), len(g.Vc)
    hm.assert_within_bound(g.sample_energies().cpu().numpy().reshape(-1), g.factors, g.disc_samples.reshape(8, Nd),
                           g.cont_samples.reshape(8, Nc), 'rand_8_8_ev: 4 chains x 2 samples', offset=g.log_const)


def test_solver_energy_equals_the_compat_function():
    from lhvi.utils import eval_joint_assignment_energy
    model, _ = hm.build('ref_mln0')
    s = exact.ExactHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc'])
    rng = np.random.RandomState(11)
    X = np.column_stack([rng.randint(0, 2, size=(70, 2)), rng.uniform(-10, 10, size=(70, 2))]).astype(np.float64)
    got = s.energy(X)
    want = np.array([float(eval_joint_assignment_energy(model['factors'], {rv: (int(x) if rv in s.Vd_idx else x)
                                                                            for rv, x in zip(model['rvs'], row)})) for row in X])
    x_d, x_c = exact.states_of(s, X)
    _, T, n_terms = hm.numpy_energy(model['factors'], x_d, x_c)
    assert (np.abs(got - want) <= hm.bound(T, n_terms)).all()
    hm.assert_within_bound(got, model['factors'], x_d, x_c, 'ref_mln0 through ExactHybridGaussian.energy, device')
