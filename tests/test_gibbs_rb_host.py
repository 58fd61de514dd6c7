"""CPU suite of the Rao-Blackwellised marginals of the block Gibbs sampler (docs/kernels_gibbs_rb.md), through the host twins
lhvi_exact_config_at_host and lhvi_gibbs_rb_disc_host, which run the device's own code with one "lane".

Tolerances: a row of digits against the configuration of the same digits: bit equality (the same operations in the same order).
Against numpy_config: rtol 1e-10 with cond(J) <= 500 asserted, the bound of docs/kernels_exact.md.  The probability sums against
the NumPy restatement: rtol 1e-9 / atol 1e-12, the tolerance of the sampler's deterministic tests (the inputs are the same
numbers, only the order of the additions differs)."""
import numpy as np
import pytest

import exact_models as em
import gibbs_models as gmod
import gibbs_rb_models as rbm
from lhvi import _abi, exact, gibbs


@pytest.mark.parametrize('name', rbm.ENUMERABLE)
def test_config_at_equals_config_bit_for_bit(name):
    """all configurations in a seeded shuffle, the first three repeated: logp, mean, var of the row of digits are the bits of
    lhvi_exact_config_host of that configuration"""
    model = gmod.build(name)
    ex = model['gm'].ex
    assert ex.Nc > 0 and ex.M >= 1
    cfg, rows = rbm.shuffled_rows(model['dstates'])
    assert rows.shape == (ex.M + min(3, ex.M), ex.Nd)
    want = {}
    for c, row in zip(cfg, rows):
        if int(c) not in want:
            want[int(c)] = exact.config_host(ex, int(c))
        lp, mu, var = exact.config_at_host(ex, row)
        wlp, wmu, wvar, _ = want[int(c)]
        assert lp == wlp, (name, c)
        np.testing.assert_array_equal(mu, wmu)
        np.testing.assert_array_equal(var, wvar)
    assert len(want) == ex.M


def test_single_row_and_gaussian_only_model():
    """S = 1 is the host twin's only shape; Nd = 0 takes an empty row"""
    ex = gmod.build('no_disc')['gm'].ex
    lp, mu, var = exact.config_at_host(ex, np.zeros(0, dtype=np.int32))
    wlp, wmu, wvar, _ = exact.config_host(ex, 0)
    assert lp == wlp
    np.testing.assert_array_equal(mu, wmu)
    np.testing.assert_array_equal(var, wvar)


def test_model_whose_configurations_cannot_be_numbered():
    """Nd = 40 (1.6e15 configurations: numbered by an int64, far past any enumeration): 64 seeded rows against numpy_config,
    cond(J) <= 500 asserted for each; the struct is accepted with M = 0 and dstride unset, the form a model with more than 2^63
    configurations flattens to"""
    model = rbm.m0_model()
    ex = model['gm'].ex
    assert ex.Nd == 40 and (ex.M == 0 or ex.M > 2 ** 50)
    rows = rbm.m0_rows(model)
    assert rows.shape == (64, 40)
    for row in rows:
        want_lp, want_mu, want_sig = em.numpy_config(model['factors'], model['dstates'], ex.Nc, tuple(int(k) for k in row))
        assert np.linalg.cond(want_sig) <= 500
        lp, mu, var = exact.config_at_host(ex, row)
        em.assert_log_close(lp, want_lp, 1e-10, 'log p~ of a row of digits')
        np.testing.assert_allclose(mu, want_mu, rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(var, np.diagonal(want_sig), rtol=1e-10, atol=1e-12)
    # dstride a null pointer, M = 0: the entry point reads neither
    s = ex.host_struct()
    s.dstride, s.M = None, 0
    logp, mean, var2 = np.zeros(1), np.zeros(ex.Nc), np.zeros(ex.Nc)
    _abi.check(_abi.lib().lhvi_exact_config_at_host(s, rows[-1].ctypes.data, logp.ctypes.data, mean.ctypes.data, var2.ctypes.data))
    assert logp[0] == lp
    np.testing.assert_array_equal(mean, mu)
    np.testing.assert_array_equal(var2, var)


def test_not_positive_definite_names_the_state():
    model = gmod.build('not_pd')
    ex = model['gm'].ex
    lp, mu, var = exact.config_at_host(ex, [0, 0])
    assert np.isfinite(lp) and (var > 0).all()
    with pytest.raises(ValueError, match=r'not positive definite at the discrete state \(0, 1\)'):
        for row in [(0, 0), (0, 1)]:
            exact.config_at_host(ex, row)


def test_arguments_of_the_host_twins():
    model = gmod.build('ref_hybrid2')
    ex = model['gm'].ex
    with pytest.raises(ValueError, match='outside'):
        exact.config_at_host(ex, [3, 0])
    with pytest.raises(ValueError, match='outside'):
        exact.config_at_host(ex, [0, -1])
    l = _abi.lib()
    s = ex.host_struct()
    bad_row = np.array([0, 2], dtype=np.int32)
    out = np.zeros(4)
    assert l.lhvi_exact_config_at_host(s, bad_row.ctypes.data, out.ctypes.data, out[1:].ctypes.data, out[2:].ctypes.data) == -1
    assert l.lhvi_exact_config_at_host(None, bad_row.ctypes.data, None, None, None) == -1
    assert l.lhvi_exact_config_at_host(s, np.zeros(2, dtype=np.int32).ctypes.data, None, None, None) == 0     # outputs may be null
    with pytest.raises(ValueError, match='outside'):
        gibbs.rb_disc_host(model['gm'], [[0, 2]], [[0., 0.]])
    with pytest.raises(_abi.LhviError):
        gibbs.rb_disc_host(model['gm'], [[0, 1]], [[0., 0.]], 0, 2)         # s_end past the samples


@pytest.fixture(scope='module', params=rbm.DISC_MODELS + ('scratch_tables', 'nd1'))
def disc_case(request):
    model = rbm.build(request.param)
    disc, cont = rbm.kept_samples(model)
    return request.param, model, disc, cont


def test_rb_disc_equals_numpy_restatement(disc_case):
    """the kept samples of the deterministic run fed back: every chain's sums against the restatement, and per chain and
    variable the sums over the states equal num_samples within num_samples * 4e-16 * states"""
    name, model, disc, cont = disc_case
    gm = model['gm']
    kept = disc.shape[1]
    assert kept == gmod.ITERS - gmod.BURNIN and disc.shape[0] == gmod.CHAINS
    for c in range(gmod.CHAINS):
        got = gibbs.rb_disc_host(gm, disc[c], cont[c])
        np.testing.assert_allclose(got, rbm.prob_sum(model, disc[c], cont[c]), rtol=1e-9, atol=1e-12)
        for n, d in enumerate(model['dstates']):
            total = got[gm.dstate_off[n]:gm.dstate_off[n + 1]].sum()
            assert abs(total - kept) <= kept * 4e-16 * d, (name, c, n, total)


def test_rb_disc_split_over_calls_is_bit_identical(disc_case):
    """[0, 4) in one call against [0, 1) + [1, 4): the sums are added in sample order"""
    _, model, disc, cont = disc_case
    gm = model['gm']
    one = gibbs.rb_disc_host(gm, disc[3], cont[3])
    two = gibbs.rb_disc_host(gm, disc[3], cont[3], 0, 1)
    two = gibbs.rb_disc_host(gm, disc[3], cont[3], 1, 4, prob_sum=two)
    np.testing.assert_array_equal(one, two)
    np.testing.assert_array_equal(gibbs.rb_disc_host(gm, disc[3], cont[3], 2, 2), np.zeros(gm.n_states))


def test_restatement_is_a_conditional_distribution():
    """the yardstick itself, before anything is compared with it: on ref_hybrid2 p(d0 = k | d1, x_c) is proportional to the
    exponential of the sum of every factor at (k, d1, x_c), written out factor by factor; likewise p(d1 = k | d0, x_c)"""
    model = gmod.build('ref_hybrid2')
    x_d, x_c = np.array([1, 0]), np.array([0.3, -1.1])
    got = rbm.cond_probs(model, x_d, x_c)
    assert got.shape == (5,) and abs(got[:3].sum() - 1) <= 1e-15 and abs(got[3:].sum() - 1) <= 1e-15

    def energy(d0, d1):
        e = 0.0
        for f in model['factors']:
            lp = f.log_potential_fun
            xd = tuple((d0, d1)[i] for i in f.disc_nb_idx)
            xc = x_c[list(f.cont_nb_idx)]
            if not f.cont_nb_idx:
                e += lp.table[xd]
            elif f.disc_nb_idx:
                A, b, c = lp.get_quadratic_params_given_x_d(xd)
                e += xc @ A @ xc + b @ xc + c
            else:
                e += xc @ np.asarray(lp.A) @ xc + np.asarray(lp.b) @ xc + lp.c
        return e
    w0 = np.exp([energy(k, 0) for k in range(3)])
    w1 = np.exp([energy(1, k) for k in range(2)])
    np.testing.assert_allclose(got[:3], w0 / w0.sum(), rtol=1e-13)
    np.testing.assert_allclose(got[3:], w1 / w1.sum(), rtol=1e-13)


def test_class_errors_before_run():
    """the four methods before run(): RuntimeError, before the GPU is asked for"""
    model = gmod.build('ref_hybrid2')
    s = gibbs.GibbsHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc'])
    for call in (s.rb_marginals, s.rb_disc_marginals, s.rb_moments, lambda: s.map(model['Vc'][0], rao_blackwell=True),
                 lambda: s.belief(0.0, model['Vc'][0], rao_blackwell=True), lambda: s.map_all(rao_blackwell=True)):
        with pytest.raises(RuntimeError, match='run'):
            call()
