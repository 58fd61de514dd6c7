"""GPU tests of the KL divergence of scalar Gaussian mixtures (csrc/gmkl.hip through ``lhvi.gmkl.kl_scalar_mixtures``): the
kernel against the host twin at the component, row and panel counts where its loops end, a row that needs deep bisection,
mixed ranges, determinism, the closed form and the reference's route, and the exact-against-Gibbs flow end to end."""
import numpy as np
import pytest

import exact_models as em
import gmkl_models as gm
from lhvi import exact, gibbs, gmkl, utils
from test_gmkl_host import kl_host, scipy_kl, within

pytestmark = pytest.mark.gpu


def kl_dev(p, q, a=-np.inf, b=np.inf, **kw):
    kl, info = gmkl.kl_scalar_mixtures(p, q, a, b, info=True, **kw)
    return kl, info['abserr'], info['status'], info['neval']


def assert_matches_twin(p, q, a=-np.inf, b=np.inf):
    """the kernel's rows against the host twin's: the bound of the CPU tests with the two estimates, equal status"""
    dev, host = kl_dev(p, q, a, b), kl_host(p, q, a, b)
    print('max |device - host| = %.3g, evaluations equal: %s' % (np.nanmax(np.abs(dev[0] - host[0])), np.array_equal(dev[3], host[3])))
    assert within(dev[0], dev[1], host[0], host[1]).all(), (dev[0], host[0])
    np.testing.assert_array_equal(dev[2], host[2])
    return dev, host


def rand_rows(rng, R, K, family='wide'):
    parts = [gm.rand_gm(rng, K, *gm.FAMILIES[family]) for _ in range(R)]
    return tuple(np.stack([t[i] for t in parts]) for i in range(3))


# the ends of the chunk loop over the components (64 a chunk; Kp + Kq <= 64 stays resident in LDS)
@pytest.mark.parametrize('Kp,Kq', [(1, 1), (1, 5), (5, 1), (32, 32), (32, 33), (63, 64), (64, 65), (65, 130), (130, 1)])
def test_component_counts(Kp, Kq):
    rng = np.random.default_rng(100 * Kp + Kq)
    dev, _ = assert_matches_twin(rand_rows(rng, 3, Kp), rand_rows(rng, 3, Kq))
    assert (dev[2] == 0).all() and np.isfinite(dev[0]).all()


@pytest.mark.parametrize('R', [1, 7, 130])
def test_row_counts_and_mixed_ranges(R):
    rows = gm.family_rows('mild', R, 30 + R)
    a = np.where(np.arange(R) % 3 == 1, -2.5, -np.inf)          # infinite, half-infinite and finite ranges in one launch
    b = np.where(np.arange(R) % 3 != 0, 3.0, np.inf)
    assert_matches_twin(tuple(rows[:3]), tuple(rows[3:]), a, b)


def panel_case(P):
    """(p, q, a, b) of one row whose plan has exactly P panels: a clipped normal for P <= 2, else a unit normal that shares
    its mean with a narrow component"""
    q = (np.ones((1, 1)), np.full((1, 1), 0.3), np.full((1, 1), 2.25))
    if P <= 2:
        c = 4.0 * (P - 0.5)
        return (np.ones((1, 1)), np.zeros((1, 1)), np.ones((1, 1))), q, -c, c
    sd = 20.0 / (8.0 * (P - 0.5))
    return (np.full((1, 2), 0.5), np.zeros((1, 2)), np.array([[1.0, sd * sd]])), q, -np.inf, np.inf


# the group tails of pass 1 (three panels a step) and the largest uncapped list
@pytest.mark.parametrize('P', [1, 2, 3, 4, 22, 64, 65, 1024])
def test_panel_counts(P):
    p, q, a, b = panel_case(P)
    assert gm.plan(tuple(t[0] for t in p), a, b)[2:] == (P, False)
    dev, host = assert_matches_twin(p, q, a, b)
    assert dev[2][0] == 0 and dev[3][0] >= 21 * P
    np.testing.assert_array_equal(dev[3], host[3])


def test_panel_cap():
    p = (np.array([[0.5, 0.5]]), np.array([[-10.0, 10.0]]), np.array([[1e-8, 1.0]]))
    q = (np.ones((1, 1)), np.zeros((1, 1)), np.full((1, 1), 25.0))
    dev, _ = assert_matches_twin(p, q)
    assert dev[2][0] & gmkl.STATUS_PANEL_CAP and np.isfinite(dev[0][0])


def test_deep_bisection():
    """a component of q a thousand times narrower than p's only one, inside its bulk, where a node of the middle panel's first
    bisection meets it: the panels of p do not resolve it, the bisection has to (depth 12 in the restatement)"""
    p = (np.ones((1, 1)), np.zeros((1, 1)), np.ones((1, 1)))
    q = (np.array([[0.5, 0.5]]), np.array([[0.0072, 0.0]]), np.array([[1e-6, 4.0]]))
    stats = {}
    tw = gm.kl_twin(tuple(t[0] for t in p), tuple(t[0] for t in q), stats=stats)
    assert stats['depth'] >= 3
    dev, host = assert_matches_twin(p, q)
    assert dev[2][0] == 0 and dev[3][0] == host[3][0] == tw[3]
    assert within(dev[0][0], dev[1][0], tw[0], tw[1])


def test_invalid_row_among_valid_ones():
    rows = [t.copy() for t in gm.family_rows('mild', 5, 41)]
    rows[2][3, 0] = -1.0
    dev, host = kl_dev(tuple(rows[:3]), tuple(rows[3:])), kl_host(tuple(rows[:3]), tuple(rows[3:]))
    assert np.isnan(dev[0][3]) and dev[2][3] == gmkl.STATUS_INVALID and dev[3][3] == 0
    keep = np.arange(5) != 3
    assert within(dev[0][keep], dev[1][keep], host[0][keep], host[1][keep]).all() and (dev[2][keep] == 0).all()


def test_a_row_has_the_same_bits_wherever_it_sits():
    rows = gm.family_rows('narrow', 130, 50)
    p, q = tuple(rows[:3]), tuple(rows[3:])
    full = kl_dev(p, q, -6.0, 7.0)
    again = kl_dev(p, q, -6.0, 7.0)
    alone = kl_dev(tuple(t[129:] for t in p), tuple(t[129:] for t in q), -6.0, 7.0)
    for x, y, z in zip(full, again, alone):
        np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(x[129:], z)


def test_normal_pairs_match_the_closed_form():
    m1, s1, m2, s2 = gm.normal_pairs(200, 1)
    kl, err, st, _ = kl_dev((np.ones(1), m1[:, None], s1[:, None] ** 2), (np.ones(1), m2[:, None], s2[:, None] ** 2))
    exact_kl = np.array([utils.kl_normal(*t) for t in zip(m1, m2, s1, s2)])
    assert within(kl, err, exact_kl).all() and (st == 0).all()


@pytest.mark.parametrize('fam', list(gm.FAMILIES))
def test_rows_match_scipy_on_the_reference_integrand(fam):
    rows = gm.family_rows(fam, 20, 60)
    for a, b in ((-np.inf, np.inf), (-6.0, 6.0)):
        kl, err, st, _ = kl_dev(tuple(rows[:3]), tuple(rows[3:]), a, b)
        warned = 0
        for r in range(20):
            ref, ref_err, w = scipy_kl(tuple(t[r] for t in rows[:3]), tuple(t[r] for t in rows[3:]), a, b)
            warned += w
            assert w or within(kl[r], err[r], ref, ref_err), (r, kl[r], ref, err[r], ref_err)
        assert warned == 0 and (st == 0).all()


def test_exact_marginals_against_gibbs_fits_end_to_end():
    """the reference's kl_err of a Gibbs run, every operand a device tensor: rand_8_8 has 8 continuous variables and one
    component per discrete configuration (M >= 256: the streamed-component path on real data)"""
    import torch
    model = em.build('rand_8_8')
    ex = exact.ExactHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc']).run()
    gb = gibbs.GibbsHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc'])
    gb.run(chains=256, num_burnin=30, num_samples=20, disc_block_its=5, seed=3, keep_samples=True)
    marg, fits = ex.marginals(), gb.fit_marginals(3)
    assert marg.K >= 64 and marg.R == len(model['Vc']) == fits.R
    kl, info = marg.kl(fits, info=True)
    assert torch.is_tensor(kl) and kl.is_cuda
    kl_h, err_h = kl.cpu().numpy(), info['abserr'].cpu().numpy()
    assert np.isfinite(kl_h).all() and (kl_h >= -err_h).all() and (info['status'].cpu().numpy() == 0).all()
    down = lambda m: tuple(np.ascontiguousarray(t.cpu().numpy()) for t in (m.w, m.mu, m.var))        # noqa: E731
    np.testing.assert_array_equal(gmkl.kl_scalar_mixtures(down(marg), down(fits)), kl_h)
    twin = kl_host(down(marg), down(fits))
    assert within(kl_h, err_h, twin[0], twin[1]).all()
    assert_marginals_are_the_exact_beliefs(ex, marg)


def assert_marginals_are_the_exact_beliefs(ex, marg):
    """the rows of ``marginals()`` are the variables of ``ex.Vc`` and their mixtures the densities ``belief_all`` tabulates"""
    w, mu, var = (t.cpu().numpy() for t in (marg.w, marg.mu, marg.var))
    assert marg.R == len(ex.Vc) and abs(w.sum(axis=1) - 1).max() < 1e-12
    x = np.tile(np.linspace(-2.5, 2.5, 5), (len(ex.rvs), 1))
    want = ex.belief_all(x).cpu().numpy()
    for r, rv in enumerate(ex.Vc):
        got = np.exp(gm.log_mixture(x[0], w[r], mu[r], var[r]))
        np.testing.assert_allclose(got, want[ex.rvs.index(rv)], rtol=1e-10, atol=0)


def test_exact_marginals_leave_the_evidence_out():
    model = em.build('rand_8_8_ev')
    for pos, v in model['evidence'].items():
        model['rvs'][pos].value = v
    ex = exact.ExactHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc']).run()
    marg = ex.marginals()
    assert marg.R == len(ex.Vc) == 6 and len(model['Vc']) == 8
    assert_marginals_are_the_exact_beliefs(ex, marg)


def test_exact_gaussian_marginals_are_its_normals():
    from lhvi import synth
    from lhvi.gauss_exact import ExactGaussian
    from lhvi.gmfit import ScalarMixtures
    g, _ = synth.gaussian_chain(10)
    ex = ExactGaussian(g).run()
    marg = ex.marginals()
    mean, var = ex.mu_var
    assert (marg.R, marg.K) == (ex.hidden.size, 1) and ex.hidden.size >= 2
    np.testing.assert_array_equal(marg.mu[:, 0], mean[ex.hidden])
    np.testing.assert_array_equal(marg.var[:, 0], var[ex.hidden])
    m2, s2 = mean[ex.hidden] + 0.3, np.sqrt(var[ex.hidden]) * 1.7
    kl, info = marg.kl(ScalarMixtures.from_normals(m2, s2 ** 2), info=True)
    want = np.array([utils.kl_normal(*t) for t in zip(mean[ex.hidden], m2, np.sqrt(var[ex.hidden]), s2)])
    assert within(kl, info['abserr'], want).all() and (info['status'] == 0).all()


def test_operands_and_sides():
    """a CPU tensor is refused; a belief built from arrays keeps giving arrays after its device side has been prepared"""
    import torch
    from lhvi.mixture import MixtureBelief
    one = np.ones((1, 1))
    with pytest.raises(ValueError, match='current device'):
        gmkl.kl_scalar_mixtures((torch.ones(1, 1, dtype=torch.float64), one, one), (one, one, one))
    belief = MixtureBelief(np.array([0.4, 0.6]), np.array([[0.0, 1.0]]), np.array([[1.0, 2.0]]))
    belief._side(False)
    sm = belief.scalar_mixtures()
    assert isinstance(sm.mu, np.ndarray)
    kl = sm.kl((one, one, one))
    assert isinstance(kl, np.ndarray) and kl.shape == (1,) and kl[0] > 0


def test_solver_belief_against_a_normal_stays_on_the_device():
    """``vi.mixture_belief().scalar_mixtures()`` of a fitted NPVI reads the solver's device arrays: its continuous rows against
    one normal each, and the same call on the downloaded parameters"""
    import torch
    import npvi_models as nm
    from lhvi.gmfit import ScalarMixtures
    from lhvi.npvi import NPVI
    s = NPVI(nm.hybrid_graph(seed=8), 3, 3, seed=4)
    s.run(its=30, lr=0.05, fix_mix_its=3)
    sm = s.mixture_belief().scalar_mixtures()
    crow = np.flatnonzero(s._cont & np.isnan(s.flat.var_value))
    assert torch.is_tensor(sm.mu) and sm.mu.is_cuda and (sm.R, sm.K) == (crow.size, 3)
    mu, var, w = s._h['eta_c'][crow, :, 0], s._h['eta_c'][crow, :, 1], s._h['w']
    np.testing.assert_array_equal(sm.mu.cpu().numpy(), mu)
    np.testing.assert_array_equal(sm.var.cpu().numpy(), var)
    np.testing.assert_array_equal(sm.w.cpu().numpy(), np.broadcast_to(w, mu.shape))
    other = ScalarMixtures.from_normals(np.zeros(crow.size), np.full(crow.size, 4.0))
    kl, info = sm.kl(other, info=True)
    assert torch.is_tensor(kl) and kl.is_cuda and (info['status'] == 0).all()
    host = kl_host((w, mu, var), (other.w, other.mu, other.var))
    assert within(kl.cpu().numpy(), info['abserr'].cpu().numpy(), host[0], host[1]).all()
    with pytest.raises(ValueError, match="normaliser 'gaussian'"):
        s.mixture_belief(normaliser='vi').scalar_mixtures()
