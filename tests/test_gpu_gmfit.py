"""GPU tests of the batched scalar Gaussian-mixture fit (csrc/gmfit.hip, lhvi/gmfit.py): the kernel against the NumPy
restatement of tests/gmfit_models.py at the row lengths where its striding and reduction can go wrong, its determinism and
the independence of its rows, and ``GibbsHybridGaussian.fit_marginals`` end to end.  tests/test_gmfit_host.py holds the CPU
half (the restatement against scikit-learn, the host twin, the argument errors)."""
import numpy as np
import pytest

import exact_models as em
import gmfit_models as gm
from lhvi import gibbs, gmfit
from test_gmfit_host import CASES, IDS, check_moment_identities, numpy_log_pdf

pytestmark = pytest.mark.gpu

OUTPUTS = ('w', 'mu', 'var', 'lower_bound', 'n_iter', 'converged')


def assert_same_bits(a, b, rows_a=slice(None), rows_b=slice(None)):
    for name in OUTPUTS:
        np.testing.assert_array_equal(np.asarray(getattr(a, name))[rows_a], np.asarray(getattr(b, name))[rows_b], err_msg=name)


# ---- the kernel is the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,K', CASES, ids=IDS)
def test_kernel_equals_restatement(n, K):
    x = gm.launch_rows(n, K)
    want, _ = gm.reference(n, K, True)
    got = gmfit.fit_scalar_gms(x, K, **gm.FIXED)
    assert isinstance(got.w, np.ndarray)                    # arrays in, arrays out
    gm.assert_fit_close(got, want, x, what='fixed iterations')
    assert (got.n_iter == 20).all() and not got.converged.any()
    want, rows = gm.reference(n, K, False)
    gm.assert_clear_of_tol(rows)
    got = gmfit.fit_scalar_gms(x, K)
    np.testing.assert_array_equal(got.n_iter, want['n_iter'])
    np.testing.assert_array_equal(got.converged, want['converged'])
    gm.assert_fit_close(got, want, x, what='default tol')
    check_moment_identities(got, x)


@pytest.mark.parametrize('n', gm.NS, ids=['n%s' % ('K' if n is None else n) for n in gm.NS])
def test_two_distinct_values_and_three_components(n):
    x = gm.two_value_row(n)                                 # R = 1
    for fixed in (True, False):
        want, _ = gm.reference(n, 3, fixed, two=True)
        got = gmfit.fit_scalar_gms(x, 3, **(gm.FIXED if fixed else {}))
        gm.assert_fit_close(got, want, x, what='two values, fixed = %s' % fixed)
        np.testing.assert_array_equal(got.n_iter, want['n_iter'])


def test_constant_row_collapses_to_reg_covar():
    got = gmfit.fit_scalar_gms(gm.launch_rows(65, 5)[5], 5)
    np.testing.assert_array_equal(got.var, np.full((1, 5), 1e-6))
    np.testing.assert_array_equal(got.mu, np.full((1, 5), 2.5))
    assert got.converged.all()


def test_given_start_and_keywords():
    x = gm.launch_rows(513, 3)
    rs = np.random.RandomState(5)
    R = x.shape[0]
    mean, sd = x.mean(axis=1, keepdims=True), np.maximum(x.std(axis=1, keepdims=True), 0.01)
    init = (rs.dirichlet(3 * np.ones(3), R), mean + sd * rs.randn(R, 3), sd ** 2 * rs.uniform(0.5, 2, (R, 3)))
    kw = dict(reg_covar=1e-4, tol=1e-5, max_iter=7)
    got = gmfit.fit_scalar_gms(x, 3, init=init, **kw)
    want_i = [gm.fit(x[r], 3, init=tuple(a[r] for a in init), **kw) for r in range(R)]
    want = {k: np.array([w[k] for w in want_i]) for k in OUTPUTS}
    gm.assert_fit_close(got, want, x, what='given start')
    np.testing.assert_array_equal(got.n_iter, want['n_iter'])
    got, (want, _) = gmfit.fit_scalar_gms(x, 3, kmeans_its=0, **gm.FIXED), gm.fit_rows(x, 3, kmeans_its=0, **gm.FIXED)
    gm.assert_fit_close(got, want, x, what='kmeans_its = 0')


def test_device_equals_host_twin():
    for n, K in ((257, 3), (5000, 16)):
        x = gm.launch_rows(n, K)
        dev, host = gmfit.fit_scalar_gms(x, K), gmfit.fit_scalar_gms(x, K, host=True)
        gm.assert_fit_close(dev, dict(w=host.w, mu=host.mu, var=host.var, lower_bound=host.lower_bound), x, what='host twin')
        np.testing.assert_array_equal(dev.n_iter, host.n_iter)


# ---- properties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [1, 2, 3])
def test_shifted_row(K):
    """a kernel that does not centre fails this: at 1e6 +- 1 the sum of r y^2 minus mu^2 keeps 4 digits"""
    z = gm.unit_grid(np.random.RandomState(40 + K), 5000)
    a, b = gmfit.fit_scalar_gms(z, K, **gm.FIXED), gmfit.fit_scalar_gms(z + 1e6, K, **gm.FIXED)
    sd = z.std()
    print('K = %d: mu %.3g sd, w %.3g, var %.3g' % (K, np.abs(b.mu - 1e6 - a.mu).max() / sd, np.abs(b.w - a.w).max(),
                                                   np.abs(b.var / a.var - 1).max()))
    assert np.abs(b.mu - 1e6 - a.mu).max() <= 1e-9 * sd
    assert np.abs(b.w - a.w).max() <= 1e-9 and np.abs(b.var / a.var - 1).max() <= 1e-9


def test_rows_are_independent_and_runs_identical():
    import torch
    x = gm.many_rows()                      # 300 rows of 65 samples: more workgroups than compute units, odd rows start
    all_rows = gmfit.fit_scalar_gms(x, 2)   # 8 bytes off a 16-byte boundary
    assert_same_bits(all_rows, gmfit.fit_scalar_gms(x, 2))
    assert len(set(all_rows.n_iter.tolist())) > 1
    xd = torch.from_numpy(x).cuda()
    for r in (0, 7, 123, 299):
        assert_same_bits(gmfit.fit_scalar_gms(x[r].copy(), 2), all_rows, 0, r)              # alone, on a fresh allocation
        view = xd[r:r + 1]                                                                  # alone, where it lies in the batch
        assert view.is_contiguous() and view.data_ptr() % 16 == (8 if r % 2 else 0)
        alone = gmfit.fit_scalar_gms(view, 2)
        assert isinstance(alone.w, torch.Tensor) and alone.w.is_cuda                        # tensors in, tensors out
        for name in OUTPUTS:
            np.testing.assert_array_equal(getattr(alone, name).cpu().numpy()[0], getattr(all_rows, name)[r], err_msg=name)
    # a long row among the others, and after them
    x = gm.launch_rows(5000, 3)
    batch = gmfit.fit_scalar_gms(x, 3)
    for r in (1, 6):
        assert_same_bits(gmfit.fit_scalar_gms(x[r].copy(), 3), batch, 0, r)
    # an odd row length puts row 1 of a batch 8 bytes off: the pairs are loaded as two words and added in the same order
    x = gm.launch_rows(513, 5)
    batch = gmfit.fit_scalar_gms(x, 5)
    for r in (1, 2):
        assert_same_bits(gmfit.fit_scalar_gms(x[r].copy(), 5), batch, 0, r)


def test_non_contiguous_tensor_and_non_finite_sample():
    import torch
    x = torch.from_numpy(gm.launch_rows(257, 2).copy()).cuda()
    want = gmfit.fit_scalar_gms(x, 2)
    got = gmfit.fit_scalar_gms(x.t().contiguous().t(), 2)           # [R, n] strides (1, R)
    for name in OUTPUTS:
        assert torch.equal(getattr(got, name), getattr(want, name)), name
    x[3, 256] = float('nan')
    x[5, 0] = float('-inf')
    with pytest.raises(ValueError, match='row 3 '):
        gmfit.fit_scalar_gms(x, 2)
    with pytest.raises(ValueError):
        gmfit.fit_scalar_gms(x.float(), 2)


def test_scalar_mixtures_on_the_device_equal_numpy():
    x = gm.many_rows()[:70]
    fit = gmfit.fit_scalar_gms(x, 3)
    pts = np.stack([np.linspace(r.min(), r.max(), 11) for r in x])
    lp = fit.log_pdf(pts)
    for r in range(70):
        np.testing.assert_allclose(lp[r], numpy_log_pdf(*fit.params(r), pts[r]), rtol=1e-10, atol=1e-10)
    bds = np.stack([x.min(axis=1), x.max(axis=1)])
    xm, fm = fit.modes(bds)
    assert (xm >= bds[0]).all() and (xm <= bds[1]).all()
    host = gmfit.ScalarMixtures(fit.w, fit.mu, fit.var, host=True)
    xh, fh = host.modes(bds)
    assert (np.abs(xm - xh) <= 1e-9 * x.std(axis=1)).all()
    np.testing.assert_allclose(fm, fh, rtol=1e-10, atol=1e-10)


# ---- end to end: the sampler's marginals ---------------------------------------------------------------------------------------------
RUN = dict(chains=1024, num_burnin=50, num_samples=32)


@pytest.fixture(scope='module', params=['ref_hybrid2', 'rand_8_8'])
def sampled(request):
    """(solver after run(keep_samples=True), the kept samples [Nc, chains * num_samples] on the host)"""
    model = em.build(request.param)
    s = gibbs.GibbsHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc'])
    with pytest.raises(RuntimeError):
        s.fit_marginals(2)                                  # before run()
    s.run(seed=20241, **RUN)
    with pytest.raises(RuntimeError, match='keep_samples=True'):
        s.fit_marginals(2)
    s.run(seed=20241, keep_samples=True, **RUN)
    for rv in s.Vc:
        with pytest.raises(NotImplementedError):
            s.belief(0.0, rv)
    x = np.ascontiguousarray(s.cont_samples.reshape(-1, len(s.Vc)).T)
    assert x.shape == (len(s.Vc), 1024 * 32)
    return s, x


def test_fit_marginals_is_the_batched_fit_of_the_kept_samples(sampled):
    import torch
    s, x = sampled
    fit = s.fit_marginals(K=2)
    assert fit is s.marginals and isinstance(fit.w, torch.Tensor) and fit.w.is_cuda and fit.w.shape == (len(s.Vc), 2)
    direct = gmfit.fit_scalar_gms(x, 2)
    for name in OUTPUTS:
        np.testing.assert_array_equal(getattr(fit, name).cpu().numpy(), getattr(direct, name), err_msg=name)
    sib = gibbs.fit_scalar_gms_from_samples(s.cont_samples.reshape(-1, len(s.Vc)), 2)
    assert_same_bits(sib, direct)
    # the restatement on those samples: a fixed number of iterations on every row, the default stop on the rows whose
    # restated |change| stays clear of tol
    want, _ = gm.fit_rows(x, 2, **gm.FIXED)
    gm.assert_fit_close(gmfit.fit_scalar_gms(x, 2, **gm.FIXED), want, x, what='fixed iterations')
    want, rows = gm.fit_rows(x, 2)
    clear = []
    for r, row in enumerate(rows):
        d = np.abs(np.abs(row['changes'][1:]) - 1e-3)
        if d.size == 0 or d.min() >= 1e-6:
            clear.append(r)
    assert len(clear) >= (len(rows) + 1) // 2
    np.testing.assert_array_equal(direct.n_iter[clear], want['n_iter'][clear])
    gm.assert_fit_close({k: getattr(direct, k)[clear] for k in ('w', 'mu', 'var', 'lower_bound')},
                        {k: want[k][clear] for k in want}, x[clear], what='default tol, rows %s' % clear)
    # the moments of the mixtures are the sampler's own
    mom = s.moments()
    m1 = (direct.w * direct.mu).sum(axis=1)
    m2 = (direct.w * (direct.var - 1e-6 + direct.mu ** 2)).sum(axis=1)
    sd = np.sqrt(np.diagonal(mom.cov))
    print('moments: first %.3g, second %.3g' % ((np.abs(m1 - mom.mean) / np.maximum(np.abs(mom.mean), sd)).max(),
                                                (np.abs(m2 / np.diagonal(mom.second) - 1)).max()))
    assert (np.abs(m1 - mom.mean) <= 1e-10 * np.maximum(np.abs(mom.mean), sd)).all()
    assert (np.abs(m2 - np.diagonal(mom.second)) <= 1e-10 * np.diagonal(mom.second)).all()


def test_belief_and_map_of_a_continuous_variable(sampled):
    s, x = sampled
    fit = s.fit_marginals(K=2)
    modes = s.map_all(num_gm_components_for_crv=2)
    assert modes.shape == (len(s.rvs),)
    for i, rv in enumerate(s.Vc):
        pts = em.query_points(rv)
        w, mu, var = fit.params(i)
        want = np.exp(numpy_log_pdf(w, mu, var, pts))
        np.testing.assert_allclose(s.belief(pts, rv), want, rtol=1e-10)
        np.testing.assert_allclose(s.belief(pts, rv), fit.pdf(pts[None, :], rows=[i]).cpu().numpy()[0], rtol=1e-14)
        assert s.belief(float(pts[4]), rv) == pytest.approx(want[4], rel=1e-10)
        lo, hi = float(rv.domain.values[0]), float(rv.domain.values[1])
        m = s.map(rv, 2)
        assert lo <= m <= hi and m == modes[s.rvs.index(rv)]
        at = numpy_log_pdf(w, mu, var, np.array([m] + list(np.clip(mu, lo, hi))))
        assert (at[0] >= at[1:] - 1e-9).all()
        assert s.map(rv) == pytest.approx(min(max(x[i].mean(), lo), hi), rel=1e-9, abs=1e-12)          # K = 1 stays the clipped mean
    for rv in s.Vd:
        assert s.map(rv, 2) == s.map(rv)


@pytest.mark.parametrize('K', [2, 3, 5])
def test_fit_is_no_worse_than_the_reference_fitter(sampled, K):
    """the lower bound of the device fit against the smallest of scikit-learn's default fits (random_state 0, 1, 2) of the same
    samples, less tol = 1e-3: the stopping rule's own resolution.  docs/kernels_gmfit.md records the worst value seen."""
    mixture = pytest.importorskip('sklearn.mixture')
    s, x = sampled
    fit = gmfit.fit_scalar_gms(x, K)
    worst = -np.inf
    for i in range(x.shape[0]):
        ref = min(mixture.GaussianMixture(n_components=K, covariance_type='diag', random_state=seed).fit(x[i][:, None]).lower_bound_
                  for seed in (0, 1, 2))
        worst = max(worst, ref - fit.lower_bound[i])
    print('K = %d: worst deficit against scikit-learn %.3g' % (K, worst))
    assert worst <= 1e-3
