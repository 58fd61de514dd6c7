"""CPU tests of the scalar Gaussian-mixture fit (lhvi/gmfit.py, csrc/gmfit.hpp through ``lhvi_gm_fit_host``): the NumPy
restatement of tests/gmfit_models.py against scikit-learn, the host twin against the restatement, the properties of the fit,
the argument errors.  tests/test_gpu_gmfit.py repeats the comparisons on the device."""
import os
import re

import numpy as np
import pytest

import gmfit_models as gm
from lhvi import gibbs, gmfit

CASES = [(n, K) for n in gm.NS for K in gm.KS]
IDS = ['n%s-K%d' % ('K' if n is None else n, K) for n, K in CASES]


def fit_host(x, K, **kw):
    return gmfit.fit_scalar_gms(x, K, host=True, **kw)


def test_the_cases_are_laid_out_for_the_compiled_workgroup_size():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'lifted-hybrid-variational-inference_amd',
                            'csrc', 'gmfit.hip')).read()
    assert int(re.search(r'#define LHVI_GMFIT_BLOCK (\d+)', src).group(1)) == gm.BLOCK
    assert gmfit.MAX_K == 16 == max(gm.KS)


# ---- the restatement is scikit-learn's fit ---------------------------------------------------------------------------------------
SK_ROWS = [(63, 1, 0), (257, 2, 1), (1000, 3, 2), (5000, 4, 3), (5000, 2, 4)]          # (n, K, kind)


def sk_row(n, K, kind):
    """Rows on which scikit-learn's own rounding is benign.  It expands the square, x^2 p - 2 x mu p + mu^2 p with p = 1 / var,
    which loses about (|x| / sd_k)^2 ulps per evaluation, where the centred (y - mu)^2 / var of the restatement loses none:
    so |mean| <= 10 sd of the row, and components of standard deviation 0.8 .. 1.2 no further than 2.5 apart, which keeps
    |x| / sd_k below ~10.  (On a row of four components 8 sd apart, |x| / sd_k ~ 25, the two disagree by 6e-12 in var after 13
    iterations -- scikit-learn's cancellation, the reason the kernel centres.)"""
    rs = np.random.RandomState(10 * n + K)
    comps = kind + 1 if kind < 4 else 2
    mus = 0.7 + 2.5 * (np.arange(comps) - 0.5 * (comps - 1))
    sds = rs.uniform(0.8, 1.2, comps)
    z = rs.choice(comps, size=n, p=rs.dirichlet(4.0 * np.ones(comps)))
    x = mus[z] + sds[z] * rs.randn(n)
    assert abs(x.mean()) <= 10 * x.std()
    w0 = rs.dirichlet(5 * np.ones(K))
    mu0 = np.quantile(x, (np.arange(K) + 0.5) / K) + 0.05 * x.std() * rs.randn(K)
    var0 = x.var() * rs.uniform(0.3, 1.0, K)
    return x, (w0, mu0, var0)


@pytest.mark.parametrize('n,K,kind', SK_ROWS)
def test_restatement_equals_scikit_learn(n, K, kind):
    mixture = pytest.importorskip('sklearn.mixture')
    x, (w0, mu0, var0) = sk_row(n, K, kind)
    clf = mixture.GaussianMixture(n_components=K, covariance_type='diag', weights_init=w0, means_init=mu0[:, None],
                                  precisions_init=1 / var0[:, None])
    clf.fit(x[:, None])
    r = gm.fit(x, K, init=(w0, mu0, var0), centre=False)
    errs = dict(w=np.abs(r['w'] / clf.weights_ - 1).max(), mu=np.abs(r['mu'] / clf.means_.ravel() - 1).max(),
                var=np.abs(r['var'] / clf.covariances_.ravel() - 1).max(),
                lower_bound=abs(r['lower_bound'] / clf.lower_bound_ - 1))
    print('n = %d, K = %d: n_iter %d / %d, relative errors %s' % (n, K, r['n_iter'], clf.n_iter_, errs))
    assert r['n_iter'] == clf.n_iter_ and r['converged'] == clf.converged_
    assert max(errs.values()) <= 1e-12
    # centring changes nothing beyond rounding on such a row, and the host twin takes the same start
    c = gm.fit(x, K, init=(w0, mu0, var0))
    got = fit_host(x, K, init=(w0[None], mu0[None], var0[None]))
    for other in (c, dict(w=got.w[0], mu=got.mu[0], var=got.var[0], lower_bound=got.lower_bound[0], n_iter=got.n_iter[0])):
        assert other['n_iter'] == clf.n_iter_
        np.testing.assert_allclose(other['w'], clf.weights_, rtol=0, atol=1e-9)
        np.testing.assert_allclose(other['mu'], clf.means_.ravel(), rtol=0, atol=1e-9 * x.std())
        np.testing.assert_allclose(other['var'], clf.covariances_.ravel(), rtol=1e-9)
        assert abs(other['lower_bound'] - clf.lower_bound_) <= 1e-9


# ---- the host twin is the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,K', CASES, ids=IDS)
def test_host_twin_equals_restatement(n, K):
    x = gm.launch_rows(n, K)
    want, _ = gm.reference(n, K, True)
    got = fit_host(x, K, **gm.FIXED)
    gm.assert_fit_close(got, want, x, what='fixed iterations')
    assert (got.n_iter == 20).all() and not got.converged.any()
    want, rows = gm.reference(n, K, False)
    gm.assert_clear_of_tol(rows)
    got = fit_host(x, K)
    np.testing.assert_array_equal(got.n_iter, want['n_iter'])
    np.testing.assert_array_equal(got.converged, want['converged'])
    gm.assert_fit_close(got, want, x, what='default tol')


def test_rows_of_one_launch_stop_at_different_iterations():
    for K in (2, 3, 5):
        assert len(set(gm.reference(5000, K, False)[0]['n_iter'].tolist())) >= 3


@pytest.mark.parametrize('n', gm.NS, ids=['n%s' % ('K' if n is None else n) for n in gm.NS])
def test_two_distinct_values_and_three_components(n):
    x = gm.two_value_row(n)
    for fixed in (True, False):
        want, rows = gm.reference(n, 3, fixed, two=True)
        got = fit_host(x, 3, **(gm.FIXED if fixed else {}))
        gm.assert_fit_close(got, want, x, what='two values, fixed = %s' % fixed)
        np.testing.assert_array_equal(got.n_iter, want['n_iter'])
    assert got.w.shape == (1, 3) and np.isfinite(got.var).all() and (got.var >= 1e-6 * (1 - 1e-9)).all()
    assert (got.var <= 1e-6 + x.var()).all()


def test_constant_row_collapses_to_reg_covar():
    got = fit_host(gm.launch_rows(65, 5)[5], 5)
    np.testing.assert_array_equal(got.var, np.full((1, 5), 1e-6))
    np.testing.assert_array_equal(got.mu, np.full((1, 5), 2.5))
    assert abs(got.w.sum() - 1) <= 1e-15 and got.converged.all()
    got = fit_host(np.full(9, 2.5), 2, reg_covar=0.25)
    np.testing.assert_array_equal(got.var, np.full((1, 2), 0.25))


def test_given_start_and_keywords():
    x = gm.launch_rows(513, 3)
    rs = np.random.RandomState(5)
    R = x.shape[0]
    mean, sd = x.mean(axis=1, keepdims=True), np.maximum(x.std(axis=1, keepdims=True), 0.01)
    init = (rs.dirichlet(3 * np.ones(3), R), mean + sd * rs.randn(R, 3), sd ** 2 * rs.uniform(0.5, 2, (R, 3)))
    kw = dict(reg_covar=1e-4, tol=1e-5, max_iter=7)
    got = fit_host(x, 3, init=init, **kw)
    want_i = [gm.fit(x[r], 3, init=tuple(a[r] for a in init), **kw) for r in range(R)]
    want = {k: np.array([w[k] for w in want_i]) for k in ('w', 'mu', 'var', 'lower_bound', 'n_iter', 'converged')}
    gm.assert_fit_close(got, want, x, what='given start')
    np.testing.assert_array_equal(got.n_iter, want['n_iter'])
    assert got.n_iter.max() == 7 and not got.converged[got.n_iter == 7].all()
    # kmeans_its = 0: the M-step from the labels of the quantile centres
    got, (want, _) = fit_host(x, 3, kmeans_its=0, **gm.FIXED), gm.fit_rows(x, 3, kmeans_its=0, **gm.FIXED)
    gm.assert_fit_close(got, want, x, what='kmeans_its = 0')
    # a 1-D input is one row
    one = fit_host(x[1], 3, **gm.FIXED)
    assert one.w.shape == (1, 3)
    np.testing.assert_array_equal(one.mu[0], fit_host(x, 3, **gm.FIXED).mu[1])


# ---- properties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [1, 2, 3])
def test_shifted_row(K):
    z = gm.unit_grid(np.random.RandomState(40 + K), 5000)
    a, b = fit_host(z, K, **gm.FIXED), fit_host(z + 1e6, K, **gm.FIXED)
    sd = z.std()
    print('K = %d: mu %.3g sd, w %.3g, var %.3g' % (K, np.abs(b.mu - 1e6 - a.mu).max() / sd, np.abs(b.w - a.w).max(),
                                                   np.abs(b.var / a.var - 1).max()))
    assert np.abs(b.mu - 1e6 - a.mu).max() <= 1e-9 * sd
    assert np.abs(b.w - a.w).max() <= 1e-9 and np.abs(b.var / a.var - 1).max() <= 1e-9
    np.testing.assert_array_equal(a.n_iter, b.n_iter)


def check_moment_identities(fit, x, reg_covar=1e-6, tol=1e-12):
    """after any M-step sum_k w_k mu_k = mean(x) and sum_k w_k (var_k - reg_covar + (mu_k - mean)^2) = var(x), relative to the
    row's scale: max(|mean|, sd) and max(var, reg_covar).  The second is checked on the rows whose reported means carry it: mu
    comes back rounded to an ulp of |mean|, which enters (mu - mean)^2 as 2 sd ulp(|mean|) -- 2e-10 on the row shifted by 1e6,
    where the identity can only be seen through the first."""
    x = np.atleast_2d(x)
    mean, var = x.mean(axis=1), x.var(axis=1)
    m1 = (fit.w * fit.mu).sum(axis=1)
    m2 = (fit.w * (fit.var - reg_covar + (fit.mu - mean[:, None]) ** 2)).sum(axis=1)
    e1 = np.abs(m1 - mean) / np.maximum(np.abs(mean), np.sqrt(var))
    e1[(m1 == mean)] = 0.0
    e2 = np.abs(m2 - var) / np.maximum(var, reg_covar)
    seen = 2 * np.sqrt(var) * np.spacing(np.abs(mean)) <= 0.01 * tol * np.maximum(var, reg_covar)
    assert seen.sum() >= x.shape[0] - 1
    print('moment identities: first %.3g, second %.3g' % (e1.max(), e2[seen].max()))
    assert e1.max() <= tol and e2[seen].max() <= tol
    return e1.max(), e2[seen].max()


@pytest.mark.parametrize('n,K', [(None, 16), (63, 3), (257, 5), (513, 16), (5000, 2), (5000, 5)])
def test_moment_identities(n, K):
    x = gm.launch_rows(n, K)
    check_moment_identities(fit_host(x, K), x)
    check_moment_identities(fit_host(x, K, tol=0.0, max_iter=3), x)


def test_rows_are_independent_and_runs_identical():
    x = gm.many_rows()
    all_rows = fit_host(x, 2)
    again = fit_host(x, 2)
    for r in (0, 7, 123, 299):
        alone = fit_host(x[r].copy(), 2)
        for name in ('w', 'mu', 'var', 'lower_bound', 'n_iter', 'converged'):
            np.testing.assert_array_equal(getattr(alone, name)[0], getattr(all_rows, name)[r])
    for name in ('w', 'mu', 'var', 'lower_bound', 'n_iter', 'converged'):
        np.testing.assert_array_equal(getattr(all_rows, name), getattr(again, name))
    assert len(set(all_rows.n_iter.tolist())) > 1


@pytest.mark.parametrize('n,K', [(63, 3), (513, 2), (5000, 3), (5000, 5)])
def test_lower_bound_never_decreases(n, K):
    """The ascent property of EM belongs to the exact M-step, reg_covar = 0: adding reg_covar to the variances is not the
    maximiser, and with the default 1e-6 the bound does drop where a variance is within a few orders of it (2e-4 on row 0 of
    the (513, 16) launch, 3e-9 on row 1 of (63, 3) -- in the restatement and in scikit-learn alike).  So: reg_covar = 0, rows
    and K at which no component collapses (the constant row is left out), the trace taken from the host twin by stopping it
    after t = 1 .. 15 iterations."""
    x = np.delete(gm.launch_rows(n, K), 5, axis=0)
    trace = np.array([fit_host(x, K, reg_covar=0.0, tol=0.0, max_iter=t).lower_bound for t in range(1, 16)])
    assert np.isfinite(trace).all()
    print('largest decrease %.3g' % -np.diff(trace, axis=0).min())
    assert np.diff(trace, axis=0).min() >= -1e-12
    # and with the default reg_covar it is the restatement's trace
    x = gm.launch_rows(n, K)
    trace = np.array([fit_host(x, K, tol=0.0, max_iter=t).lower_bound for t in range(1, 16)])
    for r in range(x.shape[0]):
        np.testing.assert_allclose(trace[:, r], gm.reference(n, K, True)[1][r]['trace'][:15], rtol=1e-9, atol=1e-9)


# ---- the fitted mixtures -----------------------------------------------------------------------------------------------------------
def numpy_log_pdf(w, mu, var, x):
    lp = -0.5 * (gm.LOG_2PI + np.log(var) + (x[:, None] - mu) ** 2 / var) + np.log(w)
    m = lp.max(axis=1)
    return m + np.log(np.exp(lp - m[:, None]).sum(axis=1))


def test_scalar_mixtures_density_modes_and_params():
    x = gm.many_rows()[:70]                # more rows than one group of the mixture kernels
    fit = fit_host(x, 3)
    pts = np.stack([np.linspace(r.min(), r.max(), 11) for r in x])
    lp = fit.log_pdf(pts)
    assert lp.shape == (70, 11)
    for r in range(70):
        np.testing.assert_allclose(lp[r], numpy_log_pdf(*fit.params(r), pts[r]), rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(fit.pdf(pts), np.exp(lp), rtol=1e-14)
    np.testing.assert_allclose(fit.log_pdf(pts[[3, 41]], rows=[3, 41]), lp[[3, 41]], rtol=0, atol=0)
    same = fit.log_pdf(pts[0])              # [P]: the same points under every mixture
    np.testing.assert_allclose(same[5], numpy_log_pdf(*fit.params(5), pts[0]), rtol=1e-10, atol=1e-10)
    bds = np.stack([x.min(axis=1), x.max(axis=1)])
    xm, fm = fit.modes(bds)
    assert xm.shape == fm.shape == (70,) and (xm >= bds[0]).all() and (xm <= bds[1]).all()
    np.testing.assert_allclose(fm, np.diagonal(fit.log_pdf(np.broadcast_to(xm, (70, 70)))), rtol=1e-10, atol=1e-10)
    for r in range(70):                     # no component mean inside the bounds is more probable than the mode
        w, mu, var = fit.params(r)
        inside = mu[(mu >= bds[0, r]) & (mu <= bds[1, r])]
        assert (numpy_log_pdf(w, mu, var, inside) <= fm[r] + 1e-9).all()
    with pytest.raises(ValueError):
        fit.modes(bds[:, :5])
    with pytest.raises(ValueError):
        fit.log_pdf(pts, rows=[0, 70])


def test_batched_sibling_of_the_reference_function():
    x = gm.launch_rows(257, 2)
    a, b = gibbs.fit_scalar_gms_from_samples(np.ascontiguousarray(x.T), 2, host=True), fit_host(x, 2)
    for name in ('w', 'mu', 'var', 'lower_bound', 'n_iter'):
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name))
    from compat import hybrid_gaussian_mrf
    assert hybrid_gaussian_mrf.fit_scalar_gms_from_samples is gibbs.fit_scalar_gms_from_samples


# ---- errors ------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_are_raised_before_any_launch():
    x = gm.launch_rows(63, 2)
    for kw in (dict(K=0), dict(K=17), dict(K=2, max_iter=0), dict(K=2, reg_covar=-1e-6), dict(K=2, kmeans_its=-1),
               dict(K=2, init=(np.ones((7, 2)), np.ones((7, 2)))), dict(K=2, init=(np.ones((7, 3)),) * 3),
               dict(K=2, init=(np.ones((6, 2)),) * 3)):
        with pytest.raises(ValueError):
            fit_host(x, **kw)
    with pytest.raises(ValueError, match='fewer than K'):
        fit_host(x[:, :4], 5)
    with pytest.raises(ValueError):
        fit_host(np.zeros((2, 3, 4)), 2)
    # the library refuses the same on its own
    from lhvi import _abi
    out = np.zeros(64)
    i32 = np.zeros(8, dtype=np.int32)
    p = lambda a: a.ctypes.data                                                           # noqa: E731
    call = lambda R, n, K, reg, its: _abi.lib().lhvi_gm_fit_host(R, n, K, p(out), None, reg, 1e-3, its, 10, p(out), p(out),    # noqa: E731
                                                                 p(out), p(out), p(i32), p(i32))
    assert call(1, 8, 2, 1e-6, 5) == 0
    for bad in ((0, 8, 2, 1e-6, 5), (1, 1, 2, 1e-6, 5), (1, 8, 0, 1e-6, 5), (1, 8, 17, 1e-6, 5), (1, 8, 2, -1.0, 5),
                (1, 8, 2, 1e-6, 0)):
        assert call(*bad) == -1


def test_non_finite_sample_names_the_first_offending_row():
    x = gm.launch_rows(65, 2).copy()
    x[4, 64] = np.nan
    x[6, 0] = np.inf
    with pytest.raises(ValueError, match='row 4 '):
        fit_host(x, 2)
    x[4, 64] = 0.0
    with pytest.raises(ValueError, match='row 6 '):
        fit_host(x, 2)
