"""The scalar Gaussian-mixture fit of csrc/gmfit.hpp restated in NumPy, and the seeded cases of tests/test_gmfit_host.py and
tests/test_gpu_gmfit.py.

``fit`` is docs/kernels_gmfit.md line by line: centring, the deterministic start (quantile centres, Lloyd iterations, one
M-step from the labels) or a given start, scikit-learn 1.7's E- and M-step, its stopping rule.  With ``centre=False`` and
``init`` it is what ``GaussianMixture(n_components=K, covariance_type='diag', weights_init=, means_init=,
precisions_init=)`` computes (test_gmfit_host.py checks that against scikit-learn itself).

Cases.  A launch is (n, K) with the rows of ``launch_rows``: draws from 1 .. 4 well-separated components, from two
overlapping ones, a constant row, a row shifted by 1e6 with standard deviation 1; K = 3 has a launch of one row with two
distinct values.  Row lengths are those at which the striding over pairs and the reduction of a workgroup of BLOCK threads
can go wrong.  Two choices keep the comparison about the kernel and not about the conditioning of the formulas:

* the unshifted rows live in [-0.6, 0.6].  When a component collapses onto one point (n = K; K = 16 on 63 samples), scikit-learn's
  ``var = s2 / nk - mu^2 + reg_covar`` cancels to ``reg_covar`` = 1e-6 plus a rounding error of ~1e-16 y^2, so two correct
  evaluations differ by 1e-10 y^2 relative: the 1e-9 of the comparison holds for |y| < 1 and would not for |y| ~ 20.
* the constant is 2.5 and the shifted row is 1e6 + z with z a multiple of 2^-20: sums and shifts of these are exact, so the
  centred row is the same numbers however the mean was added up, and no hard k-means label hangs on a rounding error.
"""
import functools
import math
from statistics import NormalDist

import numpy as np

BLOCK = 256                         # LHVI_GMFIT_BLOCK of csrc/gmfit.hip (test_gmfit_host.py checks that it is)
NS = (None, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1, 5000)        # None: n = K
KS = (1, 2, 3, 5, 16)
LOG_2PI = math.log(2 * math.pi)
EPS10 = 10 * np.finfo(np.float64).eps
DEFAULTS = dict(reg_covar=1e-6, tol=1e-3, max_iter=100, kmeans_its=10)


def quantile_centres(K):
    return np.array([NormalDist().inv_cdf((k + 0.5) / K) for k in range(K)])


def m_step(nk, s1, s2, n, reg_covar):
    nk = nk + EPS10
    mu = s1 / nk
    var = s2 / nk - mu * mu + reg_covar
    w = nk / n
    return w / w.sum(), mu, var


def fit(x, K, init=None, reg_covar=1e-6, tol=1e-3, max_iter=100, kmeans_its=10, centre=True):
    """dict: w, mu, var [K], lower_bound, n_iter, converged, trace (the lower bound of every iteration), changes"""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    mean = x.mean() if centre else 0.0
    y = x - mean
    if init is not None:
        w, mu, var = (np.array(a, dtype=np.float64) for a in init)
        mu = mu - mean
    else:
        c = np.sqrt((y * y).mean()) * quantile_centres(K)
        for t in range(kmeans_its + 1):
            lab = np.argmin(np.abs(y[:, None] - c[None, :]), axis=1)            # ties to the lowest component
            cnt = np.bincount(lab, minlength=K).astype(np.float64)
            s1, s2 = np.bincount(lab, weights=y, minlength=K), np.bincount(lab, weights=y * y, minlength=K)
            if t < kmeans_its:
                c = np.where(cnt > 0, s1 / np.maximum(cnt, 1.0), c)
            else:
                w, mu, var = m_step(cnt, s1, s2, n, reg_covar)
    prev, trace, changes, converged = -np.inf, [], [], False
    for it in range(1, max_iter + 1):
        lp = -0.5 * (LOG_2PI + np.log(var) + (y[:, None] - mu) ** 2 / var) + np.log(w)
        m = lp.max(axis=1)
        lse = m + np.log(np.exp(lp - m[:, None]).sum(axis=1))
        r = np.exp(lp - lse[:, None])
        lb = lse.mean()
        w, mu, var = m_step(r.sum(axis=0), (r * y[:, None]).sum(axis=0), (r * (y * y)[:, None]).sum(axis=0), n, reg_covar)
        change, prev = lb - prev, lb
        trace.append(lb)
        changes.append(change)
        if abs(change) < tol:
            converged = True
            break
    return dict(w=w, mu=mu + mean, var=var, lower_bound=lb, n_iter=it, converged=converged, trace=np.array(trace),
                changes=np.array(changes))


def fit_rows(x, K, **kw):
    """``fit`` of every row: dict of stacked arrays"""
    rows = [fit(r, K, **kw) for r in x]
    return {k: np.array([r[k] for r in rows]) for k in ('w', 'mu', 'var', 'lower_bound', 'n_iter', 'converged')}, rows


# ---- rows ---------------------------------------------------------------------------------------------------------------------------
def separated(rs, n, comps):
    """n draws from `comps` components 0.25 apart with standard deviations 0.015 .. 0.03 (>= 8 sd between neighbours)"""
    mus = 0.05 + 0.25 * (np.arange(comps) - 0.5 * (comps - 1))
    sds = rs.uniform(0.015, 0.03, comps)
    p = rs.dirichlet(4.0 * np.ones(comps))
    z = rs.choice(comps, size=n, p=p)
    return mus[z] + sds[z] * rs.randn(n)


def overlapping(rs, n):
    z = rs.rand(n) < 0.4
    return np.where(z, -0.08 + 0.1 * rs.randn(n), 0.07 + 0.15 * rs.randn(n)).clip(-0.6, 0.6)


def unit_grid(rs, n):
    """standard normal draws rounded to multiples of 2^-20: 1e6 + z is exact"""
    return np.round(rs.randn(n).clip(-6, 6) * 2.0 ** 20) / 2.0 ** 20


def two_values(rs, n):
    """2^-8 and -2^-7.  Every component sits on one value, so var = reg_covar + the rounding of s2 / nk - mu^2, which for a
    sum of n equal terms taken in index order can reach n ulp(y^2) / 4: 3e-17 here at n = 5000, below 1e-9 reg_covar (at
    values ~0.1 it is 1e-15, and two correct evaluations then differ by 1e-9 in var)"""
    x = np.where(rs.rand(n) < 0.35, 2.0 ** -8, -2.0 ** -7)
    x[0], x[-1] = 2.0 ** -8, -2.0 ** -7
    return x


def length(n, K):
    return K if n is None else n


@functools.lru_cache(maxsize=None)
def launch_rows(n, K):
    """[7, length(n, K)]: rows 0 .. 3 from 1 .. 4 separated components, 4 overlapping, 5 constant, 6 shifted by 1e6 (sd 1)"""
    rs = np.random.RandomState(1000 * length(n, K) + K)
    m = length(n, K)
    rows = [separated(rs, m, c) for c in (1, 2, 3, 4)] + [overlapping(rs, m), np.full(m, 2.5), 1e6 + unit_grid(rs, m)]
    x = np.ascontiguousarray(np.stack(rows))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def two_value_row(n):
    x = two_values(np.random.RandomState(77 + length(n, 3)), length(n, 3))[None, :].copy()
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def many_rows(R=300, n=65):
    """more rows than compute units, at a small odd n: every kind of row in turn"""
    rs = np.random.RandomState(300)
    kinds = [lambda: separated(rs, n, 1), lambda: separated(rs, n, 2), lambda: separated(rs, n, 3), lambda: overlapping(rs, n),
             lambda: 1e6 + unit_grid(rs, n)]
    x = np.ascontiguousarray(np.stack([kinds[r % len(kinds)]() for r in range(R)]))
    x.setflags(write=False)
    return x


FIXED = dict(tol=0.0, max_iter=20)          # a fixed number of iterations


@functools.lru_cache(maxsize=None)
def reference(n, K, fixed, two=False):
    """the restatement of a launch, computed once: (stacked outputs, per-row dicts)"""
    x = two_value_row(n) if two else launch_rows(n, K)
    return fit_rows(x, K, **(FIXED if fixed else {}))


def assert_fit_close(got, want, x, tol=1e-9, what=''):
    """the comparison of the issue: w within tol, mu within tol * sd(row), var within tol relative, lower bound within tol
    (relative to max(1, |value|)); got: ScalarMixtures (NumPy) or a dict"""
    g = got if isinstance(got, dict) else dict(w=got.w, mu=got.mu, var=got.var, lower_bound=got.lower_bound)
    sd = np.asarray(x).std(axis=1)[:, None]
    dmu = np.abs(g['mu'] - want['mu'])
    with np.errstate(divide='ignore', invalid='ignore'):
        emu = np.where(dmu == 0, 0.0, dmu / sd)             # a constant row (sd = 0) has to agree exactly
    errs = dict(w=np.abs(g['w'] - want['w']).max(),
                mu=emu.max(),
                var=(np.abs(g['var'] - want['var']) / want['var']).max(),
                lower_bound=(np.abs(g['lower_bound'] - want['lower_bound']) / np.maximum(1.0, np.abs(want['lower_bound']))).max())
    print('%s: max errors %s' % (what, ', '.join('%s %.3g' % kv for kv in errs.items())))
    for k, e in errs.items():
        assert e <= tol, '%s: %s differs by %.3g > %g' % (what, k, e, tol)
    return errs


def assert_clear_of_tol(rows, tol=1e-3, margin=1e-6):
    """the stop of the restatement must not hang on rounding: | |change| - tol | >= margin at every iteration up to the stop"""
    for i, r in enumerate(rows):
        d = np.abs(np.abs(r['changes'][1:]) - tol)          # (the first change is +inf)
        assert d.size == 0 or d.min() >= margin, 'row %d: |change| comes within %.3g of tol at iteration %d' % (
            i, d.min(), int(np.argmin(d)) + 2)
