"""CPU tests of the KL divergence of scalar Gaussian mixtures (lhvi/gmkl.py, csrc/gmkl.hpp through ``lhvi_gm_kl_host``): the
closed form, the reference's own route (scipy's ``quad`` on its integrand through ``lhvi.utils.kl_continuous_logpdf``), the
NumPy restatement of tests/gmkl_models.py, the edge cases of the method, the argument errors and the providers.
tests/test_gpu_gmkl.py repeats the comparisons on the device.

The reference's route: ``kl_continuous_logpdf`` hands its keyword arguments to ``quad`` and, like the reference, returns the
value alone (the ``full_output`` tuple is cut to its first entry), so the error estimate and the warning of that very call are
read by wrapping ``scipy.integrate.quad`` for the duration of the call (``scipy_kl``)."""
import numpy as np
import pytest

import gmkl_models as gm
from lhvi import _abi, gmkl, utils
from lhvi.gmfit import ScalarMixtures
from lhvi.mixture import MixtureBelief

EPS = 1.49e-8
RANGES = [(-np.inf, np.inf), (-6.0, 6.0)]
SEEDS = {'mild': 11, 'wide': 12, 'narrow': 13}


def kl_host(p, q, a=-np.inf, b=np.inf, **kw):
    kl, info = gmkl.kl_scalar_mixtures(p, q, a, b, host=True, info=True, **kw)
    return kl, info['abserr'], info['status'], info['neval']


def within(got, err, want, want_err=0.0):
    return np.abs(got - want) <= err + want_err + 1e-12 * np.maximum(1.0, np.abs(want))


def scipy_kl(p, q, a, b):
    """(kl, abserr, warned) of ``utils.kl_continuous_logpdf`` on the mixtures' log densities over the method's range (L, U),
    with ``points`` the means of p inside it"""
    import scipy.integrate
    L, U, P, _ = gm.plan(p, a, b)
    if P == 0:
        return 0.0, 0.0, False
    mu = p[1][p[0] > 0]
    pts = np.sort(mu[(mu > L) & (mu < U)])
    seen, real = [], scipy.integrate.quad

    def recording(f, lo, hi, *args, **kw):
        out = real(f, lo, hi, *args, **kw)
        seen.append(out)
        return out
    scipy.integrate.quad = recording
    try:
        val = utils.kl_continuous_logpdf(lambda x: float(gm.log_mixture(x, *p)[0]), lambda x: float(gm.log_mixture(x, *q)[0]), L, U,
                                         points=pts, limit=400, full_output=1)
    finally:
        scipy.integrate.quad = real
    assert len(seen) == 1 and seen[0][0] == val
    return float(val), float(seen[0][1]), len(seen[0]) > 3          # (a fourth entry is scipy's warning message)


# ---- closed form -------------------------------------------------------------------------------------------------------------------
def test_normal_pairs_match_the_closed_form():
    m1, s1, m2, s2 = gm.normal_pairs(200, 1)
    kl, err, st, ne = kl_host((np.ones(1), m1[:, None], s1[:, None] ** 2), (np.ones(1), m2[:, None], s2[:, None] ** 2))
    exact = np.array([utils.kl_normal(*t) for t in zip(m1, m2, s1, s2)])
    assert abs(exact[0] - 1192.78) < 0.01           # the pair on which plain bisection of (-15, 15) returns 1e-30
    print('worst |kl - exact| / max(1, |exact|) = %.3g, evaluations <= %d' % (np.max(np.abs(kl - exact) / np.maximum(1, np.abs(exact))), ne.max()))
    assert within(kl, err, exact).all()
    assert (st == 0).all()


# ---- the reference's route and the restatement ----------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def family_results():
    out = {}
    for fam in gm.FAMILIES:
        rows = gm.family_rows(fam, 40, SEEDS[fam])
        for a, b in RANGES:
            out[fam, a] = (rows, a, b, kl_host(tuple(rows[:3]), tuple(rows[3:]), a, b))
    return out


@pytest.mark.parametrize('a', [r[0] for r in RANGES])
@pytest.mark.parametrize('fam', list(gm.FAMILIES))
def test_rows_match_scipy_on_the_reference_integrand(family_results, fam, a):
    rows, a, b, (kl, err, st, ne) = family_results[fam, a]
    warned, bad = 0, []
    for r in range(40):
        ref, ref_err, w = scipy_kl(tuple(t[r] for t in rows[:3]), tuple(t[r] for t in rows[3:]), a, b)
        warned += w
        if not w and not within(kl[r], err[r], ref, ref_err):
            bad.append((r, kl[r], ref, err[r], ref_err))
    assert warned == 0                              # the filter above hides nothing
    assert not bad, bad
    assert (st == 0).all()


@pytest.mark.parametrize('a', [r[0] for r in RANGES])
@pytest.mark.parametrize('fam', list(gm.FAMILIES))
def test_host_twin_matches_the_restatement(family_results, fam, a):
    rows, a, b, (kl, err, st, ne) = family_results[fam, a]
    tk, te, ts, tn = gm.kl_twin_rows(rows[:3], rows[3:], a, b)
    assert within(kl, err, tk, te).all()
    np.testing.assert_array_equal(st, ts)
    np.testing.assert_array_equal(ne, tn)


@pytest.mark.parametrize('Kp,Kq', [(64, 65), (65, 130), (130, 1)])
def test_many_components_match_the_restatement(Kp, Kq):
    rng = np.random.default_rng(Kp * 1000 + Kq)
    p, q = gm.rand_gm(rng, Kp, *gm.FAMILIES['wide']), gm.rand_gm(rng, Kq, *gm.FAMILIES['wide'])
    kl, err, st, ne = kl_host(tuple(t[None] for t in p), tuple(t[None] for t in q))
    tk, te, ts, tn = gm.kl_twin(p, q)
    assert within(kl[0], err[0], tk, te) and st[0] == ts == 0 and ne[0] == tn


# ---- edge cases -----------------------------------------------------------------------------------------------------------------------
def test_equal_mixtures_give_zero():
    rows = gm.family_rows('wide', 10, 3)
    kl, err, st, _ = kl_host(tuple(rows[:3]), tuple(rows[:3]))
    assert (np.abs(kl) <= EPS).all() and (st == 0).all()
    assert (kl == 0).all()                          # the same operations on both sides: log p - log q is exactly 0


def test_zero_weight_padding_keeps_the_bits():
    rng = np.random.default_rng(5)
    p, q = gm.rand_gm(rng, 3, *gm.FAMILIES['wide']), gm.rand_gm(rng, 2, *gm.FAMILIES['wide'])
    plain = kl_host(tuple(t[None] for t in p), tuple(t[None] for t in q))

    def pad(m, K, where):
        w, mu, var = np.zeros(K), np.full(K, 77.0), np.full(K, 1e-9)           # padding no valid component resembles
        w[where], mu[where], var[where] = m
        return w[None], mu[None], var[None]
    padded = kl_host(pad(p, 7, [0, 3, 6]), pad(q, 5, [1, 4]))
    for x, y in zip(plain, padded):
        np.testing.assert_array_equal(x, y)


def test_empty_and_clipped_ranges():
    p, q = (np.ones(1), np.array([[1.0]]), np.array([[0.25]])), (np.ones(1), np.array([[0.0]]), np.array([[1.0]]))
    full = utils.kl_normal(1.0, 0.0, 0.5, 1.0)
    a = np.array([20.0, -30.0, 0.5, 2.0, 1.0, -np.inf])
    b = np.array([30.0, -20.0, 0.5, 1.0, np.inf, 1.0])
    kl, err, st, ne = kl_host(p, q, a, b)
    assert (kl[:4] == 0).all() and (err[:4] == 0).all() and (st == 0).all() and (ne[:4] == 0).all()     # U <= L; a == b; a > b
    # the range cuts the component of p at its mean: the two halves add up to the whole
    assert abs(kl[4] + kl[5] - full) <= err[4] + err[5] + 1e-12
    for r in (4, 5):
        tk, te, ts, tn = gm.kl_twin(tuple(t.reshape(-1) for t in p), tuple(t.reshape(-1) for t in q), a[r], b[r])
        assert within(kl[r], err[r], tk, te) and ne[r] == tn


def test_panel_cap_sets_its_bit_and_returns_a_value():
    p = (np.array([[0.5, 0.5]]), np.array([[-10.0, 10.0]]), np.array([[1e-8, 1.0]]))
    q = (np.ones((1, 1)), np.zeros((1, 1)), np.full((1, 1), 25.0))
    kl, err, st, ne = kl_host(p, q)
    assert st[0] & gmkl.STATUS_PANEL_CAP and np.isfinite(kl[0]) and ne[0] >= 21 * gmkl.MAX_PANELS
    tk, te, ts, tn = gm.kl_twin(tuple(t[0] for t in p), tuple(t[0] for t in q))
    assert st[0] == ts and ne[0] == tn and within(kl[0], err[0], tk, te)


@pytest.mark.parametrize('what', ['nan_mu', 'inf_var', 'zero_var', 'neg_var', 'neg_w', 'zero_w', 'nan_q', 'zero_wq', 'nan_a'])
def test_invalid_row_is_nan_and_its_neighbours_are_unchanged(what):
    rows = gm.family_rows('mild', 3, 21)
    good = kl_host(tuple(rows[:3]), tuple(rows[3:]), -4.0, 5.0)
    rows = [t.copy() for t in rows]
    a = np.full(3, -4.0)
    if what == 'nan_mu':
        rows[1][1, 0] = np.nan
    elif what == 'inf_var':
        rows[2][1, 0] = np.inf
    elif what == 'zero_var':
        rows[2][1, 4] = 0.0                         # (a padding component: its weight does not excuse it)
    elif what == 'neg_var':
        rows[2][1, 0] = -1.0
    elif what == 'neg_w':
        rows[0][1, 0] = -0.1
    elif what == 'zero_w':
        rows[0][1] = 0.0
    elif what == 'nan_q':
        rows[4][1, 0] = np.nan
    elif what == 'zero_wq':
        rows[3][1] = 0.0
    else:
        a[1] = np.nan
    kl, err, st, ne = kl_host(tuple(rows[:3]), tuple(rows[3:]), a, 5.0)
    assert np.isnan(kl[1]) and st[1] == gmkl.STATUS_INVALID and ne[1] == 0
    for r in (0, 2):
        assert (kl[r], err[r], st[r], ne[r]) == (good[0][r], good[1][r], good[2][r], good[3][r])


def test_argument_errors():
    l = _abi.lib()
    one = np.ones((2, 1))
    out = np.empty(2)
    ptr = lambda t: t.ctypes.data               # noqa: E731

    def call(R=2, Kp=1, Kq=1, epsabs=EPS, epsrel=EPS, null=None):
        args = [R, Kp, ptr(one), ptr(one), ptr(one), Kq, ptr(one), ptr(one), ptr(one), ptr(one), ptr(one), epsabs, epsrel,
                ptr(out), None, None, None]
        if null is not None:
            args[null] = None
        return l.lhvi_gm_kl_host(*args)
    assert call() == 0                          # abserr, status and neval may be NULL
    for kw in (dict(R=0), dict(R=-1), dict(Kp=0), dict(Kq=0), dict(epsabs=-1.0), dict(epsrel=-1.0), dict(epsabs=np.nan),
               dict(epsrel=np.nan)):
        assert call(**kw) == -1, kw
    for null in (2, 3, 4, 6, 7, 8, 9, 10, 13):
        assert call(null=null) == -1, null
    assert l.lhvi_gm_kl(0, 1, *([None] * 3), 1, *([None] * 5), EPS, EPS, None, None, None, None, None, None) == -1
    assert l.lhvi_gm_kl_ws_doubles(5) >= 0
    with pytest.raises(ValueError, match='negative'):
        gmkl.kl_scalar_mixtures((one[0], one, one), (one[0], one, one), epsabs=-1.0, host=True)
    with pytest.raises(ValueError, match='disagree'):
        gmkl.kl_scalar_mixtures((one[0], one, one), (one[0], np.ones((3, 1)), np.ones((3, 1))), host=True)
    with pytest.raises(ValueError, match='one K'):
        gmkl.kl_scalar_mixtures((np.ones(2), one, one), (one[0], one, one), host=True)
    with pytest.raises(ValueError, match='tuple'):
        gmkl.kl_scalar_mixtures(3.0, (one[0], one, one), host=True)


def test_zero_tolerances_stop_at_the_work_limit():
    """epsabs = epsrel = 0 can never be met: the row's 4096 bisections are spent, everything after is accepted as it stands,
    status bit 0 says so and the evaluations stay below 21 P + 42 * 4096"""
    rows = gm.family_rows('wide', 3, 17)
    p, q = tuple(rows[:3]), tuple(rows[3:])
    kl, err, st, ne = kl_host(p, q, epsabs=0.0, epsrel=0.0)
    ref = kl_host(p, q)
    for r in range(3):
        P = gm.plan(tuple(t[r] for t in p), -np.inf, np.inf)[2]
        assert st[r] == gmkl.STATUS_TOLERANCE and ne[r] == 21 * P + 42 * gm.MAX_BISECT
        # (depth first: the bisections go to the leftmost panels, the others keep their pass-1 values and estimates)
        assert within(kl[r], err[r], ref[0][r], ref[1][r])
    tk, te, ts, tn = gm.kl_twin_rows(p, q, -np.inf, np.inf, epsabs=0.0, epsrel=0.0)
    assert within(kl, err, tk, te).all()
    np.testing.assert_array_equal(st, ts)
    np.testing.assert_array_equal(ne, tn)


def test_one_row_operands_serve_every_row():
    rows = gm.family_rows('mild', 4, 23)
    full = kl_host(tuple(rows[:3]), tuple(rows[3:]))[0]
    for r in range(4):          # mu, var of one row against w [R, K] made of that row's weights; q as 1-D arrays
        p = (np.repeat(rows[0][r:r + 1], 3, axis=0), rows[1][r:r + 1], rows[2][r])
        got = kl_host(p, tuple(t[r] for t in rows[3:]))[0]
        np.testing.assert_array_equal(got, np.repeat(full[r], 3))


def test_without_a_gpu_the_default_raises():
    import torch
    if torch.cuda.is_available():
        return                                  # (with a GPU the default runs there: tests/test_gpu_gmkl.py)
    one = np.ones((1, 1))
    with pytest.raises(_abi.LhviError):
        gmkl.kl_scalar_mixtures((one[0], one, one), (one[0], one, one))


# ---- providers -----------------------------------------------------------------------------------------------------------------------
def test_scalar_mixtures_kl_and_from_normals():
    m1, s1, m2, s2 = gm.normal_pairs(12, 2)
    p, q = ScalarMixtures.from_normals(m1, s1 ** 2, host=True), ScalarMixtures.from_normals(m2, s2 ** 2)
    assert (p.R, p.K) == (12, 1) and p.host and (p.w == 1).all()
    kl, info = p.kl(q, info=True)
    assert within(kl, info['abserr'], np.array([utils.kl_normal(*t) for t in zip(m1, m2, s1, s2)])).all()
    rows = gm.family_rows('mild', 12, 4)
    mix = ScalarMixtures(*rows[3:], host=True)
    np.testing.assert_array_equal(p.kl(mix, -3.0, 4.0), kl_host((p.w, p.mu, p.var), tuple(rows[3:]), -3.0, 4.0)[0])
    np.testing.assert_array_equal(mix.kl((q.w, q.mu, q.var)), kl_host(tuple(rows[3:]), (q.w, q.mu, q.var))[0])


def test_mixture_belief_scalar_mixtures():
    rng = np.random.default_rng(8)
    K, Nc = 4, 5
    w = rng.dirichlet(np.ones(K))
    Mu, Var = rng.uniform(-3, 3, (Nc, K)), rng.uniform(0.2, 2.0, (Nc, K))
    Pi = [rng.dirichlet(np.ones(3), K)]
    belief = MixtureBelief(w, Mu, Var, Pi)
    sm = belief.scalar_mixtures(host=True)
    assert (sm.R, sm.K) == (Nc, K)
    np.testing.assert_array_equal(sm.w, np.broadcast_to(w, (Nc, K)))
    np.testing.assert_array_equal(sm.mu, Mu)
    np.testing.assert_array_equal(sm.var, Var)
    some = belief.scalar_mixtures(rows=[3, 1], host=True)
    np.testing.assert_array_equal(some.mu, Mu[[3, 1]])
    other = ScalarMixtures.from_normals(np.zeros(Nc), np.full(Nc, 4.0))
    kl = sm.kl(other)
    np.testing.assert_array_equal(kl, kl_host((w, Mu, Var), (np.ones(1), np.zeros((Nc, 1)), np.full((Nc, 1), 4.0)))[0])
    assert (kl > 0).all()
    with pytest.raises(ValueError, match='not continuous'):
        belief.scalar_mixtures(rows=[Nc])
    with pytest.raises(ValueError, match="normaliser 'gaussian'"):
        MixtureBelief(w, Mu, Var, normaliser='vi').scalar_mixtures()
    with pytest.raises(ValueError, match='no continuous rows'):
        MixtureBelief(w, Pi=Pi).scalar_mixtures()
    belief._side(True)          # a prepared side changes nothing: a belief built from arrays gives arrays
    assert isinstance(belief.scalar_mixtures(host=True).mu, np.ndarray)
