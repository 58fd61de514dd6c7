"""CPU tests of ``KL(p || q)`` with ``p`` a scalar Gaussian mixture and ``q`` any log density (docs/kernels_pbkl.md):
``lhvi.gmkl.kl_mixture_logpdf`` through ``lhvi_gm_kl_fn_host`` -- csrc/gmkl.hpp::kl_row with a host context whose q side calls
back -- against the mixture twin (``lhvi_gm_kl_host``), the reference's own route (scipy's ``quad`` on its integrand through
``lhvi.utils.kl_continuous_logpdf``), the NumPy restatement of tests/pbkl_models.py and the edge cases of the method; the ABI
of ``lhvi_pbp_kl`` and the argument checks of ``kl_from`` that come before any launch.  tests/test_gpu_pbkl.py runs the device
kernel with a particle solver's belief as ``q``."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import pbkl_models as pm
from lhvi import _abi, gmkl, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1.49e-8
RANGES = [(-np.inf, np.inf), (-6.0, 6.0)]
SEEDS = {'mild': 11, 'wide': 12, 'narrow': 13}


def kl_fn(p, log_q, a=-np.inf, b=np.inf, **kw):
    kl, info = gmkl.kl_mixture_logpdf(p, log_q, a, b, info=True, **kw)
    return kl, info['abserr'], info['status'], info['neval']


def mixture_logq(q):
    """(scalar callback, vectorised form) of the log density of the padded mixture rows q, by NumPy's log-sum-exp"""
    return (lambda x, r: float(pm.log_p(x, *(t[r] for t in q))[0])), (lambda x, r: pm.log_p(x, *(t[r] for t in q)))


# ---- T1 / T3: the callback twin against the mixture twin and against the restatement ---------------------------------------------------
@pytest.fixture(scope='module')
def family_results():
    out = {}
    for fam in pm.FAMILIES:
        rows = pm.family_rows(fam, 40, SEEDS[fam])
        p, q = tuple(rows[:3]), tuple(rows[3:])
        for a, b in RANGES:
            out[fam, a] = (p, q, a, b, kl_fn(p, mixture_logq(q)[0], a, b))
    return out


@pytest.mark.parametrize('a', [r[0] for r in RANGES])
@pytest.mark.parametrize('fam', list(pm.FAMILIES))
def test_callback_twin_matches_the_mixture_twin(family_results, fam, a):
    """the two differ only by the last bits of lq (NumPy's log-sum-exp against the running one), and a shift delta of lq moves
    the KL by at most delta"""
    p, q, a, b, (kl, err, st, ne) = family_results[fam, a]
    mk, info = gmkl.kl_scalar_mixtures(p, q, a, b, host=True, info=True)
    np.testing.assert_array_equal(st, info['status'])
    gap = np.abs(kl - mk)
    print('%s: worst |callback - mixture| = %.3g, neval equal on %d of 40 rows' % (fam, gap.max(), int((ne == info['neval']).sum())))
    assert (gap <= err + info['abserr'] + 1e-12 * np.maximum(1.0, np.abs(mk))).all()


@pytest.mark.parametrize('a', [r[0] for r in RANGES])
@pytest.mark.parametrize('fam', list(pm.FAMILIES))
def test_callback_twin_matches_the_restatement(family_results, fam, a):
    p, q, a, b, (kl, err, st, ne) = family_results[fam, a]
    tk, te, ts, tn = pm.kl_logq_rows(p, mixture_logq(q)[1], a, b)
    np.testing.assert_array_equal(st, ts)
    np.testing.assert_array_equal(ne, tn)
    assert (np.abs(kl - tk) <= err + te + 1e-12 * np.maximum(1.0, np.abs(tk))).all()


# ---- T2: log densities that are no mixtures, against the reference's method ------------------------------------------------------------
def other_densities(seed, n=12):
    """n seeded rows: p a mild mixture, q one of Laplace / Student t (3 degrees of freedom) / a Gaussian log density with a
    bounded ripple, in turn"""
    rng = np.random.default_rng(seed)
    rows = pm.family_rows('mild', n, seed)
    qs = []
    for r in range(n):
        loc, scale = rng.uniform(-2.0, 2.0), rng.uniform(0.8, 2.5)
        qs.append([pm.laplace(loc, scale), pm.student_t3(loc, scale),
                   pm.rippled_normal(loc, scale, rng.uniform(0.1, 0.5), rng.uniform(0.5, 3.0))][r % 3])
    return tuple(rows[:3]), qs


def scipy_kl(p, log_q, a, b):
    """(kl, abserr, warned) of ``utils.kl_continuous_logpdf`` over the method's range (L, U) with ``points`` the means of p
    inside it; the estimate and the warning of that very call are read by wrapping ``scipy.integrate.quad`` for its duration"""
    import scipy.integrate
    L, U, P, _ = pm.panels(p, a, b)
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
        val = utils.kl_continuous_logpdf(lambda x: float(pm.log_p(x, *p)[0]), lambda x: float(log_q(x)), L, U, points=pts,
                                         limit=400, full_output=1)
    finally:
        scipy.integrate.quad = real
    assert len(seen) == 1 and seen[0][0] == val
    return float(val), float(seen[0][1]), len(seen[0]) > 3


@pytest.mark.parametrize('a,b', RANGES)
def test_other_densities_match_scipy_on_the_reference_integrand(a, b):
    p, qs = other_densities(31)
    kl, err, st, ne = kl_fn(p, lambda x, r: float(qs[r](x)), a, b)
    warned, bad = 0, []
    for r, q in enumerate(qs):
        ref, ref_err, w = scipy_kl(tuple(t[r] for t in p), q, a, b)
        warned += w
        print('row %d: kl %.12g, scipy %.12g, abserr %.3g, scipy abserr %.3g, neval %d' % (r, kl[r], ref, err[r], ref_err, ne[r]))
        if not abs(kl[r] - ref) <= err[r] + ref_err + 1e-12 * max(1.0, abs(ref)):
            bad.append((r, kl[r], ref, err[r], ref_err))
    assert warned == 0                              # no row is dropped: scipy warns on none of them
    assert not bad, bad
    assert (st == 0).all()
    tk, te, ts, tn = pm.kl_logq_rows(p, lambda x, r: qs[r](x), a, b)       # (T3 on these rows too)
    np.testing.assert_array_equal(st, ts)
    np.testing.assert_array_equal(ne, tn)


# ---- T4: edge cases ----------------------------------------------------------------------------------------------------------------------
def running_log_p(x, w, mu, var):
    """log p(x) formed as docs/kernels_gmkl.md states it -- the running max-shifted log-sum-exp over the components in order, one
    exponential each -- in Python floats: the same operations in the same order as the library's, so the same bits"""
    m, s = -1.7976931348623157e308, 0.0
    for wk, mk, vk in zip(w, mu, var):
        if wk == 0.0:
            continue
        la = math.log(wk) - 0.5 * (1.8378770664093453 + math.log(vk))
        d = x - mk
        t = la + (-0.5 / vk) * (d * d)
        e = math.exp(-abs(t - m))
        s = s * e + 1.0 if t > m else s + e
        m = max(m, t)
    return m + math.log(s)


def test_log_q_equal_to_log_p_gives_exactly_zero():
    rows = pm.family_rows('wide', 10, 3)
    p = tuple(rows[:3])
    kl, err, st, ne = kl_fn(p, lambda x, r: running_log_p(x, *(t[r] for t in p)))
    assert (kl == 0).all() and (err == 0).all() and (st == 0).all() and (ne > 0).all()


def normal_logq(mu, var):
    c = -0.5 * math.log(2.0 * math.pi * var)
    return lambda x, r=0: c - 0.5 * (x - mu) ** 2 / var


def test_minus_infinity_inside_the_range_gives_plus_infinity():
    p = (np.ones(1), np.array([[0.5], [0.5]]), np.array([[1.0], [1.0]]))
    base = normal_logq(0.0, 4.0)
    kl, err, st, ne = kl_fn(p, lambda x, r: -math.inf if (r == 0 and 0.0 < x < 1.0) else base(x))
    assert kl[0] == np.inf and st[0] & gmkl.STATUS_TOLERANCE
    tk, te, ts, tn = pm.kl_logq((np.ones(1), np.array([0.5]), np.array([1.0])),
                                lambda x: np.where((0.0 < x) & (x < 1.0), -np.inf, np.vectorize(base)(x)))
    assert tk == np.inf and (st[0], ne[0]) == (ts, tn)       # pass 1 sees it: area0 and the bound are infinite, bit 0 still set
    assert st[1] == 0 and abs(kl[1] - utils.kl_normal(0.5, 0.0, 1.0, 2.0)) <= err[1] + 1e-12       # its neighbour is untouched


@pytest.mark.parametrize('what', ['nan_mu', 'zero_var', 'neg_w', 'zero_w', 'nan_a', 'nan_b'])
def test_invalid_row_is_nan_and_its_neighbours_are_unchanged(what):
    rows = pm.family_rows('mild', 3, 21)
    logq = normal_logq(0.3, 5.0)
    good = kl_fn(tuple(rows[:3]), logq, -4.0, 5.0)
    rows = [t.copy() for t in rows[:3]]
    a, b = np.full(3, -4.0), np.full(3, 5.0)
    if what == 'nan_mu':
        rows[1][1, 0] = np.nan
    elif what == 'zero_var':
        rows[2][1, 4] = 0.0                         # (a padding component: its weight does not excuse it)
    elif what == 'neg_w':
        rows[0][1, 0] = -0.1
    elif what == 'zero_w':
        rows[0][1] = 0.0
    elif what == 'nan_a':
        a[1] = np.nan
    else:
        b[1] = np.nan
    kl, err, st, ne = kl_fn(tuple(rows), logq, a, b)
    assert np.isnan(kl[1]) and np.isnan(err[1]) and st[1] == gmkl.STATUS_INVALID and ne[1] == 0
    for r in (0, 2):
        assert (kl[r], err[r], st[r], ne[r]) == (good[0][r], good[1][r], good[2][r], good[3][r])


def test_empty_and_clipped_ranges():
    p = (np.ones(1), np.array([[1.0]]), np.array([[0.25]]))
    logq = normal_logq(0.0, 1.0)
    full = utils.kl_normal(1.0, 0.0, 0.5, 1.0)
    a = np.array([20.0, -30.0, 0.5, 2.0, 1.0, -np.inf])
    b = np.array([30.0, -20.0, 0.5, 1.0, np.inf, 1.0])
    kl, err, st, ne = kl_fn(p, logq, a, b)
    assert (kl[:4] == 0).all() and (err[:4] == 0).all() and (st == 0).all() and (ne[:4] == 0).all()     # U <= L; a == b; a > b
    assert abs(kl[4] + kl[5] - full) <= err[4] + err[5] + 1e-12     # the range cuts p at its mean: the halves add up
    for r in (4, 5):
        tk, te, ts, tn = pm.kl_logq(tuple(t.reshape(-1) for t in p), np.vectorize(logq), a[r], b[r])
        assert abs(kl[r] - tk) <= err[r] + te + 1e-12 and ne[r] == tn and ts == 0


def test_panel_cap_sets_its_bit_and_returns_a_value():
    p = (np.array([[0.5, 0.5]]), np.array([[-10.0, 10.0]]), np.array([[1e-8, 1.0]]))
    logq = normal_logq(0.0, 25.0)
    kl, err, st, ne = kl_fn(p, logq)
    assert st[0] & gmkl.STATUS_PANEL_CAP and np.isfinite(kl[0]) and ne[0] >= 21 * gmkl.MAX_PANELS
    tk, te, ts, tn = pm.kl_logq(tuple(t[0] for t in p), lambda x: logq(np.asarray(x)))
    assert st[0] == ts and ne[0] == tn and abs(kl[0] - tk) <= err[0] + te + 1e-12 * max(1.0, abs(tk))


def test_zero_tolerances_stop_at_the_work_limit():
    """epsabs = epsrel = 0 can never be met: the row's 4096 bisections are spent, every interval after them is accepted as it
    stands, status bit 0 says so and the evaluations are exactly 21 P + 42 * 4096"""
    rows = pm.family_rows('wide', 2, 17)
    p = tuple(rows[:3])
    logq = normal_logq(1.0, 30.0)
    kl, err, st, ne = kl_fn(p, logq, epsabs=0.0, epsrel=0.0)
    ref = kl_fn(p, logq)
    for r in range(2):
        P = pm.panels(tuple(t[r] for t in p), -np.inf, np.inf)[2]
        assert st[r] == gmkl.STATUS_TOLERANCE and ne[r] == 21 * P + 42 * pm.BISECT_CAP
        assert abs(kl[r] - ref[0][r]) <= err[r] + ref[1][r] + 1e-12 * max(1.0, abs(ref[0][r]))
    tk, te, ts, tn = pm.kl_logq(tuple(t[0] for t in p), lambda x: logq(np.asarray(x)), epsabs=0.0, epsrel=0.0)
    assert (st[0], ne[0]) == (ts, tn) and abs(kl[0] - tk) <= err[0] + te + 1e-12 * max(1.0, abs(tk))


def test_argument_errors():
    l = _abi.lib()
    one = np.ones((2, 1))
    out = np.empty(2)
    ptr = lambda t: t.ctypes.data               # noqa: E731
    cb = _abi.GMKL_LOGQ(lambda x, r, u: -0.5 * x * x)

    def call(R=2, Kp=1, epsabs=EPS, epsrel=EPS, null=None, logq=cb):
        args = [R, Kp, ptr(one), ptr(one), ptr(one), logq, None, ptr(one), ptr(one), epsabs, epsrel, ptr(out), None, None, None]
        if null is not None:
            args[null] = None
        return l.lhvi_gm_kl_fn_host(*args)
    assert call() == 0                          # user, abserr, status and neval may be NULL
    for kw in (dict(R=0), dict(R=-1), dict(Kp=0), dict(epsabs=-1.0), dict(epsrel=-1.0), dict(epsabs=np.nan), dict(epsrel=np.nan),
               dict(logq=_abi.GMKL_LOGQ())):
        assert call(**kw) == -1, kw
    for null in (2, 3, 4, 7, 8, 11):
        assert call(null=null) == -1, null
    # lhvi_pbp_kl: every argument error is found on the host, before anything is launched
    g, pots, s = _abi.GraphStruct(), _abi.PotsStruct(), _abi.PbpStruct()
    some = C.c_void_p(ptr(one))

    def dev(nq=1, Kp=1, epsabs=EPS, epsrel=EPS, null=None, g=g, s=s):
        args = [g, pots, s, some, nq, some, None, None, None, some, Kp, some, some, some, some, some, epsabs, epsrel, some, None, None,
                None, None]
        if null is not None:
            args[null] = None
        return l.lhvi_pbp_kl(*args)
    assert dev() == -1                          # an empty graph / solver state
    g.V, s.n = 1, 4
    for f in ('var_ptr', 'var_edge', 'var_value', 'var_dom', 'dom_cont', 'dom_ptr', 'dom_lo', 'dom_hi', 'dom_val'):
        setattr(g, f, some)
    s.particles = s.np = some
    for kw in (dict(nq=0), dict(nq=-3), dict(Kp=0), dict(epsabs=-1.0), dict(epsrel=-1.0), dict(epsabs=np.nan), dict(epsrel=np.nan),
               dict(g=None), dict(s=None)):
        assert dev(**kw) == -1, kw
    for null in (1, 3, 5, 9, 11, 12, 13, 14, 15, 18):
        assert dev(null=null) == -1, null
    args = [g, pots, s, some, 1, some, some, None, None, some, 1, some, some, some, some, some, EPS, EPS, some, None, None, None, None]
    assert l.lhvi_pbp_kl(*args) == -1           # the pairs form needs qedge and qmult with qptr
    one_row = (one[0], one, one)
    with pytest.raises(ValueError, match='negative'):
        gmkl.kl_mixture_logpdf(one_row, cb, epsabs=-1.0)
    with pytest.raises(ValueError, match='disagree'):
        gmkl.kl_mixture_logpdf(one_row, lambda x, r: 0.0, a=np.zeros(3))
    with pytest.raises(ValueError, match='callable'):
        gmkl.kl_mixture_logpdf(one_row, 3.0)
    with pytest.raises(ZeroDivisionError):      # an exception of the callback is raised again after the call
        gmkl.kl_mixture_logpdf(one_row, lambda x, r: 1.0 / 0.0)


# ---- T5: the ABI ----------------------------------------------------------------------------------------------------------------------------
def header_arguments(name):
    """the parameter types of `name` as include/lhvi.h declares them, each reduced to the ctypes class of its kind"""
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'lhvi.h')).read(), flags=re.S)
    at = re.search(r'\bint\s+%s\s*\(' % name, text).end()
    depth, parts, cur = 1, [], ''
    while depth:
        ch = text[at]
        at += 1
        depth += (ch == '(') - (ch == ')')
        if ch == ',' and depth == 1:
            parts.append(cur)
            cur = ''
        elif depth:
            cur += ch
    parts.append(cur)
    kinds = []
    for decl in (' '.join(d.split()) for d in parts):
        if '(*' in decl:
            kinds.append(_abi.GMKL_LOGQ)
        elif 'lhvi_graph_t' in decl:
            kinds.append(C.POINTER(_abi.GraphStruct))
        elif 'lhvi_pots_t' in decl:
            kinds.append(C.POINTER(_abi.PotsStruct))
        elif 'lhvi_pbp_t' in decl:
            kinds.append(C.POINTER(_abi.PbpStruct))
        elif '*' in decl:
            kinds.append(C.c_void_p)
        else:
            kinds.append({'int32_t': C.c_int32, 'int64_t': C.c_int64, 'double': C.c_double}[decl.split()[0]])
    return kinds


@pytest.mark.parametrize('name', ['lhvi_pbp_kl', 'lhvi_gm_kl_fn_host'])
def test_new_entry_points_are_bound_with_the_header_signature(name):
    res, args = _abi.SIGNATURES[name]
    assert res is C.c_int and list(args) == header_arguments(name)
    assert len(header_arguments('lhvi_pbp_kl')) == 23
    fn = getattr(_abi.lib(), name)
    assert name not in _abi.MISSING and list(fn.argtypes) == list(args)
    header = open(os.path.join(ROOT, 'include', 'lhvi.h')).read()
    assert int(re.search(r'#define\s+LHVI_ABI_VERSION\s+(\d+)', header).group(1)) == _abi.ABI_VERSION == _abi.lib().lhvi_version() >= 26


# ---- T6: the argument checks of kl_from come before any launch ----------------------------------------------------------------------------
def unlaunched_solver():
    """an EPBP over a small graph with the flat arrays of a run but no device state: every check below precedes the device"""
    from lhvi.flat import flatten
    from lhvi.graph import F, RV, Domain, Graph
    from lhvi.pbp import EPBP
    from lhvi.potentials import GaussianPotential, TablePotential
    dc, dd = Domain((-5, 5), continuous=True), Domain((0, 1))
    x, y, obs, d = RV(dc), RV(dc), RV(dc, value=1.0), RV(dd)
    pair = GaussianPotential([0.0, 0.0], [[2.0, 0.5], [0.5, 1.0]])
    g = Graph()
    g.rvs = [x, y, obs, d]
    g.factors = [F(pair, (x, y)), F(pair, (y, obs)), F(TablePotential(np.array([0.6, 0.4])), (d,))]
    g.init_nb()
    bp = EPBP(g, n=8, proposal_approximation='simple')
    bp.flat = flatten(g)
    return bp, (x, y, obs, d)


def test_kl_from_refuses_bad_rows_before_any_launch():
    bp, (x, y, obs, d) = unlaunched_solver()
    flat = bp.flat
    ix, iy, iobs, idd = (flat.var_index[rv] for rv in (x, y, obs, d))
    np.testing.assert_array_equal(bp._kl_rows(None), sorted([ix, iy]))          # every continuous hidden variable, in index order
    np.testing.assert_array_equal(bp._kl_rows([y, ix]), [iy, ix])
    p1 = (np.ones(1), np.zeros((1, 1)), np.ones((1, 1)))
    p3 = (np.ones(1), np.zeros((3, 1)), np.ones((3, 1)))
    with pytest.raises(ValueError, match='observed or discrete'):
        bp.kl_from(p1, rows=[ix, iobs])
    with pytest.raises(ValueError, match='observed or discrete'):
        bp.kl_from(p1, rows=[idd])
    with pytest.raises(ValueError, match='variables of the solver'):
        bp.kl_from(p1, rows=[flat.V])
    with pytest.raises(ValueError, match='as many as rows'):
        bp.kl_from(p3)                          # three rows of p, two continuous hidden variables
    with pytest.raises(ValueError, match='as many as rows'):
        bp.kl_from(p1, rows=[ix, iy], a=np.zeros(3))
    with pytest.raises(ValueError, match='negative'):
        bp.kl_from(p1, epsrel=-1.0)
    from lhvi.gmfit import ScalarMixtures
    with pytest.raises(ValueError, match='observed or discrete'):            # ScalarMixtures.kl hands a solver to kl_from
        ScalarMixtures(np.ones((1, 1)), np.zeros((1, 1)), np.ones((1, 1))).kl(bp, rows=[iobs])
    with pytest.raises(ValueError, match='particle solver'):
        ScalarMixtures(np.ones((1, 1)), np.zeros((1, 1)), np.ones((1, 1)), host=True).kl(p1, rows=[0])
