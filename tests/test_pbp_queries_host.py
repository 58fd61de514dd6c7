"""CPU tests of the references of tests/pbp_query_models.py, which tests/test_gpu_pbp_queries.py holds the particle-BP query
kernels to: the oracle's belief against an mpmath closed form; the NumPy dqage against the closed-form normaliser and against
``scipy.integrate.quad``; how far SciPy's ``fminbound`` itself moves under a rounding-level change of its objective (the cap the
device test allows on unequal evaluation counts is twice the share measured here); the twins of the grid kernels on cases worked
out by hand."""
import numpy as np
import pytest

import pbp_query_models as pq

ROWS = 200          # mixture rows per particle count


@pytest.fixture(scope='module')
def mixtures():
    return {n: pq.mixture(n, ROWS, 100 + n) for n in pq.PARTICLE_COUNTS}


def test_constants_of_the_brent_kernel():
    """csrc/pbp.hip writes sqrt(2.2e-16) and the golden mean as hexadecimal literals"""
    assert (2.2e-16 ** 0.5).hex() == '0x1.fda324be34921p-27' and pq.GOLDEN_MEAN.hex() == '0x1.8722191a02d60p-2'


@pytest.mark.parametrize('n', pq.PARTICLE_COUNTS)
def test_oracle_belief_against_the_closed_form(mixtures, n):
    """log-beliefs of the mixture family at 41 points of the widened domain, wherever no message comes near the floor.  Bound: an
    exponent of magnitude up to 745 formed in about six roundings, and the cancellation in x1 - a x0 magnified by d / var <= 600,
    stay below 1e-11 per message; three messages and the logarithms: 1e-10 absolute is ten times that, 1e-12 relative covers the
    sums of large messages."""
    st = mixtures[n]
    xs = np.linspace(pq.LO - pq.MARGIN, pq.HI + pq.MARGIN, 41)
    worst, compared = 0.0, 0
    for v in st.rows[:60]:
        exact, safe = pq.log_belief_closed_form(st, v, xs)
        got = st.log_belief(v, xs)
        err = np.abs(got - exact)[safe]
        compared += int(safe.sum())
        worst = max(worst, float(err.max()) if err.size else 0.0)
        assert (err <= 1e-10 + 1e-12 * np.abs(exact[safe])).all(), (n, int(v))
        twin = np.array([pq.numpy_log_belief(st, v, x) for x in xs[::8]])
        np.testing.assert_allclose(twin, got[::8], rtol=1e-12, atol=1e-10)
    print('n = %d: %d points compared, worst |oracle - closed form| = %.3g' % (n, compared, worst))
    assert compared > 60 * 41 // 4


@pytest.fixture(scope='module')
def normalisers(mixtures):
    return {n: pq.dqage_state(st, st.rows) for n, st in mixtures.items()}


@pytest.mark.parametrize('n', pq.PARTICLE_COUNTS)
def test_dqage_against_the_closed_form(mixtures, normalisers, n):
    """every mixture row converges at the default tolerances, and the rows of degree 1 lie within their own estimate of the erf
    closed form"""
    st = mixtures[n]
    z, err, status = normalisers[n]
    assert (status == 0).all(), np.flatnonzero(status)
    rows = [r for r, v in enumerate(st.rows) if pq.has_closed_form(st, v)]
    assert len(rows) > ROWS // 5
    exact = np.array([pq.z_closed_form(st, st.rows[r]) for r in rows])
    gap = np.abs(z[rows] - exact)
    print('n = %d: %d rows with a closed form, worst |z - exact| / exact = %.3g' % (n, len(rows), float((gap / exact).max())))
    assert (gap <= err[rows] + 1e-12 * exact).all(), [int(st.rows[r]) for r in np.array(rows)[gap > err[rows] + 1e-12 * exact]]


@pytest.mark.parametrize('n', pq.PARTICLE_COUNTS)
def test_dqage_against_scipy_quad(mixtures, normalisers, n):
    """the same function through ``scipy.integrate.quad`` (dqagse: the same rule and bisection plus extrapolation): 1e-6
    relative, the bound tests/test_gpu_pbp.py holds ``quad_all`` to"""
    from scipy.integrate import quad
    st = mixtures[n]
    z = normalisers[n][0]
    worst = 0.0
    for r in range(0, ROWS, 4):
        v = st.rows[r]
        lo, hi = st.domain(v)
        ref = quad(lambda x: float(np.exp(st.log_belief(v, [x])[0])), lo - pq.MARGIN, hi + pq.MARGIN)[0]
        worst = max(worst, abs(z[r] - ref) / abs(ref))
    print('n = %d: worst |dqage - quad| / quad = %.3g' % (n, worst))
    assert worst <= 1e-6


def test_dqage_statuses():
    """a constant (first-rule shortcut), a kink at a tolerance no 50 intervals reach (status 1), an overflow (status 3, NaN),
    the first of two equal estimates is the one halved, and a peak that only the centre node of the first rule sees: that
    rule's estimate is at its ceiling ``resasc`` and below ``epsabs``, and QUADPACK does not stop there"""
    z, err, status = pq.dqage(lambda x: 1e-9 * np.exp(-0.5 * (x / 0.05) ** 2), -30.0, 30.0)
    assert status == 0 and abs(z - 1e-9 * 0.05 * np.sqrt(2 * np.pi)) <= err and z < 2e-10
    z, err, status = pq.dqage(lambda x: np.ones_like(x), -1.0, 3.0)
    assert (z, status) == (4.0, 0) and err <= 50 * 2.3e-16 * 4.0
    z, err, status = pq.dqage(lambda x: np.sqrt(np.abs(x - 0.3)), -1.0, 2.0, epsabs=0.0, epsrel=1e-14)
    exact = 2.0 / 3.0 * (1.3 ** 1.5 + 1.7 ** 1.5)
    assert status == 1 and abs(z - exact) <= err
    z, err, status = pq.dqage(lambda x: np.exp(800.0 - x * x), -1.0, 1.0)
    assert status == 3 and np.isnan(z)
    seen = []

    def even(x):
        seen.append(float(x[10]))
        return np.abs(x)                            # symmetric about 0: the halves [-1, 0] and [0, 1] have equal estimates
    pq.dqage(even, -1.0, 1.0, epsabs=0.0, epsrel=1e-15)
    assert seen[:5] == [0.0, -0.5, 0.5, -0.75, -0.25]


def test_brent_moves_this_little_under_a_rounding_level_change(mixtures):
    """``fminbound`` on the oracle's belief and on the NumPy restatement that adds every message's terms in the reverse order: the
    share of rows whose evaluation counts differ is the noise floor of "same iterates" (cap: 0.5 % of the rows; the device test
    allows twice that), and on the rows that agree the minimisers agree far below the 2e-6 the project uses for it"""
    differ = total = 0
    worst_same = worst_all = 0.0
    for n, st in mixtures.items():
        lo, hi = np.array([st.domain(v) for v in st.rows]).T
        xa, _, ka, _ = pq.brent_rows(lambda r, x: st.log_belief(st.rows[r], [x])[0], lo, hi)
        xb, _, kb, _ = pq.brent_rows(lambda r, x: pq.numpy_log_belief(st, st.rows[r], x, reverse=True), lo, hi)
        gap = np.abs(xa - xb) / np.maximum(1.0, np.abs(xa))
        same = ka == kb
        differ, total = differ + int((~same).sum()), total + same.size
        worst_same, worst_all = max(worst_same, float(gap[same].max())), max(worst_all, float(gap.max()))
        assert 0 < ka.min() and ka.max() < 500
    print('fminbound under a rounding-level change: nfev differs on %d of %d rows (%.3f %%); worst |dx| / max(1, |x|) = %.3g on '
          'the rows that agree, %.3g over all' % (differ, total, 100.0 * differ / total, worst_same, worst_all))
    assert differ <= 0.005 * total
    assert worst_same <= 2e-6


def test_brent_reference_on_the_edge_families():
    """what the device test takes for granted about SciPy: one evaluation at the golden-section point on a domain narrower than
    the tolerance; a run into the domain end on a monotone belief; the limit flag with ``maxfun`` evaluations (two when
    ``maxfun`` is 1: the loop counts before it looks at the limit)"""
    st = pq.narrow(5, 8, 3)
    x, f, nfev, flag = pq.brent_state(st, st.rows)
    lo, hi = np.array([st.domain(v) for v in st.rows]).T
    assert (nfev == 1).all() and not flag.any() and (x == lo + pq.GOLDEN_MEAN * (hi - lo)).all()
    st = pq.end(5, 12, 1)
    x, f, nfev, flag = pq.brent_state(st, st.rows)
    assert (np.abs(x - st.info['side'] * pq.HI) < 1e-4).all()
    for maxfun in (1, 2, 5):
        x, f, nfev, flag = pq.brent_state(st, st.rows, maxfun=maxfun)
        assert flag.all() and (nfev == max(maxfun, 2)).all()
    st = pq.flat_family(5, 6, 2)
    x, f, nfev, flag = pq.brent_state(st, st.rows)
    assert (f == pq.FLOOR * np.diff(st.flat.var_ptr)[st.rows]).all() and len(set(nfev.tolist())) == 1
    st = pq.discrete(4)
    x, f, nfev, flag = pq.brent_state(st, st.rows)
    for r, pair in enumerate(st.info['tie']):
        assert nfev[r] == st.states(st.rows[r]).size
        if pair is not None:
            vals = st.log_belief(st.rows[r], st.states(st.rows[r]))
            assert vals[pair[0]] == vals[pair[1]] == vals.max() and x[r] == float(pair[0])


# ---- the twins of the grid kernels on cases worked out by hand ------------------------------------------------------------------------
def _tiny(n):
    """continuous variables 0 .. 2 on [-1, 3], variable 3 observed at 0.5, variable 4 with the states (0, 1) where n has room"""
    b = pq._Builder([pq._cont(-1.0, 3.0, 4), pq._disc(2)])
    for _ in range(3):
        b.var(0)
    b.var(0, 0.5)
    if n >= 2:
        b.var(1)
    for u, v in ((0, 1), (1, 2), (2, 3)) + (((4, 0),) if n >= 2 else ()):
        b.factor((u, v), pq.LINEAR_GAUSSIAN if u != 4 else pq.HYBRID_QUADRATIC,
                 [1.0, 1.0] if u != 4 else [1, 1, 2, -0.1, -0.2, 0.0, 0.0, 0.0, 0.0])
    flat = b.flat()
    from oracle import oracle
    return flat, oracle.pbp_counts(flat, n)


@pytest.mark.parametrize('n', [1, 2, 3])
def test_domain_grid_twin_by_hand(n):
    flat, counts = _tiny(n)
    x = pq.domain_grid_twin(flat, counts, n)
    want = {1: [3.0], 2: [-1.0, 3.0], 3: [-1.0, 1.0, 3.0]}[n]
    assert (x[:3] == want).all() and (x[3] == 0.0).all()
    if n >= 2:
        assert x[4].tolist() == [0.0, 1.0] + [0.0] * (n - 2)


def test_refine_grid_twin_by_hand():
    """n = 3 on [-1, 1, 3]: the maximum in the middle, at either end (the bracket is clamped to the grid), a tie (the first wins),
    the observed and the discrete row; n = 5 with an uneven old grid; n = 2: no new grid below three points"""
    flat, counts = _tiny(3)
    x0 = pq.domain_grid_twin(flat, counts, 3)
    logb = np.array([[0.0, 2.0, 1.0], [5.0, 1.0, 0.0], [0.0, 1.0, 1.0], [9.0, 9.0, 9.0], [1.0, 1.0, 7.0]])
    x, best, val = pq.refine_grid_twin(flat, counts, logb, x0)
    assert x[0].tolist() == [-1.0, 1.0, 3.0] and (best[0], val[0]) == (1.0, 2.0)
    assert x[1].tolist() == [-1.0, 0.0, 1.0] and (best[1], val[1]) == (-1.0, 5.0)
    assert x[2].tolist() == [-1.0, 1.0, 3.0] and (best[2], val[2]) == (1.0, 1.0)
    assert x[3].tolist() == x0[3].tolist() and (best[3], val[3]) == (0.5, 0.0)
    assert x[4].tolist() == [0.0, 1.0, 0.0] and (best[4], val[4]) == (0.0, 1.0)                # two states: column 2 is not read
    logb[2] = [0.0, 1.0, 4.0]
    x, best, val = pq.refine_grid_twin(flat, counts, logb, x0)
    assert x[2].tolist() == [1.0, 2.0, 3.0] and (best[2], val[2]) == (3.0, 4.0)
    flat, counts = _tiny(5)
    x0 = np.tile([-1.0, 0.0, 0.5, 2.5, 3.0], (flat.V, 1))
    logb = np.zeros((flat.V, 5))
    logb[0, 2] = logb[1, 4] = 1.0
    x, best, val = pq.refine_grid_twin(flat, counts, logb, x0)
    assert x[0].tolist() == [0.0, 0.625, 1.25, 1.875, 2.5] and x[1].tolist() == [2.5, 2.625, 2.75, 2.875, 3.0] and best[1] == 3.0
    flat, counts = _tiny(2)
    x0 = pq.domain_grid_twin(flat, counts, 2)
    x, best, val = pq.refine_grid_twin(flat, counts, np.array([[0.0, 1.0]] * flat.V), x0)
    assert (x == x0).all() and best[:3].tolist() == [3.0] * 3 and best[4] == 1.0


def test_var_sum_and_trapezoid_twins_by_hand():
    flat, counts = _tiny(2)
    f2v = np.arange(flat.E * 4, dtype=np.float64).reshape(flat.E, 4)         # S = n + T = 2 + ... : only the first n columns are read
    out = pq.var_sum_twin(flat, counts, 2, f2v)
    for v in range(flat.V):
        edges = flat.var_edge[flat.var_ptr[v]:flat.var_ptr[v + 1]]
        want = f2v[edges][:, :2].sum(axis=0) if flat.var_hidden[v] else np.zeros(2)
        assert out[v].tolist() == want.tolist()
    area, shift = pq.log_area_twin(lambda x: np.zeros_like(x), 0.0, 2.0, 5)
    assert (area, shift) == (2.0, 0.0)
    area, shift = pq.log_area_twin(lambda x: np.where(x < 1.9, -1400.0, 3.0), 0.0, 2.0, 20)
    assert shift == 3.0 - 700.0 and area == pytest.approx(np.exp(700.0) * (2.0 / 19) * 0.5)
    area, shift = pq.log_area_twin(lambda x: np.where(x < 1.9, -1400.0, 3.0), 0.0, 2.0, 5, shift=0.0)
    assert area == pytest.approx(np.exp(3.0) * 0.5 * 0.5)
