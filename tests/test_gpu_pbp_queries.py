"""The particle-BP query kernels of csrc/pbp.hip row for row on the hand-built states of tests/pbp_query_models.py:
``lhvi_pbp_belief_points`` / ``lhvi_pbp_edge_points`` against the C oracle, ``lhvi_pbp_map_brent`` against SciPy's ``fminbound``
on the oracle's belief (and, bit for bit, on the device's own), ``lhvi_pbp_quad`` against an erf closed form and a NumPy dqage,
the explicit (edge, multiplicity) rows of both, the grid kernels against NumPy twins bit for bit, and the scan queries
(``log_area_all``, ``probability_all``, ``belief_all``) against the trapezoid twin.

Bounds: RTOL / ATOL = 1e-9 / 1e-8 for a log-belief (tests/test_gpu_pbp.py); 2e-6 max(1, |x|) for a minimiser that took the same
number of evaluations, which at least 99 % of a launch's rows must (tests/test_pbp_queries_host.py measures how often SciPy itself
changes its count under a rounding-level change of the objective, and caps that at half this share); the kernel's own ``abserr``
plus the twin's for a normaliser; 1e-7 relative for the trapezoids; everything else is an equality.

Row counts are chosen around the block of 256 threads, and ``row_var`` is drawn with repeats, in no order."""
import numpy as np
import pytest

import pbp_query_models as pq

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-9, 1e-8
X_RTOL = 2e-6
NFEV_SHARE = 0.99
ROW_COUNTS = (257, 256, 255, 1)


@pytest.fixture(scope='module')
def api():
    from lhvi import _abi
    _abi.require_gpu()
    return _abi


# ---- states, solvers and launches ---------------------------------------------------------------------------------------------------
_BUILD = {
    'mixture1': lambda: pq.mixture(1, 250, 101), 'mixture2': lambda: pq.mixture(2, 250, 102), 'mixture5': lambda: pq.mixture(5, 250, 105),
    'mixture16': lambda: pq.mixture(16, 250, 116), 'mixture64': lambda: pq.mixture(64, 250, 164),
    'end': lambda: pq.end(5, 40, 1), 'flat': lambda: pq.flat_family(5, 40, 2), 'narrow': lambda: pq.narrow(5, 40, 3),
    'discrete': lambda: pq.discrete(4), 'observed': lambda: pq.observed(5), 'lifted': lambda: pq.lifted(6),
    'overflow': lambda: pq.overflow(7),
}
FAMILIES = list(_BUILD)
MIXTURES = [f for f in FAMILIES if f.startswith('mixture')]
_cache = {}


def make_solver(api, st):
    """a solver on the state's graph with the state's particles and v -> f messages copied over its own; no sweep is run"""
    from lhvi.pbp import EPBP, HybridLBP
    if st.epbp:
        bp = EPBP(None, n=st.n, proposal_approximation='simple', sampler='device', seed=1)
    else:
        bp = HybridLBP.on_flat(st.flat, n=st.n, proposal_approximation='simple', sampler='device', seed=1)
    bp._setup(None, flat=st.flat)
    api.check(api.lib().lhvi_pbp_init(bp.dg.g, bp._struct(), api.ptr(bp.eta), api.ptr(bp.q_dev), api.ptr(bp.f2v), api.ptr(bp.v2f),
                                      api.stream_ptr()))
    assert tuple(bp.particles.shape) == st.particles.shape and tuple(bp.v2f.shape) == st.v2f.shape
    assert (bp.np_host == st.counts).all()
    bp.particles.copy_(api.to_dev(st.particles))
    bp.old_particles.copy_(api.to_dev(st.particles))
    bp.v2f.copy_(api.to_dev(st.v2f))
    bp._stable_partition = True
    return bp


def family(api, name):
    if name not in _cache:
        st = _BUILD[name]()
        _cache[name] = (st, make_solver(api, st))
    return _cache[name]


def draw_rows(st, count, seed, among=None):
    """`count` rows from the family's variables in no order: as many different ones as there are, then repeats (with fewer
    variables than rows most are repeats).  A variable whose evaluation count differs from SciPy's weighs on the 99 % of a launch
    once per row it fills, so the large families have nearly as many variables as a launch has rows."""
    rng = np.random.default_rng(seed)
    pool = rng.permutation(st.rows if among is None else np.asarray(among))
    rows = np.concatenate([pool[:count], rng.choice(pool, size=max(count - pool.size, 0))])
    return rng.permutation(rows).astype(np.int32)


def dev_belief(api, bp, qvar, x):
    import torch
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(len(qvar), -1)
    xt, qt = api.to_dev(x), api.to_dev(np.asarray(qvar, dtype=np.int32))
    out = torch.full_like(xt, np.nan)
    api.check(api.lib().lhvi_pbp_belief_points(bp.dg.g, bp.dg.p, bp._struct(), api.ptr(bp.v2f), len(qvar), api.ptr(qt),
                                               int(x.shape[1]), api.ptr(xt), api.ptr(out), api.stream_ptr()))
    return out.cpu().numpy()


def dev_edges(api, bp, qedge, x):
    import torch
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(len(qedge), -1)
    xt, qt = api.to_dev(x), api.to_dev(np.asarray(qedge, dtype=np.int32))
    out = torch.full_like(xt, np.nan)
    api.check(api.lib().lhvi_pbp_edge_points(bp.dg.g, bp.dg.p, bp._struct(), api.ptr(bp.v2f), len(qedge), api.ptr(qt),
                                             int(x.shape[1]), api.ptr(xt), api.ptr(out), api.stream_ptr()))
    return out.cpu().numpy()


def _pairs(api, pairs):
    if pairs is None:
        return None, None, None
    ptr, edge, mult = pairs
    edge = np.asarray(edge, dtype=np.int32)
    mult = np.asarray(mult, dtype=np.float64)
    # (an empty list still needs a pointer: one unused entry)
    return (api.to_dev(np.asarray(ptr, dtype=np.int64)), api.to_dev(edge if edge.size else np.zeros(1, dtype=np.int32)),
            api.to_dev(mult if mult.size else np.zeros(1)))


def dev_brent(api, bp, row_var, pairs=None, xtol=1e-5, maxfun=500, want_f=True, want_nfev=True):
    import torch
    rv = api.to_dev(np.asarray(row_var, dtype=np.int32))
    nq = int(rv.numel())
    x = torch.full((nq,), np.nan, dtype=torch.float64, device=rv.device)
    f = torch.full_like(x, np.nan)
    k = torch.full((nq,), -1, dtype=torch.int32, device=rv.device)
    qptr, qedge, qmult = _pairs(api, pairs)
    api.check(api.lib().lhvi_pbp_map_brent(bp.dg.g, bp.dg.p, bp._struct(), api.ptr(bp.v2f), nq, api.ptr(rv), api.ptr(qptr),
                                           api.ptr(qedge), api.ptr(qmult), float(xtol), int(maxfun), api.ptr(x),
                                           api.ptr(f if want_f else None), api.ptr(k if want_nfev else None), api.stream_ptr()))
    return x.cpu().numpy(), f.cpu().numpy(), k.cpu().numpy()


def dev_quad(api, bp, row_var, lo, hi, pairs=None, epsabs=1.49e-8, epsrel=1.49e-8):
    import torch
    rv = api.to_dev(np.asarray(row_var, dtype=np.int32))
    nq = int(rv.numel())
    assert len(lo) == nq and len(hi) == nq
    z = torch.full((nq,), -1.0, dtype=torch.float64, device=rv.device)
    err = torch.full_like(z, -1.0)
    status = torch.full((nq,), -1, dtype=torch.int32, device=rv.device)
    qptr, qedge, qmult = _pairs(api, pairs)
    lot, hit = api.to_dev(np.asarray(lo, dtype=np.float64)), api.to_dev(np.asarray(hi, dtype=np.float64))
    api.check(api.lib().lhvi_pbp_quad(bp.dg.g, bp.dg.p, bp._struct(), api.ptr(bp.v2f), nq, api.ptr(rv), api.ptr(qptr), api.ptr(qedge),
                                      api.ptr(qmult), api.ptr(lot), api.ptr(hit), float(epsabs), float(epsrel),
                                      api.ptr(z), api.ptr(err), api.ptr(status), api.stream_ptr()))
    return z.cpu().numpy(), err.cpu().numpy(), status.cpu().numpy()


def per_variable(st, key, rows, fn):
    """``fn(variables)`` -> tuple of arrays, evaluated once per distinct variable of the state and handed out per row"""
    store = _cache.setdefault(('ref', id(st), key), {})
    need = [int(v) for v in np.unique(rows) if int(v) not in store]
    if need:
        for v, vals in zip(need, zip(*fn(np.array(need)))):
            store[v] = vals
    return tuple(np.array(col) for col in zip(*(store[int(v)] for v in rows)))


def widened(st, rows):
    lo, hi = np.array([st.domain(v) for v in rows]).T
    return lo - pq.MARGIN, hi + pq.MARGIN


# ---- beliefs at given points ---------------------------------------------------------------------------------------------------------
def assert_close(got, want, allow, label):
    """RTOL / ATOL, widened by `allow` (``State.allowance``: 0 unless a message's term sum is subnormal); what fails is printed"""
    allow = np.asarray(allow).reshape(np.shape(got))
    bad = np.abs(got - want) > ATOL + RTOL * np.abs(want) + allow
    for i in np.argwhere(bad)[:12]:
        print('%s: at %s device %.17g, oracle %.17g, allowance %.3g' % (label, tuple(i), got[tuple(i)], want[tuple(i)], allow[tuple(i)]))
    assert not bad.any(), '%s: %d of %d values differ' % (label, int(bad.sum()), bad.size)


def _query_points(st, rows, npts, seed):
    rng = np.random.default_rng(seed)
    x = np.zeros((len(rows), npts))
    for r, v in enumerate(rows):
        if st.flat.var_cont[v]:
            lo, hi = st.domain(v)
            x[r] = rng.uniform(lo, hi, npts)
            x[r, 0], x[r, -1] = lo, hi
        else:
            x[r] = rng.choice(st.states(v), npts)
    return x


@pytest.mark.parametrize('name', FAMILIES)
def test_belief_points_and_edge_points(api, name):
    st, bp = family(api, name)
    worst = 0.0
    for count in ROW_COUNTS:
        rows = draw_rows(st, count, 10 + count)
        x = _query_points(st, rows, 5, count)
        got, want = dev_belief(api, bp, rows, x), st.oracle.belief_points(rows, x)
        allow = np.array([st.belief_allowance(v, t) for v, t in zip(rows, x)])
        worst = max(worst, float(np.abs(got - want)[allow == 0].max()))
        assert_close(got, want, allow, '%s / %d rows' % (name, count))
        if name == 'flat':
            assert (got == (pq.FLOOR * np.diff(st.flat.var_ptr)[rows])[:, None]).all()
    # every edge into one of the family's variables
    fl = st.flat
    edges = np.concatenate([fl.var_edge[fl.var_ptr[v]:fl.var_ptr[v + 1]] for v in st.rows])
    edges = np.random.default_rng(3).permutation(np.concatenate([edges, edges[:7]]))[:257]
    x = _query_points(st, fl.edge_var[edges], 3, 9)
    got, want = dev_edges(api, bp, edges, x), st.oracle.edge_points(edges, x)
    allow = np.array([st.allowance([e], [1.0], t) for e, t in zip(edges, x)])
    assert_close(got, want, allow, '%s / messages' % name)
    print('%s: worst |belief - oracle| = %.3g, worst |message - oracle| = %.3g (off the subnormal range; %d of %d points in it)'
          % (name, worst, float(np.abs(got - want)[allow == 0].max()), int((allow > 0).sum()), allow.size))


def test_flat_belief_on_a_lifted_graph_is_the_counted_floor_sum(api):
    """every message at the floor on the hub graph without unary factors: exactly -700 times the sum of the row's edge counts"""
    st = pq.lifted(6, unary=False)
    st = pq.State(st.flat, st.n, st.particles, np.full_like(st.v2f, -800.0), st.rows, epbp=False)
    bp = make_solver(api, st)
    fl = st.flat
    counts = np.array([fl.edge_count[fl.var_edge[fl.var_ptr[v]:fl.var_ptr[v + 1]]].sum() for v in st.rows])
    assert counts.max() >= 4 and counts.min() == 1
    rows = draw_rows(st, 33, 1)
    got = dev_belief(api, bp, rows, _query_points(st, rows, 4, 2))
    assert (got == (pq.FLOOR * counts[rows])[:, None]).all()
    x, f, k = dev_brent(api, bp, rows)
    assert (f == pq.FLOOR * counts[rows]).all()


# ---- Brent ---------------------------------------------------------------------------------------------------------------------------
def check_brent(st, rows, got, ref, label, log_belief_at=None, allow=None, edge_allow=None, exact=False):
    """the criteria of the module's head for one launch; `exact`: no cap, every row takes SciPy's count.  A row whose SciPy
    minimiser lies where a message's sum of terms is subnormal (``State.allowance`` is not 0 there: the search ended on the edge
    of the plateau that the floor -700 makes of an underflowing message, and where that edge is depends on the last bits of the
    evaluation) is counted with the rows whose counts differ, whatever its count"""
    x, f, k = got
    xr, fr, kr, _ = ref
    cont = st.flat.var_cont[rows]
    on_edge = (np.array([st.belief_allowance(v, [t])[0] for v, t in zip(rows, xr)]) if edge_allow is None else edge_allow) > 0
    same = (k == kr) & ~on_edge
    at = log_belief_at if log_belief_at is not None else np.array([st.log_belief(v, [t])[0] for v, t in zip(rows, x)])
    allow = allow if allow is not None else np.array([st.belief_allowance(v, [t])[0] for v, t in zip(rows, x)])
    assert_close(f, at, allow, label)
    for r in np.flatnonzero(~same)[:20]:
        print('%s: row %d (variable %d): nfev %d, SciPy %d; x %.17g, SciPy %.17g%s'
              % (label, r, rows[r], k[r], kr[r], x[r], xr[r], ' (on the edge of a floor plateau)' if on_edge[r] else ''))
    gap = np.abs(x - xr) / np.maximum(1.0, np.abs(xr))
    print('%s: %d rows, nfev differs (or the minimiser is on a floor edge) on %d (%.2f %%), worst |dx| / max(1, |x|) on the others = %.3g'
          % (label, len(rows), int((~same).sum()), 100.0 * (~same).mean(), float(gap[same].max()) if same.any() else 0.0))
    for r in np.flatnonzero(same & (gap > X_RTOL))[:20]:
        print('%s: row %d (variable %d): nfev %d on both sides, but x %.17g, SciPy %.17g; f %.17g, SciPy %.17g'
              % (label, r, rows[r], k[r], x[r], xr[r], f[r], fr[r]))
    assert same.all() if exact else same.mean() >= NFEV_SHARE
    assert (gap[same] <= X_RTOL).all()
    assert (x[~cont] == xr[~cont]).all()
    return same


@pytest.mark.parametrize('name', FAMILIES)
def test_brent_against_scipy_on_the_oracle(api, name):
    st, bp = family(api, name)
    exact = name in ('narrow', 'flat', 'end', 'discrete')
    for count in ROW_COUNTS[:2] if name in ('mixture64', 'lifted') else ROW_COUNTS:
        rows = draw_rows(st, count, 20 + count)
        ref = per_variable(st, 'brent', rows, lambda vs: pq.brent_state(st, vs))
        got = dev_brent(api, bp, rows)
        check_brent(st, rows, got, ref, '%s / %d rows' % (name, count), exact=exact)
        x, f, k = got
        lo, hi = np.array([st.domain(v) for v in rows]).T
        if name == 'narrow':
            assert (k == 1).all() and (x == lo + pq.GOLDEN_MEAN * (hi - lo)).all()
        if name == 'flat':
            assert (x == ref[0]).all()
        if name == 'end':
            edge = np.where(st.info['side'][np.searchsorted(st.rows, rows)] > 0, hi, lo)
            assert (np.abs(ref[0] - edge) < 1e-4).all() and (np.abs(x - edge) < 1e-4).all()
        if name == 'discrete':
            assert (k == [st.states(v).size for v in rows]).all()
            for r, v in enumerate(rows):
                pair = st.info['tie'][int(np.searchsorted(st.rows, v))]
                if pair is not None:
                    assert x[r] == float(pair[0])


@pytest.mark.parametrize('maxfun', [1, 2, 5])
def test_brent_evaluation_limit(api, maxfun):
    """SciPy counts an evaluation before it looks at the limit, so ``maxfun = 1`` ends with two evaluations wherever the loop is
    entered at all; otherwise a row at the limit has made exactly ``maxfun``"""
    for name in ('mixture5', 'end', 'narrow'):
        st, bp = family(api, name)
        rows = draw_rows(st, 257, 30 + maxfun)
        ref = per_variable(st, ('brent', maxfun), rows, lambda vs: pq.brent_state(st, vs, maxfun=maxfun))
        got = dev_brent(api, bp, rows, maxfun=maxfun)
        flag = ref[3]
        assert flag.all() == (name != 'narrow') and (got[2][flag] == ref[2][flag]).all() and (ref[2][flag] == max(maxfun, 2)).all()
        check_brent(st, rows, got, ref, '%s / maxfun %d' % (name, maxfun), exact=name != 'mixture5')


def test_brent_optional_outputs(api):
    st, bp = family(api, 'mixture16')
    rows = draw_rows(st, 257, 40)
    x, f, k = dev_brent(api, bp, rows)
    x1, f1, k1 = dev_brent(api, bp, rows, want_f=False)
    x2, f2, k2 = dev_brent(api, bp, rows, want_nfev=False)
    assert x.tobytes() == x1.tobytes() == x2.tobytes() and np.isnan(f1).all() and (k2 == -1).all()
    assert (k1 == k).all() and f2.tobytes() == f.tobytes()


def test_brent_on_the_device_function_bit_for_bit(api):
    """``fminbound`` with ``lhvi_pbp_belief_points`` as its objective, a launch per evaluation (what ``exact_queries = True``
    does), against the one launch of ``lhvi_pbp_map_brent``: the same function and IEEE double on both sides, so the same
    evaluation count and the same minimiser, bit for bit"""
    st, bp = family(api, 'mixture16')
    rows = st.rows[:32]
    lo, hi = np.array([st.domain(v) for v in rows]).T
    xr, fr, kr, _ = pq.brent_rows(lambda r, t: dev_belief(api, bp, rows[r:r + 1], [[t]])[0, 0], lo, hi)
    x, f, k = dev_brent(api, bp, rows)
    differ = np.flatnonzero((k != kr) | (x != xr))
    for r in differ:
        print('row %d: nfev %d / %d, x %.17g / %.17g, f %.17g / %.17g' % (r, k[r], kr[r], x[r], xr[r], f[r], fr[r]))
    print('device function: %d of 32 rows bit for bit' % (32 - differ.size))
    assert differ.size == 0
    assert f.tobytes() == fr.tobytes()


# ---- explicit (edge, multiplicity) rows ----------------------------------------------------------------------------------------------
def own_edges(st, rows):
    fl = st.flat
    lists = [fl.var_edge[fl.var_ptr[v]:fl.var_ptr[v + 1]] for v in rows]
    ptr = np.concatenate([[0], np.cumsum([len(e) for e in lists])])
    return ptr, np.concatenate(lists), np.ones(int(ptr[-1]))


@pytest.mark.parametrize('name', ['mixture16', 'discrete', 'observed'])
def test_explicit_rows_of_a_variables_own_edges_give_the_bits_of_the_variable_path(api, name):
    """multiplicity 1.0 on the variable's edges in ``var_edge`` order: ``lhvi_pbp_map_brent`` and ``lhvi_pbp_quad`` (whose explicit
    rows no caller in the package uses) return what the ``row_var`` path returns"""
    st, bp = family(api, name)
    rows = draw_rows(st, 257, 50)
    pairs = own_edges(st, rows)
    a, b = dev_brent(api, bp, rows), dev_brent(api, bp, rows, pairs=pairs)
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()
    rows = rows[st.flat.var_cont[rows]]
    if rows.size:
        lo, hi = widened(st, rows)
        a, b = dev_quad(api, bp, rows, lo, hi), dev_quad(api, bp, rows, lo, hi, pairs=own_edges(st, rows))
        assert (a[2] == 0).all()
        for u, v in zip(a, b):
            assert u.tobytes() == v.tobytes()


def check_quad(got, twin, label, exact=None):
    z, err, status = got
    zt, et, stt = twin
    assert (status == stt).all(), (label, np.flatnonzero(status != stt))
    ok = status != 3
    gap = np.abs(z - zt)[ok]
    tight = int((gap <= 1e-12 * np.abs(zt[ok])).sum())
    print('%s: %d rows, %d agree with the twin to 1e-12 relative (the same bisections); worst |z - twin| / twin = %.3g'
          % (label, int(ok.sum()), tight, float((gap / np.maximum(np.abs(zt[ok]), 1e-300)).max()) if ok.any() else 0.0))
    assert (gap <= err[ok] + et[ok] + 1e-9 * np.abs(zt[ok])).all()
    assert np.isnan(z[~ok]).all()
    if exact is not None:
        have = np.isfinite(exact) & ok
        assert (np.abs(z - exact)[have] <= err[have] + 1e-12 * np.abs(exact[have])).all()
        print('%s: %d rows with a closed form, worst |z - exact| / exact = %.3g'
              % (label, int(have.sum()), float((np.abs(z - exact)[have] / exact[have]).max()) if have.any() else 0.0))


def test_explicit_rows_with_multiplicities(api):
    """multiplicities 2, 3, 0.5 and 0, an edge listed twice, and an empty row (belief 0 everywhere: the normaliser is the interval
    width, Brent runs on a constant), against ``fminbound`` / the NumPy dqage on ``sum mult * edge_points``"""
    st, bp = family(api, 'mixture16')
    rng = np.random.default_rng(60)
    fl = st.flat
    rows = draw_rows(st, 255, 61, among=st.rows[:120])
    lists, mults = [], []
    for r, v in enumerate(rows):
        e = fl.var_edge[fl.var_ptr[v]:fl.var_ptr[v + 1]].tolist()
        if r % 8 == 7:
            e = []
        elif r % 8 == 3:
            e = e + e[:1]
        lists.append(e)
        mults.append(rng.choice([2.0, 3.0, 0.5, 0.0, 1.0], len(e)).tolist())
    ptr = np.concatenate([[0], np.cumsum([len(e) for e in lists])])
    pairs = (ptr, np.array(sum(lists, []), dtype=np.int32), np.array(sum(mults, [])))
    assert {2.0, 3.0, 0.5, 0.0} <= set(pairs[2].tolist())
    fun = lambda r, t: st.log_belief_pairs(lists[r], mults[r], t)
    lo, hi = np.array([st.domain(v) for v in rows]).T
    ref = pq.brent_rows(lambda r, t: fun(r, [t])[0], lo, hi)
    got = dev_brent(api, bp, rows, pairs=pairs)
    at = np.array([fun(r, [t])[0] for r, t in enumerate(got[0])])
    allow = np.array([st.allowance(lists[r], mults[r], [t])[0] for r, t in enumerate(got[0])])
    edge = np.array([st.allowance(lists[r], mults[r], [t])[0] for r, t in enumerate(ref[0])])
    check_brent(st, rows, got, ref, 'explicit rows', log_belief_at=at, allow=allow, edge_allow=edge)
    empty = np.array([len(e) == 0 for e in lists])
    assert (got[0][empty] == ref[0][empty]).all() and (got[2][empty] == ref[2][empty]).all() and (got[1][empty] == 0.0).all()
    # (a multiplicity of 3 on three large messages can push e ** belief out of range: status 3 on both sides then)
    z, err, status = dev_quad(api, bp, rows, lo - pq.MARGIN, hi + pq.MARGIN, pairs=pairs)
    check_quad((z, err, status), pq.dqage_rows(fun, lo - pq.MARGIN, hi + pq.MARGIN), 'explicit rows')
    assert (status[empty] == 0).all() and (np.abs(z[empty] - (hi - lo + 2 * pq.MARGIN)[empty]) <= err[empty]).all()


# ---- the normaliser ------------------------------------------------------------------------------------------------------------------
def _closed_forms(st, rows):
    return per_variable(st, 'exact', rows, lambda vs: ([pq.z_closed_form(st, v) if pq.has_closed_form(st, v) else np.nan for v in vs],))[0]


@pytest.mark.parametrize('name', MIXTURES + ['lifted', 'observed'])
def test_quad_against_the_closed_form_and_the_twin(api, name):
    st, bp = family(api, name)
    pool = st.info['cont'] if name == 'observed' else st.rows[:96]          # (the NumPy dqage takes 10 - 30 ms per row)
    for count in ROW_COUNTS[:2] if name in ('mixture64', 'lifted') else ROW_COUNTS:
        rows = draw_rows(st, count, 70 + count, among=pool)
        lo, hi = widened(st, rows)
        got = dev_quad(api, bp, rows, lo, hi)
        assert (got[2] == 0).all(), np.flatnonzero(got[2])
        twin = per_variable(st, 'dqage', rows, lambda vs: pq.dqage_state(st, vs))
        check_quad(got, twin, '%s / %d rows' % (name, count), exact=_closed_forms(st, rows) if name in MIXTURES else None)


def test_quad_first_rule_does_not_trust_an_estimate_at_its_ceiling(api):
    """mixture16's variable of row 184 of a 200-row build: three narrow factors whose product one node of the first rule sees and
    no other.  The estimate of that rule equals dqk21's ``resasc`` -- its ceiling -- and is below ``epsabs``; QUADPACK (and SciPy's
    ``quad``: 14620.25) bisects then.  A kernel that accepts the first rule returns 3.7e-10."""
    from scipy.integrate import quad
    st = pq.mixture(16, 200, 116)
    bp = make_solver(api, st)
    rows = st.rows[[184, 56, 0]]
    lo, hi = widened(st, rows)
    z, err, status = dev_quad(api, bp, rows, lo, hi)
    for r, v in enumerate(rows):
        want = quad(lambda t: float(np.exp(st.log_belief(v, [t])[0])), lo[r], hi[r])[0]
        assert status[r] == 0 and z[r] == pytest.approx(want, rel=1e-6)
    assert z[0] > 1e4


def test_quad_interval_limit(api):
    """``epsabs = 0, epsrel = 1e-14`` is out of reach for most rows: status 1 where the twin reaches the 50 intervals too, and the
    value is still within the reported estimate of the closed form"""
    st, bp = family(api, 'mixture5')
    rows = draw_rows(st, 64, 80)
    lo, hi = widened(st, rows)
    got = dev_quad(api, bp, rows, lo, hi, epsabs=0.0, epsrel=1e-14)
    twin = per_variable(st, 'dqage tight', rows, lambda vs: pq.dqage_state(st, vs, epsabs=0.0, epsrel=1e-14))
    assert (twin[2] == 1).sum() >= 16
    check_quad(got, twin, 'interval limit', exact=_closed_forms(st, rows))


def test_quad_overflow(api):
    """rows whose ``e ** belief`` is inf: status 3 and NaN, ``EPBP.belief`` raises like the reference, and the other rows of the
    launch are what a launch without the overflow rows returns"""
    st, bp = family(api, 'overflow')
    hot = st.info['hot']
    rows = np.concatenate([st.rows, st.rows[::-1]]).astype(np.int32)
    mask = np.concatenate([hot, hot[::-1]])
    lo, hi = widened(st, rows)
    z, err, status = dev_quad(api, bp, rows, lo, hi)
    assert (status[mask] == 3).all() and np.isnan(z[mask]).all() and (status[~mask] == 0).all()
    z1, err1, status1 = dev_quad(api, bp, rows[~mask], lo[~mask], hi[~mask])
    assert z1.tobytes() == z[~mask].tobytes() and err1.tobytes() == err[~mask].tobytes() and (status1 == 0).all()
    twin = per_variable(st, 'dqage', rows, lambda vs: pq.dqage_state(st, vs))
    check_quad((z, err, status), twin, 'overflow')

    class Variable:         # what EPBP.belief reads of a random variable
        value = None
        domain = st.flat.domains[0]
    hot_rv, cool_rv = Variable(), Variable()
    bp.flat.var_index.update({hot_rv: int(st.rows[hot][0]), cool_rv: int(st.rows[~hot][0])})
    bp.cache = {}
    with pytest.raises(OverflowError):
        bp.belief(0.0, hot_rv)
    want = np.exp(st.log_belief(st.rows[~hot][0], [0.5])[0]) / twin[0][~mask][0]
    assert bp.belief(0.5, cool_rv) == pytest.approx(want, rel=1e-6)


# ---- the grid kernels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 2, 3, 5, 64])
def test_grid_kernels_against_their_twins_bit_for_bit(api, n):
    import torch
    st = pq.grid_state(n)
    bp = make_solver(api, st)
    fl, l, s = st.flat, api.lib(), bp._struct()
    rng = np.random.default_rng(n)
    # domain grid: every entry is written, 0 beyond a row's count and for observed rows
    x = torch.full((fl.V, n), 7.25, dtype=torch.float64, device=bp.v2f.device)
    api.check(l.lhvi_pbp_domain_grid(bp.dg.g, s, api.ptr(x), api.stream_ptr()))
    want = pq.domain_grid_twin(fl, st.counts, n)
    assert x.cpu().numpy().tobytes() == want.tobytes()
    cont = np.flatnonzero(fl.var_hidden & fl.var_cont)
    assert (want[cont, n - 1] == fl.dom_hi[fl.var_dom[cont]]).all()
    # var sum on arbitrary tables
    S = n + bp.T
    f2v = rng.normal(0.0, 30.0, (fl.E, S))
    out = torch.full((fl.V, n), 7.25, dtype=torch.float64, device=bp.v2f.device)
    api.check(l.lhvi_pbp_var_sum(bp.dg.g, s, api.ptr(api.to_dev(f2v)), api.ptr(out), api.stream_ptr()))
    assert out.cpu().numpy().tobytes() == pq.var_sum_twin(fl, st.counts, n, f2v).tobytes()
    # refinement: random values, then the maximum in the first and in the last column, then ties (first and last, all equal)
    cases = [rng.normal(0.0, 5.0, (fl.V, n)) for _ in range(2)]
    first, last, tie, level = (rng.normal(0.0, 5.0, (fl.V, n)) for _ in range(4))
    first[:, 0], tie[:, 0] = 50.0, 50.0
    for v in range(fl.V):
        cnt = max(int(st.counts[v]), 1)
        last[v, cnt - 1] = tie[v, cnt - 1] = 50.0
    level[:] = 1.5
    grid = want.copy()
    grid[np.arange(n)[None, :] >= st.counts[:, None]] = -3.5          # marks what must stay
    for logb in cases + [first, last, tie, level]:
        for start in (grid, grid * 0.37 + 0.11):                 # the domain grid, and an uneven one
            xt = api.to_dev(start.copy())
            best = torch.full((fl.V,), np.nan, dtype=torch.float64, device=xt.device)
            val = torch.full_like(best, np.nan)
            api.check(l.lhvi_pbp_refine_grid(bp.dg.g, s, api.ptr(api.to_dev(logb)), api.ptr(xt), api.ptr(best), api.ptr(val), api.stream_ptr()))
            wx, wb, wv = pq.refine_grid_twin(fl, st.counts, logb, start)
            assert xt.cpu().numpy().tobytes() == wx.tobytes()
            assert best.cpu().numpy().tobytes() == wb.tobytes() and val.cpu().numpy().tobytes() == wv.tobytes()
    wx, wb, _ = pq.refine_grid_twin(fl, st.counts, tie, grid)
    assert (wb[cont] == grid[cont, 0]).all()                     # a tie between the first and the last column: the first


# ---- the scan queries ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 3, 7, 20, 64])
def test_scan_queries_against_the_trapezoid_twin(api, n):
    """``log_area_all(lo, hi, 20)`` (in passes of n points: 20 alone, 7 + 7 + 6, ...), ``probability_all`` and ``belief_all`` on
    the oracle's beliefs at 1e-7 relative, the bound of the ``probability`` checks of tests/test_gpu_pbp.py"""
    st = pq.area(n, 90 + n)
    bp = make_solver(api, st)
    fl = st.flat
    cont = fl.var_hidden & fl.var_cont
    lo = np.where(fl.var_cont, fl.dom_lo[fl.var_dom], 0.0)
    hi = np.where(fl.var_cont, fl.dom_hi[fl.var_dom], 1.0)
    z, shift = (t.cpu().numpy() for t in bp.log_area_all(lo, hi, 20))
    assert np.isnan(z[~cont]).all() and np.isnan(shift[~cont]).all() and np.isfinite(z[cont]).all()
    twin = {int(v): pq.log_area_twin(lambda x, v=v: st.log_belief(v, x), lo[v], hi[v], 20) for v in st.rows}
    for v in st.rows:
        zt, sht = twin[int(v)]
        assert shift[v] == pytest.approx(sht, rel=1e-7, abs=1e-7)
        assert z[v] * np.exp(shift[v] - sht) == pytest.approx(zt, rel=1e-7)
    for v in st.info['steep']:                       # the shift of these rows is max - 700
        y = st.log_belief(v, np.linspace(lo[v], hi[v], 20))
        assert y.max() - y.mean() > 700.0 and twin[int(v)][1] == y.max() - 700.0
    a, b = -2.0, 3.5
    prob = bp.probability_all(a, b).cpu().numpy()
    assert np.isnan(prob[~cont]).all()
    for v in st.rows:
        zt, sht = twin[int(v)]
        num, _ = pq.log_area_twin(lambda x, v=v: st.log_belief(v, x), a, b, 5, shift=sht)
        assert prob[v] == pytest.approx(num / zt, rel=1e-7, abs=1e-300)
    m = min(n, 3)
    rng = np.random.default_rng(n)
    x = rng.uniform(-9.0, 9.0, (fl.V, m))
    x[st.info['obs'], 0] = fl.var_value[st.info['obs']]
    got = bp.belief_all(x).cpu().numpy()
    for v in st.rows:
        zt, sht = twin[int(v)]
        want = np.exp(st.log_belief(v, x[v]) - sht - np.log(zt))
        np.testing.assert_allclose(got[v], want, rtol=1e-7, atol=1e-300)
    assert got[st.info['obs']].tolist() == [1.0] + [0.0] * (m - 1)
    d = st.info['disc']
    if d is not None and m >= 2:
        w = np.exp(st.log_belief(d, st.states(d)))
        np.testing.assert_allclose(got[d, :2], w / w.sum(), rtol=1e-7)
