"""The per-variable query API of ``EPBP`` and ``HybridLBP`` (``map``, ``probability``, ``belief``, ``belief_rv_batch``) and the cached
domain normaliser of the batched calls, on two fixed small relational instances after real sweeps.

The per-variable assertions are those of tests/soak/soak_queries_random.py, with its tolerances, made for EVERY hidden variable: the
batched answer (``exact_queries = False``) against the per-call form of the reference (``True``: scipy's fminbound, the host 20-point
``log_area``).  Three solvers: ``EPBP``, ``HybridLBP`` on the stable partition (rows are clusters) and ``HybridLBP`` coarse to fine
(``c2f=0``: the partition is not stable, the batched answers come from the GROUND arrays)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, SWEEPS = 10, 2
INSTANCES = ('rgm', 'paper_popularity')
SOLVERS = ('epbp', 'hlbp', 'hlbp_c2f')
_cache = {}


@pytest.fixture(scope='module')
def api():
    from lhvi import _abi
    _abi.require_gpu()
    return _abi


def instance(name):
    """(graph, hidden variables in sorted order): ``rgm(4, 2)`` with three observed atoms, ``paper_popularity(3, 2, points=8)`` with
    a third of its atoms observed; which atoms and which values from a fixed seed, values as the soak draws them"""
    from lhvi import generators
    rng = np.random.default_rng(11)
    rel = generators.rgm(4, 2) if name == 'rgm' else generators.paper_popularity(3, 2, points=8)
    rel.ground_graph()
    keys = sorted(rel.rvs_dict)
    picked = [keys[i] for i in rng.choice(len(keys), 3 if name == 'rgm' else len(keys) // 3, replace=False)]
    if name == 'rgm':
        data = {k: float(np.round(rng.uniform(-30, 30), 2)) for k in picked}
    else:
        data = {k: int(rng.integers(0, 2)) if k[0] in ('SameSession', 'PaperIn') else float(np.round(rng.uniform(0, 10), 2)) for k in picked}
    g, _ = rel.add_evidence(data)
    return g, sorted(rv for rv in g.rvs if rv.value is None)


def solve(name, solver):
    from lhvi.pbp import EPBP, HybridLBP
    g, hidden = instance(name)
    if solver == 'epbp':
        bp = EPBP(g, n=N, proposal_approximation='simple', sampler='device', seed=5)
        bp.run(SWEEPS)
    else:
        bp = HybridLBP(g, n=N, proposal_approximation='simple', sampler='device', seed=5)
        bp.run(SWEEPS, **({'c2f': 0} if solver == 'hlbp_c2f' else {}))
    return bp, hidden


def solved(name, solver):
    """one run per (instance, solver), shared by the tests that only query it"""
    if (name, solver) not in _cache:
        _cache[name, solver] = solve(name, solver)
    return _cache[name, solver]


def log_belief(bp, rv, x):
    return float(bp._belief_rv_points(bp._var_of(rv), [x])[0])


@pytest.mark.parametrize('solver', SOLVERS)
@pytest.mark.parametrize('name', INSTANCES)
def test_batched_answers_are_the_per_call_answers(api, name, solver):
    from lhvi.pbp import HybridLBP
    bp, hidden = solved(name, solver)
    rng = np.random.default_rng(3)
    assert hidden and any(rv.domain.continuous for rv in hidden)
    try:
        for rv in hidden:
            bp.exact_queries, bp.map_mode = False, 'fminbound'
            m_d = bp.map(rv)                        # the default: every row's fminbound iteration in one launch
            bp.map_mode = 'global'
            m_b = bp.map(rv)                        # the scan form
            bp.map_mode = 'fminbound'
            bp.exact_queries = True
            m_e = bp.map(rv)                        # scipy's fminbound, a launch per evaluation
            if not rv.domain.continuous:
                assert m_b == m_e and m_d == m_e, 'discrete map %r %r %r' % (m_d, m_b, m_e)
                assert type(m_d) is type(m_e) is type(rv.domain.values[0])
                continue
            assert type(m_d) is float
            assert abs(m_d - m_e) <= 2e-6 * max(1.0, abs(m_e)), 'batched fminbound left the per-call iterates: %r %r' % (m_d, m_e)
            gap = log_belief(bp, rv, m_e) - log_belief(bp, rv, m_b)
            if gap > 1e-9 * max(1.0, abs(log_belief(bp, rv, m_e))):
                assert gap < 0.02, 'scan map well below fminbound: %r %r' % (m_b, m_e)      # a near-tie of two modes at the most
            lo, hi = rv.domain.values
            a, b = sorted(rng.uniform(lo, hi, 2).tolist())
            got, want = {}, {}
            for exact, out in ((False, got), (True, want)):
                bp.exact_queries = exact
                out['p'] = bp.probability(a, b, rv)
                if isinstance(bp, HybridLBP):
                    bp.query_cache = dict()         # (belief keeps its normaliser per cluster: each form computes its own)
                    out['belief'] = bp.belief(0.5 * (a + b), rv)
            for k in got:
                np.testing.assert_allclose(got[k], want[k], rtol=1e-9, atol=1e-300, err_msg=k)
        # the batched passes were made, and made over the rows this solver can batch over
        keys = ('ground_map', 'ground_map_global', 'ground_area') if solver == 'hlbp_c2f' else ('map', 'map_global', 'area')
        assert all(k in bp._batched for k in keys), sorted(bp._batched)
    finally:
        bp.exact_queries, bp.map_mode = False, 'fminbound'


@pytest.mark.parametrize('solver', SOLVERS)
@pytest.mark.parametrize('name', INSTANCES)
def test_belief_rv_batch_rows_are_the_per_variable_rows(api, name, solver):
    bp, hidden = solved(name, solver)
    rng = np.random.default_rng(4)
    cont = [rv for rv in hidden if rv.domain.continuous]
    xs = np.stack([rng.uniform(rv.domain.values[0], rv.domain.values[1], 7) for rv in cont])
    got = bp.belief_rv_batch(cont, xs)
    assert got.shape == xs.shape and np.isfinite(got).all()
    for i, rv in enumerate(cont):
        np.testing.assert_array_equal(got[i], bp._belief_rv_points(bp._var_of(rv), xs[i]))       # bit for bit
    disc = [rv for rv in hidden if not rv.domain.continuous]
    if disc:                                                                                      # rows of states
        states = np.array([list(rv.domain.values) for rv in disc], dtype=np.float64)
        got = bp.belief_rv_batch(disc, states)
        for i, rv in enumerate(disc):
            np.testing.assert_array_equal(got[i], bp._belief_rv_points(bp._var_of(rv), states[i]))


@pytest.mark.parametrize('solver', ('epbp', 'hlbp'))
@pytest.mark.parametrize('name', INSTANCES)
def test_a_new_sample_drops_the_domain_normaliser(api, name, solver):
    """``probability_all`` divides by the 20-point ``log_area_all`` over the domain.  Whatever of it is kept between calls belongs to
    one sample: after a sweep the answer is the one built from a normaliser computed after that sweep, bit for bit"""
    bp, _ = solve(name, solver)
    flat = bp.flat
    cont = flat.var_hidden & flat.var_cont
    lo = np.array([flat.dom_lo[flat.var_dom[v]] if flat.var_cont[v] else 0.0 for v in range(flat.V)])
    hi = np.array([flat.dom_hi[flat.var_dom[v]] if flat.var_cont[v] else 1.0 for v in range(flat.V)])
    a, b = lo + 0.25 * (hi - lo), lo + 0.6 * (hi - lo)
    before = bp.probability_all(a, b).cpu().numpy()
    bp.belief_all(np.tile((0.5 * (a + b))[:, None], (1, 3)))
    bp.sweep()
    got = bp.probability_all(a, b).cpu().numpy()
    z, shift = bp.log_area_all(lo, hi, 20)
    want = (bp.log_area_all(a, b, 5, shift)[0] / z).cpu().numpy()
    assert cont.any() and np.isfinite(got[cont]).all() and np.isnan(got[~cont]).all()
    np.testing.assert_array_equal(got, want)
    assert (got[cont] != before[cont]).any()             # (the sweep did change the beliefs)
    # a last sweep draws no sample but renews the v -> f messages the queries read: the same holds after it
    bp.sweep(last=True)
    after_last = bp.probability_all(a, b).cpu().numpy()
    z, shift = bp.log_area_all(lo, hi, 20)
    np.testing.assert_array_equal(after_last, (bp.log_area_all(a, b, 5, shift)[0] / z).cpu().numpy())
    assert (after_last[cont] != got[cont]).any()
