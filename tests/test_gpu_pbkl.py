"""GPU tests of ``KL(p || belief)`` with the belief of a particle solver as the second operand (``lhvi_pbp_kl``,
``EPBP.kl_from`` / ``HybridLBP.kl_from``, docs/kernels_pbkl.md): closed forms, the NumPy restatement of tests/pbkl_models.py fed
by ``lhvi_pbp_belief_points`` on the same solver state, the shapes at which the kernel takes another path (the chunked ``p``
side, the panel counts, a bisection), rows and positions, the lifted solver, and the drivers' flow end to end.

Bounds.  Against a closed form: ``abserr + 2 * 1.49e-8 + 1e-12 max(1, |kl|)`` -- the normaliser ``z`` of ``quad_all`` enters as
``log z`` and carries its own relative tolerance.  Against the restatement: ``abserr_dev + abserr_twin + 1e-9 max(1, |kl|)``,
1e-9 being the project's stated tolerance of log messages (docs/parity.md): the two sides take ``belief_rv`` from two kernels."""
import numpy as np
import pytest

import pbkl_models as pm

pytestmark = pytest.mark.gpu
EPS = 1.49e-8


@pytest.fixture(scope='module')
def api():
    from lhvi import _abi
    _abi.require_gpu()
    return _abi


# ---- graphs ------------------------------------------------------------------------------------------------------------------------------
def graph_of(rvs, factors):
    from lhvi.graph import Graph
    g = Graph()
    g.rvs, g.factors = list(rvs), list(factors)
    g.init_nb()
    return g


def unary_graph(m, var):
    from lhvi.graph import F, RV, Domain
    from lhvi.potentials import GaussianPotential
    x = RV(Domain((-10, 10), continuous=True))
    return graph_of([x], [F(GaussianPotential([m], [[var]]), (x,))]), x


def observed_pair_graph(mu, sig, yobs):
    from lhvi.graph import F, RV, Domain
    from lhvi.potentials import GaussianPotential
    d = Domain((-10, 10), continuous=True)
    x, y = RV(d), RV(d, value=yobs)
    return graph_of([x, y], [F(GaussianPotential(mu, sig), (x, y))]), x


def hand_graph():
    """ten variables: x0 of degree 6, x1 and x2 of degree 2, x6 of degree 1; Gaussian pair factors, a hybrid factor with a
    hidden discrete partner (d0, x2), a table (d0, d1), a formula that is not conditionally quadratic (x3, x4), an observed
    neighbour (x5, xo) and a unary factor"""
    from lhvi.graph import F, RV, Domain
    from lhvi.mln import MLNPotential, eq_op
    from lhvi.potentials import GaussianPotential, HybridQuadraticPotential, TablePotential
    dc, dd = Domain((-10, 10), continuous=True), Domain((0, 1))
    x = [RV(dc) for _ in range(7)]
    xo, d0, d1 = RV(dc, value=2.0), RV(dd), RV(dd)
    pair = lambda m0, m1, c: GaussianPotential([m0, m1], [[2.0, c], [c, 1.5]])       # noqa: E731
    factors = [F(pair(0.0, 1.0, 0.8), (x[0], x[1])), F(pair(1.0, -1.0, -0.5), (x[0], x[2])), F(pair(-1.0, 0.0, 0.3), (x[0], x[3])),
               F(pair(0.5, 0.5, 1.0), (x[0], x[4])), F(pair(0.0, 2.0, -0.9), (x[0], x[5])), F(pair(2.0, -2.0, 0.4), (x[1], x[6])),
               F(HybridQuadraticPotential(A=-0.5 * np.array([[[1.0]], [[0.4]]]), b=np.array([[-1.5], [1.0]]), c=np.array([0.0, 0.3])),
                 (d0, x[2])),
               F(TablePotential(np.array([[0.7, 0.3], [0.2, 0.8]])), (d0, d1)),
               F(MLNPotential(lambda a: -eq_op(a[0], a[1]) * eq_op(a[0], a[1]), w=0.01), (x[3], x[4])),
               F(pair(1.0, 1.0, 0.6), (x[5], xo)), F(GaussianPotential([0.5], [[4.0]]), (x[0],))]
    return graph_of(x + [xo, d0, d1], factors), x


def epbp(g, n, sweeps=3, seed=5):
    from lhvi.pbp import EPBP
    bp = EPBP(g, n=n, proposal_approximation='simple', sampler='device', seed=seed)
    bp.run(sweeps)
    return bp


def mixtures(R, K, seed, centre=0.0, spread=3.0, vlo=0.25, vhi=4.0):
    rng = np.random.default_rng(seed)
    w, mu, var = (np.empty((R, K)) for _ in range(3))
    for r in range(R):
        w[r], mu[r], var[r] = pm.rand_gm(rng, K, spread, vlo, vhi)
    return w, mu + centre, var


# ---- the restatement on the solver's own state -------------------------------------------------------------------------------------------
def logz_of(bp):
    return bp._query_cache('kl_logz', bp._kl_logz)


def twin_rows(bp, rows, p, a=-np.inf, b=np.inf, logz=None, **kw):
    """tests/pbkl_models.py::kl_logq per row with log q(x) = belief_rv(x) from ``lhvi_pbp_belief_points`` (21 points a call) less
    the same log z; the stats of every row come back as a fifth entry"""
    from lhvi.pbp import _ParticleSweep
    logz = logz_of(bp) if logz is None else logz
    a, b = np.broadcast_to(a, (len(rows),)), np.broadcast_to(b, (len(rows),))
    out, stats = [], []
    for r, v in enumerate(rows):
        st = {}
        out.append(pm.kl_logq(tuple(t[r] for t in p), lambda x, v=v: _ParticleSweep._belief_rv_points(bp, int(v), x) - logz[v],
                              float(a[r]), float(b[r]), stats=st, **kw))
        stats.append(st)
    kl, err, st, ne = zip(*out)
    return np.array(kl), np.array(err), np.array(st, dtype=np.int32), np.array(ne, dtype=np.int32), stats


def check_against_twin(bp, rows, p, what, **kw):
    kl, info = bp.kl_from(p, rows=rows, info=True, **kw)
    tk, te, ts, tn, stats = twin_rows(bp, rows, p, **kw)
    gap = np.abs(kl - tk)
    print('%s: %d rows, worst |device - restatement| = %.3g (abserr %.3g + %.3g), neval equal on %d rows, neval <= %d, P %s, depth %s'
          % (what, len(rows), gap.max(), info['abserr'].max(), te.max(), int((info['neval'] == tn).sum()), info['neval'].max(),
             sorted({s['P'] for s in stats}), max(s['depth'] for s in stats)))
    np.testing.assert_array_equal(info['status'], ts)
    assert (gap <= info['abserr'] + te + 1e-9 * np.maximum(1.0, np.abs(tk))).all(), (kl, tk)
    return kl, info, stats


def closed_form_bound(kl, err, exact):
    return abs(kl - exact) <= err + 2 * EPS + 1e-12 * max(1.0, abs(kl))


# ---- G1 / G2: closed forms ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [8, 20, 64])
def test_unary_gaussian_factor_matches_the_closed_form(api, n):
    """belief_rv is the factor's log potential: q = N(1.5, 2.25) whatever the particles are"""
    from lhvi import utils
    g, x = unary_graph(1.5, 2.25)
    bp = epbp(g, n)
    for mu_p, sd_p in ((0.0, 1.0), (2.5, 0.4), (-1.0, 2.0)):
        kl, info = bp.kl_from((np.ones(1), np.array([[mu_p]]), np.array([[sd_p ** 2]])), info=True)
        exact = utils.kl_normal(mu_p, 1.5, sd_p, 1.5)
        print('n = %d, p = N(%g, %g^2): kl %.12g, exact %.12g, abserr %.3g, neval %d' % (n, mu_p, sd_p, kl[0], exact, info['abserr'][0],
                                                                                         info['neval'][0]))
        assert info['status'][0] == 0 and closed_form_bound(kl[0], info['abserr'][0], exact)


@pytest.mark.parametrize('n', [8, 64])
def test_pair_factor_to_an_observed_neighbour_matches_the_closed_form(api, n):
    """log phi(x, y_obs) of a Gaussian pair factor is a normal in x: precision P11, mean m1 - P12 (y - m2) / P11"""
    from lhvi import utils
    mu, sig, yobs = [0.5, -1.0], np.array([[2.0, 0.9], [0.9, 1.2]]), 0.7
    prec = np.linalg.inv(sig)
    mq, sdq = mu[0] - prec[0, 1] * (yobs - mu[1]) / prec[0, 0], 1.0 / np.sqrt(prec[0, 0])
    g, x = observed_pair_graph(mu, sig, yobs)
    bp = epbp(g, n)
    for mu_p, sd_p in ((1.0, 0.8), (-0.5, 1.6)):
        kl, info = bp.kl_from((np.ones(1), np.array([[mu_p]]), np.array([[sd_p ** 2]])), info=True)
        exact = utils.kl_normal(mu_p, mq, sd_p, sdq)
        print('n = %d: kl %.12g, exact %.12g, abserr %.3g' % (n, kl[0], exact, info['abserr'][0]))
        assert info['status'][0] == 0 and closed_form_bound(kl[0], info['abserr'][0], exact)


# ---- G3: the restatement, factor kinds and degrees -----------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def hand20(api):
    g, x = hand_graph()
    return epbp(g, 20), x


@pytest.mark.parametrize('n', [8, 20, 64])
def test_hand_graph_matches_the_restatement(api, n):
    g, x = hand_graph()
    bp = epbp(g, n)
    flat = bp.flat
    rows = np.array([flat.var_index[rv] for rv in x], dtype=np.int32)
    deg = np.diff(flat.var_ptr)[rows]
    assert deg.max() >= 5 and {1, 2} <= set(deg.tolist())
    np.testing.assert_array_equal(bp._kl_rows(None), np.sort(rows))
    check_against_twin(bp, rows, mixtures(len(rows), 3, 40 + n), 'hand graph, n = %d' % n)


def test_paper_popularity_grounding_matches_the_restatement(api):
    """the 6 x 3 paper-popularity grounding: conditionally quadratic formulas of arity 3 with a hidden boolean"""
    from test_gpu_pbp import paper_popularity
    g, table = paper_popularity(6, 3, seed=5)
    bp = epbp(g, 20)
    rows = bp._kl_rows(None)
    assert rows.size >= 2 and bp.n_cq + bp.n_heavy_class + bp.n_light > 0          # the conditionally quadratic routes occur
    check_against_twin(bp, rows, mixtures(rows.size, 3, 7, centre=5.0), 'paper popularity 6 x 3')


# ---- G4 / G5: the shapes of p ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Kp', [1, 3, 64, 65, 130])
def test_component_counts_of_p(api, hand20, Kp):
    """Kp <= 64: the components are resident in LDS; 65 and 130 stream them in chunks of 64 in front of every evaluation, with
    the barriers inside the evaluation"""
    bp, x = hand20
    rows = np.array([bp.flat.var_index[x[0]], bp.flat.var_index[x[6]]], dtype=np.int32)
    check_against_twin(bp, rows, mixtures(2, Kp, 100 + Kp, spread=4.0, vlo=0.3, vhi=4.0), 'Kp = %d' % Kp)


def test_panel_counts_and_a_bisection(api, hand20):
    """P in {1, 2, 4, 65}, forced by p's narrowest component (a clipped range for 1 and 2), and a row with epsrel = 1e-12
    that bisects"""
    bp, x = hand20
    v = int(bp.flat.var_index[x[1]])
    wide = lambda s: (np.array([[0.5, 0.5]]), np.array([[0.0, 0.5]]), np.array([[1.0, s * s]]))      # noqa: E731
    cases = [(1, wide(1.0), -4.0, 4.0), (2, wide(1.0), -8.0, 8.0), (4, wide(0.625), -np.inf, np.inf),
             (65, wide(20.0 / (8.0 * 64.5)), -np.inf, np.inf)]
    for P, p, a, b in cases:
        kl, info, stats = check_against_twin(bp, [v], p, 'P = %d' % P, a=a, b=b)
        assert stats[0]['P'] == P and info['neval'][0] >= 21 * P
    kl, info, stats = check_against_twin(bp, [v], wide(0.625), 'epsrel = 1e-12', epsrel=1e-12, epsabs=0.0)
    assert stats[0]['depth'] >= 1 and info['neval'][0] > 21 * 4


# ---- G6: rows and positions -------------------------------------------------------------------------------------------------------------
def launch(api, bp, rows, p, logz, a=-np.inf, b=np.inf, pairs=None, epsabs=EPS, epsrel=EPS):
    """``lhvi_pbp_kl`` itself on explicit rows and normalisers: (kl, abserr, status, neval) as host arrays"""
    import torch
    R, Kp = len(rows), p[1].shape[1]
    dev = [api.to_dev(np.array(np.broadcast_to(t, (R, Kp)), dtype=np.float64)) for t in p]
    at, bt = (api.to_dev(np.array(np.broadcast_to(t, (R,)), dtype=np.float64)) for t in (a, b))
    rv, lz = api.to_dev(np.asarray(rows, dtype=np.int32)), api.to_dev(np.asarray(logz, dtype=np.float64))
    kl, err = torch.empty(R, dtype=torch.float64, device='cuda'), torch.empty(R, dtype=torch.float64, device='cuda')
    st, ne = torch.empty(R, dtype=torch.int32, device='cuda'), torch.empty(R, dtype=torch.int32, device='cuda')
    qp = [api.ptr(t) for t in pairs] if pairs else [None, None, None]
    api.check(api.lib().lhvi_pbp_kl(bp.dg.g, bp.dg.p, bp._struct(), api.ptr(bp.v2f), R, api.ptr(rv), *qp, api.ptr(lz), Kp,
                                    *(api.ptr(t) for t in dev), api.ptr(at), api.ptr(bt), epsabs, epsrel, api.ptr(kl), api.ptr(err),
                                    api.ptr(st), api.ptr(ne), api.stream_ptr()))
    return tuple(t.cpu().numpy() for t in (kl, err, st, ne))


def test_rows_positions_launches_and_an_invalid_row(api, hand20):
    bp, x = hand20
    flat = bp.flat
    rows = np.array([flat.var_index[rv] for rv in x], dtype=np.int32)          # seven rows
    p = mixtures(7, 3, 77)
    logz = logz_of(bp)[rows]
    full = launch(api, bp, rows, p, logz)
    assert (full[2] == 0).all() and np.isfinite(full[0]).all()
    again = launch(api, bp, rows, p, logz)
    for u, v in zip(full, again):
        np.testing.assert_array_equal(u, v)                                    # a second launch: the same bits
    alone = launch(api, bp, rows[6:], tuple(t[6:] for t in p), logz[6:])       # nq = 1 against the last position of 7
    for u, v in zip(full, alone):
        assert u[6] == v[0]
    # kl_from is that launch
    kl, info = bp.kl_from(p, rows=rows, info=True)
    np.testing.assert_array_equal(kl, full[0])
    np.testing.assert_array_equal(info['neval'], full[3])
    # a NaN normaliser: that row is NaN with status bit 2, its neighbours keep their bits
    bad = logz.copy()
    bad[3] = np.nan
    got = launch(api, bp, rows, p, bad)
    assert np.isnan(got[0][3]) and np.isnan(got[1][3]) and got[2][3] == 4 and got[3][3] == 0
    keep = np.arange(7) != 3
    for u, v in zip(full, got):
        np.testing.assert_array_equal(u[keep], v[keep])
    # so are an observed and a discrete variable handed to the entry point (kl_from refuses them before the launch)
    others = np.flatnonzero(~(flat.var_hidden & flat.var_cont)).astype(np.int32)
    assert others.size == 3
    got = launch(api, bp, np.concatenate([rows[:1], others]), tuple(t[:4] for t in p), np.zeros(4) + logz[0])
    assert got[0][0] == full[0][0] and np.isnan(got[0][1:]).all() and (got[2][1:] == 4).all()
    # an invalid p row
    pbad = tuple(t.copy() for t in p)
    pbad[2][2, 1] = -1.0
    got = launch(api, bp, rows, pbad, logz)
    assert np.isnan(got[0][2]) and got[2][2] == 4
    np.testing.assert_array_equal(got[0][np.arange(7) != 2], full[0][np.arange(7) != 2])
    # the pairs form with each row's own edges at multiplicity 1 gives the bits of the row_var form
    ptr = np.zeros(8, dtype=np.int64)
    ptr[1:] = np.cumsum(flat.var_ptr[rows + 1] - flat.var_ptr[rows])
    edges = np.concatenate([flat.var_edge[flat.var_ptr[v]:flat.var_ptr[v + 1]] for v in rows]).astype(np.int32)
    pairs = (api.to_dev(ptr), api.to_dev(edges), api.to_dev(np.ones(edges.size)))
    by_pairs = launch(api, bp, rows, p, logz, pairs=pairs)
    for u, v in zip(full, by_pairs):
        np.testing.assert_array_equal(u, v)


# ---- G7: the lifted solver ------------------------------------------------------------------------------------------------------------------
def test_hybrid_lbp_on_a_stable_partition_matches_the_restatement(api):
    from lhvi import generators
    from lhvi.pbp import HybridLBP
    rel = generators.rgm(4, 3)
    g, table = rel.ground_graph()
    rel.add_evidence({('market', 'c0'): 1.5, ('loss', 'c1', 'b0'): -2.0})       # (two observations: 12 clusters of the 20 atoms)
    g.rvs, g.factors = sorted(g.rvs), sorted(g.factors)
    g.init_nb()
    assert len(g.rvs) == 20
    bp = HybridLBP(g, n=20, proposal_approximation='simple', sampler='device', seed=3)
    bp.run(3, c2f=-1)
    flat = bp.flat
    assert flat.lifted and flat.edge_count is not None and flat.V == 12 and (flat.edge_count > 1).any()
    rows = bp._kl_rows(None)
    p = mixtures(rows.size, 3, 9, spread=6.0, vlo=2.0, vhi=30.0)
    check_against_twin(bp, rows, p, 'HybridLBP, rgm(4, 3)')
    # the normaliser is HybridLBP.belief's: log(area) + shift of the 20-point log_area over the domain
    z, shift = bp._cached_area()
    np.testing.assert_array_equal(logz_of(bp)[rows], (np.log(z) + shift)[rows])


# ---- G8 / G9: the drivers' flow, tensor placement --------------------------------------------------------------------------------------------
def test_exact_marginals_against_epbp_end_to_end(api):
    """hybrid_mln_test_0 through the MLN conversion: KL(exact marginal || EPBP belief) per continuous variable, on device
    tensors; by Gibbs' inequality no value is negative beyond the error"""
    import torch
    import exact_models as em
    from lhvi import exact
    from lhvi.pbp import EPBP
    model = em.build('ref_mln0')
    g = graph_of(model['rvs'], model['factors'])
    s = exact.ExactHybridGaussian(g).run()
    bp = EPBP(g, n=20, proposal_approximation='simple')
    bp.run(10)
    rows = [bp.flat.var_index[rv] for rv in s.Vc]
    marg = s.marginals()
    kl, info = marg.kl(bp, rows=rows, info=True)
    assert torch.is_tensor(kl) and kl.is_cuda and all(t.is_cuda for t in info.values())
    k, e, st = kl.cpu().numpy(), info['abserr'].cpu().numpy(), info['status'].cpu().numpy()
    print('KL(exact || EPBP) = %s, abserr %s, neval %s' % (k, e, info['neval'].cpu().numpy()))
    assert (st == 0).all() and np.isfinite(k).all()
    assert (k >= -(e + 2 * EPS)).all()
    host = tuple(t.cpu().numpy() for t in (marg.w, marg.mu, marg.var))
    k2, info2 = bp.kl_from(host, rows=rows, info=True)
    assert isinstance(k2, np.ndarray)
    np.testing.assert_array_equal(k2, k)
    np.testing.assert_array_equal(info2['abserr'], e)
    np.testing.assert_array_equal(info2['neval'], info['neval'].cpu().numpy())


def test_tensor_placement(api, hand20):
    import torch
    bp, x = hand20
    rows = [bp.flat.var_index[x[0]]]
    w, mu, var = (torch.from_numpy(t) for t in mixtures(1, 3, 1))
    with pytest.raises(ValueError, match='current device'):
        bp.kl_from((w, mu, var), rows=rows)                                    # a CPU tensor is refused
    kl = bp.kl_from((w.cuda(), mu.cuda(), var.cuda()), rows=rows)
    assert torch.is_tensor(kl) and kl.is_cuda and kl.dtype == torch.float64
    np.testing.assert_array_equal(kl.cpu().numpy(), bp.kl_from((w.numpy(), mu.numpy(), var.numpy()), rows=rows))
