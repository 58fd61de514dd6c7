"""GPU: the variational MAP query in one launch (``map_rows_device`` / ``map_mode = 'device'``, lhvi_vi_map_bfgs of
csrc/vi_map.hip) against the host path it replaces -- ``scipy.optimize.minimize`` per row, the reference's call -- row for row,
iteration count and exit status included, and against the reference's golden MAPs."""
import numpy as np
import pytest

import modelio
from test_oracle_golden import API
from test_oracle_vi import VI_CASES, LVI_CASES, load_vi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def api():
    from lhvi import _abi
    _abi.require_gpu()
    return _abi


def scipy_rows(vi, rows):
    """(x, belief, nit, status) of the reference's map() call on each continuous row of `rows` (VI:355-376)"""
    from scipy.optimize import minimize
    out = []
    for v in rows:
        p = {x: vi._row_belief(v, x) for x in vi._host('eta_c')[v][:, 0]}
        x0 = max(p.keys(), key=lambda k: p[k])
        r = minimize(lambda val, v=v: -vi._row_belief(v, val), x0=np.array([x0]), options={'disp': False})
        out.append((r.x[0], -r.fun, r.nit, r.status))
    return np.array(out).reshape(-1, 4)


def check_rows_equal_host(vi):
    """map_rows_device() == the host map_rows() on every hidden row, with scipy's nit and status.  The iterates are scipy's bit for
    bit given the same objective values; the kernel's np.e ** y is correctly rounded, libm's pow is 1 ulp off on ~0.1 % of
    exponents, and at a converged maximum one such ulp in f moves the forward-difference gradient (h = 1.5e-8) and with it the last
    step by up to a few 1e-8 -- so x to 1e-7 (with libm's pow in its place a host build of the kernel reproduces every row exactly)"""
    flat = vi.flat
    x, (f, nit, status) = vi.map_rows_device(info=True)
    host = vi.map_rows()
    hid = flat.var_hidden
    assert np.isnan(x[~hid]).all() and (status[~hid] == -1).all()
    np.testing.assert_array_equal(x[hid & ~flat.var_cont], host[hid & ~flat.var_cont])
    cont = np.flatnonzero(hid & flat.var_cont)
    ref = scipy_rows(vi, cont)
    np.testing.assert_array_equal(ref[:, 0], host[cont])
    np.testing.assert_allclose(x[cont], ref[:, 0], rtol=1e-7, atol=1e-7)
    np.testing.assert_array_equal(nit[cont], ref[:, 2].astype(np.int32))
    np.testing.assert_array_equal(status[cont], ref[:, 3].astype(np.int32))
    np.testing.assert_allclose(f[cont], ref[:, 1], rtol=1e-9, atol=1e-300)


@pytest.mark.parametrize('name', VI_CASES + LVI_CASES)
def test_device_map_equals_scipy_after_the_golden_trajectory(api, golden_dir, name):
    from lhvi.vi import VarInference, LiftedVarInference
    z, meta = load_vi(golden_dir, name)
    g, rvs, factors = modelio.load_model(meta['model'], API)
    vi = (LiftedVarInference if meta['lifted'] else VarInference)(g, meta['K'], meta['T'])
    assert vi.map_mode == 'scipy'
    if not meta['lifted']:
        np.random.seed(meta['seed'])
        vi.run(meta['iterations'], lr=meta['lr'])
    else:
        vi._setup(vi._graph_like())
        flat = vi.flat
        gather = np.array([flat.var_index[rv.cluster] for rv in rvs])

        def scatter(key):
            out = np.full((flat.V,) + z[key].shape[1:], np.nan)
            out[gather] = z[key]
            return out
        vi.run(0, lr=meta['lr'])
        vi._upload_params(z['w_tau0'], scatter('eta_c0'), scatter('tau_d0'))
        vi.ADAM_update(meta['iterations'])
    np.testing.assert_allclose([x[1] for x in vi.time_log], z['fe_log'], rtol=1e-8)
    check_rows_equal_host(vi)
    vi.map_mode = 'device'
    cont = [i for i, rv in enumerate(rvs) if rv.value is None and rv.domain.continuous]
    disc = [i for i, rv in enumerate(rvs) if rv.value is None and not rv.domain.continuous]
    for i in cont[:4] + disc[:3]:
        assert vi.map(rvs[i]) == pytest.approx(z['map'][i], rel=1e-5, abs=1e-5)


@pytest.mark.parametrize('name', ['c2f_rgm_k2', 'c2f_hmln_k2', 'c2f_robot_k2', 'c2f_rkf_tree_k1', 'c2f_rkf_cycle_k1',
                                  'c2f_hmln_mixed_k2', 'c2f_hmln_mean_k2'])
def test_device_map_equals_scipy_after_the_c2fvi_golden_run(api, golden_dir, name):
    from lhvi.c2fvi import VarInference as C2FVI
    from test_oracle_vi import kmeans_order_of
    z, meta = load_vi(golden_dir, name)
    g, rvs, factors = modelio.load_model(meta['model'], API)
    vi = C2FVI(g, meta['K'], meta['T'])
    vi.update_obs_its = meta['update_obs_its']
    vi.gaussian_obs = meta.get('gaussian_obs', True)
    vi.kmeans_member_order = kmeans_order_of(meta)
    vi.init = (z['eta_c0'], z['tau_d0'])
    vi.run(meta['iterations'], lr=meta['lr'])
    np.testing.assert_allclose([fe for _, fe in vi.time_log], z['fe_log'], rtol=1e-8)
    check_rows_equal_host(vi)
    vi.map_mode = 'device'
    hidden = [i for i, rv in enumerate(rvs) if rv.value is None]
    for i, rv in enumerate(rvs):
        if rv.value is None:
            if len(hidden) > 60 and i not in hidden[::4]:
                continue
            assert vi.map(rv) == pytest.approx(z['map'][i], abs=1e-4)
        elif i % 16 == 0 or len(rvs) < 200:
            assert vi.map(rv) == rv.value


@pytest.mark.parametrize('name', ['c2f_rgm_k2_loglik', 'c2f_hmln_k2_loglik'])
def test_c2fvi_logs_the_map_likelihood_at_device_maps(api, golden_dir, name):
    """``run(log_fe=False)`` with ``map_mode = 'device'``: every logged update takes its MAPs from one launch, through the
    objects and through the array schedule, and the log is the reference's"""
    from lhvi import c2fvi
    from lhvi.flat import flatten
    from test_oracle_vi import kmeans_order_of
    z, meta = load_vi(golden_dir, name)
    g, rvs, factors = modelio.load_model(meta['model'], API)
    vi = c2fvi.VarInference(g, meta['K'], meta['T'])
    vi.map_mode = 'device'
    vi.update_obs_its = meta['update_obs_its']
    vi.kmeans_member_order = kmeans_order_of(meta)
    vi.init = (z['eta_c0'], z['tau_d0'])
    vi.run(meta['iterations'], lr=meta['lr'], log_fe=False)
    got = [fe for _, fe in vi.time_log]
    assert len(got) == meta['iterations']
    np.testing.assert_allclose(got, z['fe_log'], rtol=1e-6, atol=1e-6)
    vi.is_log, vi.log_fe = True, False
    engine = c2fvi._DeviceEngine(vi)
    res = c2fvi.run_c2fvi_flat(flatten(g, require_device_potentials=True), engine, meta['K'], meta['iterations'],
                               meta['lr'], vi._options(), init=(z['eta_c0'], z['tau_d0']))
    assert res['stage'].map_mode == 'device'
    np.testing.assert_allclose(res['fe_log'], z['fe_log'], rtol=1e-6, atol=1e-6)


def isolated_rows(V, obs=(), disc=()):
    """V variables without neighbours (a unary factor each): continuous hidden, except observed rows `obs` and three-state rows `disc`"""
    from lhvi.graph import Domain, F, Graph, RV
    from lhvi.potentials import TablePotential, X2Potential
    dc = Domain((-50, 50), continuous=True, integral_points=np.linspace(-50, 50, 8))
    dd = Domain((0, 1, 2), continuous=False)
    rvs = []
    for i in range(V):
        if i in disc:
            rvs.append(RV(dd, None))
        else:
            rvs.append(RV(dc, 0.25 * i if i in obs else None))
    fs = [F(TablePotential(np.array([1.0, 2.0, 3.0])) if i in disc else X2Potential(1.0, 3.0), [rv]) for i, rv in enumerate(rvs)]
    g = Graph()
    g.rvs, g.factors = rvs, fs
    g.init_nb()
    return g, rvs


def regime_params(rng, V, K):
    """means ~ N(0, 5), variances log-uniform on [1e-3, 316] (below var_threshold included), duplicated
    means on every 7th row, beliefs that underflow to 0 (variance 1e308: the normaliser overflows) on every 97th row"""
    w_tau = rng.random(K) * 4
    eta = np.empty((V, K, 2))
    eta[:, :, 0] = rng.normal(0, 5, (V, K))
    eta[:, :, 1] = 10 ** rng.uniform(-3, 2.5, (V, K))
    if K > 1:
        eta[::7, 1, 0] = eta[::7, 0, 0]
    eta[::97, :, 1] = 1e308
    return w_tau, eta


def test_device_map_follows_scipy_where_scipy_misses_the_mode(api):
    """4 000 isolated rows, K = 1..8 and 12 (numpy's pairwise sum from 8 terms on): each K's launch covers every row, scipy checks
    a ninth of them (a different ninth per K).  The sample holds line-search failures (status 2) and rows that stop at the
    start point although it is not the local maximum -- rows that only the same iterates reproduce"""
    from lhvi.vi import VarInference
    V = 4000
    g, rvs = isolated_rows(V)
    rng = np.random.default_rng(7)
    Ks = list(range(1, 9)) + [12]
    diff, n, n_status2, n_stuck = [], 0, 0, 0
    with np.errstate(over='ignore'):
        for j, K in enumerate(Ks):
            vi = VarInference(g, K, 3)
            vi._setup(vi._graph_like())
            w_tau, eta = regime_params(rng, V, K)
            vi._upload_params(w_tau, eta, np.zeros((V, K, 1)))
            x, (f, nit, status) = vi.map_rows_device(info=True)
            assert (status >= 0).all()
            under = np.arange(0, V, 97)
            np.testing.assert_array_equal(x[under], eta[under, 0, 0])     # belief 0 everywhere: the first mean, no iteration
            assert (nit[under] == 0).all()
            rows = np.arange(j, V, len(Ks))
            ref = scipy_rows(vi, rows)
            for r, (xr, fr, itr, str_) in zip(rows, ref):
                n += 1
                if not (abs(x[r] - xr) <= 1e-9 * max(1.0, abs(xr)) and nit[r] == itr and status[r] == str_):
                    diff.append((K, int(r), float(x[r]), int(nit[r]), int(status[r]), float(xr), int(itr), int(str_)))
                    continue
                n_status2 += int(str_ == 2)
                if itr == 0:
                    bx = vi._row_belief(r, xr)
                    n_stuck += int(any(vi._row_belief(r, xr + s) > bx for s in (-1e-2, -1e-3, 1e-3, 1e-2)))
    for d in diff:
        print('K=%d row %d: device x=%r nit=%d status=%d, scipy x=%r nit=%d status=%d' % d)
    print('%d rows, %d differ, %d line-search failures, %d stuck at a point that is not the local maximum' % (n, len(diff), n_status2, n_stuck))
    assert n >= 4000
    assert len(diff) <= 0.001 * n
    assert n_status2 > 0 and n_stuck > 0


def test_discrete_ties_and_observed_rows(api):
    from lhvi.vi import VarInference
    g, rvs = isolated_rows(6, obs=(1, 4), disc=(2, 5))
    vi = VarInference(g, 3, 3)
    vi._setup(vi._graph_like())
    flat = vi.flat
    V = flat.V
    eta = np.ones((V, 3, 2))
    eta[:, :, 0] = [[-1.0, 0.5, 2.0]]
    tau = np.zeros((V, 3, 3))
    tau[:, :, :] = [0.0, 2.0, 2.0]                     # states 1 and 2 tie in every component
    tau[flat.var_index[rvs[5]]] = [[0.0, 1.0, 3.0]] * 3
    vi._upload_params(np.array([0.1, 0.2, 0.3]), eta, tau)
    x, (f, nit, status) = vi.map_rows_device(info=True)
    i2, i5 = flat.var_index[rvs[2]], flat.var_index[rvs[5]]
    assert x[i2] == 1 and x[i5] == 2 and status[i2] == 0
    for i in (1, 4):
        v = flat.var_index[rvs[i]]
        assert np.isnan(x[v]) and status[v] == -1
    np.testing.assert_array_equal(np.isnan(x), np.isnan(vi.map_rows()))
    check_rows_equal_host(vi)
    vi.map_mode = 'scipy'
    host = [vi.map(rv) for rv in rvs]
    vi.map_mode = 'device'
    dev = [vi.map(rv) for rv in rvs]
    assert host[1] == dev[1] == 0.25 and host[4] == dev[4] == 1.0          # observed: rv.value
    assert host[2] == dev[2] == 1 and host[5] == dev[5] == 2                # discrete: the first of the tied states, the domain's value
    np.testing.assert_allclose([dev[0], dev[3]], [host[0], host[3]], rtol=1e-9)
    # the cached answer follows the parameters
    before = vi.map_rows_device().copy()
    eta[:, :, 0] += 1.0
    vi._upload_params(np.array([0.1, 0.2, 0.3]), eta, tau)
    assert vi.map(rvs[0]) != dev[0]
    vi.map_mode = 'scipy'
    check_rows_equal_host(vi)
    assert not np.array_equal(vi.map_rows_device()[[0, 3]], before[[0, 3]])
