"""Seeded Gaussian chains for the block-tridiagonal solver (lhvi.gauss_chain, lhvi.kalman) and their dense NumPy yardstick.

Kalman models: ``KalmanFilter`` with A = 0.9 I + 0.3 randn / sqrt(n), q = 0.7, r = 0.4, C = diag(U(0.5, 1.5)) and 40 % missing
observations.  The dense ``J``, ``h`` and constant come from ``grounded_flat`` -> ``conditioned_quadratics`` -> the reference's
joint quadratic (osi/utils.py), never from ``block_tridiagonal``; the yardstick is ``np.linalg.inv`` / ``slogdet`` on that ``J``.
The solver's input blocks are cut out of the same dense ``J`` (``blocks_of`` asserts nothing lies outside the band).

SHAPES (n, M): the smallest that reach every path -- one block, two blocks, the padded edges 8 / 16 / 32 / 64 / 128 with ragged
n, the 64-tile exactly and one past it (2 x 2 tiles), the widest block, and a long recursion.  'ragged' is an object graph of
QuadraticPotential / GaussianPotential factors on blocks of 3, 1, 5 and 2 variables with one observed variable.

Tolerance: tol = 10 N cond(J) 1.1e-16 with N = M n (docs/kernels_gauss_chain.md); ``dense_reference`` asserts cond(J) <= 500.
"""
import os

import numpy as np

from gauss_exact_models import first_bad_pivot, report  # noqa: F401

SHAPES = ((1, 1), (1, 2), (3, 4), (5, 7), (17, 5), (63, 3), (64, 3), (65, 3), (128, 2), (4, 300))
U = 1.1e-16
MISSING = 5000
T_FIXTURE = 20
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_cache = {}


def tolerance(N, cond):
    return 10 * max(N, 1) * cond * U


def _domain():
    from lhvi.graph import Domain
    return Domain((-4, 4), continuous=True, integral_points=np.linspace(-4, 4, 30))


def kalman_model(n, M, seed=None):
    """(KalmanFilter, T = M + 1, data [n][T]); cached"""
    key = ('kf', n, M, seed)
    if key not in _cache:
        from lhvi.kalman import KalmanFilter
        rng = np.random.default_rng(1000 * n + M if seed is None else seed)
        A = 0.9 * np.eye(n) + 0.3 * rng.normal(size=(n, n)) / np.sqrt(n)
        C = np.diag(rng.uniform(0.5, 1.5, size=n))
        T = M + 1
        data = rng.normal(size=(n, T))
        data[:, 1:][rng.random((n, M)) < 0.4] = MISSING
        _cache[key] = (KalmanFilter(_domain(), A, 0.7, C, 0.4), T, data)
    return _cache[key]


def assembled(kf, T, data):
    """dense (J [N][N], h [N], const) of the conditioned model of ``grounded_flat`` over the hidden states in (t, i) order, t >= 1,
    by the reference's route: condition every factor, sum the joint quadratic; plus the flat graph and state_id"""
    from lhvi.gauss_exact import conditioned_quadratics
    from lhvi.utils import get_joint_quadratic_params
    flat, state_id = kf.grounded_flat(T, data)
    params, scopes, const, hidden = conditioned_quadratics(flat)
    assert np.array_equal(hidden, state_id[1:].ravel())
    A, b, c = get_joint_quadratic_params(params, scopes, hidden.size)
    return -(A + A.T), np.asarray(b, dtype=np.float64), float(c) + const, flat, state_id


def blocks_of(J, h, sizes):
    """(D [M][n][n], O [M-1][n][n], h [M][n]) cut out of a dense J for blocks of the given sizes, padded to the widest with the
    identity; asserts that no entry of J links blocks more than one apart"""
    M, n = len(sizes), max(sizes)
    start = np.concatenate([[0], np.cumsum(sizes)])
    D, O, hb = np.zeros((M, n, n)), np.zeros((max(M - 1, 0), n, n)), np.zeros((M, n))
    band = np.zeros_like(J, dtype=bool)
    for t in range(M):
        a, b = start[t], start[t + 1]
        D[t] = np.eye(n)
        D[t, :b - a, :b - a] = J[a:b, a:b]
        hb[t, :b - a] = h[a:b]
        band[a:b, a:b] = True
        if t + 1 < M:
            e = start[t + 2]
            O[t, :b - a, :e - b] = J[a:b, b:e]
            band[a:b, b:e] = band[b:e, a:b] = True
    assert not J[~band].any()
    return D, O, hb


def dense_reference(J, h):
    """the yardstick: dict with mu, Sig, logdet, cond (asserted <= 500), N"""
    N = J.shape[0]
    eig = np.linalg.eigvalsh(J)
    cond = float(eig[-1] / eig[0])
    assert eig[0] > 0 and cond <= 500, cond
    Sig = np.linalg.inv(J)
    return dict(N=N, cond=cond, Sig=Sig, mu=np.linalg.solve(J, h), logdet=float(np.linalg.slogdet(J)[1]), J=J, h=h)


def shape_case(n, M):
    """a Kalman model of the shape with its dense yardstick and the solver's input blocks; cached"""
    key = ('shape', n, M)
    if key not in _cache:
        kf, T, data = kalman_model(n, M)
        J, h, const, flat, state_id = assembled(kf, T, data)
        ref = dense_reference(J, h)
        ref.update(const=const, kf=kf, T=T, data=data, flat=flat, state_id=state_id, blocks=blocks_of(J, h, [n] * M), sizes=[n] * M)
        ref['logZ'] = ref['N'] / 2 * np.log(2 * np.pi) - 0.5 * ref['logdet'] + 0.5 * float(ref['mu'] @ h) + const
        _cache[key] = ref
    return _cache[key]


def check_solution(what, ref, sizes, mu, var, logdet, cov=None, cross=None):
    """the blocks' results against the dense yardstick at tol: variances and log det J relative per entry, means, covariances and
    cross-covariances max |d| <= tol max(1, max |ref|); the padding of a ragged block is ignored"""
    tol = tolerance(ref['N'], ref['cond'])
    start = np.concatenate([[0], np.cumsum(sizes)])
    M = len(sizes)
    cut = lambda x: np.concatenate([x[t, :sizes[t]] for t in range(M)])
    e, bnd = report(what + ' mu', float(np.abs(cut(mu) - ref['mu']).max()), tol * max(1.0, float(np.abs(ref['mu']).max())))
    assert e <= bnd
    e, bnd = report(what + ' var (rel)', float(np.abs(cut(var) / np.diag(ref['Sig']) - 1).max()), tol)
    assert e <= bnd
    e, bnd = report(what + ' log det J (rel)', abs(logdet - ref['logdet']) / abs(ref['logdet']) if ref['logdet'] else abs(logdet), tol)
    assert e <= bnd
    if cov is not None:
        Sig, scale = ref['Sig'], tol * max(1.0, float(np.abs(ref['Sig']).max()))
        ec = max(float(np.abs(cov[t, :sizes[t], :sizes[t]] - Sig[start[t]:start[t + 1], start[t]:start[t + 1]]).max()) for t in range(M))
        ex = max([float(np.abs(cross[t, :sizes[t], :sizes[t + 1]] - Sig[start[t]:start[t + 1], start[t + 1]:start[t + 2]]).max())
                  for t in range(M - 1)] + [0.0])
        report(what + ' cov', ec, scale)
        report(what + ' cross', ex, scale)
        assert ec <= scale and ex <= scale


def twin_gap(dev, host):
    """device against host twin: the largest |difference| of each array as a share of the array's largest entry"""
    return max(float(np.abs(np.asarray(d) - np.asarray(h)).max()) / max(float(np.abs(np.asarray(h)).max()), 1e-300)
               for d, h in zip(dev, host) if np.size(h))


def fixture(which):
    """the demos' inputs (tests/golden/rkf.npz): dict with data, the five KalmanFilters of the parameter sets
    (LRKFDemoTree.py:50-54, LRKFDemoCycle.py:56-60), the recorded GaBP(20) marginals of parameter set 0; cached"""
    key = ('fixture', which)
    if key not in _cache:
        from lhvi.kalman import KalmanFilter
        z = np.load(os.path.join(GOLDEN, 'rkf.npz'))
        data, param = z[which + '_data'], z[which + '_param']
        n = data.shape[0]
        dom = _domain()
        kfs = [KalmanFilter(dom, np.eye(n) * param[2, k] + (0.01 if which == 'cycle' else 0.0), param[0, k], np.eye(n), param[1, k])
               for k in range(param.shape[1])]
        _cache[key] = dict(data=data, filters=kfs, gabp=z[which + '_gabp'], n=n)
    return _cache[key]


def fixture_reference(which, k):
    """dense yardstick of parameter set k of a fixture (``assembled`` route); cached"""
    key = ('fixture_ref', which, k)
    if key not in _cache:
        fx = fixture(which)
        J, h, const, flat, state_id = assembled(fx['filters'][k], T_FIXTURE, fx['data'])
        ref = dense_reference(J, h)
        ref.update(const=const, flat=flat, state_id=state_id)
        ref['logZ'] = ref['N'] / 2 * np.log(2 * np.pi) - 0.5 * ref['logdet'] + 0.5 * float(ref['mu'] @ h) + const
        _cache[key] = ref
    return _cache[key]


RAGGED = (3, 1, 5, 2)


def ragged_chain():
    """(graph, rvs, blocks [list of lists of RVs], dense yardstick over the hidden variables in block order): unary
    QuadraticPotential on every variable, GaussianPotential / QuadraticPotential pairs inside a block and between neighbouring
    blocks, one three-variable QuadraticPotential across blocks 1 and 2, and one observed variable tied to block 0; cached"""
    if 'ragged' in _cache:
        return _cache['ragged']
    from lhvi import potentials as P
    from lhvi.graph import F, Graph, RV
    rng = np.random.default_rng(77)
    d = _domain()
    blocks = [[RV(d) for _ in range(s)] for s in RAGGED]
    obs = RV(d, 0.8)
    rvs = [rv for blk in blocks for rv in blk] + [obs]
    fs = []
    for rv in rvs[:-1]:
        dd = float(rng.uniform(2.0, 3.0))
        fs.append(F(P.QuadraticPotential(np.array([[-dd / 2]]), np.array([float(rng.normal())]), float(rng.normal())), [rv]))

    def pair(a, b):
        o = float(rng.uniform(0.1, 0.3)) * (1 if rng.random() < 0.5 else -1)
        prec = np.array([[abs(o) + 0.1, o], [o, abs(o) + 0.2]])
        if rng.random() < 0.5:
            return F(P.GaussianPotential([float(rng.normal()), float(rng.normal())], np.linalg.inv(prec).tolist()), [a, b])
        return F(P.QuadraticPotential(-0.5 * prec, rng.normal(size=2), float(rng.normal())), [a, b])
    for t, blk in enumerate(blocks):
        for i in range(len(blk) - 1):
            fs.append(pair(blk[i], blk[i + 1]))
        if t + 1 < len(blocks):
            nxt = blocks[t + 1]
            fs.append(pair(blk[0], nxt[-1]))
            fs.append(pair(nxt[0], blk[-1]))               # later block first: the scatter must transpose
    prec3 = np.array([[0.5, 0.1, -0.1], [0.1, 0.6, 0.15], [-0.1, 0.15, 0.4]])
    fs.append(F(P.QuadraticPotential(-0.5 * prec3, rng.normal(size=3), 0.3), [blocks[2][1], blocks[1][0], blocks[2][3]]))
    fs.append(pair(obs, blocks[0][1]))
    g = Graph()
    g.rvs, g.factors = rvs, fs
    g.init_nb()
    # yardstick by the NumPy restatement of the reference route (tests/gauss_exact_models.py): hidden = rvs[:-1] in block order
    import gauss_exact_models as gm
    route = gm.reference_route(g, rvs)
    ref = dense_reference(route['J'], route['b'])
    ref['logZ'] = route['logZ']
    _cache['ragged'] = (g, rvs, blocks, ref)
    return _cache['ragged']
