"""Seeded Gaussian MRFs for the exact Gaussian solver (lhvi.gauss_exact) and a NumPy restatement of the reference route
(osi/utils.py: condition on the evidence, sum the joint quadratic in factor, i, j order, np.linalg.inv of J = -2A).

Models: diagonally dominant graphs of pair and unary factors drawn from the five exp-quadratic potential classes.  Every
variable gets a unary factor worth at least 2 on the diagonal of J and at most four pair factors worth at most 0.35 off the
diagonal each, so J is strictly diagonally dominant with eigenvalues in about [0.6, 6]: cond(J) stays far below the 500 the
tolerance assumes (each user asserts it).  SHAPES covers one tile of NB = 64, the ragged last tile, and two and more panel
steps; 'ev30' has 30 % evidence; 'indefinite' carries one pair factor on variables 70 and 71 whose off-diagonal exceeds the
diagonal, so the first bad pivot lies in the second tile.
"""
import ast
import os

import numpy as np

NB = 64
SHAPES = (1, 2, 63, 64, 65, 127, 128, 130, 200)
NAMES = tuple('n%d' % n for n in SHAPES) + ('ev30',)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
U = 1.1e-16
_cache = {}


def tolerance(N, cond):
    """the c n cond(J) u bound of docs/kernels_exact.md with c = 10"""
    return 10 * max(N, 1) * cond * U


def _unary(rng, P):
    kind = int(rng.integers(0, 3))
    d = float(rng.uniform(2.0, 3.0))                     # contribution to the diagonal of J
    if kind == 0:
        return P.X2Potential(d, 1.0)
    if kind == 1:
        return P.GaussianPotential([float(rng.normal())], [[1.0 / d]])
    return P.QuadraticPotential(np.array([[-d / 2]]), np.array([float(rng.normal())]), float(rng.normal()))


def _pair(rng, P):
    kind = int(rng.integers(0, 4))
    o = float(rng.uniform(0.1, 0.35)) * (1 if rng.random() < 0.5 else -1)      # off-diagonal of J
    if kind == 0:        # J = [[a^2, -a], [-a, 1]] / sig
        a = float(rng.uniform(0.5, 1.0)) * np.sign(o)
        return P.LinearGaussianPotential(a, abs(a / o))
    if kind == 1:        # J = [[0, c/2s], [c/2s, 0]]
        return P.XYPotential(2 * o, 1.0)
    prec = np.array([[abs(o) + float(rng.uniform(0.05, 0.3)), o], [o, abs(o) + float(rng.uniform(0.05, 0.3))]])
    if kind == 2:
        return P.GaussianPotential([float(rng.normal()), float(rng.normal())], np.linalg.inv(prec).tolist())
    return P.QuadraticPotential(-0.5 * prec, rng.normal(size=2), float(rng.normal()))


def build(name):
    """(graph, rvs) of lhvi objects; cached (the graphs are not modified by the tests)"""
    if name in _cache:
        return _cache[name]
    from lhvi import potentials as P
    from lhvi.graph import Domain, F, Graph, RV
    if name == 'indefinite':
        N, seed, share = 130, 7, 0.0
    elif name == 'ev30':
        N, seed, share = 150, 11, 0.3
    else:
        N, seed, share = int(name[1:]), 100 + int(name[1:]), 0.0
    rng = np.random.default_rng(seed)
    d = Domain((-20, 20), continuous=True, integral_points=np.linspace(-20, 20, 30))
    rvs = [RV(d) for _ in range(N)]
    fs = [F(_unary(rng, P), [rv]) for rv in rvs]
    deg = np.zeros(N, dtype=int)
    for i in range(N):
        for _ in range(2):
            j = int(rng.integers(0, N))
            if j == i or deg[i] >= 4 or deg[j] >= 4:
                continue
            deg[i] += 1
            deg[j] += 1
            fs.append(F(_pair(rng, P), [rvs[i], rvs[j]] if rng.random() < 0.5 else [rvs[j], rvs[i]]))
    if name == 'indefinite':
        fs.append(F(P.QuadraticPotential(np.array([[0.0, -10.0], [-10.0, 0.0]]), np.zeros(2), 0.0), [rvs[70], rvs[71]]))
    if share:
        for i in rng.choice(N, int(N * share), replace=False):
            rvs[int(i)].value = float(rng.uniform(-3, 3))
    g = Graph()
    g.rvs, g.factors = rvs, fs
    g.init_nb()
    _cache[name] = (g, rvs)
    return g, rvs


def conditional_quadratic(A, b, c, obs):
    """osi/utils.py:249-276 restated"""
    n = len(b)
    yi = np.array(sorted(obs), dtype=int)
    y = np.array([obs[i] for i in yi], dtype=np.float64)
    xi = np.array([i for i in range(n) if i not in obs], dtype=int)
    bc = A[np.ix_(xi, yi)] @ y + A[np.ix_(yi, xi)].T @ y + b[xi]
    cc = np.dot(y, A[np.ix_(yi, yi)] @ y) + np.dot(b[yi], y) + c
    return A[np.ix_(xi, xi)], bc, cc


def reference_route(g, rvs):
    """the reference's three calls in NumPy: dict with hidden (positions in rvs), A, b, c (conditioned, non-empty factors, the
    reference's summation order), const (fully observed factors), J, and, when J is positive definite, mu, Sig, logdet, cond"""
    key = ('route', id(g))
    if key in _cache:
        return _cache[key]
    hidden = [i for i, rv in enumerate(rvs) if rv.value is None]
    pos = {rvs[i]: k for k, i in enumerate(hidden)}
    N = len(hidden)
    A, b, c, const = np.zeros((N, N)), np.zeros(N), 0, 0.0
    for f in g.factors_list:
        A_, b_, c_ = f.potential.get_quadratic_params()
        A_, b_ = np.asarray(A_, dtype=np.float64), np.asarray(b_, dtype=np.float64)
        obs = {i: float(rv.value) for i, rv in enumerate(f.nb) if rv.value is not None}
        if obs:
            A_, b_, c_ = conditional_quadratic(A_, b_, c_, obs)
        scope = [pos[rv] for rv in f.nb if rv.value is None]
        if not scope:
            const += float(c_)
            continue
        for i in range(len(scope)):
            for j in range(len(scope)):
                A[scope[i], scope[j]] += A_[i, j]
            b[scope[i]] += b_[i]
        c += c_
    J = -2.0 * A
    out = dict(hidden=hidden, A=A, b=b, c=c, const=const, J=J)
    eig = np.linalg.eigvalsh(J) if N else np.ones(1)
    if eig[0] > 0:
        Sig = np.linalg.inv(J) if N else np.zeros((0, 0))
        mu = Sig @ b
        logdet = float(np.linalg.slogdet(J)[1]) if N else 0.0
        out.update(mu=mu, Sig=Sig, logdet=logdet, cond=float(eig[-1] / eig[0]),
                   logZ=N / 2 * np.log(2 * np.pi) - 0.5 * logdet + 0.5 * float(mu @ b) + float(c) + const)
    _cache[key] = out
    return out


def first_bad_pivot(J):
    """the column at which an unblocked Cholesky of J meets its first pivot <= 0"""
    L = np.array(J, dtype=np.float64)
    n = L.shape[0]
    for j in range(n):
        d = L[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            return j
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (L[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return -1


def report(what, err, bound):
    print('%-40s max err %.3e   bound %.3e' % (what, err, bound))
    return err, bound


def check_moments(what, N, cond, mu, var, logdet, ref_mu, ref_var, ref_logdet):
    """means: max |d mu| <= tol max(1, max |mu_ref|); variances and log det J: per entry relative"""
    tol = tolerance(N, cond)
    if N:
        e, bnd = report(what + ' mu', float(np.abs(mu - ref_mu).max()), tol * max(1.0, float(np.abs(ref_mu).max())))
        assert e <= bnd
        e, bnd = report(what + ' var (rel)', float(np.abs(var / ref_var - 1).max()), tol)
        assert e <= bnd
    e, bnd = report(what + ' log det J (rel)', abs(logdet - ref_logdet) / max(abs(ref_logdet), 1e-300) if ref_logdet else abs(logdet), tol)
    assert e <= bnd


def load_fixture(i):
    """gauss_exact_rgm{i}.npz with the keys parsed: evidence dict, hidden key list"""
    key = ('fixture', i)
    if key not in _cache:
        z = np.load(os.path.join(GOLDEN, 'gauss_exact_rgm%d.npz' % i))
        fx = {k: z[k] for k in z.files}
        fx['evidence'] = {ast.literal_eval(str(k)): float(v) for k, v in zip(fx['ev_keys'], fx['ev_vals'])}
        fx['hidden'] = [ast.literal_eval(str(k)) for k in fx['hidden_keys']]
        _cache[key] = fx
    return _cache[key]


def rgm_solver(i):
    """(ExactGaussian on generators.rgm() with the fixture's evidence through ground_flat, variable index of every recorded
    hidden key, fixture); cached"""
    key = ('rgm', i)
    if key not in _cache:
        from lhvi import generators
        from lhvi.gauss_exact import ExactGaussian
        fx = load_fixture(i)
        flat, keys = generators.rgm().ground_flat(fx['evidence'])
        vid = np.array([keys.var_id(k) for k in fx['hidden']], dtype=np.int64)
        _cache[key] = (ExactGaussian(flat), vid, fx)
    return _cache[key]
