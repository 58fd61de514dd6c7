"""Models of the flat-graph Gibbs sampler's tests (lhvi/fgibbs.py, csrc/fgibbs.hpp) and the NumPy restatement of its schedule.

The restatement runs one chain in the sequential order (colour 0, 1, ...; ascending ids within a colour) from injected
uniforms, evaluates every potential through the Python classes' ``get`` (never through the device evaluator) and asserts its own
margins: every accept test ``g(x1) >= y`` is decided by at least MARGIN, every discrete uniform is at least MARGIN away from
every cumulative sum it is compared with, and no row of log masses is all -inf unless the model says so (``stuck_ok``).  The
seeds below were picked on the CPU so that the restatement alone passes these asserts on every model."""
import math
import types

import numpy as np

from lhvi.flat import flatten
from lhvi.graph import F, RV, Domain, Graph
from lhvi.mln import MLNHardPotential, MLNPotential, eq_op
from lhvi.potentials import (GaussianPotential, HybridQuadraticPotential, ImageEdgePotential, ImageNodePotential,
                             LinearGaussianPotential, QuadraticPotential, TablePotential, X2Potential, XYPotential)

MARGIN = 1e-9
CHAINS, ITERS = 4, 6
DET_MODELS = ('kinds', 'wide', 'hub', 'hard_stuck', 'cap', 'isolated')
# per model: seed of the injected draws (picked so that the restatement's margins hold), max_shrink
SEEDS = {'kinds': 11, 'wide': 12, 'hub': 13, 'hard_stuck': 14, 'cap': 15, 'isolated': 16}
MAX_SHRINK = {'kinds': 24, 'wide': 24, 'hub': 24, 'hard_stuck': 24, 'cap': 2, 'isolated': 24}


def _graph(rvs, factors):
    g = Graph()
    g.rvs, g.factors = list(rvs), list(factors)
    g.init_nb()
    return g


def _model(rvs, factors, init=None, stuck_ok=False):
    g = _graph(rvs, factors)
    return types.SimpleNamespace(g=g, rvs=list(rvs), factors=list(factors), flat=flatten(g, require_device_potentials=True),
                                 init=init, stuck_ok=stuck_ok)


def kinds():
    """one factor of every potential kind the flattener emits"""
    b2, b3 = Domain((0, 1)), Domain((0, 1, 2))
    dc = Domain((-4, 4), continuous=True)
    dp = Domain((0, 1), continuous=True)
    d0, d1 = RV(b2), RV(b3)
    c0, c1, c2, c3 = RV(dc), RV(dc), RV(dc), RV(dc)
    p0, p1 = RV(dp), RV(dp)
    pix = RV(dp, value=0.35)
    A = -np.array([[[0.6, 0.1], [0.1, 0.4]], [[0.3, -0.1], [-0.1, 0.7]]])
    fs = [F(TablePotential(np.array([[0.7, 1.3, 0.4], [1.1, 0.2, 0.9]])), nb=[d0, d1]),
          F(GaussianPotential([0.5, -0.3], [[1.2, 0.4], [0.4, 0.9]]), nb=[c0, c1]),
          F(QuadraticPotential(np.array([[-0.4]]), np.array([0.3]), 0.1), nb=[c1]),
          F(HybridQuadraticPotential(A, np.array([[0.5, -0.2], [-0.4, 0.3]]), np.array([0.1, -0.2])), nb=[d0, c0, c2]),
          F(LinearGaussianPotential(0.8, 1.5), nb=[c2, c3]),
          F(X2Potential(0.7, 1.1), nb=[c3]),
          F(XYPotential(0.5, 1.3), nb=[c0, c3]),
          F(MLNPotential(lambda x: x[0] * eq_op(x[1], x[2]), w=0.5), nb=[d0, c1, c2]),
          F(MLNPotential(lambda x: -abs(x[0] - x[1]) * (1 + x[2]), w=0.7), nb=[c2, c3, d1]),
          F(ImageNodePotential(0, 0.2), nb=[p0, pix]),
          F(ImageEdgePotential(0.3, 0.25, 0.5), nb=[p0, p1])]
    return _model([d0, d1, c0, c1, c2, c3, p0, p1, pix], fs)


def wide():
    """a 9-state hidden variable, an arity-6 factor, observed neighbours of both kinds"""
    rng = np.random.RandomState(3)
    b9, b2, b3 = Domain(tuple(range(9))), Domain((0, 1)), Domain((0, 1, 2))
    dc = Domain((-3, 3), continuous=True)
    w, a, b, t = RV(b9), RV(b2), RV(b2), RV(b3)
    ob, ot = RV(b2, value=1), RV(b3, value=2)
    c, oc = RV(dc), RV(dc, value=0.8)
    fs = [F(TablePotential(rng.uniform(0.2, 1.5, (9, 2, 2, 3, 2, 3))), nb=[w, a, b, t, ob, ot]),
          F(TablePotential(rng.uniform(0.2, 1.5, (9,))), nb=[w]),
          F(HybridQuadraticPotential(-rng.uniform(0.2, 1.0, (9, 1, 1)), rng.randn(9, 1), 0.3 * rng.randn(9)), nb=[w, c]),
          F(GaussianPotential([0., 0.], [[1., 0.5], [0.5, 1.]]), nb=[c, oc]),
          F(MLNPotential(lambda x: x[0] * eq_op(x[1], x[2]), w=0.8), nb=[ob, c, oc]),
          F(TablePotential(rng.uniform(0.2, 1.5, (3, 2))), nb=[t, a])]
    return _model([w, a, b, t, ob, ot, c, oc], fs)


def hub():
    """a continuous and a 3-state variable of degree 70 each: the second trip of the hub kernel's 64-lane stride"""
    rng = np.random.RandomState(5)
    b2, b3 = Domain((0, 1)), Domain((0, 1, 2))
    dc = Domain((-3, 3), continuous=True)
    hc, hd = RV(dc), RV(b3)
    c1, c2, oc = RV(dc), RV(dc), RV(dc, value=-0.4)
    a, ob = RV(b2), RV(b2, value=1)
    fs = []
    for i in range(70):
        k = i % 5
        if k == 0:
            fs.append(F(LinearGaussianPotential(rng.uniform(-1, 1), rng.uniform(20, 60)), nb=[hc, c1]))
        elif k == 1:
            fs.append(F(LinearGaussianPotential(rng.uniform(-1, 1), rng.uniform(20, 60)), nb=[c2, hc]))
        elif k == 2:
            fs.append(F(MLNPotential(lambda x: x[0] * eq_op(x[1], x[2]), w=rng.uniform(0.01, 0.05)), nb=[a, hc, oc]))
        elif k == 3:
            fs.append(F(X2Potential(rng.uniform(0.5, 1.5), rng.uniform(20, 60)), nb=[hc]))
        else:
            fs.append(F(MLNPotential(lambda x: -abs(x[0] - x[1]), w=rng.uniform(0.01, 0.05)), nb=[hc, c1]))
    for i in range(70):
        k = i % 3
        if k == 0:
            fs.append(F(TablePotential(rng.uniform(0.8, 1.25, (3, 2))), nb=[hd, a]))
        elif k == 1:
            fs.append(F(HybridQuadraticPotential(-rng.uniform(0.005, 0.02, (3, 1, 1)), 0.05 * rng.randn(3, 1), 0.05 * rng.randn(3)),
                        nb=[hd, c2]))
        else:
            fs.append(F(TablePotential(rng.uniform(0.8, 1.25, (2, 3))), nb=[ob, hd]))
    fs.append(F(X2Potential(1.0, 2.0), nb=[c1]))
    fs.append(F(X2Potential(1.0, 2.0), nb=[c2]))
    return _model([hc, hd, c1, c2, oc, a, ob], fs)


def hard_stuck():
    """a hard formula that zeroes every state of `a` given the fixed start b = 0, and a continuous variable that starts where
    its hard factor is zero (the slice sampler leaves through the first proposal)"""
    b2 = Domain((0, 1))
    dc = Domain((0, 1), continuous=True)
    a, b, c = RV(b2), RV(b2), RV(dc)
    fs = [F(MLNHardPotential(lambda x: x[0] * x[1]), nb=[a, b]),
          F(MLNHardPotential(lambda x: x[0] > 0.5), nb=[c]),
          F(X2Potential(1.0, 1.0), nb=[c])]
    return _model([a, b, c], fs, init=np.array([1., 0., 0.2]), stuck_ok=True)


def isolated():
    """a hidden variable of each kind with no factor (and one factor elsewhere, so that the graph has a potential table)"""
    b3 = Domain((0, 1, 2))
    dc = Domain((-2, 5), continuous=True)
    a, c, other = RV(b3), RV(dc), RV(dc)
    return _model([a, c, other], [F(X2Potential(1.0, 1.0), nb=[other])])


def build(name):
    return {'kinds': kinds, 'wide': wide, 'hub': hub, 'hard_stuck': hard_stuck, 'cap': kinds, 'isolated': isolated}[name]()


def draws(name, model, chains=CHAINS, iters=ITERS):
    """(x0 [chains, V], u [iters, chains, V, 1 + max_shrink]) of the model's seed"""
    fl = model.flat
    rng = np.random.RandomState(SEEDS[name])
    ms = MAX_SHRINK[name]
    u = rng.rand(iters, chains, fl.V, 1 + ms)
    if model.init is not None:
        x0 = np.broadcast_to(model.init, (chains, fl.V)).copy()
    else:
        x0 = np.empty((chains, fl.V))
        for v in range(fl.V):
            d = fl.var_dom[v]
            if not np.isnan(fl.var_value[v]):
                x0[:, v] = fl.var_value[v]
            elif fl.dom_cont[d]:
                x0[:, v] = fl.dom_lo[d] + rng.rand(chains) * (fl.dom_hi[d] - fl.dom_lo[d])
            else:
                x0[:, v] = fl.dom_val[fl.dom_ptr[d] + rng.randint(0, fl.dom_ptr[d + 1] - fl.dom_ptr[d], chains)]
    return x0, u


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def schedule(model):
    """the sequential order: greedy colours in variable order, restated -- the smallest colour no earlier hidden variable
    sharing a factor holds; then colour by colour, ascending ids"""
    hidden = [rv.value is None for rv in model.rvs]
    index = {rv: i for i, rv in enumerate(model.rvs)}
    colour = [-1] * len(model.rvs)
    for i, rv in enumerate(model.rvs):
        if not hidden[i]:
            continue
        used = {colour[index[o]] for f in rv.nb for o in f.nb if o is not rv and hidden[index[o]]}
        c = 0
        while c in used:
            c += 1
        colour[i] = c
    order = sorted((c, i) for i, c in enumerate(colour) if c >= 0)
    return colour, [i for _, i in order]


def _arg(rv, value):
    return float(value) if rv.domain.continuous else int(value)


def cond_logp(model, x, v, t):
    """g_v(t) through the classes' get, factors in rv.nb order"""
    rv = model.rvs[v]
    index = model.index
    total = 0.0
    for f in rv.nb:
        args = tuple(_arg(o, t if o is rv else x[index[o]]) for o in f.nb)
        phi = float(f.potential.get(args))
        total += -math.inf if phi == 0 else math.log(phi)
    return total


def restate(model, x0, u, max_shrink, num_burnin=0, thin=1, num_samples=None):
    """one chain: x0 [V], u [iters, V, 1 + max_shrink].  Returns a namespace: x [iters, V] (the state after each iteration),
    stuck, capped, evals, closest (the smallest margin met)"""
    model.index = {rv: i for i, rv in enumerate(model.rvs)}
    _, order = schedule(model)
    x = np.array(x0, dtype=np.float64)
    out = np.empty((u.shape[0], x.size))
    stuck = capped = evals = 0
    closest = math.inf
    for it in range(u.shape[0]):
        for v in order:
            rv = model.rvs[v]
            if rv.domain.continuous:
                lo, hi = float(rv.domain.values[0]), float(rv.domain.values[1])
                x_old = x[v]
                y = cond_logp(model, x, v, x_old) + math.log(1.0 - u[it, v, 0])
                evals += 1
                L, R, got = lo, hi, False
                for k in range(1, max_shrink + 1):
                    x1 = L + u[it, v, k] * (R - L)
                    g1 = cond_logp(model, x, v, x1)
                    evals += 1
                    if not (math.isinf(y) and y < 0):
                        assert not math.isnan(g1)
                        m = math.inf if math.isinf(g1) else abs(g1 - y)
                        assert m >= MARGIN, 'accept test within %g' % m
                        closest = min(closest, m)
                    if g1 >= y:
                        x[v], got = x1, True
                        break
                    if x1 < x_old:
                        L = x1
                    else:
                        R = x1
                capped += 0 if got else 1
            else:
                states = rv.domain.values
                lp = [cond_logp(model, x, v, s) for s in states]
                evals += len(states)
                mx = max(lp)
                if mx == -math.inf:
                    assert model.stuck_ok, 'a row of log masses is all -inf'
                    stuck += 1
                    continue
                total = 0.0
                for a in lp:
                    total += math.exp(a - mx)
                scale = mx + math.log(total)
                cum, pick = 0.0, len(states) - 1
                for j, a in enumerate(lp[:-1]):          # (the last state is the pick whatever its comparison says)
                    cum += math.exp(a - scale)
                    m = abs(u[it, v, 0] - cum)
                    assert m >= MARGIN, 'uniform within %g of a cumulative sum' % m
                    closest = min(closest, m)
                    if u[it, v, 0] <= cum:
                        pick = j
                        break
                x[v] = states[pick]
        out[it] = x
    return types.SimpleNamespace(x=out, stuck=stuck, capped=capped, evals=evals, closest=closest)


def state_index(model, x):
    """idx [..., V] of values x [..., V]: the state index of a discrete variable, 0 of a continuous one"""
    idx = np.zeros(x.shape, dtype=np.int32)
    for v, rv in enumerate(model.rvs):
        if not rv.domain.continuous:
            idx[..., v] = np.searchsorted(np.asarray(rv.domain.values, dtype=np.float64), x[..., v])
    return idx


# ---- the Philox layout of the generator, restated (docs/kernels_fgibbs.md, "Random numbers") ------------------------------------------
TAG_SWEEP, TAG_INIT = 0x46475355, 0x46475849       # "FGSU", "FGXI"

def _philox(c, seed):
    c = [np.asarray(w, dtype=np.uint64) for w in c]
    k0, k1 = np.uint64(seed & 0xffffffff), np.uint64((seed >> 32) & 0xffffffff)
    m32 = np.uint64(0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return c


def _uniform2(seed, a, b, c, tag):
    w = _philox(np.broadcast_arrays(a, b, c, tag), seed)
    r0, r1 = (w[0] << np.uint64(32)) | w[1], (w[2] << np.uint64(32)) | w[3]
    return (r0 >> np.uint64(11)).astype(np.float64) / 9007199254740992.0, (r1 >> np.uint64(11)).astype(np.float64) / 9007199254740992.0


def philox_uniforms(seed, its, chains, V, max_shrink):
    """u [its, chains, V, 1 + max_shrink]: the sweep uniforms the generator draws, in the layout ``u=`` injects"""
    it, c, v, p = np.meshgrid(np.arange(its), np.arange(chains), np.arange(V), np.arange(max_shrink // 2 + 1), indexing='ij')
    u0, u1 = _uniform2(int(seed), c | (p << 24), it, v, TAG_SWEEP)
    return np.stack([u0, u1], axis=-1).reshape(its, chains, V, -1)[..., :1 + max_shrink].copy()


def philox_init(seed, chains, flat):
    """x [chains, V]: the initial state the generator draws (observed variables: their value)"""
    c, v = np.meshgrid(np.arange(chains), np.arange(flat.V), indexing='ij')
    u0, _ = _uniform2(int(seed), c, 0, v, TAG_INIT)
    d = flat.var_dom
    S = (flat.dom_ptr[1:] - flat.dom_ptr[:-1])[d]
    k = np.minimum((u0 * S[None, :]).astype(np.int64), S[None, :] - 1)
    disc = flat.dom_val[np.minimum(flat.dom_ptr[d][None, :] + k, max(flat.dom_val.size - 1, 0))] if flat.dom_val.size else u0
    cont = flat.dom_lo[d][None, :] + u0 * (flat.dom_hi[d] - flat.dom_lo[d])[None, :]
    x = np.where(flat.dom_cont[d].astype(bool)[None, :], cont, disc)
    return np.where(np.isnan(flat.var_value)[None, :], x, flat.var_value[None, :])


# ---- statistical models with a quadrature of their own ------------------------------------------------------------------------------
IMAGE_OBS = (0.2, 0.55, 0.7)
IMAGE_NODE, IMAGE_EDGE = (0.0, 0.15), (0.4, 0.2, 0.45)


def image():
    """three hidden pixels in a chain, each under an ImageNodePotential against its observed pixel, ImageEdgePotentials between"""
    dp = Domain((0, 1), continuous=True)
    y = [RV(dp) for _ in range(3)]
    o = [RV(dp, value=val) for val in IMAGE_OBS]
    node, edge = ImageNodePotential(*IMAGE_NODE), ImageEdgePotential(*IMAGE_EDGE)
    fs = [F(node, nb=[y[i], o[i]]) for i in range(3)] + [F(edge, nb=[y[0], y[1]]), F(edge, nb=[y[1], y[2]])]
    return _model(y + o, fs)


def image_quadrature(n):
    """E[y_i], E[y_i^2] of the three pixels by the midpoint rule on n points a pixel: the chain's forward / backward sums as
    n x n matrix products"""
    t = (np.arange(n) + 0.5) / n
    mu, sig = IMAGE_NODE
    dist, scale, thr = IMAGE_EDGE
    node = [np.exp(-0.5 * ((t - o - mu) / sig) ** 2) / (2.506628274631 * sig) for o in IMAGE_OBS]
    d = np.abs(t[:, None] - t[None, :])
    edge = d * dist + np.where(d > thr, math.exp(-thr / scale), np.exp(-d / scale))
    f1 = edge.T @ node[0]                   # sum over y0
    b1 = edge @ node[2]                     # sum over y2
    p = [node[0] * (edge @ (node[1] * b1)), node[1] * f1 * b1, node[2] * (edge.T @ (node[1] * f1))]
    p = [q / q.sum() for q in p]
    return np.array([q @ t for q in p]), np.array([q @ (t * t) for q in p])


ABS_W = (0.9, 0.6)
ABS_TABLE = (0.8, 1.3)


def abs_mln():
    """a binary d and two continuous a, b on (-3, 3): exp(-0.9 |a - b|), exp(0.6 d |a|) (neither has a conditional-quadratic
    view: the interpreter evaluates them), unary quadratics and a table on d"""
    b2 = Domain((0, 1))
    dc = Domain((-3, 3), continuous=True)
    d, a, b = RV(b2), RV(dc), RV(dc)
    fs = [F(MLNPotential(lambda x: -abs(x[0] - x[1]), w=ABS_W[0]), nb=[a, b]),
          F(MLNPotential(lambda x: x[0] * abs(x[1]), w=ABS_W[1]), nb=[d, a]),
          F(QuadraticPotential(np.array([[-0.5]]), np.array([0.4]), 0.0), nb=[a]),
          F(QuadraticPotential(np.array([[-0.3]]), np.array([-0.2]), 0.0), nb=[b]),
          F(TablePotential(np.array(ABS_TABLE)), nb=[d])]
    return _model([d, a, b], fs)


def abs_quadrature(n):
    """(p(d) [2], E[a], E[a^2], E[b], E[b^2]) by the midpoint rule on an n x n grid over (a, b), d summed"""
    t = -3 + 6 * (np.arange(n) + 0.5) / n
    a, b = t[:, None], t[None, :]
    base = np.exp(-ABS_W[0] * np.abs(a - b) + (-0.5 * a * a + 0.4 * a) + (-0.3 * b * b - 0.2 * b))
    pd = [ABS_TABLE[k] * base * np.exp(ABS_W[1] * k * np.abs(a)) for k in (0, 1)]
    Z = pd[0].sum() + pd[1].sum()
    joint = (pd[0] + pd[1]) / Z
    pa, pb = joint.sum(axis=1), joint.sum(axis=0)
    return np.array([pd[0].sum() / Z, pd[1].sum() / Z]), np.array([pa @ t, pb @ t]), np.array([pa @ (t * t), pb @ (t * t)])


def with_potentials(model):
    """a model of tests/exact_models.py (log_potential_fun on every factor) with the equal ``potential`` set on each factor, as a
    Graph in rvs order: what FlatGibbs flattens and ExactHybridGaussian reads alike"""
    from lhvi.potentials import LogHybridQuadratic, LogQuadratic, LogTable
    for f in model['factors']:
        lp = f.log_potential_fun
        if isinstance(lp, LogTable):
            f.potential = TablePotential(np.exp(np.asarray(lp.table, dtype=np.float64)))
        elif isinstance(lp, LogQuadratic):
            f.potential = QuadraticPotential(np.asarray(lp.A, dtype=np.float64), np.asarray(lp.b, dtype=np.float64), float(lp.c))
        elif isinstance(lp, LogHybridQuadratic):
            f.potential = HybridQuadraticPotential(lp.A, lp.b, lp.c)
        else:
            raise TypeError(type(lp).__name__)
        f.nb = list(f.nb)
    return _graph(model['rvs'], model['factors'])
