"""Models of the exact hybrid-Gaussian baseline tests, shared by scripts/capture_exact.py (built there from the reference's
classes) and the CPU / GPU tests (built from this package's).  ``ns`` is a namespace with the classes to build from:
F, RV, Domain, LogTable, LogQuadratic, LogHybridQuadratic, TablePotential, QuadraticPotential, HybridQuadraticPotential,
MLNPotential, eq_op, and_op.

``build(name, ns)`` returns a dict: rvs (all variables, discrete first), factors (in factor order, log_potential_fun set
unless the model is meant to be converted), Vd, Vc, evidence ({position in rvs: value}, not applied to the variables).
"""
import types

import numpy as np

NAMES = ('ref_hybrid2', 'ref_mln0', 'rand_3_2', 'rand_8_8', 'rand_12_16', 'rand_8_8_ev')
FULL = ('ref_hybrid2', 'ref_mln0', 'rand_3_2', 'rand_8_8', 'rand_8_8_ev')       # fixtures with every configuration recorded
RAND = {'rand_3_2': (3, 2, 1), 'rand_8_8': (8, 8, 1), 'rand_12_16': (12, 16, 1), 'rand_8_8_ev': (8, 8, 1)}
EVIDENCE_8_8 = {1: 1, 4: 0, 9: 0.75, 14: -1.5}          # two discrete (states), two continuous variables of rand_8_8
SAMPLED_CONFIGS = 512                                   # rows of rand_12_16 the fixture records (seeded)


def local_ns():
    """this package's classes"""
    from lhvi import graph, mln, potentials
    return types.SimpleNamespace(
        F=graph.F, RV=graph.RV, Domain=graph.Domain, Graph=graph.Graph, LogTable=potentials.LogTable,
        LogQuadratic=potentials.LogQuadratic, LogHybridQuadratic=potentials.LogHybridQuadratic,
        TablePotential=potentials.TablePotential, QuadraticPotential=potentials.QuadraticPotential,
        HybridQuadraticPotential=potentials.HybridQuadraticPotential, MLNPotential=mln.MLNPotential, eq_op=mln.eq_op,
        and_op=mln.and_op)


def _pack(rvs, factors, evidence=None):
    Vd = [rv for rv in rvs if rv.domain_type[0] == 'd']
    Vc = [rv for rv in rvs if rv.domain_type[0] == 'c']
    return dict(rvs=rvs, factors=factors, Vd=Vd, Vc=Vc, evidence=evidence or {})


def set_indices(model, hidden_only=False):
    """factor.disc_nb_idx / cont_nb_idx over the model's Vd / Vc (utils.set_nbrs_idx_in_factors)"""
    Vd_idx = {rv: i for i, rv in enumerate(model['Vd'])}
    Vc_idx = {rv: i for i, rv in enumerate(model['Vc'])}
    for f in model['factors']:
        f.disc_nb_idx = tuple(Vd_idx[rv] for rv in f.nb if rv.domain_type[0] == 'd')
        f.cont_nb_idx = tuple(Vc_idx[rv] for rv in f.nb if rv.domain_type[0] == 'c')
    return Vd_idx, Vc_idx


def ref_hybrid2(ns):
    """gibbs/test_hybrid2.py"""
    rvs = [ns.RV(domain=ns.Domain(values=(0, 1, 2), continuous=False)), ns.RV(domain=ns.Domain(values=(0, 1), continuous=False)),
           ns.RV(domain=ns.Domain(values=(-5, 5), continuous=True)), ns.RV(domain=ns.Domain(values=(-5, 5), continuous=True))]
    covs = np.array([np.eye(2)] * 3)
    means = np.array([[-2., -2.], [0., 1.], [3., 0.]])
    factors = [ns.F(nb=(rvs[0], rvs[2], rvs[3]),
                    log_potential_fun=ns.LogHybridQuadratic(A=-0.5 * covs, b=means,
                                                            c=-0.5 * np.array([np.dot(m, m) for m in means]))),
               ns.F(nb=(rvs[0],), log_potential_fun=ns.LogTable(np.array([-0.1, 0, 2.]))),
               ns.F(nb=(rvs[0], rvs[1]), log_potential_fun=ns.LogTable(np.array([[2., 0], [-0.1, 1], [0, 0.2]]))),
               ns.F(nb=(rvs[2],), log_potential_fun=ns.LogQuadratic(A=-0.5 * np.ones([1, 1]), b=np.zeros([1]), c=0.))]
    return _pack(rvs, factors)


def ref_mln0(ns, hand=False):
    """osi/hybrid_mln_test_0.py: with its MLN potentials (hand = False: the conversion is the code under test), or with the
    hand conversion of its lines 89-99 (hand = True: what the reference feeds its baseline)"""
    domain_bool = ns.Domain(values=(0, 1), continuous=False)
    domain_real = ns.Domain(values=(-10, 10), continuous=True)
    rvs = [ns.RV(domain=domain_bool), ns.RV(domain=domain_bool), ns.RV(domain=domain_real), ns.RV(domain=domain_real)]
    eq_op, and_op = ns.eq_op, ns.and_op
    factors = [ns.F(nb=(rvs[0], rvs[2], rvs[3]),
                    potential=ns.MLNPotential(lambda x: (1 - x[0]) * eq_op(x[1], 8.) + x[0] * eq_op(x[2], -7.), w=0.5)),
               ns.F(nb=(rvs[0], rvs[1]), potential=ns.MLNPotential(lambda x: and_op(x[0], x[1]), w=0.1)),
               ns.F(nb=(rvs[2], rvs[3]), potential=ns.QuadraticPotential(A=-0.5 * np.eye(2), b=np.array([1., 0.]), c=0.))]
    if hand:
        w = factors[0].potential.w
        factors[0].potential = ns.HybridQuadraticPotential(
            A=-w * np.array([np.array([[1., 0], [0, 0]]), np.array([[0., 0.], [0., 1.]])]),
            b=-w * np.array([[-16., 0], [0., 14.]]), c=-w * np.array([64., 49.]))
        pot = factors[1].potential
        table = np.empty([2, 2])
        for i in range(2):
            for j in range(2):
                table[i, j] = pot.get((i, j))
        factors[1].potential = ns.TablePotential(table, symmetric=bool(np.all(table == table.T)))
        for f in factors:
            f.log_potential_fun = f.potential.to_log_potential()
    return _pack(rvs, factors)


def rand_model(ns, Nd, Nc, seed):
    """seeded generator: Nd discrete variables (30 % ternary, else binary), Nc continuous on (-10, 10); a unary LogQuadratic
    with A = -(0.5 + U) on every continuous variable, 2 Nc pairwise -(w/2)(a x - y)^2, Nd hybrid factors with 1-2 discrete and
    1-2 continuous arguments and blocks -1/2 M M^T (M ~ 0.6 N(0, 1)), Nd log tables of arity 1-2"""
    rng = np.random.RandomState(seed)
    dom3, dom2 = ns.Domain(values=(0, 1, 2), continuous=False), ns.Domain(values=(0, 1), continuous=False)
    domc = ns.Domain(values=(-10, 10), continuous=True)
    Vd = [ns.RV(domain=dom3 if rng.rand() < 0.3 else dom2) for _ in range(Nd)]
    Vc = [ns.RV(domain=domc) for _ in range(Nc)]
    factors = []
    for rv in Vc:
        factors.append(ns.F(nb=(rv,), log_potential_fun=ns.LogQuadratic(A=-(0.5 + rng.rand(1, 1)), b=rng.randn(1), c=0.)))
    for _ in range(2 * Nc if Nc > 1 else 0):
        i, j = rng.choice(Nc, 2, replace=False)
        w, a = rng.uniform(0.2, 1.0), rng.randn()
        A = -(w / 2) * np.array([[a * a, -a], [-a, 1.]])
        factors.append(ns.F(nb=(Vc[i], Vc[j]), log_potential_fun=ns.LogQuadratic(A=A, b=np.zeros(2), c=0.)))
    for _ in range(Nd):
        ds = [Vd[i] for i in rng.choice(Nd, min(Nd, rng.randint(1, 3)), replace=False)]
        cs = [Vc[i] for i in rng.choice(Nc, min(Nc, rng.randint(1, 3)), replace=False)]
        dims, nc = [len(rv.domain.values) for rv in ds], len(cs)
        A = np.empty(dims + [nc, nc])
        for idx in np.ndindex(*dims):
            m = 0.6 * rng.randn(nc, nc)
            A[idx] = -0.5 * m @ m.T
        factors.append(ns.F(nb=tuple(ds + cs), log_potential_fun=ns.LogHybridQuadratic(A=A, b=rng.randn(*(dims + [nc])),
                                                                                      c=0.5 * rng.randn(*dims))))
    for _ in range(Nd):
        ds = [Vd[i] for i in rng.choice(Nd, min(Nd, rng.randint(1, 3)), replace=False)]
        factors.append(ns.F(nb=tuple(ds), log_potential_fun=ns.LogTable(rng.randn(*[len(rv.domain.values) for rv in ds]))))
    return _pack(Vd + Vc, factors)


# ---- shape models: explicit states, Nc and scopes (the CPU / GPU tests of the shapes the fixtures lack) ---------------------------
CDOM = (-10, 10)
SHAPES = ('wide_states', 'deep_scope', 'nc1', 'nc7', 'nc33', 'nc63', 'nc64')
# name: (seed, dstates, Nc, hybrid scopes (discrete, continuous), table scopes, quadratic scopes or 'dense', tables sharing the
# log potential of an earlier table {later: earlier})
SHAPE_SPECS = {
    # d > lanes at 4 and 8 lanes: a unary table on every variable, one 9 x 5 table, one hybrid factor on the 9-state variable
    'wide_states': (101, (9, 5, 2), 3, [((0,), (1,))], [(0,), (1,), (2,), (0, 1)], [(0,), (1,), (2,), (0, 1), (1, 2)], {}),
    # three strides in scope order (2, 0, 1) with three continuous arguments (12 local states), a table of arity 3 over
    # (3, 1, 0), variable 1 in the middle of a second hybrid scope, tables 2 and 3 sharing one log potential
    'deep_scope': (102, (2, 3, 2, 2), 4, [((2, 0, 1), (3, 0, 2)), ((3, 1, 0), (1,))], [(3, 1, 0), (1,), (0, 2), (3, 2)],
                   [(0,), (1,), (2,), (3,), (0, 1), (3, 2)], {3: 2}),
    'nc1': (103, (2,), 1, [((0,), (0,))], [(0,)], 'dense', {}),
    'nc7': (104, (3, 2), 7, [((0,), (6, 2)), ((1,), (3, 0))], [(1, 0)], 'dense', {}),
    'nc33': (105, (2, 3), 33, [((0,), (32, 5)), ((1,), (16, 31))], [(1, 0)], 'dense', {}),
    'nc63': (106, (2,), 63, [((0,), (62, 7))], [(0,)], 'dense', {}),
    'nc64': (107, (2, 3), 64, [((0,), (63, 11)), ((1,), (32, 0))], [(1, 0)], 'dense', {}),
    # the reduced table of one hybrid factor is 625 doubles a chain: more than a workgroup of 16 chains holds in LDS
    'scratch_tables': (108, (5, 5, 5, 5), 2, [((3, 0, 2, 1), (1, 0)), ((1,), (0,))], [(0, 2), (3,)], [(0,), (1,), (0, 1)], {}),
}


def shape_model(ns, seed, dstates, Nc, hybrids, tables, quads, share=None, cdom=CDOM):
    """seeded generator with a stream of its own (never rand_model's): discrete variable i has dstates[i] states; factors in
    the order quadratics, hybrids, tables, every scope as given (positions in Vd / Vc, any order).  quads = 'dense': one
    quadratic over all of Vc, -1/2 (B B^T + I) with B ~ N(0, 1 / Nc) (big_model of the GPU tests); else a list of scopes:
    arity 1 gives A = -(0.5 + U), arity 2 gives -(w / 2)(a x - y)^2.  A hybrid block is -1/2 m m^T with m ~ 0.5 N(0, 1), so
    every J is the base plus positive semi-definite terms.  share {j: i}: table j takes the log potential object of table i."""
    rng = np.random.RandomState(seed)
    Vd = [ns.RV(domain=ns.Domain(values=tuple(range(d)), continuous=False)) for d in dstates]
    Vc = [ns.RV(domain=ns.Domain(values=tuple(cdom), continuous=True)) for _ in range(Nc)]
    factors = []
    if quads == 'dense':
        B = rng.randn(Nc, Nc) / np.sqrt(Nc)
        factors.append(ns.F(nb=tuple(Vc), log_potential_fun=ns.LogQuadratic(A=-0.5 * (B @ B.T + np.eye(Nc)), b=rng.randn(Nc), c=0.)))
    else:
        for sc in quads:
            if len(sc) == 1:
                lp = ns.LogQuadratic(A=-(0.5 + rng.rand(1, 1)), b=rng.randn(1), c=0.)
            else:
                w, a = rng.uniform(0.2, 1.0), rng.randn()
                lp = ns.LogQuadratic(A=-(w / 2) * np.array([[a * a, -a], [-a, 1.]]), b=np.zeros(2), c=0.)
            factors.append(ns.F(nb=tuple(Vc[i] for i in sc), log_potential_fun=lp))
    for ds, cs in hybrids:
        dims, nc = [dstates[i] for i in ds], len(cs)
        A = np.empty(dims + [nc, nc])
        for idx in np.ndindex(*dims):
            m = 0.5 * rng.randn(nc, 1)
            A[idx] = -0.5 * m @ m.T
        lp = ns.LogHybridQuadratic(A=A, b=rng.randn(*(dims + [nc])), c=0.5 * rng.randn(*dims))
        factors.append(ns.F(nb=tuple([Vd[i] for i in ds] + [Vc[i] for i in cs]), log_potential_fun=lp))
    made = []
    for j, sc in enumerate(tables):
        lp = made[share[j]] if share and j in share else ns.LogTable(rng.randn(*[dstates[i] for i in sc]))
        made.append(lp)
        factors.append(ns.F(nb=tuple(Vd[i] for i in sc), log_potential_fun=lp))
    return _pack(Vd + Vc, factors)


def reduction_model(ns, dstates, seed=109, span=66., cdom=CDOM):
    """Nc = 1, for the reductions and the mixtures at large M: a unary table on every discrete variable, its entries spread over
    span / Nd (log p~ then spans about `span` over the configurations, centred on 0), and a hybrid factor (variable, x) on
    every variable that moves J within [1, 1.25] and the mean by a few tenths"""
    rng = np.random.RandomState(seed)
    n = len(dstates)
    Vd = [ns.RV(domain=ns.Domain(values=tuple(range(d)), continuous=False)) for d in dstates]
    x = ns.RV(domain=ns.Domain(values=tuple(cdom), continuous=True))
    factors = [ns.F(nb=(x,), log_potential_fun=ns.LogQuadratic(A=-0.5 * np.ones((1, 1)), b=rng.randn(1), c=0.))]
    for rv, d in zip(Vd, dstates):
        lp = ns.LogHybridQuadratic(A=-0.5 * (0.25 / n) * rng.rand(d, 1, 1), b=0.3 * rng.randn(d, 1), c=0.1 * rng.randn(d))
        factors.append(ns.F(nb=(rv, x), log_potential_fun=lp))
    for rv, d in zip(Vd, dstates):
        t = rng.rand(d)
        t = ((t - t.min()) / (t.max() - t.min()) - 0.5) * (span / n)
        factors.append(ns.F(nb=(rv,), log_potential_fun=ns.LogTable(t)))
    return _pack(Vd + [x], factors)


def numpy_config(factors, dstates, Nc, config):
    """convert_to_bn's loop body (:30-65) restated on this package's classes: (log p~, mu, Sig)"""
    from lhvi.potentials import LogQuadratic, LogTable
    A, b, c, t = np.zeros((Nc, Nc)), np.zeros(Nc), 0.0, 0.0
    for f in factors:
        lp = f.log_potential_fun
        xd = tuple(config[i] for i in f.disc_nb_idx)
        if isinstance(lp, LogTable):
            t += lp(xd)
            continue
        A_, b_, c_ = (lp.A, lp.b, lp.c) if isinstance(lp, LogQuadratic) else lp.get_quadratic_params_given_x_d(xd)
        sc = f.cont_nb_idx
        for i in range(len(sc)):
            for j in range(len(sc)):
                A[sc[i], sc[j]] += A_[i, j]
            b[sc[i]] += b_[i]
        c += c_
    Sig = np.linalg.inv(-2. * A)
    mu = Sig @ b
    return t + (Nc / 2 * np.log(2 * np.pi) + 0.5 * np.linalg.slogdet(Sig)[1] + 0.5 * mu @ b + c), mu, Sig


def enumerate_numpy(model):
    """numpy_config over every configuration of a model with its indices set: (logp [M], mu [M, Nc], Sig [M, Nc, Nc],
    largest cond(J))"""
    dstates, Nc = [rv.dstates for rv in model['Vd']], len(model['Vc'])
    M = int(np.prod(dstates))
    logp, mu, sig, cond = np.zeros(M), np.zeros((M, Nc)), np.zeros((M, Nc, Nc)), 0.0
    for cfg in range(M):
        logp[cfg], mu[cfg], sig[cfg] = numpy_config(model['factors'], dstates, Nc, np.unravel_index(cfg, dstates))
        cond = max(cond, np.linalg.cond(sig[cfg]))
    return logp, mu, sig, cond


def build(name, ns=None, **kw):
    ns = ns or local_ns()
    if name in SHAPE_SPECS:
        seed, dstates, Nc, hybrids, tables, quads, share = SHAPE_SPECS[name]
        return shape_model(ns, seed, list(dstates), Nc, hybrids, tables, quads, share, **kw)
    if name == 'ref_hybrid2':
        return ref_hybrid2(ns)
    if name == 'ref_mln0':
        return ref_mln0(ns, **kw)
    model = rand_model(ns, *RAND[name])
    if name == 'rand_8_8_ev':
        model['evidence'] = dict(EVIDENCE_8_8)
    return model


def sampled_configs(M):
    """the configurations of rand_12_16 the fixture records"""
    return np.sort(np.random.RandomState(12).choice(M, SAMPLED_CONFIGS, replace=False))


def query_points(rv, m=9):
    """belief query points of a continuous variable"""
    lo, hi = float(rv.domain.values[0]), float(rv.domain.values[1])
    return np.linspace(lo + 0.05 * (hi - lo), hi - 0.05 * (hi - lo), m)


# ---- shared by the CPU and GPU tests ---------------------------------------------------------------------------------------------
def load_golden(name):
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'exact_%s.npz' % name)
    return dict(np.load(path))


def solver(name):
    """(model, ExactHybridGaussian over it): the evidence applied to the variables, MLN potentials left to the conversion"""
    from lhvi.exact import ExactHybridGaussian
    model = build(name)
    for p, v in model['evidence'].items():
        model['rvs'][p].value = v
    return model, ExactHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc'])


def assert_log_close(got, want, rtol=1e-10, what=''):
    """log quantities: relative to max(1, |value|)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    assert err.max() <= rtol, '%s: max error %.3g relative to max(1, |value|)' % (what, err.max())


def tril(covs):
    i, j = np.tril_indices(covs.shape[-1])
    return covs[..., i, j]
