"""Shapes of the variational expectation step (csrc/vi.hip, ``lhvi_vi_grad``) beyond K = 2, T = 5, arity 3: a wide random
generator, constructed graphs whose factors sit on the thresholds of the host split (``lhvi/vi.py::factor_lists``), and a plain
NumPy reference of the step in ``np.longdouble``.  No test functions: tests/test_vi_shapes_host.py (CPU) and
tests/test_gpu_vi_shapes.py (MI355X) use it, and tests/soak/soak_vi_random.py with its third argument."""
import itertools

import numpy as np

CC, TINY, GRP3, GRP6, REST3, REST6 = range(6)
SEGMENTS = ('cc', 'tiny', 'grp3', 'grp6', 'rest3', 'rest6')
MAX_NODES = 4096                 # grid nodes of one factor: six four-state axes, the largest grid the group kernel takes
TABLE_WORDS = {'slim': (0, 1024), 'mid': (1024, 3072), 'large': (3072, 1 << 30)}     # (above, up to): VI_TINY_PAR_SLIM, VI_TINY_PAR


# ---- graphs on arrays -------------------------------------------------------------------------------------------------------
class Builder:
    """a ground factor graph put together variable by variable and factor by factor, then handed to ``flat.build_flat``: unlike
    ``flatten`` that keeps a scope which names a variable twice.  ``flat.potentials[flat.fac_pot[f]]`` is factor f's potential
    object (the longdouble reference evaluates through it), ``names`` maps the label of a constructed factor to its id"""

    def __init__(self):
        self.domains, self.var_dom, self.var_value, self.obs_var, self.factors, self.names = [], [], [], [], [], {}

    def var(self, domain, value=None, obs_var=0.0):
        if not any(domain is d for d in self.domains):
            self.domains.append(domain)
        self.var_dom.append([i for i, d in enumerate(self.domains) if d is domain][0])
        self.var_value.append(np.nan if value is None else float(value))
        self.obs_var.append(float(obs_var))
        return len(self.var_dom) - 1

    def fac(self, pot, scope, name=None):
        if name is not None:
            assert name not in self.names
            self.names[name] = len(self.factors)
        self.factors.append((pot, [int(v) for v in scope]))
        return len(self.factors) - 1

    def flat(self):
        """(FlatGraph, obs_var): potential rows are shared like ``flatten`` shares them, by (potential object, domains of the scope)"""
        from lhvi.flat import build_flat
        rows, pots, index, fac_pot = [], [], {}, []
        for pot, scope in self.factors:
            key = (id(pot),) + tuple(self.var_dom[v] for v in scope)
            if key not in index:
                index[key] = len(rows)
                rows.append(pot.device_spec(tuple(self.domains[self.var_dom[v]] for v in scope)))
                pots.append(pot)
            fac_pot.append(index[key])
        fac_ptr = np.concatenate([[0], np.cumsum([len(s) for _, s in self.factors])])
        edge_var = np.array([v for _, s in self.factors for v in s], dtype=np.int32)
        assert np.bincount(edge_var, minlength=len(self.var_dom)).min() > 0, 'a variable without a factor'
        flat = build_flat(fac_ptr, edge_var, fac_pot, rows, np.array(self.var_value), np.array(self.var_dom, dtype=np.int32),
                          self.domains)
        flat.potentials = pots
        return flat, np.array(self.obs_var)


def domains():
    """(the discrete domains of 2, 3, 4, 5, 8 and 32 states by their size, the continuous domain)"""
    from lhvi.graph import Domain
    disc = {2: Domain((0, 1)), 3: Domain((0, 1, 2)), 4: Domain((1, 2, 3, 5)), 5: Domain((0, 1, 2, 3, 4)), 8: Domain(tuple(range(8))),
            32: Domain(tuple(range(32)))}
    return disc, Domain((-10, 10), continuous=True, integral_points=np.linspace(-10, 10, 9))


_COEF = (1.0, -1.0, 0.5, -0.5, 0.25, 1.0)


def formulas():
    """MLN formulas written for any arity, bounded on the grids of these graphs (|x| < 10): with |w| <= 2, |w * formula| < 400"""
    from lhvi import mln as M
    return {'lin': lambda x: -0.05 * sum(_COEF[i] * x[i] for i in range(len(x))) ** 2,
            'abs': lambda x: -0.3 * abs(x[0] - 0.5 * x[-1] - 1),
            'eq': lambda x: 0.2 * M.eq_op(x[0], x[-1] - 1),
            'or': lambda x: M.or_op(M.neg_op(x[0] > 0), M.neg_op(x[-1] <= 1))}


def device_words(flat, obs_var):
    from lhvi import _abi
    return int(_abi.device_potentials(flat, obs_var)[1].size)


def wide_graph(rng, T, n_rv=60, n_f=160, one_discrete_domain=False, table_words='large', n_repeat=0):
    """a random hybrid graph like test_gpu_vi.py::_random_hybrid_graph, wider: factors of arity 1-6; discrete domains of 2, 3, 4, 5
    and 8 states (`one_discrete_domain`: a single one, which the reference's quirk 10 needs); evidence on ~28 % of the variables,
    every other observed continuous one a Gaussian observation; MLN formulas of any arity, dict-keyed tables over same-domain
    scopes of arity <= 3, the three pair potentials over continuous pairs.  A factor's grid at `T` quadrature points has at most
    MAX_NODES nodes.  `table_words` ('slim' / 'mid' / 'large'): the device's parameter table is at most VI_TINY_PAR_SLIM words
    and holds no formula to interpret / lies between that and VI_TINY_PAR / is larger -- by the number of templates (formula,
    weight, domains of the scope) and the size of the largest domain.  `n_repeat`: that many factors name a variable twice.
    Returns (FlatGraph, obs_var)."""
    from lhvi import mln as M, potentials as P
    disc, dc = domains()
    sizes, n_templates, forms = {'slim': ((2, 3), 40, ('lin', 'eq')), 'mid': ((2, 3, 4), 60, ('lin', 'abs', 'eq', 'or')),
                                 'large': ((2, 3, 4, 5, 8), 70, ('lin', 'abs', 'eq', 'or'))}[table_words]
    if one_discrete_domain:
        sizes = sizes[-1:]
    pool = [disc[s] for s in sizes] + [dc] * max(2, len(sizes) * 2 // 3)
    b = Builder()
    by_dom = {}
    for i in range(n_rv):
        dom = pool[i % len(pool)]
        val, ov = None, 0.0
        if rng.random() < 0.28:
            val = float(np.round(rng.uniform(-3, 3), 2)) if dom.continuous else dom.values[rng.integers(len(dom.values))]
            if dom.continuous and len(by_dom.get(id(dom), [])) % 2:
                ov = float(rng.uniform(0.3, 1.5))
        by_dom.setdefault(id(dom), []).append(b.var(dom, val, ov))
    fs = formulas()
    pair_pots = [P.GaussianPotential([0.0, 0.0], [[2.0, 0.6], [0.6, 1.5]]), P.LinearGaussianPotential(0.8, 1.3), P.XYPotential(0.7, 2.0)]
    templates = [(p, (dc, dc)) for p in pair_pots]
    for s in sizes:                                        # dict-keyed tables over one domain, arity 1..3
        for a in (1, 2, 3):
            if table_words == 'slim' and len(disc[s].values) ** a > 30:
                continue
            table = {vals: float(rng.uniform(0.2, 2.0)) for vals in itertools.product(*[disc[s].values] * a)}
            templates.append((P.TablePotential(table), (disc[s],) * a))
    doms = [disc[s] for s in sizes] + [dc]
    row_words = lambda row: 3 + len(row) - int(row[2]) if row[2] else len(row)          # what _abi.device_potentials ships of it
    budget, row_max = {'slim': (800, 150), 'mid': (2000, 500), 'large': (1 << 30, 1 << 30)}[table_words]
    words = sum(len(p.device_spec(sig)[1]) for p, sig in templates)
    while len(templates) < n_templates and words < budget:
        a = int(rng.integers(1, 7))
        sig = tuple(doms[rng.integers(len(doms))] for _ in range(a))
        pot = M.MLNPotential(fs[forms[rng.integers(len(forms))]], w=float(np.round(rng.uniform(-1, 2), 2)))
        row = pot.device_spec(sig)[1]
        if row_words(row) > row_max or (table_words == 'slim' and row[2] == 0):
            continue                                       # (slim: no formula without a conditional-quadratic view, which the device would interpret)
        templates.append((pot, sig))
        words += row_words(row)
    value, ovar = np.array(b.var_value), np.array(b.obs_var)
    n_axis = lambda v: T if (np.isnan(value[v]) and b.domains[b.var_dom[v]].continuous) or ovar[v] > 0 else \
        (len(b.domains[b.var_dom[v]].values) if np.isnan(value[v]) else 1)
    used = np.zeros(n_rv, dtype=bool)
    pending = list(range(len(templates)))              # every template once (where its grid fits), then at random
    while len(b.factors) < n_f or not used.all():
        pot, sig = templates[pending.pop(0) if pending else rng.integers(len(templates))]
        for attempt in range(40):
            scope, taken = [], set()
            for d in sig:
                free = [v for v in by_dom[id(d)] if v not in taken]
                if len(b.factors) >= n_f:                  # (past the count: only to give every variable a factor)
                    free = [v for v in free if not used[v]] or free
                if not free:                               # (a small graph: fewer variables of this domain than the template names)
                    break
                scope.append(free[rng.integers(len(free))])
                taken.add(scope[-1])
            if len(scope) < len(sig):
                continue
            twice = [(i, j) for i in range(len(sig)) for j in range(i + 1, len(sig)) if sig[i] is sig[j] and np.isnan(value[scope[i]])]
            if twice and pot.__class__ is M.MLNPotential and sum(len(set(s)) < len(s) for _, s in b.factors) < n_repeat:
                scope[twice[0][1]] = scope[twice[0][0]]
            if np.prod([float(n_axis(v)) for v in scope]) <= MAX_NODES:
                break
        else:
            continue
        used[scope] = True
        b.fac(pot, scope)
    flat, obs_var = b.flat()
    lo, hi = TABLE_WORDS[table_words]
    words = device_words(flat, obs_var)
    assert lo < words <= hi, 'the parameter table has %d words, %s asks for (%d, %d]' % (words, table_words, lo, hi)
    assert sum(len(set(s)) < len(s) for _, s in b.factors) == n_repeat
    return flat, obs_var


def random_params(rng, flat, K):
    """(w_tau, eta_c, tau_d) drawn like test_gpu_vi.py::_random_hybrid_check draws them"""
    disc = flat.var_hidden & ~flat.var_cont
    Dmax = int(flat.var_nstates[disc].max()) if disc.any() else 1
    w_tau = rng.normal(size=K)
    eta_c = np.ones((flat.V, K, 2))
    eta_c[:, :, 0] = rng.uniform(-1.5, 1.5, (flat.V, K))
    eta_c[:, :, 1] = rng.uniform(0.5, 3.0, (flat.V, K))
    return w_tau, eta_c, rng.uniform(0, 2, (flat.V, K, Dmax))


# ---- constructed graphs on the thresholds of factor_lists ------------------------------------------------------------------
def boundary_tiny_graph(table_words='slim'):
    """the thresholds of the thread-per-(factor, k) kernel, scopes that name a variable twice, stars around hidden hubs of degree
    64 and 65, pairwise continuous factors: (FlatGraph, obs_var, names, hubs).  `table_words` 'mid' adds two formulas over
    five-state scopes whose rows lift the parameter table over VI_TINY_PAR_SLIM.  Every formula has a conditional-quadratic view
    (nothing to interpret: at most VI_TINY_PAR_SLIM words take the slim build of the kernel)."""
    from lhvi import mln as M, potentials as P
    disc, dc = domains()
    fs = formulas()
    rng = np.random.default_rng(7)
    table = lambda *sizes: P.TablePotential({vals: float(rng.uniform(0.2, 2.0))
                                             for vals in itertools.product(*[disc[s].values for s in sizes])})
    b = Builder()
    # the node limit: 32 nodes on a unary factor (Dmax = 32 for the whole case) and on a 4 x 8 pair, against 5 x 8 = 40
    b.fac(table(32), [b.var(disc[32])], 'u32')
    b.fac(table(4, 8), [b.var(disc[4]), b.var(disc[8])], 'p32')
    b.fac(table(5, 8), [b.var(disc[5]), b.var(disc[8])], 'p40')
    # a variable twice in a scope: hidden continuous (arity 2 and 5), hidden discrete (arity 2, 3 and 5)
    lg = P.LinearGaussianPotential(0.8, 1.3)
    x, y, z, d = b.var(dc), b.var(disc[3]), b.var(disc[2]), b.var(disc[3])
    e = b.var(disc[2], 1)
    b.fac(lg, [x, x], 'r2c')
    b.fac(M.MLNPotential(fs['eq'], w=0.7), [y, y], 'r2d')
    b.fac(M.MLNPotential(fs['lin'], w=-0.6), [y, y, z], 'r3d')
    b.fac(M.MLNPotential(fs['lin'], w=0.9), [x, d, x, e, d], 'r5')
    # stars: a hidden three-state hub and a hidden continuous hub, each at degree 64 and 65; leaves alternate between hidden
    # binary and hidden continuous, the continuous hubs' continuous leaves make pairwise continuous factors (every third of those
    # observed, every sixth a Gaussian observation)
    gauss = P.GaussianPotential([0.0, 0.0], [[2.0, 0.6], [0.6, 1.5]])
    hub_d, hub_c = M.MLNPotential(fs['eq'], w=0.8), M.MLNPotential(fs['lin'], w=1.1)
    hubs = {}
    for kind, deg in (('d', 64), ('d', 65), ('c', 64), ('c', 65)):
        h = hubs[kind, deg] = b.var(disc[3] if kind == 'd' else dc)
        for i in range(deg):
            if i % 2:
                leaf = b.var(disc[2])
                b.fac(hub_d if kind == 'd' else hub_c, [h, leaf])
            else:
                leaf = b.var(dc, *((None, 0.0), (0.4 * (i % 5) - 1, 0.0), (None, 0.0), (0.25 * (i % 7), 0.6))[(i // 2) % 4] if kind == 'c' else ())
                b.fac(hub_d if kind == 'd' else (gauss, lg)[(i // 2) % 2], [leaf, h] if i % 4 else [h, leaf])
    if table_words == 'mid':
        a5 = [b.var(disc[5]) for _ in range(3)]
        b.fac(M.MLNPotential(fs['lin'], w=0.5), a5, 'pad0')
        b.fac(M.MLNPotential(fs['eq'], w=0.5), [a5[0], a5[1], b.var(disc[4])], 'pad1')
    flat, obs_var = b.flat()
    return flat, obs_var, b.names, hubs


# the segment of every named factor of boundary_tiny_graph() with tiny_kernel = 'always', per (K, T).  Axis lengths: u32 32;
# p32 4 + 8; p40 5 + 8; r2c T + T; r2d 3 + 3; r3d 3 + 3 + 2; r5 T + 3 + T + 1 + 3.  tiny: arity <= 3, <= 32 nodes, K <= 2.
# group: S <= 24 and K * S <= 48.
BOUNDARY_TINY_EXPECT = {
    (2, 1): dict(u32=TINY, p32=TINY, p40=GRP3, r2c=TINY, r2d=TINY, r3d=TINY, r5=GRP6),          # r5: S = 9
    (2, 4): dict(u32=TINY, p32=TINY, p40=GRP3, r2c=TINY, r2d=TINY, r3d=TINY, r5=GRP6),          # r2c: 16 nodes; r5: S = 15, 30 <= 48
    (1, 6): dict(u32=TINY, p32=TINY, p40=GRP3, r2c=GRP3, r2d=TINY, r3d=TINY, r5=GRP6),          # r2c: 36 nodes, S = 12; r5: S = 19
    (2, 9): dict(u32=TINY, p32=TINY, p40=GRP3, r2c=GRP3, r2d=TINY, r3d=TINY, r5=REST6),         # r2c: S = 18, 36 <= 48; r5: S = 25
    (3, 5): dict(u32=REST3, p32=GRP3, p40=GRP3, r2c=GRP3, r2d=GRP3, r3d=GRP3, r5=REST6),        # no tiny at K = 3; u32: S = 32; r5: 3 * 17
    (8, 3): dict(u32=REST3, p32=REST3, p40=REST3, r2c=GRP3, r2d=GRP3, r3d=REST3, r5=REST6),     # r2c, r2d: 8 * 6 = 48; r3d: 8 * 8
}


def boundary_group_graph(big=True):
    """the thresholds of the group kernel on hidden discrete scopes (their axis lengths do not depend on T), next to copies of the
    node-limit factors of boundary_tiny_graph(): the formulas over four and more discrete arguments take the parameter table past
    VI_TINY_PAR, so no factor may go to the thread-per-(factor, k) kernel.  `big` = False leaves out the two six-argument factors
    of the slot limit (4096 and 5120 nodes: at K = 16 and 24 a single thread of the thread-per-factor kernel would walk each of
    them for seconds, and what those K test are the short scopes).  (FlatGraph, obs_var, names)"""
    from lhvi import mln as M, potentials as P
    disc, dc = domains()
    fs = formulas()
    rng = np.random.default_rng(8)
    table = lambda *sizes: P.TablePotential({vals: float(rng.uniform(0.2, 2.0))
                                             for vals in itertools.product(*[disc[s].values for s in sizes])})
    b = Builder()
    hid = lambda *sizes: [b.var(disc[s]) for s in sizes]
    if big:
        b.fac(M.MLNPotential(fs['or'], w=0.8), hid(4, 4, 4, 4, 4, 4), 's24')       # slot limit: S = 24, 4096 nodes
        b.fac(M.MLNPotential(fs['lin'], w=0.4), hid(4, 4, 4, 4, 4, 5), 's25')
    b.fac(M.MLNPotential(fs['abs'], w=1.2), hid(4, 4, 4, 4), 's16')                # component limit at K = 3: 48 against 51
    b.fac(M.MLNPotential(fs['eq'], w=0.9), hid(4, 4, 4, 5), 's17')
    b.fac(table(8, 8), hid(8, 8), 't16')                                           # the same at arity <= 3
    b.fac(table(8, 5, 4), hid(8, 5, 4), 't17')
    b.fac(table(8, 8, 8), hid(8, 8, 8), 't24')                                     # S = 24 at arity 3
    b.fac(table(3), hid(3), 'u3')                                                  # K = 16: 48 against 64
    b.fac(table(4), hid(4), 'u4')
    o = [b.var(disc[2], 1), b.var(disc[3], 2), b.var(disc[2], 0)]
    b.fac(table(2, 3), o[:2], 'p2')                                                # K = 24: two observed arguments, 48 against 72
    b.fac(table(2, 2), [o[2]] + hid(2), 'p3')
    b.fac(table(32), hid(32), 'u32')                                               # 32 nodes, but S = 32 > 24 and no tiny kernel
    b.fac(table(4, 8), hid(4, 8), 'p32')
    b.fac(P.LinearGaussianPotential(0.8, 1.3), [b.var(dc), b.var(dc, 0.5)], 'cc')
    flat, obs_var = b.flat()
    return flat, obs_var, b.names


# S: s24 24, s25 25, s16 16, s17 17, t16 16, t17 17, t24 24, u3 3, u4 4, p2 2, p3 3, u32 32, p32 12; K <= 3 with `big`, K >= 16 without
BOUNDARY_GROUP_EXPECT = {
    (1, 3): dict(s24=GRP6, s25=REST6, s16=GRP6, s17=GRP6, t16=GRP3, t17=GRP3, t24=GRP3, u3=GRP3, u4=GRP3, p2=GRP3, p3=GRP3,
                 u32=REST3, p32=GRP3, cc=CC),
    (3, 5): dict(s24=REST6, s25=REST6, s16=GRP6, s17=REST6, t16=GRP3, t17=REST3, t24=REST3, u3=GRP3, u4=GRP3, p2=GRP3, p3=GRP3,
                 u32=REST3, p32=GRP3, cc=CC),
    (16, 6): dict(s16=REST6, s17=REST6, t16=REST3, t17=REST3, t24=REST3, u3=GRP3, u4=REST3, p2=GRP3,
                  p3=GRP3, u32=REST3, p32=REST3, cc=CC),
    (24, 9): dict(s16=REST6, s17=REST6, t16=REST3, t17=REST3, t24=REST3, u3=REST3, u4=REST3, p2=GRP3,
                  p3=REST3, u32=REST3, p32=REST3, cc=CC),
}


def segment_of(order, counts):
    """segment index of every factor from a factor list and its six segment lengths"""
    seg = np.empty(order.size, dtype=np.int64)
    seg[order] = np.repeat(np.arange(6), counts)
    return seg


# ---- the expectation step in np.longdouble ---------------------------------------------------------------------------------
LD = np.longdouble


def _phi(pot, cols):
    """potential values at the points whose coordinates are the columns `cols` (one longdouble array per argument), through the
    host classes' ``get``: formulas and the single-coefficient pair potentials take arrays as they are, a dict-keyed table is read
    point by point, the Gaussian's quadratic form is written out (its ``get`` rounds the arguments to float64)"""
    from lhvi import potentials as P
    if isinstance(pot, P.TablePotential):
        return np.array([pot.get(tuple(float(c[i]) for c in cols)) for i in range(cols[0].size)], dtype=LD)
    if isinstance(pot, P.GaussianPotential):
        d = [c - LD(m) for c, m in zip(cols, pot.mu)]
        prec = np.asarray(pot.prec)
        q = sum(d[i] * LD(prec[i, j]) * d[j] for i in range(len(d)) for j in range(len(d)))
        return np.exp(-q / 2)
    return np.asarray(pot.get(cols), dtype=LD) * np.ones(cols[0].size, dtype=LD)


def _pdf(x, mu, var):
    """VarInference.norm_pdf (VI:26-30): the normaliser is 2.5066 * var"""
    return np.exp(-(x - mu) ** 2 / 2 / var) / (LD('2.506628274631') * var)


def reference_grad(flat, K, T, w, eta_c, eta_d, obs_var):
    """(g_w, g_c, g_d, fe) of the expectation step with ``quirks = 0`` in np.longdouble, from the formulas of VarInference.py:57-195
    as oracle/c/vi_oracle.c's comments state them: F_f = log(phi_f + 1e-100) - log(b_f + 1e-100) on the tensor grid of the factor's
    axes (Gauss-Hermite nodes of a hidden continuous argument under component k or of a Gaussian observation, the states of a
    hidden discrete one weighted by eta, the value of plain evidence); per variable (N - 1) log b_v; E, E (x - mu), E ((x - mu)^2 -
    var) per continuous slot; per state of a hidden discrete slot (first position of its variable only) the expectation over
    the other slots; the two softmax projections.  The inputs are the step's own: mixture weights w [K], eta_c [V, K, 2], category
    probabilities eta_d [V, K, Dmax], the float64 Gauss-Hermite rule."""
    from numpy.polynomial.hermite import hermgauss
    gx, gw_ = hermgauss(T)
    gx, gw_ = gx.astype(LD), (gw_ / np.sqrt(np.pi)).astype(LD)
    w, eta_c, eta_d = np.asarray(w, dtype=LD), np.asarray(eta_c, dtype=LD), np.asarray(eta_d, dtype=LD)
    V, Dmax = flat.V, eta_d.shape[2]
    value, hidden, cont, nst = flat.var_value, flat.var_hidden, flat.var_cont, flat.var_nstates
    gobs = ~hidden & (np.asarray(obs_var) > 0)
    states = lambda v: flat.dom_val[flat.dom_ptr[flat.var_dom[v]]:flat.dom_ptr[flat.var_dom[v] + 1]].astype(LD)

    def axis(v, k):                                    # nodes and weights of variable v under component k
        if gobs[v]:
            return np.sqrt(2 * LD(obs_var[v])) * gx + LD(value[v]), gw_
        if not hidden[v]:
            return np.array([value[v]], dtype=LD), np.ones(1, dtype=LD)
        if cont[v]:
            return np.sqrt(2 * eta_c[v, k, 1]) * gx + eta_c[v, k, 0], gw_
        return states(v), eta_d[v, k, :nst[v]]

    def comp(v, kk, x):                                # variable v's factor of component kk of a belief, at v's own nodes x
        if gobs[v]:
            return _pdf(x, LD(value[v]), LD(obs_var[v]))
        if not hidden[v]:
            return np.ones(x.size, dtype=LD)
        if cont[v]:
            return _pdf(x, eta_c[v, kk, 0], eta_c[v, kk, 1])
        return eta_d[v, kk, :nst[v]]

    gw, energy = np.zeros(K, dtype=LD), LD(0)
    g_c, g_d = np.zeros((V, K, 2), dtype=LD), np.zeros((V, K, Dmax), dtype=LD)
    degree = np.diff(flat.var_ptr)
    for v in range(V):
        for k in range(K):
            x, wt = axis(v, k)
            R = (LD(degree[v]) - 1) * np.log(sum(w[kk] * comp(v, kk, x) for kk in range(K)) + LD('1e-100'))
            E = np.sum(wt * R)
            gw[k] -= E
            energy -= w[k] * E
            if hidden[v] and cont[v]:
                mu, var = eta_c[v, k]
                g_c[v, k, 0] -= np.sum(wt * R * (x - mu)) / var
                g_c[v, k, 1] -= np.sum(wt * R * ((x - mu) ** 2 - var)) / (2 * var * var)
            elif hidden[v]:
                g_d[v, k, :nst[v]] -= R
    for f in range(flat.F):
        scope = flat.edge_var[flat.fac_ptr[f]:flat.fac_ptr[f + 1]]
        pot, arity = flat.potentials[flat.fac_pot[f]], len(scope)
        for k in range(K):
            axes = [axis(v, k) for v in scope]
            shape = tuple(x.size for x, _ in axes)
            grid = lambda a, vec: np.broadcast_to(vec.reshape([-1 if i == a else 1 for i in range(arity)]), shape)
            cols = [grid(a, axes[a][0]).reshape(-1) for a in range(arity)]
            belief = sum(w[kk] * np.prod([grid(a, comp(v, kk, axes[a][0])) for a, v in enumerate(scope)], axis=0) for kk in range(K))
            Fv = (np.log(_phi(pot, cols) + LD('1e-100')).reshape(shape) - np.log(belief + LD('1e-100')))
            weight = lambda skip: np.prod([grid(a, axes[a][1]) for a in range(arity) if a != skip] + [np.ones(shape, dtype=LD)], axis=0)
            Wt = weight(None)
            E = np.sum(Wt * Fv)
            gw[k] -= E
            energy -= w[k] * E
            for a, v in enumerate(scope):
                if not hidden[v] or list(scope).index(v) != a:
                    continue
                if cont[v]:
                    mu, var = eta_c[v, k]
                    u = grid(a, axes[a][0]) - mu
                    g_c[v, k, 0] -= np.sum(Wt * Fv * u) / var
                    g_c[v, k, 1] -= np.sum(Wt * Fv * (u * u - var)) / (2 * var * var)
                else:                                   # slot a pinned to each state: the other slots' weights only
                    g_d[v, k, :nst[v]] -= np.sum(weight(a) * Fv, axis=tuple(i for i in range(arity) if i != a))
    g_w = w * (gw - np.sum(gw * w))
    for v in np.flatnonzero(hidden & ~cont):
        for k in range(K):
            row, eta = g_d[v, k, :nst[v]], eta_d[v, k, :nst[v]]
            g_d[v, k, :nst[v]] = eta * (row - np.sum(row * eta))
    g_c[~(hidden & cont)] = 0
    g_d[~(hidden & ~cont)] = 0
    return g_w, g_c, g_d, energy


# ---- the case tables ----------------------------------------------------------------------------------------------------------
def wide_case(seed, K, T, quirks, table_words, n_rv=60, n_f=160, n_repeat=2):
    """(FlatGraph, obs_var, (w_tau, eta_c, tau_d)) of one random case: the generator and the parameters from one stream"""
    rng = np.random.default_rng(200 + seed)
    flat, obs_var = wide_graph(rng, T, n_rv=n_rv, n_f=n_f, one_discrete_domain=quirks, table_words=table_words, n_repeat=n_repeat)
    return flat, obs_var, random_params(rng, flat, K)


# (seed, K, T, quirks, table_words) -> the segments that hold factors with the lists on and tiny_kernel = 'always' (checked on the
# CPU by tests/test_vi_shapes_host.py, on the device by tests/test_gpu_vi_shapes.py)
WIDE_CASES = [
    ((0, 2, 3, False, 'slim'), 'cc tiny grp6'),
    ((0, 1, 9, True, 'slim'), 'cc tiny grp3 grp6'),
    ((0, 2, 3, True, 'mid'), 'cc tiny grp3 grp6'),
    ((1, 1, 9, True, 'mid'), 'cc tiny grp3 grp6 rest6'),
    ((1, 2, 6, False, 'mid'), 'cc tiny grp3 grp6'),
    ((0, 2, 4, False, 'large'), 'cc grp3 grp6 rest6'),
    ((0, 4, 6, False, 'large'), 'cc grp3 grp6 rest3 rest6'),
    ((1, 16, 2, False, 'large'), 'cc grp3 rest3 rest6'),
    ((1, 8, 1, True, 'large'), 'cc grp3 grp6 rest3 rest6'),
    ((1, 3, 4, True, 'large'), 'cc grp3 grp6 rest3 rest6'),
    ((1, 1, 9, False, 'large'), 'cc grp3 grp6 rest6'),
]

# (seed, K, T) of the small graphs on which the longdouble reference anchors the C oracle (15 variables, 30 factors)
SMALL_CASES = [(0, 4, 6), (1, 8, 2), (7, 1, 9)]
