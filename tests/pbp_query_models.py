"""Hand-built particle-BP states and independent references for the query kernels of csrc/pbp.hip (``lhvi_pbp_belief_points``,
``lhvi_pbp_edge_points``, ``lhvi_pbp_map_brent``, ``lhvi_pbp_quad``, ``lhvi_pbp_var_sum``, ``lhvi_pbp_domain_grid``,
``lhvi_pbp_refine_grid`` and the scan queries built on them).

A state is a small ``FlatGraph`` with chosen ``particles [V, n]`` and ``v2f [E, n]``: no sweep is run, so the belief of a row is
what the builder wrote, ``sum_f log sum_j phi(x, y_j) exp(v2f_j)`` (a sum that is 0 becomes the floor -700).  The same arrays go
into ``oracle.PbpOracle`` here and into a solver on the device in tests/test_gpu_pbp_queries.py.

References: the C oracle's ``belief_points`` / ``edge_points`` for the log-belief; SciPy's ``fminbound`` on it for the MAP
(``brent_rows``); a plain NumPy dqage on QUADPACK's 21-point rule for the normaliser (``dqage_rows``, on the tables of
tests/pbkl_models.py); ``mpmath`` closed forms of the log-belief and of the normaliser for the mixture family; NumPy twins of the
grid kernels and of the 20 / 5-point trapezoid.  ``numpy_log_belief`` restates the mixture family's belief with NumPy, each
message's terms added in either order: a rounding-level perturbation of the oracle's value.

Nothing here imports ``lhvi`` at module level or shares code with the kernels."""
from fractions import Fraction

import numpy as np

import pbkl_models as pk

LO, HI = -10.0, 10.0
MARGIN = 20.0                   # EPBP.belief integrates over the domain widened by this much on both sides
FLOOR = -700.0
SUBNORMAL_LOG = float(np.log(np.finfo(np.float64).tiny))
QUAD_LIMIT = 50
GOLDEN_MEAN = 0.5 * (3.0 - 5.0 ** 0.5)
# potential kinds (lhvi/potentials.py)
TABLE, GAUSSIAN, QUADRATIC, HYBRID_QUADRATIC, LINEAR_GAUSSIAN, X2, XY = 1, 2, 3, 4, 5, 6, 7
PAIR_KINDS = (LINEAR_GAUSSIAN, GAUSSIAN, QUADRATIC, XY)
PARTICLE_COUNTS = (1, 2, 5, 16, 64)


# ---- states ------------------------------------------------------------------------------------------------------------------------
class State:
    """``flat``, ``n``, ``particles [V, n]`` (discrete rows hold the states, as ``PbpOracle.set_particles`` writes them),
    ``v2f [E, n]``, ``rows`` (the variables the family is about) and ``info`` (what the family's tests need besides);
    ``epbp``: the flags of EPBP (else HybridLBP's)"""

    def __init__(self, flat, n, particles, v2f, rows, epbp=True, **info):
        from oracle import oracle
        self.flat, self.n, self.epbp, self.info = flat, int(n), epbp, info
        self.rows = np.asarray(rows, dtype=np.int32)
        o = oracle.PbpOracle(flat, self.n, ep=False, epbp=epbp, var_threshold=3 if epbp else 5)
        o.set_particles(particles)
        o.old_particles = o.particles
        o.v2f = np.ascontiguousarray(v2f, dtype=np.float64)
        assert o.v2f.shape == (flat.E, self.n) and int(o.np.max()) <= self.n
        self.oracle, self.particles, self.v2f, self.counts = o, o.particles, o.v2f, o.np

    def log_belief(self, v, x):
        """the oracle's ``belief_rv`` of variable v at the points x"""
        x = np.atleast_1d(np.asarray(x, dtype=np.float64))
        return self.oracle.belief_points([int(v)], x[None, :])[0]

    def log_belief_pairs(self, edges, mult, x):
        """``sum mult * message_f_to_rv`` over an explicit (edge, multiplicity) list, added in list order from 0.0"""
        x = np.atleast_1d(np.asarray(x, dtype=np.float64))
        out = np.zeros_like(x)
        for e, m in zip(edges, mult):
            out = out + self.oracle.edge_points([int(e)], x[None, :])[0] * float(m)
        return out

    def exact_message(self, e, x):
        """the message of edge e at the points x without the floor and without underflow: log-sum-exp of ``log phi + m`` for a pair
        factor of the mixture kinds with a hidden partner (where the family's messages can underflow); the oracle's value elsewhere"""
        fl = self.flat
        f = fl.edge_fac[e]
        base, pot = fl.fac_ptr[f], fl.fac_pot[f]
        kind = int(fl.pot_kind[pot])
        pe = base + 1 - (e - base)
        if fl.fac_ptr[f + 1] - base != 2 or kind not in PAIR_KINDS or not fl.var_hidden[fl.edge_var[pe]]:
            return self.oracle.edge_points([int(e)], x[None, :])[0], 1.0
        par = fl.pot_param[fl.pot_off[pot]:fl.pot_off[pot + 1]]
        y, m = self.particles[fl.edge_var[pe]][None, :], self.v2f[pe][None, :]
        t = _log_phi(kind, par, (x[:, None], y) if e == base else (y, x[:, None])) + m
        top = t.max(axis=1)
        return top + np.log(np.exp(t - top[:, None]).sum(axis=1)), float(np.exp(m).sum()) + self.n

    def allowance(self, edges, mult, x):
        """what two correct evaluations of ``sum mult * message`` may differ by at the points x on top of the project's bound: 0,
        except where a message's sum of terms is subnormal (its exact value L below log(2^-1022) = -708.4; the floor -700 lies
        above).  Down there every term -- and in the oracle, which forms ``phi * e ** m``, every phi before it is scaled by e ** m --
        is rounded to a multiple of 2^-1074, so the sum carries a relative error of up to u = (sum_j e ** m_j + n) 2^-1074 / e ** L
        and its logarithm about as much: 2 u is allowed.  From u = 1/4 on, one evaluation may round the sum to 0 -- the message
        is then the floor -700 -- where the other keeps a nonzero one (down to -745): 50 is allowed.  Below -760 every term is 0
        in any evaluation and both give the floor."""
        x = np.atleast_1d(np.asarray(x, dtype=np.float64))
        out = np.zeros_like(x)
        for e, m in zip(edges, mult):
            L, scale = self.exact_message(int(e), x)
            with np.errstate(over='ignore'):
                u = scale * np.exp(np.log(2.0) * -1074 - L)
            out += np.where((L < SUBNORMAL_LOG) & (L > -760.0), np.where(u < 0.25, 2.0 * u, 50.0), 0.0) * abs(float(m))
        return out

    def belief_allowance(self, v, x):
        fl = self.flat
        edges = fl.var_edge[fl.var_ptr[v]:fl.var_ptr[v + 1]]
        return self.allowance(edges, fl.edge_count[edges], x)

    def domain(self, v):
        d = self.flat.var_dom[v]
        return float(self.flat.dom_lo[d]), float(self.flat.dom_hi[d])

    def states(self, v):
        d = self.flat.var_dom[v]
        return self.flat.dom_val[self.flat.dom_ptr[d]:self.flat.dom_ptr[d + 1]]


class _Builder:
    def __init__(self, domains):
        self.domains, self.var_dom, self.var_value, self.scopes, self.specs = list(domains), [], [], [], []

    def var(self, dom=0, value=np.nan):
        self.var_dom.append(dom)
        self.var_value.append(value)
        return len(self.var_dom) - 1

    def factor(self, scope, kind, par):
        self.scopes.append(tuple(int(v) for v in scope))
        self.specs.append((int(kind), [float(t) for t in par]))
        return len(self.scopes) - 1

    def flat(self):
        from lhvi.flat import build_flat
        fac_ptr = np.concatenate([[0], np.cumsum([len(s) for s in self.scopes])]).astype(np.int32)
        edge_var = np.array([v for s in self.scopes for v in s], dtype=np.int32)
        return build_flat(fac_ptr, edge_var, np.arange(len(self.scopes), dtype=np.int32), self.specs,
                          np.array(self.var_value, dtype=np.float64), np.array(self.var_dom, dtype=np.int32), self.domains)


def _cont(lo=LO, hi=HI, points=8):
    from lhvi.graph import Domain
    return Domain((lo, hi), continuous=True, integral_points=np.linspace(lo, hi, points))


def _disc(k):
    from lhvi.graph import Domain
    return Domain(tuple(float(i) for i in range(k)), continuous=False)


def _pair_spec(rng, kind, sd):
    """(parameter row, position of the target) of a pair potential under which the target given a partner particle has the
    standard deviation `sd` (XY is log-linear in the target and has none)"""
    t = int(rng.integers(2))
    if kind == LINEAR_GAUSSIAN:                     # exp(-(x1 - a x0)^2 / (2 var))
        a = float(rng.uniform(0.3, 1.5) * rng.choice([-1.0, 1.0]))
        return [a, sd * sd if t == 1 else (sd * abs(a)) ** 2], t
    if kind == GAUSSIAN:                            # exp(-0.5 (x - mu)' P (x - mu))
        ptt, ppp, rho = 1.0 / (sd * sd), float(rng.uniform(0.02, 0.5)), float(rng.uniform(-0.8, 0.8))
        off = rho * np.sqrt(ptt * ppp)
        P = np.array([[ptt, off], [off, ppp]]) if t == 0 else np.array([[ppp, off], [off, ptt]])
        return [2.0] + rng.uniform(-2, 2, 2).tolist() + P.ravel().tolist(), t
    if kind == QUADRATIC:                           # exp(x'Ax + b'x + c) = exp(-0.5 p (x_t - (k y + h))^2 + s y + c0), expanded
        p, k, h = 1.0 / (sd * sd), float(rng.uniform(-1, 1)), float(rng.uniform(-2, 2))
        s, c0, split = float(rng.uniform(-0.3, 0.3)), float(rng.uniform(-1, 1)), float(rng.uniform(0, 1))
        A = np.zeros((2, 2))
        A[t, t], A[1 - t, 1 - t], A[t, 1 - t], A[1 - t, t] = -0.5 * p, -0.5 * p * k * k, split * p * k, (1 - split) * p * k
        b = np.zeros(2)
        b[t], b[1 - t] = p * h, -p * k * h + s
        return [2.0] + A.ravel().tolist() + b.tolist() + [-0.5 * p * h * h + c0], t
    if kind == XY:                                  # exp(-coef x0 x1 / (2 var))
        return [float(rng.uniform(-0.5, 0.5)), float(rng.uniform(1, 3))], t
    raise ValueError(kind)


def mixture(n, count, seed, min_sd=0.2, max_sd=3.0, unary=True, degrees=(1, 2, 3), kinds=PAIR_KINDS, raise_v2f=None):
    """`count` continuous targets on [-10, 10], each with 1 to 3 pair factors to continuous partners of its own (n particles
    uniform on [-14, 14], log-messages N(0, 2)) and, for every other one or so, a unary X2.  The standard deviation of the target
    given a partner particle is log-uniform on [min_sd, max_sd].  ``raise_v2f [count]``: added to the
    log-messages into the target's factors (the overflow family)."""
    rng = np.random.default_rng(seed)
    b = _Builder([_cont()])
    targets = [b.var() for _ in range(count)]
    for i, t in enumerate(targets):
        for _ in range(int(rng.choice(degrees))):
            kind = int(rng.choice(kinds))
            sd = float(np.exp(rng.uniform(np.log(min_sd), np.log(max_sd))))
            par, pos = _pair_spec(rng, kind, sd)
            p = b.var()
            b.factor((t, p) if pos == 0 else (p, t), kind, par)
        if unary and rng.random() < 0.5:
            b.factor((t,), X2, [rng.uniform(0.5, 1.5), rng.uniform(2, 10)])
    flat = b.flat()
    particles = rng.uniform(-14, 14, (flat.V, n))
    particles[targets] = rng.uniform(LO, HI, (count, n))
    v2f = rng.normal(0.0, np.sqrt(2.0), (flat.E, n))
    if raise_v2f is not None:
        for i, t in enumerate(targets):
            for k in range(flat.var_ptr[t], flat.var_ptr[t + 1]):
                e = flat.var_edge[k]
                f = flat.edge_fac[e]
                if flat.fac_ptr[f + 1] - flat.fac_ptr[f] == 2:
                    v2f[flat.fac_ptr[f] + 1 - flat.edge_pos[e]] += raise_v2f[i]
    return State(flat, n, particles, v2f, targets)


def end(n, count, seed):
    """every partner particle beyond +14 (first half of the rows) or beyond -14 (second half), LinearGaussian x ~ N(y, sd^2):
    every component rises (falls) over the whole domain, so the belief is monotone and its maximum is at a domain end"""
    rng = np.random.default_rng(seed)
    b = _Builder([_cont()])
    targets, side = [b.var() for _ in range(count)], []
    partners = []
    for i, t in enumerate(targets):
        side.append(1.0 if i < count // 2 else -1.0)
        for _ in range(int(rng.integers(1, 3))):
            sd, pos = float(rng.uniform(1.5, 3.0)), int(rng.integers(2))
            p = b.var()
            partners.append((p, side[-1]))
            b.factor((t, p) if pos == 0 else (p, t), LINEAR_GAUSSIAN, [1.0, sd * sd])
    flat = b.flat()
    particles = rng.uniform(LO, HI, (flat.V, n))
    for p, s in partners:
        particles[p] = s * rng.uniform(14.5, 18.0, n)
    return State(flat, n, particles, rng.normal(0.0, np.sqrt(2.0), (flat.E, n)), targets, side=np.array(side))


def flat_family(n, count, seed):
    """the mixture family without unary factors and with every log-message at -800: every term is 0, every message the floor"""
    st = mixture(n, count, seed, unary=False)
    return State(st.flat, n, st.particles, np.full_like(st.v2f, -800.0), st.rows)


def narrow(n, count, seed):
    """targets on domains of width 1e-6 (partners on [-10, 10]): Brent's loop makes no iteration there"""
    rng = np.random.default_rng(seed)
    los = rng.uniform(-8, 8, count)
    b = _Builder([_cont()] + [_cont(float(lo), float(lo) + 1e-6) for lo in los])
    targets = []
    for i in range(count):
        t, p = b.var(1 + i), b.var(0)
        targets.append(t)
        par, pos = _pair_spec(rng, LINEAR_GAUSSIAN, 1.0)
        b.factor((t, p) if pos == 0 else (p, t), LINEAR_GAUSSIAN, par)
    flat = b.flat()
    particles = rng.uniform(-14, 14, (flat.V, n))
    return State(flat, n, particles, rng.normal(0.0, np.sqrt(2.0), (flat.E, n)), targets)


TIES = {2: [None, (0, 1)], 3: [None, (0, 2), (0, 1), (1, 2)], 5: [None, (0, 4), (0, 1), (3, 4), (1, 3)]}


def discrete(seed, n=8, copies=3):
    """discrete targets of 2, 3 and 5 states, each with a table to a hidden two-state partner and a HybridQuadratic factor to a
    continuous partner.  ``info['tie'][row]``: None, or the two states that share every parameter (their beliefs are then equal
    bit for bit) and carry the largest constant term, so that the maximum is tied between them."""
    rng = np.random.default_rng(seed)
    sizes = (2, 3, 5)
    b = _Builder([_cont()] + [_disc(k) for k in sizes])
    targets, tie = [], []
    for _ in range(copies):
        for di, k in enumerate(sizes):
            for pair in TIES[k]:
                t, d2, c = b.var(1 + di), b.var(1), b.var(0)
                table = rng.uniform(0.5, 2.0, (k, 2))
                A, bb, cc = rng.uniform(-0.02, -0.005, k), rng.uniform(-0.1, 0.1, k), rng.uniform(-5, -4, k)
                if pair is not None:
                    i, j = pair
                    table[j], A[j], bb[j] = table[i], A[i], bb[i]
                    cc[i] = cc[j] = 5.0
                b.factor((t, d2), TABLE, [2, k, 2] + table.ravel().tolist())
                b.factor((t, c), HYBRID_QUADRATIC, [1, 1, k] + A.tolist() + bb.tolist() + cc.tolist())
                targets.append(t)
                tie.append(pair)
    flat = b.flat()
    particles = rng.uniform(-14, 14, (flat.V, n))
    return State(flat, n, particles, rng.normal(0.0, np.sqrt(2.0), (flat.E, n)), targets, tie=tie)


def observed(seed, n=8, copies=6):
    """observed partners and arity 3 with one observed argument.  Continuous targets: (a) a LinearGaussian to an observed
    partner and one to a hidden partner; (b) the MLN formula ``x0 * near(x1, x2)`` of the paper-popularity model with the
    Boolean x0 observed and a hidden continuous partner; (c) the same with the continuous partner observed and the Boolean
    hidden, plus a unary X2.  Discrete targets (d): a three-argument table with a hidden and an observed partner and a
    two-argument table.  ``info['cont']`` / ``info['disc']``: the rows of either type."""
    from lhvi.mln import MLNPotential, eq_op
    rng = np.random.default_rng(seed)
    doms = [_cont(), _disc(2), _disc(3)]
    b = _Builder(doms)
    cont, disc = [], []
    for _ in range(copies):
        t, o, p = b.var(0), b.var(0, float(rng.uniform(-6, 6))), b.var(0)                     # (a)
        b.factor((o, t), LINEAR_GAUSSIAN, [float(rng.uniform(0.5, 1.2)), float(rng.uniform(1, 4))])
        b.factor((t, p), LINEAR_GAUSSIAN, [float(rng.uniform(0.5, 1.2)), float(rng.uniform(1, 4))])
        cont.append(t)
        w = float(rng.uniform(0.3, 1.0))                                                      # (b)
        t, o, p = b.var(0), b.var(1, 1.0), b.var(0)
        kind, par = MLNPotential(lambda x: x[0] * eq_op(x[1], x[2]), w=w).device_spec((doms[1], doms[0], doms[0]))
        b.factor((o, t, p), kind, par)
        cont.append(t)
        t, o, p = b.var(0), b.var(0, float(rng.uniform(-6, 6))), b.var(1)                     # (c)
        b.factor((p, t, o), kind, par)
        b.factor((t,), X2, [1.0, float(rng.uniform(4, 10))])
        cont.append(t)
        t, h, o = b.var(2), b.var(1), b.var(1, float(rng.integers(2)))                        # (d)
        b.factor((t, h, o), TABLE, [3, 3, 2, 2] + rng.uniform(0.2, 3.0, 12).tolist())
        b.factor((h, t), TABLE, [2, 2, 3] + rng.uniform(0.2, 3.0, 6).tolist())
        disc.append(t)
    flat = b.flat()
    particles = rng.uniform(-14, 14, (flat.V, n))
    return State(flat, n, particles, rng.normal(0.0, np.sqrt(2.0), (flat.E, n)), cont + disc, cont=np.array(cont), disc=np.array(disc))


def lifted(seed, n=16, groups=(2, 3, 4, 3), unary=True):
    """hubs with m identical leaves each (one LinearGaussian potential per hub and, with `unary`, an X2 on every variable): colour
    passing merges a hub's leaves, so the lifted graph has one edge of count m per hub.  The ground graph is refined with the
    oracle's colour passing and lifted with ``lifting.lift_flat`` on the host; messages and particles are then written for the
    LIFTED graph.  Rows: every cluster."""
    from lhvi import lifting
    from oracle import oracle
    rng = np.random.default_rng(seed)
    b = _Builder([_cont()])
    f_color = []
    for gi, m in enumerate(groups):
        hub = b.var()
        sd, a = float(rng.uniform(1.0, 2.5)), float(rng.uniform(0.5, 1.2))
        ux = [1.0, float(rng.uniform(4, 10))]
        if unary:
            b.factor((hub,), X2, [1.0, float(rng.uniform(4, 10))])
            f_color.append(3 * gi)
        for _ in range(m):
            leaf = b.var()
            b.factor((hub, leaf), LINEAR_GAUSSIAN, [a, sd * sd])
            f_color.append(3 * gi + 1)
            if unary:
                b.factor((leaf,), X2, ux)
                f_color.append(3 * gi + 2)
    ground = b.flat()
    rvc, fc = oracle.color_passing(ground, np.zeros(ground.F, dtype=np.uint8), np.zeros(ground.V, dtype=np.int32),
                                   np.array(f_color, dtype=np.int32))
    flat = lifting.lift_flat(ground, np.asarray(rvc, dtype=np.int32), np.asarray(fc, dtype=np.int32))
    assert flat.lifted and flat.V == 2 * len(groups) and sorted(set(flat.edge_count.tolist())) == sorted({1.0} | {float(m) for m in groups})
    particles = rng.uniform(-12, 12, (flat.V, n))
    return State(flat, n, particles, rng.normal(0.0, np.sqrt(2.0), (flat.E, n)), np.arange(flat.V), epbp=False)


def overflow(seed, n=16, count=40, hot=(3, 17, 18, 39)):
    """two LinearGaussian factors per row; on the rows `hot` the log-messages are raised by 400, so each message peaks near
    +400 and ``e ** belief`` is inf at the peak.  ``info['hot']``: mask over the rows."""
    up = np.zeros(count)
    up[list(hot)] = 400.0
    st = mixture(n, count, seed, min_sd=1.0, max_sd=2.0, unary=False, degrees=(2,), kinds=(LINEAR_GAUSSIAN,), raise_v2f=up)
    part = st.particles.copy()
    part[len(st.rows):] *= 5.0 / 14.0              # partners within [-5, 5]: the peak lies inside the domain
    return State(st.flat, n, part, st.v2f, st.rows, hot=up > 0)


def area(n, seed, count=24):
    """the rows of the scan queries (``log_area_all``, ``probability_all``, ``belief_all``): mixture rows with standard deviations
    from 1 (a 20-point trapezoid needs no more); two rows of two LinearGaussian factors with standard deviation 0.2 whose partner
    particles all lie near one end, so the belief falls to the floor sum -1400 over most of the domain and the shift of
    ``log_message_balance`` is max - 700; an observed variable; and, where n has room for its two states, a discrete one."""
    rng = np.random.default_rng(seed)
    b = _Builder([_cont(), _disc(2)])
    cont, steep, near = [], [], []
    for i in range(count + 2):
        t = b.var()
        cont.append(t)
        if i < count:
            for _ in range(int(rng.integers(1, 4))):
                kind = int(rng.choice(PAIR_KINDS))
                par, pos = _pair_spec(rng, kind, float(rng.uniform(1.0, 3.0)))
                p = b.var()
                b.factor((t, p) if pos == 0 else (p, t), kind, par)
            continue
        steep.append(t)
        for _ in range(2):
            p = b.var()
            near.append((p, 1.0 if i == count else -1.0))
            b.factor((p, t), LINEAR_GAUSSIAN, [1.0, 0.04])
    obs = b.var(0, 1.25)
    t = b.var()
    cont.append(t)
    b.factor((obs, t), LINEAR_GAUSSIAN, [0.8, 2.0])
    disc = None
    if n >= 2:
        disc, c = b.var(1), b.var()
        b.factor((disc, c), HYBRID_QUADRATIC, [1, 1, 2, -0.01, -0.02, 0.05, -0.05, 0.3, -0.2])
    flat = b.flat()
    particles = rng.uniform(-14, 14, (flat.V, n))
    for p, s in near:
        particles[p] = s * rng.uniform(9.0, 9.9, n)
    return State(flat, n, particles, rng.normal(0.0, np.sqrt(2.0), (flat.E, n)), cont, steep=np.array(steep), obs=obs, disc=disc)


def grid_state(n, seed=5):
    """variables of every type for the grid kernels: continuous on [-10, 10] and on a domain of width 1e-6, one observed, and
    discrete ones of 2, 3 and 5 states as far as n has room for them; chained by pair factors so that every variable has edges"""
    rng = np.random.default_rng(seed)
    sizes = [k for k in (2, 3, 5) if k <= n]
    b = _Builder([_cont(), _cont(2.0, 2.0 + 1e-6), _cont(-3.0, 7.5)] + [_disc(k) for k in sizes])
    cont = [b.var(0) for _ in range(5)] + [b.var(1), b.var(2), b.var(2)]
    obs = b.var(0, -1.5)
    disc = [b.var(3 + i) for i in range(len(sizes))] * 1 + [b.var(3 + i) for i in range(len(sizes))]
    for u, v in zip(cont[:-1] + [obs], cont[1:] + [cont[0]]):
        b.factor((u, v), LINEAR_GAUSSIAN, [0.9, 2.0])
    for d in disc:
        k = len(b.domains[b.var_dom[d]].values)
        b.factor((d, cont[int(rng.integers(len(cont)))]), HYBRID_QUADRATIC,
                 [1, 1, k] + rng.uniform(-0.02, -0.01, k).tolist() + rng.uniform(-0.1, 0.1, k).tolist() + rng.uniform(-1, 1, k).tolist())
    flat = b.flat()
    return State(flat, n, rng.uniform(-9, 9, (flat.V, n)), rng.normal(0.0, 1.0, (flat.E, n)), cont, obs=obs, disc=np.array(disc, dtype=np.int64))


# ---- the mixture family restated: NumPy, and mpmath closed forms ---------------------------------------------------------------------
def _edges_of(flat, v):
    for k in range(flat.var_ptr[v], flat.var_ptr[v + 1]):
        e = int(flat.var_edge[k])
        f = int(flat.edge_fac[e])
        base, pot = int(flat.fac_ptr[f]), int(flat.fac_pot[f])
        yield (e, base, int(flat.fac_ptr[f + 1]) - base, int(flat.pot_kind[pot]),
               flat.pot_param[flat.pot_off[pot]:flat.pot_off[pot + 1]])


def _phi(kind, par, x):
    """the potential at the argument tuple x (the formulas of the reference's ``get`` methods)"""
    if kind == LINEAR_GAUSSIAN:
        d = x[1] - par[0] * x[0]
        return np.exp(-(d * d) * 0.5 / par[1])
    if kind == X2:
        return np.exp(-par[0] * (x[0] * x[0]) * 0.5 / par[1])
    if kind == XY:
        return np.exp(-par[0] * x[0] * x[1] * 0.5 / par[1])
    if kind == GAUSSIAN:
        mu, P = par[1:3], par[3:7].reshape(2, 2)
        d0, d1 = x[0] - mu[0], x[1] - mu[1]
        return np.e ** (-0.5 * ((d0 * P[0, 0] + d1 * P[1, 0]) * d0 + (d0 * P[0, 1] + d1 * P[1, 1]) * d1))
    if kind == QUADRATIC:
        A, b, c = par[1:5].reshape(2, 2), par[5:7], par[7]
        return np.e ** (x[0] * (A[0, 0] * x[0] + A[0, 1] * x[1]) + x[1] * (A[1, 0] * x[0] + A[1, 1] * x[1]) + (b[0] * x[0] + b[1] * x[1]) + c)
    raise ValueError(kind)


def _log_phi(kind, par, x):
    """log of ``_phi`` for the pair kinds: the exponent itself"""
    if kind == LINEAR_GAUSSIAN:
        d = x[1] - par[0] * x[0]
        return -(d * d) * 0.5 / par[1]
    if kind == XY:
        return -par[0] * x[0] * x[1] * 0.5 / par[1]
    if kind == GAUSSIAN:
        mu, P = par[1:3], par[3:7].reshape(2, 2)
        d0, d1 = x[0] - mu[0], x[1] - mu[1]
        return -0.5 * ((d0 * P[0, 0] + d1 * P[1, 0]) * d0 + (d0 * P[0, 1] + d1 * P[1, 1]) * d1)
    if kind == QUADRATIC:
        A, b, c = par[1:5].reshape(2, 2), par[5:7], par[7]
        return x[0] * (A[0, 0] * x[0] + A[0, 1] * x[1]) + x[1] * (A[1, 0] * x[0] + A[1, 1] * x[1]) + (b[0] * x[0] + b[1] * x[1]) + c
    raise ValueError(kind)


def numpy_log_belief(st, v, x, reverse=False):
    """``belief_rv`` of a mixture-family row at the scalar x: per factor the terms ``phi(x, y_j) e ** m_j`` added one after the
    other, from the first particle or (`reverse`) from the last"""
    total = 0.0
    with np.errstate(over='ignore', under='ignore'):
        for e, base, arity, kind, par in _edges_of(st.flat, v):
            if arity == 1:
                res = float(_phi(kind, par, (x,)))
            else:
                pe = base + 1 - (e - base)
                y, m = st.particles[st.flat.edge_var[pe]], st.v2f[pe]
                terms = _phi(kind, par, (x, y) if e == base else (y, x)) * np.e ** m
                res = float(np.cumsum(terms[::-1] if reverse else terms)[-1])
            total += float(np.log(res)) if res > 0 else FLOOR
    return total


def _coefficients(mp, kind, par, tpos, y):
    """(alpha, beta, gamma) with log phi = alpha x^2 + beta x + gamma in the target x, the partner at y; exact in the parameters"""
    par = [mp.mpf(float(t)) for t in par]
    y = mp.mpf(float(y)) if y is not None else None
    if kind == X2:
        return -par[0] / (2 * par[1]), mp.mpf(0), mp.mpf(0)
    if kind == LINEAR_GAUSSIAN:
        a, var = par
        if tpos == 1:
            return -1 / (2 * var), a * y / var, -(a * y) ** 2 / (2 * var)
        return -a * a / (2 * var), a * y / var, -y * y / (2 * var)
    if kind == XY:
        return mp.mpf(0), -par[0] * y / (2 * par[1]), mp.mpf(0)
    if kind == GAUSSIAN:
        mu, P = par[1:3], (par[3:5], par[5:7])
        t, p = tpos, 1 - tpos
        d, cross = y - mu[p], P[t][p] + P[p][t]
        return -P[t][t] / 2, P[t][t] * mu[t] - cross * d / 2, -P[t][t] * mu[t] ** 2 / 2 + cross * mu[t] * d / 2 - P[p][p] * d * d / 2
    if kind == QUADRATIC:
        A, b, c = (par[1:3], par[3:5]), par[5:7], par[7]
        t, p = tpos, 1 - tpos
        return A[t][t], (A[t][p] + A[p][t]) * y + b[t], A[p][p] * y * y + b[p] * y + c
    raise ValueError(kind)


def _factor_terms(mp, st, v):
    """per factor of the mixture-family row v: (arity, list of (alpha, beta, gamma) with the log-message folded into gamma)"""
    out = []
    for e, base, arity, kind, par in _edges_of(st.flat, v):
        if arity == 1:
            out.append((1, [_coefficients(mp, kind, par, 0, None)]))
            continue
        pe = base + 1 - (e - base)
        pv = st.flat.edge_var[pe]
        terms = []
        for j in range(st.n):
            a, b, c = _coefficients(mp, kind, par, e - base, st.particles[pv, j])
            terms.append((a, b, c + mp.mpf(float(st.v2f[pe, j]))))
        out.append((2, terms))
    return out


def log_belief_closed_form(st, v, xs, dps=30):
    """(log-belief [len(xs)], safe [len(xs)]) of a mixture-family row by mpmath.  ``safe``: every factor's exact log-message lies
    above -690, so that no term sum of the double-precision evaluation comes near the underflow that turns it into the floor"""
    import mpmath as mp
    with mp.workdps(dps):
        factors = _factor_terms(mp, st, v)
        vals, safe = [], []
        for x in xs:
            x = mp.mpf(float(x))
            logs = [mp.log(mp.fsum(mp.exp(a * x * x + b * x + c) for a, b, c in terms)) for _, terms in factors]
            vals.append(float(mp.fsum(logs)))
            safe.append(all(t > -690 for t in logs))
    return np.array(vals), np.array(safe)


def has_closed_form(st, v):
    """one pair factor, with or without the unary one"""
    arity = [a for _, _, a, _, _ in _edges_of(st.flat, v)]
    return arity.count(2) == 1 and len(arity) <= 2


def z_closed_form(st, v, dps=30):
    """the integral of ``e ** belief_rv`` over the domain widened by 20 for a mixture-family row of degree 1 (with or without the
    unary factor): a sum of integrals of exp(alpha x^2 + beta x + gamma), by erf.  (Where the double-precision term sum is 0 the
    belief is the floor -700 instead, which changes the integral by less than 60 e^-700.)"""
    import mpmath as mp
    assert has_closed_form(st, v)
    lo, hi = st.domain(v)
    with mp.workdps(dps):
        lo, hi = mp.mpf(lo) - MARGIN, mp.mpf(hi) + MARGIN
        factors = _factor_terms(mp, st, v)
        pair = [terms for arity, terms in factors if arity == 2][0]
        ua = mp.fsum(terms[0][0] for arity, terms in factors if arity == 1)
        total = mp.mpf(0)
        for a, b, c in pair:
            a = a + ua
            if a < 0:
                r, mu = mp.sqrt(-a), -b / (2 * a)
                total += mp.exp(c - b * b / (4 * a)) * mp.sqrt(mp.pi) / (2 * r) * (mp.erf(r * (hi - mu)) - mp.erf(r * (lo - mu)))
            elif b != 0:
                total += mp.exp(c) * (mp.exp(b * hi) - mp.exp(b * lo)) / b
            else:
                total += mp.exp(c) * (hi - lo)
        return float(total)


# ---- Brent ---------------------------------------------------------------------------------------------------------------------------
def brent_rows(fun, lo, hi, xtol=1e-5, maxfun=500):
    """``scipy.optimize.fminbound`` on ``-fun(r, x)`` for every row r: (x, log-belief at x, nfev, limit reached)"""
    from scipy.optimize import fminbound
    R = len(lo)
    x, f, nfev, flag = np.zeros(R), np.zeros(R), np.zeros(R, dtype=np.int32), np.zeros(R, dtype=bool)
    for r in range(R):
        xr, fr, ierr, num = fminbound(lambda t, r=r: -float(fun(r, float(t))), float(lo[r]), float(hi[r]), xtol=xtol, maxfun=maxfun,
                                      full_output=True, disp=0)
        x[r], f[r], nfev[r], flag[r] = xr, -fr, num, ierr == 1
    return x, f, nfev, flag


def brent_state(st, variables, xtol=1e-5, maxfun=500):
    """``brent_rows`` on the oracle's belief of the given variables; a discrete one takes the first state with the largest belief
    and as many evaluations as it has states"""
    variables = np.asarray(variables)
    x, f, nfev, flag = (np.zeros(variables.size), np.zeros(variables.size), np.zeros(variables.size, dtype=np.int32),
                        np.zeros(variables.size, dtype=bool))
    for r, v in enumerate(variables):
        if st.flat.var_cont[v]:
            lo, hi = st.domain(v)
            x[r], f[r], nfev[r], flag[r] = (t[0] for t in brent_rows(lambda _, t, v=v: st.log_belief(v, [t])[0], [lo], [hi], xtol, maxfun))
        else:
            states = st.states(v)
            vals = st.log_belief(v, states)
            k = int(np.argmax(vals))                # (the first of the largest)
            x[r], f[r], nfev[r] = states[k], vals[k], states.size
    return x, f, nfev, flag


# ---- dqage ---------------------------------------------------------------------------------------------------------------------------
def rule21(values, lo, hi):
    """(result, abserr, resabs, resasc) of QUADPACK's dqk21 from the 21 values at ``pbkl_models.nodes(lo, hi)``:
    ``pbkl_models.rule`` with the two sums of magnitudes handed out too.  dqage's first-rule shortcut compares the estimate with
    ``resasc``, the integral of |f - mean| (dqage.f receives it in a variable it calls ``resabs``): an estimate equal to it has
    been cut off at its ceiling and proves nothing."""
    h = 0.5 * (hi - lo)
    left, mid, right = values[9::-1], float(values[10]), values[11:]
    kron, gauss, mag = pk._WK0 * mid, 0.0, abs(pk._WK0 * mid)
    for i in (8, 6, 4, 2, 0):
        pair = left[i] + right[i]
        gauss += pk._WG[i] * pair
        kron += pk._WK[i] * pair
        mag += pk._WK[i] * (abs(left[i]) + abs(right[i]))
    for i in (9, 7, 5, 3, 1):
        kron += pk._WK[i] * (left[i] + right[i])
        mag += pk._WK[i] * (abs(left[i]) + abs(right[i]))
    mean = 0.5 * kron
    dev = pk._WK0 * abs(mid - mean)
    for i in range(9, -1, -1):
        dev += pk._WK[i] * (abs(left[i] - mean) + abs(right[i] - mean))
    mag, dev = mag * abs(h), dev * abs(h)
    est = abs((kron - gauss) * h)
    if dev != 0.0 and est != 0.0:
        est = dev * min(1.0, (200.0 * est / dev) ** 1.5)
    if mag > pk._TINY / (50.0 * pk._EPS):
        est = max(50.0 * pk._EPS * mag, est)
    return float(kron * h), float(est), float(mag), float(dev)


def dqage(f, lo, hi, epsabs=1.49e-8, epsrel=1.49e-8, limit=QUAD_LIMIT):
    """(z, abserr, status) of the integral of f over [lo, hi]: the 21-point rule, then the interval with the largest estimate
    (the first of them) is halved until the summed estimate is at most max(epsabs, epsrel |area|) or `limit` intervals exist.
    status 0: tolerance met; 1: interval limit; 3: a rule's sum was not finite (z is NaN then)."""
    with np.errstate(over='ignore', invalid='ignore'):
        r, e, _, asc = rule21(f(pk.nodes(lo, hi)), lo, hi)
        if not np.isfinite(r):
            return np.nan, e, 3
        a_, b_, r_, e_ = [lo], [hi], [r], [e]
        area, errsum, status = r, e, 0
        bound = max(epsabs, epsrel * abs(area))
        if not ((e <= bound and e != asc) or e == 0.0):
            status = 1
            while len(a_) < limit:
                m = int(np.argmax(e_))
                a1, b2 = a_[m], b_[m]
                mid = 0.5 * (a1 + b2)
                r1, e1, _, _ = rule21(f(pk.nodes(a1, mid)), a1, mid)
                r2, e2, _, _ = rule21(f(pk.nodes(mid, b2)), mid, b2)
                if not (np.isfinite(r1) and np.isfinite(r2)):
                    return np.nan, errsum, 3
                errsum += (e1 + e2) - e_[m]
                area += (r1 + r2) - r_[m]
                b_[m], r_[m], e_[m] = mid, r1, e1
                a_.append(mid), b_.append(b2), r_.append(r2), e_.append(e2)
                bound = max(epsabs, epsrel * abs(area))
                if errsum <= bound:
                    status = 0
                    break
        total = 0.0
        for t in r_:
            total += t
    return total, errsum, status


def dqage_rows(fun, lo, hi, epsabs=1.49e-8, epsrel=1.49e-8):
    """``dqage`` of ``e ** fun(r, x)`` for every row r (``fun`` takes the 21 points of a rule at once)"""
    with np.errstate(over='ignore'):
        out = [dqage(lambda x, r=r: np.exp(fun(r, x)), float(lo[r]), float(hi[r]), epsabs, epsrel) for r in range(len(lo))]
    z, err, st = zip(*out)
    return np.array(z), np.array(err), np.array(st, dtype=np.int32)


def dqage_state(st, variables, epsabs=1.49e-8, epsrel=1.49e-8):
    variables = np.asarray(variables)
    lo, hi = np.array([st.domain(v) for v in variables]).T
    return dqage_rows(lambda r, x: st.log_belief(variables[r], x), lo - MARGIN, hi + MARGIN, epsabs, epsrel)


# ---- twins of the grid kernels -------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """a * b + c rounded once: the grid kernels are compiled with the compiler's default contraction, which fuses ``lo + step * j``"""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def domain_grid_twin(flat, counts, n):
    """``lhvi_pbp_domain_grid``: x [V, n]; a uniform cnt-point grid on a continuous hidden variable's domain whose last point is the
    upper end itself, the states of a discrete one, 0 in every other place"""
    x = np.zeros((flat.V, n))
    for v in range(flat.V):
        d, cnt = flat.var_dom[v], int(counts[v])
        if not flat.var_hidden[v]:
            continue
        for j in range(min(cnt, n)):
            if flat.dom_cont[d]:
                lo, hi = flat.dom_lo[d], flat.dom_hi[d]
                x[v, j] = hi if j == cnt - 1 else _fma((hi - lo) / float(cnt - 1), float(j), lo)
            else:
                x[v, j] = flat.dom_val[flat.dom_ptr[d] + j]
    return x


def refine_grid_twin(flat, counts, logb, x):
    """``lhvi_pbp_refine_grid``: (x', best, best_val).  The first maximum of the row's cnt values; a continuous hidden variable with
    at least 3 points gets a new uniform grid on [x_(arg-1), x_(arg+1)], clamped to the old grid's ends, whose last point is the
    bracket's upper end itself; columns from cnt on, discrete and observed rows keep their points"""
    x = np.array(x, dtype=np.float64)
    best, val = np.zeros(flat.V), np.zeros(flat.V)
    for v in range(flat.V):
        if not flat.var_hidden[v]:
            best[v], val[v] = flat.var_value[v], 0.0
            continue
        cnt = int(counts[v])
        arg = 0
        for j in range(1, cnt):
            if logb[v, j] > logb[v, arg]:
                arg = j
        best[v], val[v] = x[v, arg], logb[v, arg]
        if not flat.var_cont[v] or cnt < 3:
            continue
        lo, hi = x[v, max(arg - 1, 0)], x[v, min(arg + 1, cnt - 1)]
        step = (hi - lo) / float(cnt - 1)
        x[v, :cnt] = [hi if j == cnt - 1 else _fma(step, float(j), lo) for j in range(cnt)]
    return x, best, val


def var_sum_twin(flat, counts, n, f2v):
    """``lhvi_pbp_var_sum``: out[v, j] = the sum over v's edges, in ``var_edge`` order from 0.0, of f2v[e, j] (times the edge's count
    on a lifted graph, rounded before the addition); 0 for observed rows and for j from the row's count on"""
    out = np.zeros((flat.V, n))
    for v in range(flat.V):
        if not flat.var_hidden[v]:
            continue
        for j in range(min(int(counts[v]), n)):
            acc = 0.0
            for k in range(flat.var_ptr[v], flat.var_ptr[v + 1]):
                e = flat.var_edge[k]
                acc = acc + (f2v[e, j] * flat.edge_count[e] if flat.lifted else f2v[e, j])
            out[v, j] = acc
    return out


def log_area_twin(log_belief, a, b, npts, shift=None, max_log_value=700.0):
    """``log_area`` (EPBP:291-308): (area, shift) of the trapezoid of exp(belief - shift) on linspace(a, b, npts); the shift is the
    mean of the tabulated values, or max - 700 once max - mean exceeds 700"""
    x = np.linspace(a, b, npts)
    y = np.asarray(log_belief(x), dtype=np.float64)
    if shift is None:
        mean, top = float(y.mean()), float(y.max())
        shift = top - max_log_value if top - mean > max_log_value else mean
    w = np.exp(y - shift)
    return float((w[:-1] + w[1:]).sum() * (x[1] - x[0]) * 0.5), shift
