"""Hand-built particle-BP states, a NumPy ``np.longdouble`` twin of ``message_f_to_rv`` and a derived error bound for the f -> v
kernels of csrc/pbp.hip (heavy, small16 / small32, light / pair, fast, cq, generic).

A state is a small ``FlatGraph`` with chosen ``particles [V, n]`` (the targets' points), ``old_particles [V, n]`` (the partners'
points), ``v2f [E, n]`` and the counts ``np[var]``: no sweep is run.  The same arrays go into ``oracle.PbpOracle`` in
tests/test_pbp_f2v_host.py and into a solver on the device in tests/test_gpu_pbp_f2v.py.

The twin ``f2v_twin`` restates oracle/c/pbp_oracle.c::f2v_point (EPBP:176-194, HLBP:193-215): the joint particles of the hidden
partners in ``itertools.product`` order, observed partners at their value, a repeated variable iterated without a message,
messages read through ``edge_canon``, counts ``np[var]``.  Per output point it returns the max-shifted log-sum-exp ``L`` of
``log phi + sum m`` over the terms, ``M`` = the largest over the terms of the sum of |addend| over everything that is added up
to form the exponent (every coefficient product of the expanded polynomial, every message, the constant), the number of terms
and the largest exponent.  log phi is a plain longdouble restatement of csrc/potential.hpp; a table entry or hard formula that is
0 drops its term.

The bound (``f2v_bound``), in units of u = 2^-53 (one rounding to nearest; a rounding toward -inf costs 2 u):

    |out - L| <= u (c_t M + c_s n_terms + c_l max(1, |L|))

Direct paths (heavy rounds and range-guard fallback, small16 / small32 rounds, fast, cq; csrc/pbp.hip, csrc/fastmath.hpp):
  c_t = 18, the roundings proportional to the exponent's addends:
     3  the resolved coefficients (``quad2_of`` / ``cq_analyze``: at most three roundings per coefficient, e.g. -h h / (2 sig))
     5  the record's a_j = (ay y + by) y + c + m, five roundings, each on a partial sum of addends
     2  the record's b_j = axy y + bx, two roundings, multiplied by the point's x
     3  the scaling of (a_j, b_j) by 1 / step: the constant's own rounding and one per record half
     2  s = fma(b_j, x, a_j), rounded toward -inf in the floor form of the loop
     2  the point's own C = kx x x, two roundings
     1  the accumulating exponential's 3.8e-17 |t| (0.34 u |t|; ``test_device_exp_accumulate_accuracy``)
  c_s = 2: one addition per term, rounded toward -inf in the floor form (the terms are positive, so a chain of k additions
     costs at most 2 k u of the sum, whatever the order and the number of partial sums)
  c_l = 12: ``log_table``'s 2 ulp = 4 u |L| or 2.5e-16 = 2.3 u absolute (``test_device_log_accuracy``), plus what does not grow
     with M: the accumulating exponential's 6e-16 = 5.4 u, the product with exp(C_r) and its polynomial (2 u) -- 8 u, counted
     under max(1, |L|) so that the bound keeps its three-term form (this overcounts where |L| > 1)
ocml paths (generic, light, pair: ``exp`` and ``log`` of the device library, 1 ulp = 2 u each): the exponent is evaluated from
  the potential's parameters with at most as many roundings as above (c_t = 18 kept), c_s = 1 (additions to nearest),
  c_l = 6 (2 u |L| for the logarithm, 2 u for the exponential, one rounding each for v + m and for phi * exp(m)).
Grid recurrence (heavy and small kernels on a uniform grid; point t of the grid, t counted from the grid's first point, since the
  kernels carry G_t = G_0 q^t through all batches of 32): M is taken over the WHOLE grid of the edge (M_grid), as the range guard
  does, and
     c_t = 25 + 3 g: 11 for exp_core's argument a_j + b_j x_0 (coefficients 3, a_j 5, b_j 2, fma 1); 12 for t steps of
        q = exp_core(b_j h): b_j carries 5 u and the product b_j h one more, t |b_j h| <= 2 |b_j| X <= 2 M_grid; 2 for the
        epilogue's kx x_t x_t; 3 g for x_t = x_0 + t h in place of the tabulated point, g = their largest distance in units of
        u max|x| (``lhvi_pbp_describe`` accepts up to 16.2; a ``np.linspace`` grid has g of 1 to 2)
     + 5 t: per step exp_core's 2 ulp of q (4 u) and one multiplication -- the "~ t ulp" of docs/kernels_particle.md
     c_s = 2, c_l = 12 as above (4 u for the start value's exp_core is inside the 8).
  At M = 600, n = 64, |L| = 600: direct 2.0e-12, ocml 1.6e-12, recurrence at t = 127 and g = 2: 3.0e-12.  No path needs more
  than 1e-11.

Every output point of every state is *regular* (L >= -600 and every exponent <= 600: held to the bound) or *dead* (every
exponent <= -800, or no term at all: the fp64 sum is exactly 0 in any order, held to == -700.0); ``classify`` asserts that no
point lies between, and the builders assert it for every state.  The margin between -600 and -800 is the reason no test has to
decide what a partially denormal sum should be (the floor form carries its terms scaled by 2^-24).

Nothing here imports ``lhvi`` at module level or shares code with the kernels."""
import itertools
from dataclasses import dataclass, field

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -53
FLOOR = -700.0
REGULAR_MIN_L, REGULAR_MAX_EXPONENT, DEAD_MAX_EXPONENT = -600.0, 600.0, -800.0
LO, HI = -10.0, 10.0
# potential kinds (lhvi/potentials.py)
TABLE, GAUSSIAN, QUADRATIC, HYBRID_QUADRATIC, LINEAR_GAUSSIAN, X2, XY, MLN, MLN_HARD, IMAGE_NODE, IMAGE_EDGE = range(1, 12)
CQ_MAGIC = 17233.0
FAMILIES = ('heavy', 'small', 'light', 'pair', 'fast', 'cq', 'generic')      # 'pair': the light edges served per factor (paired_light)

C_T = {'direct': 18.0, 'ocml': 18.0, 'recurrence': 25.0}
C_S = {'direct': 2.0, 'ocml': 1.0, 'recurrence': 2.0}
C_L = {'direct': 12.0, 'ocml': 6.0, 'recurrence': 12.0}
C_GRID, C_STEP = 3.0, 5.0
PATH_OF_FAMILY = {'heavy': 'direct', 'small': 'direct', 'fast': 'direct', 'cq': 'direct', 'light': 'ocml', 'pair': 'ocml', 'generic': 'ocml'}


def f2v_bound(M, n_terms, L, path, t=None, grid_dev=0.0):
    """the bound of the module docstring; `path` in C_T.  'recurrence': `M` is the edge's M_grid, `t` the index of the point in
    its grid and `grid_dev` the grid's g"""
    M, L = np.asarray(M, dtype=np.float64), np.abs(np.asarray(L, dtype=np.float64))
    c_t = C_T[path] + (C_GRID * grid_dev if path == 'recurrence' else 0.0)
    out = c_t * M + C_S[path] * np.asarray(n_terms, dtype=np.float64) + C_L[path] * np.maximum(1.0, L)
    if path == 'recurrence':
        out = out + C_STEP * np.asarray(t, dtype=np.float64)
    return EPS * out


def oracle_bound(M, n_terms, L):
    """what the C oracle's own fp64 evaluation may differ from L by: it forms ``phi * pow(M_E, m)`` per term, phi itself mostly as
    ``pow(M_E, log phi)`` (oracle/c/potential_oracle.c), and adds the terms one after the other.  u (c_t M + n_terms +
    4 max(1, |L|)) with c_t = 14: the potential's exponent with at most twelve roundings on its addends (the quadratic forms are
    evaluated entry by entry), one for the message sum, and 0.53 (|log phi| + |m|) <= M for M_E = e (1 - 0.53 u) under the two
    ``pow``; n_terms roundings of the running sum; the two ``pow``, their product and ``log``, one rounding each (glibc: below
    1 ulp), the last one on |L|"""
    M, L = np.asarray(M, dtype=np.float64), np.abs(np.asarray(L, dtype=np.float64))
    return EPS * (14.0 * M + np.asarray(n_terms, dtype=np.float64) + 4.0 * np.maximum(1.0, L))


# ---- log phi in longdouble (or, with `num`, in any number type NumPy can hold in object arrays: mpmath's mpf) -------------------------
def _arr(a, num):
    a = np.asarray(a)
    if num is LD:
        return a.astype(LD)
    out = np.empty(a.shape, dtype=object)
    out.ravel()[:] = [num(float(v)) for v in a.ravel()] if a.dtype != object else list(a.ravel())
    return out


def _fn(a, num, name):
    """elementwise log / exp: NumPy's for longdouble, the number type's own (``num.log`` / ``num.exp``) on object arrays"""
    if num is LD:
        return getattr(np, name)(a)
    return np.frompyfunc(getattr(num, name), 1, 1)(a)


def _mln_formula(code, xs, num):
    """the postfix program of lhvi/expr.py (csrc/potential.hpp::mln_formula_on)"""
    st = []
    for op, val in zip(code[0::2], code[1::2]):
        op = int(op)
        if op == 0:
            st.append(xs[int(val)] + num(0))
        elif op == 1:
            st.append(num(float(val)))
        elif op == 7:
            st[-1] = -st[-1]
        elif op == 8:
            st[-1] = st[-1] * st[-1]
        elif op == 15:
            st[-1] = abs(st[-1])
        else:
            b, a = st.pop(), st.pop()
            if op == 2:
                r = a + b
            elif op == 3:
                r = a - b
            elif op == 4:
                r = a * b
            elif op == 5:
                r = a / b
            elif op == 6:
                r = a ** b
            else:
                cmp = {9: np.equal, 10: np.not_equal, 11: np.less, 12: np.less_equal, 13: np.greater, 14: np.greater_equal}[op]
                r = np.where(cmp(a, b).astype(bool), num(1), num(0))
            st.append(r)
    return st[0]


def _log_or_drop(value, num):
    pos = np.asarray(value > 0).astype(bool)
    lp = np.where(pos, _fn(np.where(pos, value, num(1)), num, 'log'), num(-np.inf))
    return lp, np.where(pos, abs(lp), num(0))


def log_phi(kind, par, xs, ix, num=LD):
    """(log phi, sum of |addend| of its expansion) at the argument arrays xs (broadcastable; discrete arguments hold their state
    VALUES) and state indices ix (int arrays; 0 for continuous arguments).  -inf: the term is dropped"""
    par = np.asarray(par, dtype=np.float64)
    p = _arr(par, num)
    half = num(1) / num(2)
    if kind == TABLE:
        nd = int(par[0])
        off = 0
        for i in range(nd):
            off = off * int(par[1 + i]) + ix[i]
        return _log_or_drop(p[1 + nd:][off], num)
    if kind == GAUSSIAN:
        n = int(par[0])
        mu, P = p[1:1 + n], p[1 + n:1 + n + n * n].reshape(n, n)
        lp, mm = num(0), num(0)
        for i in range(n):
            for j in range(n):
                lp = lp - half * (xs[i] - mu[i]) * P[i, j] * (xs[j] - mu[j])
                mm = mm + half * abs(P[i, j]) * (abs(xs[i]) + abs(mu[i])) * (abs(xs[j]) + abs(mu[j]))
        return lp, mm
    if kind in (QUADRATIC, HYBRID_QUADRATIC):
        if kind == QUADRATIC:
            n = int(par[0])
            A, b, c, args = p[1:1 + n * n].reshape(n, n), p[1 + n * n:1 + n * n + n], p[1 + n * n + n], xs
        else:
            Nd, n = int(par[0]), int(par[1])
            cfg, ncfg = 0, 1
            for i in range(Nd):
                cfg = cfg * int(par[2 + i]) + np.asarray(xs[i]).astype(np.float64).astype(np.int64)      # (indexed by the state's VALUE)
                ncfg *= int(par[2 + i])
            A = p[2 + Nd:2 + Nd + ncfg * n * n].reshape(ncfg, n, n)
            b = p[2 + Nd + ncfg * n * n:2 + Nd + ncfg * n * n + ncfg * n].reshape(ncfg, n)
            c = p[2 + Nd + ncfg * n * n + ncfg * n:2 + Nd + ncfg * n * n + ncfg * n + ncfg]
            args = xs[Nd:]
            A, b, c = np.moveaxis(A[cfg], (-2, -1), (0, 1)), np.moveaxis(b[cfg], -1, 0), c[cfg]
        lp, mm = c + num(0), abs(c) + num(0)
        for i in range(n):
            for j in range(n):
                t = A[i, j] * args[i] * args[j]
                lp, mm = lp + t, mm + abs(t)
            t = b[i] * args[i]
            lp, mm = lp + t, mm + abs(t)
        return lp, mm
    if kind == LINEAR_GAUSSIAN:
        a, sig = p[0], p[1]
        d = xs[1] - a * xs[0]
        return -(d * d) * half / sig, (xs[1] * xs[1] + 2 * abs(a * xs[0] * xs[1]) + a * a * xs[0] * xs[0]) * half / abs(sig)
    if kind == X2:
        t = -p[0] * (xs[0] * xs[0]) * half / p[1]
        return t, abs(t)
    if kind == XY:
        t = -p[0] * xs[0] * xs[1] * half / p[1]
        return t, abs(t)
    if kind in (MLN, MLN_HARD):
        f = _mln_formula(par[3:3 + 2 * int(par[1])], xs, num)
        if kind == MLN_HARD:
            return np.where(np.asarray(f > 0).astype(bool), num(0), num(-np.inf)), f * num(0)
        lp = f * p[0]
        head = int(par[2])
        if head < 3 or par[head] != CQ_MAGIC:
            return lp, abs(lp)
        # the conditional-quadratic block [CQ_MAGIC, arity, Nd, Nc, role[arity], dims[Nd], coef[ncfg][6]]: the addends the kernels form
        arity, Nd = int(par[head + 1]), int(par[head + 2])
        role, dims = par[head + 4:head + 4 + arity], par[head + 4 + arity:head + 4 + arity + Nd]
        coef = p[head + 4 + arity + Nd:].reshape(-1, 6)
        cfg, uv = 0, [num(0), num(0)]
        for a in range(arity):
            r = int(role[a])
            if r >= 0:
                cfg = cfg * int(dims[r]) + ix[a]
            else:
                uv[-1 - r] = xs[a]
        c = np.moveaxis(coef[cfg], -1, 0)
        u, v = uv
        return lp, abs(c[0] * u * u) + abs(c[1] * u * v) + abs(c[2] * v * v) + abs(c[3] * u) + abs(c[4] * v) + abs(c[5])
    if kind == IMAGE_NODE:
        u = (xs[0] - xs[1] - p[0]) / p[1]
        norm = _fn(_arr([2.506628274631], num) * p[1], num, 'log')[0]
        return -u * u * half - norm, ((abs(xs[0]) + abs(xs[1]) + abs(p[0])) / p[1]) ** 2 * half + abs(norm)
    if kind == IMAGE_EDGE:
        d = abs(xs[0] - xs[1])
        return _log_or_drop(d * p[0] + np.where(np.asarray(d > p[2]).astype(bool), p[3], _fn(-d / p[1], num, 'exp')), num)
    raise ValueError(kind)


# ---- the twin ------------------------------------------------------------------------------------------------------------------------
@dataclass
class Twin:
    L: np.ndarray           # [P]; -inf where no term is left
    M: np.ndarray           # float64 [P]
    n_terms: int
    top: np.ndarray         # float64 [P]: largest exponent per point; -inf where no term is left
    np_: int                # the first np_ points are the target's particles, the rest its integral points
    x: np.ndarray           # the points


def state_index(flat, v, x):
    d = flat.var_dom[v]
    if flat.dom_cont[d]:
        return 0
    vals = flat.dom_val[flat.dom_ptr[d]:flat.dom_ptr[d + 1]]
    hit = np.flatnonzero(vals == x)
    return int(hit[0]) if hit.size else int(x)


def f2v_twin(flat, state, e, nj=None, np_=None, T=None, partner_value=None, mutant=None, num=LD, points=None):
    """the message of edge e at the target's first `np_` particles and first `T` integral points (default: all of them), from the
    first `nj` particles of each hidden partner (default: np[partner]); `partner_value`: the partner(s) observed at that value.
    `mutant`: a deliberately wrong twin -- 'swap' (arguments 0 and 1 exchanged in the potential), 'drop' (the last partner
    particle left out), 'nomsg' (the first partner's message omitted), 'shift' (integral point t + 1 in place of t).
    `num`: the number type (``np.longdouble``; tests/test_pbp_f2v_host.py passes a 50-digit mpmath type); `points`: only these"""
    e = int(e)
    f = int(flat.edge_fac[e])
    base, arity = int(flat.fac_ptr[f]), int(flat.fac_ptr[f + 1] - flat.fac_ptr[f])
    pos, tv = e - base, int(flat.edge_var[e])
    pot = int(flat.fac_pot[f])
    kind, par = int(flat.pot_kind[pot]), flat.pot_param[flat.pot_off[pot]:flat.pot_off[pot + 1]]
    d = int(flat.var_dom[tv])
    cont = bool(flat.dom_cont[d])
    grid = flat.dom_val[flat.dom_ptr[d]:flat.dom_ptr[d + 1]] if cont else np.zeros(0)
    np_ = int(state.counts[tv]) if np_ is None else int(np_)
    T = grid.size if T is None else int(T)
    grid = grid[:T]
    if mutant == 'shift' and T > 1:
        grid = np.roll(grid, -1)
    x = np.concatenate([state.particles[tv, :np_], grid])
    xi = np.concatenate([np.arange(np_), np.arange(T)]) if not cont else np.zeros(np_ + T, dtype=np.int64)
    if points is not None:
        x, xi = x[points], xi[points]
    # the partners: (values, state indices, messages) per argument
    vals, idxs, msgs, first = [], [], [], True
    for a in range(arity):
        if a == pos:
            vals.append(None), idxs.append(None), msgs.append(None)
            continue
        v = int(flat.edge_var[base + a])
        value = flat.var_value[v] if partner_value is None else float(partner_value)
        if np.isnan(value):
            cnt = int(state.counts[v]) if nj is None else min(int(nj), int(state.counts[v]))
            if mutant == 'drop':
                cnt -= 1
            y = state.old_particles[v, :cnt]
            m = state.v2f[int(flat.edge_canon[base + a]), :cnt] if v != tv else np.zeros(cnt)     # (a repeated variable: no message)
            if mutant == 'nomsg' and first:
                m = np.zeros(cnt)
            first = False
            vals.append(y), idxs.append(np.arange(cnt)), msgs.append(m)
        else:
            vals.append(np.array([value])), idxs.append(np.array([state_index(flat, v, value)])), msgs.append(np.zeros(1))
    others = [a for a in range(arity) if a != pos]
    sizes = [vals[a].size for a in others]
    n_terms = int(np.prod(sizes)) if others else 1
    # the joint particles in itertools.product order (last argument fastest): an index array per partner
    joint = list(zip(*itertools.product(*[range(k) for k in sizes]))) if others and n_terms else [()] * len(others)
    xs, ix = [None] * arity, [None] * arity
    msum, mabs = _arr(np.zeros((n_terms, 1)), num), _arr(np.zeros((n_terms, 1)), num)
    for a, sel in zip(others, joint):
        sel = np.asarray(sel, dtype=np.int64)
        xs[a], ix[a] = _arr(vals[a][sel], num)[:, None], idxs[a][sel][:, None]
        msum, mabs = msum + _arr(msgs[a][sel], num)[:, None], mabs + _arr(np.abs(msgs[a][sel]), num)[:, None]
    xs[pos], ix[pos] = _arr(x, num)[None, :], xi[None, :]
    if mutant == 'swap':
        xs[0], xs[1], ix[0], ix[1] = xs[1], xs[0], ix[1], ix[0]
    ninf = num(-np.inf)
    with np.errstate(invalid='ignore', over='ignore'):
        lp, mm = log_phi(kind, par, xs, ix, num)
        t = np.broadcast_to(lp + msum, (n_terms, x.size))
        live = np.asarray(t > ninf).astype(bool)
        absum = np.where(live, np.broadcast_to(mm + mabs, (n_terms, x.size)), num(0))
        if n_terms == 0:
            return Twin(L=np.full(x.size, ninf), M=np.zeros(x.size), n_terms=0, top=np.full(x.size, -np.inf), np_=np_, x=x)
        top = t.max(axis=0)
        has = np.asarray(top > ninf).astype(bool)
        safe = np.where(has, top, num(0))
        L = np.where(has, safe + _fn(_fn(np.where(live, t - safe[None, :], ninf), num, 'exp').sum(axis=0) + np.where(has, num(0), num(1)), num, 'log'), ninf)
    if num is LD:
        L = L.astype(LD)
    return Twin(L=L, M=absum.max(axis=0).astype(np.float64), n_terms=n_terms, top=top.astype(np.float64), np_=np_, x=x)


def classify(tw):
    """(regular, dead) masks over the twin's points; asserts that every point is exactly one of the two"""
    L = np.asarray(tw.L, dtype=np.float64)
    regular = (L >= REGULAR_MIN_L) & (tw.top <= REGULAR_MAX_EXPONENT)
    dead = tw.top <= DEAD_MAX_EXPONENT
    assert (regular ^ dead).all(), 'a point between the classes: L = %s, top = %s' % (L[~(regular ^ dead)], tw.top[~(regular ^ dead)])
    return regular, dead


def grid_deviation(flat, d):
    """g of the bound: the largest distance of a continuous domain's integral points from x_0 + t h, in units of u max|x|"""
    pts = flat.dom_val[flat.dom_ptr[d]:flat.dom_ptr[d + 1]].astype(LD)
    if pts.size < 2:
        return 0.0
    h = LD(np.float64(pts[-1] - pts[0]) / np.float64(pts.size - 1))
    dev = np.abs(pts - (pts[0] + np.arange(pts.size).astype(LD) * h)).max()
    return float(dev / (LD(EPS) * max(abs(pts[0]), abs(pts[-1])))) + 1.0       # (+ 1: the kernel's own fma(t, h, x_0))


# ---- states --------------------------------------------------------------------------------------------------------------------------
@dataclass
class F2vState:
    """``flat``, ``n``, ``particles`` / ``old_particles [V, n]`` (discrete rows hold the states, as ``PbpOracle.set_particles`` writes
    them), ``v2f [E, n]``, ``counts [V]``, ``epbp`` (the flags of EPBP, else HybridLBP's), ``labels [F]``: what the builder put
    there (the class of docs/kernels_particle.md 4.3 follows from it and from the evidence: ``expected_family``), ``kinds [E]``:
    the range kind of the message row of edge e ('ordinary', 'dominated', 'up', 'down', 'dead')"""
    flat: object
    n: int
    particles: np.ndarray
    old_particles: np.ndarray
    v2f: np.ndarray
    counts: np.ndarray
    epbp: bool
    labels: list
    uniform: bool = True
    kinds: list = field(default_factory=list)
    _twins: dict = field(default_factory=dict, repr=False)

    def oracle(self):
        from oracle import oracle
        o = oracle.PbpOracle(self.flat, self.n, ep=False, epbp=self.epbp, var_threshold=3 if self.epbp else 5)
        o.set_particles(self.old_particles)
        o.set_particles(self.particles)
        o.v2f = np.ascontiguousarray(self.v2f)
        assert (o.np == self.counts).all() and (o.particles == self.particles).all() and (o.old_particles == self.old_particles).all()
        return o

    def edges(self):
        """the hidden, canonical edges: those a sweep computes a message for"""
        fl = self.flat
        return np.flatnonzero(fl.var_hidden[fl.edge_var] & (fl.edge_canon == np.arange(fl.E)))

    def twin(self, e):
        """the twin of edge e, computed once and kept"""
        if int(e) not in self._twins:
            self._twins[int(e)] = f2v_twin(self.flat, self, e)
        return self._twins[int(e)]

    def check_classes(self):
        for e in self.edges():
            classify(self.twin(e))
        return self


def _finish(flat, n, particles, old, v2f, epbp, labels, **kw):
    from oracle import oracle
    counts = oracle.pbp_counts(flat, n)
    out = []
    for p in (particles, old):
        p = np.array(p, dtype=np.float64)
        for v in np.flatnonzero(flat.var_hidden & ~flat.var_cont):
            vals = flat.dom_val[flat.dom_ptr[flat.var_dom[v]]:flat.dom_ptr[flat.var_dom[v] + 1]]
            p[v, :vals.size] = vals
        out.append(np.ascontiguousarray(p))
    return F2vState(flat=flat, n=int(n), particles=out[0], old_particles=out[1], v2f=np.ascontiguousarray(v2f, dtype=np.float64),
                    counts=np.asarray(counts), epbp=epbp, labels=labels, **kw)


class _Builder:
    def __init__(self, domains):
        self.domains, self.var_dom, self.var_value, self.scopes, self.specs, self.labels = list(domains), [], [], [], [], []

    def var(self, dom=0, value=np.nan):
        self.var_dom.append(dom)
        self.var_value.append(value)
        return len(self.var_dom) - 1

    def factor(self, scope, kind, par, label):
        assert len(set(scope)) == len(scope)
        self.scopes.append(tuple(int(v) for v in scope))
        self.specs.append((int(kind), [float(t) for t in par]))
        self.labels.append(label)

    def flat(self):
        from lhvi.flat import build_flat
        fac_ptr = np.concatenate([[0], np.cumsum([len(s) for s in self.scopes])]).astype(np.int32)
        edge_var = np.array([v for s in self.scopes for v in s], dtype=np.int32)
        return build_flat(fac_ptr, edge_var, np.arange(len(self.scopes), dtype=np.int32), self.specs,
                          np.array(self.var_value, dtype=np.float64), np.array(self.var_dom, dtype=np.int32), self.domains)


def grid_points(T, uneven=False):
    pts = np.linspace(LO, HI, T) if T else np.zeros(0)
    return np.sign(pts) * np.abs(pts) ** 1.3 / 10 ** 0.3 if uneven else pts


def _domains(T, uneven):
    from lhvi.graph import Domain
    return [Domain((LO, HI), continuous=True, integral_points=grid_points(T, uneven))] + \
           [Domain(tuple(float(i) for i in range(k)), continuous=False) for k in (2, 3, 4, 5)]


def _pair_par(rng, kind):
    """a weak pair potential of the given kind: |log phi| stays below ~250 on [-10, 10]^2"""
    if kind == LINEAR_GAUSSIAN:
        return [float(rng.uniform(0.3, 1.5) * rng.choice([-1.0, 1.0])), float(rng.uniform(1.5, 4.0))]
    if kind == GAUSSIAN:
        p0, p1, rho = rng.uniform(0.05, 0.5, 2).tolist() + [float(rng.uniform(-0.8, 0.8))]
        off = rho * np.sqrt(p0 * p1)
        return [2.0] + rng.uniform(-2, 2, 2).tolist() + [p0, off, off, p1]
    if kind == QUADRATIC:                  # -0.5 p (x0 - (k x1 + h))^2 + s x1 + c0 with the cross term split unevenly over A01 / A10
        p, k, h = float(rng.uniform(0.1, 0.45)), float(rng.uniform(-1, 1)), float(rng.uniform(-2, 2))
        s, c0, split = float(rng.uniform(-0.3, 0.3)), float(rng.uniform(-1, 1)), float(rng.uniform(0, 1))
        return [2.0, -0.5 * p, split * p * k, (1 - split) * p * k, -0.5 * p * k * k, p * h, -p * k * h + s, -0.5 * p * h * h + c0]
    if kind == XY:
        return [float(rng.uniform(0.1, 0.5) * rng.choice([-1.0, 1.0])), float(rng.uniform(1, 3))]
    raise ValueError(kind)


PAIR_KINDS = {'gaussian': GAUSSIAN, 'quadratic': QUADRATIC, 'linear_gaussian': LINEAR_GAUSSIAN, 'xy': XY}


def zoo_graph(T, uneven=False, seed=3, reps=8):
    """every class of the routing table of docs/kernels_particle.md 4.3 in one graph; returns (flat, labels).  Each pattern comes
    `reps` times with every argument hidden and reps / 2 times per observed argument; every factor has variables of its own"""
    from lhvi.mln import MLNPotential, eq_op
    rng = np.random.default_rng(seed)
    doms = _domains(T, uneven)
    b = _Builder(doms)
    C, D = 0, {2: 1, 3: 2, 4: 3, 5: 4}

    def cv(obs=False):
        return b.var(C, float(rng.uniform(-8, 8)) if obs else np.nan)

    def dv(k, obs=False):
        return b.var(D[k], float(rng.integers(k)) if obs else np.nan)

    def patterns(arity):
        """hidden / observed patterns: all hidden `reps` times, each single observed argument reps / 2 times"""
        out = [(False,) * arity] * reps
        for a in range(arity):
            out += [tuple(i == a for i in range(arity))] * (reps // 2)
        return out

    for name, kind in PAIR_KINDS.items():
        for o0, o1 in patterns(2):
            b.factor((cv(o0), cv(o1)), kind, _pair_par(rng, kind), name)
    for _ in range(reps):
        b.factor((cv(),), X2, [float(rng.uniform(0.5, 1.5)), float(rng.uniform(2, 10))], 'x2')
    for k in (2, 3, 4):
        for o0, o1 in patterns(2):
            par = [1, 1, k] + rng.uniform(-0.5, -0.05, k).tolist() + rng.uniform(-1, 1, k).tolist() + rng.uniform(-1, 1, k).tolist()
            b.factor((dv(k, o0), cv(o1)), HYBRID_QUADRATIC, par, 'hybrid%d' % k)
    for (k0, k1), name in (((2, 2), 'table22'), ((3, 4), 'table34'), ((5, 2), 'table52')):
        for o0, o1 in patterns(2):
            tab = rng.uniform(0.2, 3.0, (k0, k1))
            if name == 'table34':
                tab[int(rng.integers(k0)), int(rng.integers(k1))] = 0.0           # (a zero entry drops its term)
            b.factor((dv(k0, o0), dv(k1, o1)), TABLE, [2, k0, k1] + tab.ravel().tolist(), name)
    for o in patterns(3):
        b.factor((dv(2, o[0]), dv(3, o[1]), dv(2, o[2])), TABLE, [3, 2, 3, 2] + rng.uniform(0.2, 3.0, 12).tolist(), 'table232')
    # conditionally quadratic MLN formulas: unary eq_op(x[0], 1) and x[0] * eq_op(x[1], x[2]) under every evidence pattern
    for _ in range(reps):
        kind, par = MLNPotential(lambda x: eq_op(x[0], 1), w=float(rng.uniform(0.1, 0.5))).device_spec((doms[C],))
        b.factor((cv(),), kind, par, 'cq1')
    cq_patterns = [(False, False, False)] * reps + [(True, False, False)] * reps + [(False, True, False)] * reps + \
                  [(False, False, True)] * reps + [(True, True, False), (True, False, True), (False, True, True)] * (reps // 2)
    for o in cq_patterns:
        kind, par = MLNPotential(lambda x: x[0] * eq_op(x[1], x[2]), w=float(rng.uniform(0.1, 0.5))).device_spec((doms[D[2]], doms[C], doms[C]))
        b.factor((dv(2, o[0]), cv(o[1]), cv(o[2])), kind, par, 'cq3')
    for o0, o1 in patterns(2):
        kind, par = MLNPotential(lambda x: -abs(x[0] - 2 * x[1]), w=float(rng.uniform(0.3, 1.0))).device_spec((doms[C], doms[C]))
        assert par[2] == 0.0                # not conditionally quadratic: no block
        b.factor((cv(o0), cv(o1)), kind, par, 'formula')
    for o0, o1 in patterns(2):
        b.factor((cv(o0), cv(o1)), IMAGE_NODE, [float(rng.uniform(-1, 1)), float(rng.uniform(1.5, 3.0))], 'image_node')
        b.factor((cv(o0), cv(o1)), IMAGE_EDGE, [0.01, 2.0, 6.0, float(np.e ** (-6.0 / 2.0))], 'image_edge')
    return b.flat(), b.labels


def _spice(rng, flat, p, n):
    """the domain's bounds, a duplicate and +-0.0 among a hidden continuous variable's particles, as far as n has room"""
    for v in np.flatnonzero(flat.var_hidden & flat.var_cont):
        special = [LO, HI, None, 0.0, -0.0]
        cols = rng.permutation(n)[:len(special) + 1]
        for c, s in zip(cols[1:], special):
            p[v, c] = p[v, cols[0]] if s is None else s
    return p


def zoo(n, T, uneven=False, seed=3, reps=8):
    """the zoo's graph with particles uniform on the domain and log-messages uniform on [-5, 5]: every row 'ordinary'"""
    flat, labels = zoo_graph(T, uneven, seed, reps)
    rng = np.random.default_rng(seed + 1000 * n + T)
    st = _finish(flat, n, rng.uniform(LO, HI, (flat.V, n)), rng.uniform(LO, HI, (flat.V, n)), rng.uniform(-5, 5, (flat.E, n)),
                 True, labels, uniform=not uneven, kinds=['ordinary'] * flat.E)
    return st.check_classes()


RANGE_KINDS = ('ordinary', 'dominated', 'up', 'down', 'dead')


def ranges(n, T, seed=3, reps=8):
    """the zoo's graph with hand-written message rows of five kinds -- ordinary (|m| <= 5), dominated (one particle's message 500
    above the others), up / down (the whole row at +550 / -550) and dead (the whole row at -900) -- and with the domain's bounds,
    duplicates and +-0.0 among the particles.  Per factor one argument's row is rewritten, the kinds in turn; a row under which an
    output point of the factor's other edges would fall between the classes (a potential too strong for it) stays ordinary"""
    flat, labels = zoo_graph(T, False, seed, reps)
    rng = np.random.default_rng(seed + 2000 * n + T)
    st = _finish(flat, n, _spice(rng, flat, rng.uniform(LO, HI, (flat.V, n)), n), _spice(rng, flat, rng.uniform(LO, HI, (flat.V, n)), n),
                 rng.uniform(-5, 5, (flat.E, n)), True, labels, kinds=['ordinary'] * flat.E)
    turn = 0
    for f in range(flat.F):
        base, arity = int(flat.fac_ptr[f]), int(flat.fac_ptr[f + 1] - flat.fac_ptr[f])
        hidden = [a for a in range(arity) if flat.var_hidden[flat.edge_var[base + a]]]
        if arity < 2 or len(hidden) < 2:
            continue                            # (a row matters only where another hidden argument reads it)
        kind = RANGE_KINDS[turn % len(RANGE_KINDS)]
        a = hidden[(turn // len(RANGE_KINDS)) % len(hidden)]
        turn += 1
        row, cnt = base + a, int(st.counts[flat.edge_var[base + a]])
        keep = st.v2f[row].copy()
        if kind == 'dominated':
            st.v2f[row, int(rng.integers(cnt))] += 500.0
        elif kind in ('up', 'down'):
            st.v2f[row, :cnt] = (550.0 if kind == 'up' else -550.0) + rng.uniform(-2, 2, cnt)
        elif kind == 'dead':
            st.v2f[row, :cnt] = -900.0
        try:
            for t in hidden:
                if t != a:
                    classify(f2v_twin(flat, st, base + t))
            st.kinds[row] = kind
        except AssertionError:
            st.v2f[row] = keep
    have = {k: st.kinds.count(k) for k in RANGE_KINDS}
    assert all(have[k] >= 8 for k in RANGE_KINDS), have
    return st.check_classes()


def lifted(n=16, T=20, seed=5, groups=(3, 4, 3, 5, 4, 3, 6, 5)):
    """a lifted graph with counts and a scope that repeats a cluster: hubs with m leaves each (a LinearGaussian per leaf, an X2 on
    every variable) whose leaves are joined in a ring by one XY potential per hub.  Every leaf is once argument 0 and once
    argument 1 of a ring factor, so the partition 'one cluster per hub, one for its leaves' is stable; the ring factors of a hub
    collapse into one factor whose scope is (leaves, leaves).  Lifted with ``lifting.lift_flat`` on the host; particles and
    messages are written for the LIFTED graph"""
    from lhvi import lifting
    rng = np.random.default_rng(seed)
    b = _Builder(_domains(T, False))
    rv_color, f_color, labels_by_color = [], [], {}
    for gi, m in enumerate(groups):
        hub = b.var()
        rv_color.append(2 * gi)
        leaves = [b.var() for _ in range(m)]
        rv_color += [2 * gi + 1] * m
        specs = {'x2 hub': (X2, [1.0, float(rng.uniform(4, 10))]), 'x2 leaf': (X2, [1.0, float(rng.uniform(4, 10))]),
                 'linear_gaussian': (LINEAR_GAUSSIAN, _pair_par(rng, LINEAR_GAUSSIAN)), 'ring': (XY, _pair_par(rng, XY))}

        def add(scope, name):
            b.factor(scope, *specs[name], name.split()[0])
            f_color.append(4 * gi + list(specs).index(name))
        add((hub,), 'x2 hub')
        for i, leaf in enumerate(leaves):
            add((hub, leaf), 'linear_gaussian')
            add((leaf,), 'x2 leaf')
            add((leaf, leaves[(i + 1) % m]), 'ring')
    ground = b.flat()
    remap = {c: i for i, c in enumerate(dict.fromkeys(f_color))}
    fc = np.array([remap[c] for c in f_color], dtype=np.int32)
    flat = lifting.lift_flat(ground, np.array(rv_color, dtype=np.int32), fc)
    assert flat.lifted and flat.V == 2 * len(groups) and (flat.edge_canon != np.arange(flat.E)).sum() == len(groups)
    assert sorted(set(flat.edge_count.tolist())) != [1.0]
    first = {}
    for i, c in enumerate(fc):
        first.setdefault(int(c), b.labels[i])
    labels = [first[c] for c in range(flat.F)]
    for f in np.flatnonzero(np.diff(flat.fac_ptr) == 2):
        if flat.edge_var[flat.fac_ptr[f]] == flat.edge_var[flat.fac_ptr[f] + 1]:
            labels[f] = 'repeat'
    st = _finish(flat, n, rng.uniform(LO, HI, (flat.V, n)), rng.uniform(LO, HI, (flat.V, n)), rng.uniform(-5, 5, (flat.E, n)),
                 False, labels, kinds=['ordinary'] * flat.E)
    return st.check_classes()


# ---- which family serves which edge (docs/kernels_particle.md 4.3), from the builder's labels and the evidence -------------------------
def _expected_family(st, e, cq_routing, small_f2v, long_grid):
    fl, n = st.flat, st.n
    f = int(fl.edge_fac[e])
    base, arity = int(fl.fac_ptr[f]), int(fl.fac_ptr[f + 1] - fl.fac_ptr[f])
    pos, tv, label = int(e) - base, int(fl.edge_var[e]), st.labels[f]
    tcont = bool(fl.var_cont[tv])
    np_t = int(st.counts[tv])
    T = int(fl.var_nstates[tv]) if tcont else 0
    hidden = [bool(fl.var_hidden[fl.edge_var[base + a]]) for a in range(arity)]

    def heavy_class(nj):
        """continuous target, constant x^2 coefficient, nj partner particles (1: observed or none)"""
        if small_f2v and nj <= 32 and np_t <= 32:
            return 'small'
        two_rounds = np_t + T <= 128
        recurrence = long_grid and st.uniform and T >= 2 and nj >= 24 and T <= 128 and np_t <= 128
        return 'heavy' if nj <= 64 and (two_rounds or recurrence) else 'fast'

    if label in PAIR_KINDS or label == 'ring':
        pv = int(fl.edge_var[base + 1 - pos])
        return heavy_class(int(st.counts[pv]) if hidden[1 - pos] else 1)
    if label.startswith('hybrid'):
        states = int(label[6:])
        if tcont:                               # continuous target, discrete partner
            npt = states if hidden[0] else 1
            return 'light' if npt <= 2 and np_t + T <= 128 else 'fast'
        nj = int(st.counts[fl.edge_var[base + 1]]) if hidden[1] else 1
        return 'light' if states <= 2 and nj <= 64 else 'fast'
    if label == 'cq1' and cq_routing:
        return heavy_class(1) if np_t + T <= 128 and np_t <= 64 else 'generic'
    if label == 'cq3' and cq_routing:
        if (tcont and (np_t + T > 128 or np_t > 64)) or n > 64:
            return 'generic'                    # the descriptor kernels' limits: output points, staged particles
        if tcont:
            other = 3 - pos
            if not hidden[0]:
                return heavy_class(n if hidden[other] else 1)
            return 'cq' if hidden[other] else 'light'
        nh = int(hidden[1]) + int(hidden[2])
        return {2: 'cq', 1: 'light', 0: 'generic'}[nh]
    return 'generic'                            # tables, unary X2, arity 3, image potentials, other formulas, a repeated cluster


def expected_family(st, e, paired_light=True, cq_routing=True, small_f2v=True, long_grid=False):
    """the family of FAMILIES that the routing table names for the hidden, canonical edge e.  `long_grid`: edges with more than
    128 output points on a uniform grid of at most 128 points join the heavy list (``long_grid_min_edges`` = 0)"""
    fam = _expected_family(st, e, cq_routing, small_f2v, long_grid)
    return 'pair' if fam == 'light' and paired_light else fam
