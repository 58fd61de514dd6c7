"""Small hybrid MLNs for the HybridMaxWalkSAT tests (host-built object graphs; no data files)."""
import numpy as np

from lhvi.graph import F, RV, Domain, Graph
from lhvi.mln import MLNHardPotential, MLNPotential, eq_op, or_op
from lhvi.potentials import GaussianPotential


def small_hybrid():
    """an MLNHardPotential, a GaussianPotential, a clause with a hidden discrete variable, one all-observed factor"""
    db = Domain((0, 1))
    dc = Domain((-3, 3), continuous=True, integral_points=np.linspace(-3, 3, 20))
    d1, d2, d3 = RV(db), RV(db), RV(db)
    c1, c2, c3 = RV(dc), RV(dc), RV(dc, value=0.7)
    o1 = RV(db, value=1)
    fs = [F(MLNHardPotential(lambda x: or_op(x[0], x[1])), nb=[d1, d2]),
          F(GaussianPotential([0.5, -0.5], [[1.0, 0.3], [0.3, 2.0]]), nb=[c1, c2]),
          F(MLNPotential(lambda x: x[0] * eq_op(x[1], x[2]), w=1.5), nb=[d1, c1, c3]),
          F(MLNPotential(lambda x: x[0], w=-0.8), nb=[d2]),
          F(MLNPotential(lambda x: 1 - x[0] * x[1], w=0.6), nb=[d3, d2]),
          F(MLNPotential(lambda x: x[0] * eq_op(x[1], 0.2), w=2.0), nb=[o1, c3])]
    g = Graph()
    g.rvs = {d1, d2, d3, c1, c2, c3, o1}
    g.factors = set(fs)
    g.init_nb()
    return g


# ---- models for the free-running check (tests/mws_twin.py): shapes the three models above leave unvisited -------------------------
def _weights(rng, n, lo=0.3, hi=2.5, signed=False):
    """n weights from rng.uniform, rounded to 3 decimals, no two of equal size: generic, so exact score ties are rare"""
    out, seen = [], set()
    while len(out) < n:
        w = round(float(rng.uniform(lo, hi)), 3)
        if w not in seen:
            seen.add(w)
            out.append(-w if signed and rng.random() < 0.5 else w)
    return out


def _graph(rvs, fs):
    g = Graph()
    g.rvs, g.factors = set(rvs), set(fs)
    g.init_nb()
    return g


def many_clauses(n, seed=0):
    """n discrete clauses of arity 1-3 in factor order over about n / 2 binary variables (a fifth observed): about a quarter
    MLNHardPotential -- monotone disjunctions over a pool of eight variables, so that a walk always repairs one and the search
    does get past the hard branch --, the rest MLNPotential whose formula is 0 on some states (phi == 1: unsatisfied there).
    Every clause keeps a hidden variable, so the discrete list has exactly n entries: n = 63 / 64 / 65 / 130 put its end on
    either side of the 64-clause chunks of the unsatisfied scan.  Two continuous variables under three numeric factors."""
    rng = np.random.default_rng(1000 + n + seed)
    db = Domain((0, 1))
    dc = Domain((-4, 4), continuous=True, integral_points=np.linspace(-4, 4, 9))
    nv = max(10, n // 2)
    rvs = [RV(db) for _ in range(nv)]
    pool = rvs[:8]                                   # the hard clauses' variables: all hidden
    for rv in rvs[8:]:
        if rng.random() < 0.25:                      # a fifth of all discrete variables
            rv.value = int(rng.integers(0, 2))
    hidden = [rv for rv in rvs if rv.value is None]
    hard_forms = {1: lambda x: x[0], 2: lambda x: or_op(x[0], x[1]), 3: lambda x: or_op(or_op(x[0], x[1]), x[2])}
    soft_forms = {1: [lambda x: x[0], lambda x: 1 - x[0]],
                  2: [lambda x: or_op(x[0], x[1]), lambda x: x[0] * (1 - x[1]), lambda x: 1 - x[0] * x[1]],
                  3: [lambda x: or_op(or_op(x[0], x[1]), x[2]), lambda x: 1 - x[0] * x[1] * x[2], lambda x: x[0] * or_op(x[1], x[2])]}
    ws = _weights(rng, n, signed=True)
    fs = []
    for i in range(n):
        tail = i >= n - 3                            # the last clauses: soft and unsatisfied on most states
        if not tail and rng.random() < 0.25:
            a = int(rng.choice([1, 1, 1, 2, 2, 3]))
            nb = [pool[j] for j in rng.choice(len(pool), size=a, replace=False)]
            fs.append(F(MLNHardPotential(hard_forms[a]), nb=nb))
            continue
        a = 3 if tail else int(rng.integers(1, 4))
        first = hidden[int(rng.integers(len(hidden)))]
        rest = [rv for rv in rvs if rv is not first]
        nb = [first] + [rest[j] for j in rng.choice(len(rest), size=a - 1, replace=False)]
        form = (lambda x: x[0] * x[1] * x[2]) if tail else soft_forms[a][int(rng.integers(len(soft_forms[a])))]
        fs.append(F(MLNPotential(form, w=ws[i]), nb=nb))
    c1, c2 = RV(dc), RV(dc)
    wc = _weights(rng, 3)
    fs += [F(MLNPotential(lambda x: eq_op(x[0], x[1]), w=wc[0]), nb=[c1, c2]),
           F(MLNPotential(lambda x: eq_op(x[0], 1.5), w=wc[1]), nb=[c1]),
           F(MLNPotential(lambda x: eq_op(x[0], -0.7), w=wc[2]), nb=[c2])]
    return _graph(rvs + [c1, c2], fs)


def wide_hub(seed=0):
    """continuous hubs of 65, 70 and 130 factors, each leaf tied to its hub by a soft eq_op formula (a quarter of the leaves
    observed); a binary hub of 70 soft clauses; one arity-3 clause over the 65- and the 70-factor hub and a leaf, whose
    neighbourhood scan runs across two long rows.  A variable of more than 64 factors takes the lane-strided loops round twice."""
    rng = np.random.default_rng(2000 + seed)
    # values of order 1: a hub's local score is then a sum of ~100 terms of order 1, whose rounding (~1e-14) stays below what
    # L-BFGS-B's forward difference (step 1e-8) can turn into a gradient of pgtol = 1e-5; on (-5, 5) the sums reach 1e3-1e4,
    # the gradient noise pgtol, and two correct summation orders end 2e-7 apart
    dc = Domain((-1, 1), continuous=True, integral_points=np.linspace(-1, 1, 11))
    db = Domain((0, 1))
    hubs = [RV(dc) for _ in range(3)]
    rvs, fs = list(hubs), []
    first_leaf = None
    for hub, leaves in zip(hubs, (64, 69, 130)):        # the arity-3 clause below is the 65th / 70th factor of the first two
        for w in _weights(rng, leaves, 0.2, 1.5):
            leaf = RV(dc, value=round(float(rng.uniform(-0.8, 0.8)), 3) if rng.random() < 0.25 else None)
            first_leaf = first_leaf if first_leaf is not None or leaf.value is not None else leaf
            rvs.append(leaf)
            fs.append(F(MLNPotential(lambda x: eq_op(x[0], x[1]), w=w), nb=[hub, leaf]))
    w3 = _weights(rng, 1)[0]
    fs.insert(40, F(MLNPotential(lambda x: eq_op(x[0] + x[1], x[2]), w=w3), nb=[hubs[0], hubs[1], first_leaf]))
    b = RV(db)
    partners = [RV(db, value=v) for v in (None, None, 1, None, 0, None, None)]
    forms = [lambda x: or_op(x[0], x[1]), lambda x: x[0] * x[1], lambda x: 1 - x[0] * x[1], lambda x: x[0] * (1 - x[1])]
    for i, w in enumerate(_weights(rng, 70, signed=True)):
        fs.append(F(MLNPotential(forms[int(rng.integers(len(forms)))], w=w), nb=[b, partners[i % 7]]))
    # factor ids follow creation order, not list order: renumber so that the arity-3 clause sits inside the first hub's row
    for f in fs:
        f.id = next(F.id_counter)
    return _graph(rvs + [b] + partners, fs)


def multi_state(seed=0):
    """hidden variables over Domain((0, 1, 2)) and Domain((1, 2, 3, 5)), read by MLN formulas only (a table lookup of an
    off-domain value is a valid input nowhere; the walk's 1 - x does reach such values and the formulas evaluate there):
    about 20 soft clauses, 4 hard ones, two continuous variables tied to the discrete ones by mixed formulas"""
    rng = np.random.default_rng(3000 + seed)
    d3, d4 = Domain((0, 1, 2)), Domain((1, 2, 3, 5))
    dc = Domain((-2, 6), continuous=True, integral_points=np.linspace(-2, 6, 9))
    a = [RV(d3) for _ in range(4)] + [RV(d3, value=2)]
    b = [RV(d4) for _ in range(3)] + [RV(d4, value=3)]
    c1, c2 = RV(dc), RV(dc)
    soft = [(lambda x: eq_op(x[0], 2), 1), (lambda x: eq_op(x[0], x[1]), 2), (lambda x: x[0] * (x[1] - 1), 2),
            (lambda x: (x[0] - 1) * (x[1] - 2), 2), (lambda x: x[0] * (x[1] - 3) * x[2], 3), (lambda x: eq_op(x[0] + x[1], x[2]), 3),
            (lambda x: (x[0] - 2) * x[0], 1), (lambda x: (x[0] - 5) * (x[1] - 2), 2)]
    ws = _weights(rng, 20, 0.05, 0.6, signed=True)
    disc = a + b
    hid = [rv for rv in disc if rv.value is None]
    fs = []
    for i in range(20):
        form, ar = soft[i % len(soft)]
        first = hid[i % len(hid)]
        rest = [rv for rv in disc if rv is not first]
        fs.append(F(MLNPotential(form, w=ws[i]), nb=[first] + [rest[j] for j in rng.choice(len(rest), size=ar - 1, replace=False)]))
    fs += [F(MLNHardPotential(lambda x: x[0] + x[1] - 1), nb=[a[0], a[1]]),          # a state sum above 1
           F(MLNHardPotential(lambda x: 4 - x[0]), nb=[b[0]]),                        # not the state 5
           F(MLNHardPotential(lambda x: x[0] * (x[1] - 1)), nb=[a[2], b[1]]),
           F(MLNHardPotential(lambda x: 3 - x[0] - x[1] + x[2]), nb=[a[3], a[0], b[2]])]
    wc = _weights(rng, 4, 0.3, 1.5)
    fs += [F(MLNPotential(lambda x: eq_op(x[1], x[0]), w=wc[0]), nb=[a[1], c1]),
           F(MLNPotential(lambda x: x[0] * x[0] * eq_op(x[1], 1.0), w=wc[1]), nb=[b[1], c2]),      # x0 squared: bounded off-domain too
           F(MLNPotential(lambda x: eq_op(x[0], x[1]), w=wc[2]), nb=[c1, c2]),
           F(MLNPotential(lambda x: eq_op(x[0], 0.5 * x[1]), w=wc[3]), nb=[c2, b[3]])]
    return _graph(disc + [c1, c2], fs)


def shared_scope(seed=0):
    """two and three factors over the same pair of variables, a clause whose three variables all share one further factor
    (continuous and binary alike), a unary factor on every variable: local_score counts a shared factor once, from the first
    variable that has it"""
    rng = np.random.default_rng(4000 + seed)
    db = Domain((0, 1))
    dc = Domain((-3, 3), continuous=True, integral_points=np.linspace(-3, 3, 7))
    x, y, z = RV(dc), RV(dc), RV(dc)
    p, q, r, o = RV(db), RV(db), RV(db), RV(db, value=1)
    w = iter(_weights(rng, 24, 0.2, 2.0))
    s = iter([1, -1, 1, 1, -1, 1, -1, 1, 1, -1, 1, 1])
    M = lambda form, nb, sign=1: F(MLNPotential(form, w=sign * next(w)), nb=nb)
    fs = [M(lambda v: eq_op(v[0], v[1]), [x, y]), M(lambda v: eq_op(v[0] + v[1], 1), [x, y]),
          M(lambda v: or_op(v[0], v[1]), [p, q], next(s)), M(lambda v: v[0] * v[1], [p, q], next(s)),
          M(lambda v: v[0] * (1 - v[1]), [p, q], next(s)),
          M(lambda v: eq_op(v[0] + v[1], v[2]), [x, y, z]), M(lambda v: eq_op(v[0], v[2]) + eq_op(v[1], v[2]), [z, x, y]),
          M(lambda v: v[0] * v[1] * v[2], [p, q, r], next(s)), M(lambda v: or_op(or_op(v[0], v[1]), v[2]), [r, p, q], next(s)),
          M(lambda v: v[0] * eq_op(v[1], 1), [p, x]), M(lambda v: (1 - v[0]) * eq_op(v[1], -1), [p, x]),
          M(lambda v: v[0] * v[1] * eq_op(v[2], 0.5), [o, q, z]),
          F(MLNHardPotential(lambda v: or_op(v[0], v[1])), nb=[q, r])]
    fs += [M(lambda v, c=c: eq_op(v[0], c), [rv]) for rv, c in ((x, 0.4), (y, -1.2), (z, 2.1))]
    fs += [M(lambda v: v[0], [rv], next(s)) for rv in (p, q, r)]
    return _graph([x, y, z, p, q, r, o], fs)


def every_kind(seed=0):
    """the potential kinds the three models above lack: hidden binary variables under a TablePotential (class 0: never
    unsatisfied, always scored), continuous pairs under GaussianPotential, LinearGaussianPotential and XYPotential, X2
    unaries, one soft factor whose w * formula falls below -745 on part of its range (phi underflows to 0: the term is -700
    and the state counts a vanishing factor), one hard clause"""
    from lhvi.potentials import LinearGaussianPotential, TablePotential, X2Potential, XYPotential
    rng = np.random.default_rng(5000 + seed)
    db = Domain((0, 1))
    dc = Domain((-10, 10), continuous=True, integral_points=np.linspace(-10, 10, 11))
    t1, t2, t3 = RV(db), RV(db), RV(db)
    c1, c2, c3, c4, c5 = (RV(dc) for _ in range(5))
    w = _weights(rng, 12, 0.2, 1.5)
    tab = lambda shape: np.round(rng.uniform(0.2, 3.0, size=shape), 3)
    fs = [F(TablePotential(tab((2, 2))), nb=[t1, t2]), F(TablePotential(tab((2, 2, 2))), nb=[t3, t1, t2]),
          F(TablePotential(tab((2,))), nb=[t3]),
          F(MLNHardPotential(lambda x: or_op(x[0], x[1])), nb=[t1, t3]),
          F(MLNPotential(lambda x: x[0] * x[1], w=w[0]), nb=[t2, t3]), F(MLNPotential(lambda x: 1 - x[0], w=-w[1]), nb=[t1]),
          F(GaussianPotential([w[2], -w[3]], [[1.0 + w[4], 0.3], [0.3, 2.0]]), nb=[c1, c2]),
          F(LinearGaussianPotential(w[5], 0.5 + w[6]), nb=[c2, c3]),
          F(XYPotential(w[7], 1.0), nb=[c3, c4]),
          F(X2Potential(1.0 + w[8], 0.5), nb=[c3]), F(X2Potential(1.0 + w[9], 0.5), nb=[c4]),
          F(X2Potential(w[10], 4.0), nb=[c5]), F(X2Potential(w[11], 3.0), nb=[c1]),
          F(MLNPotential(lambda x: eq_op(x[0], 3.0), w=40.0), nb=[c5]),          # 40 (x - 3)^2 > 745 beyond |x - 3| > 4.32
          F(MLNPotential(lambda x: x[0] * eq_op(x[1], x[2]), w=w[0] + 1), nb=[t2, c4, c5])]
    return _graph([t1, t2, t3, c1, c2, c3, c4, c5], fs)


def paper_popularity(P=40, T=5, seed=0):
    from lhvi.generators import paper_popularity as pp
    rg = pp(P=P, T=T)
    g, _ = rg.ground_graph()
    rng = np.random.default_rng(seed)
    data = {}
    for key in rg.rvs_dict:
        if key[0] in ('SameSession', 'PaperIn'):
            data[key] = int(rng.integers(0, 2))
        elif key[0] == 'PaperPopularity' and rng.random() < 0.5:
            data[key] = float(rng.uniform(0, 10))
    rg.add_evidence(data)
    return g


def robot_mapping(segments=8):
    from lhvi.generators import robot_mapping as rm
    rg = rm(segments=segments)
    g, _ = rg.ground_graph()
    rng = np.random.default_rng(1)
    data = {}
    for key in rg.rvs_dict:
        if key[0] in ('PartOf', 'Aligned'):
            data[key] = int(rng.integers(0, 2))
        elif key[0] in ('Length', 'Depth'):
            data[key] = float(rng.uniform(0, 0.5))
    rg.add_evidence(data)
    return g
