"""Graphs and helpers for testing colour refinement (csrc/color.hip) and the lifting reductions (``lhvi/lifting.py``) half round
by half round: ragged graphs whose variable degrees sit on ``LHVI_HUB_DEGREE``, arities 1 to 6 with repeated variables in a scope,
disjoint permuted copies, graphs that drive the sort network of the symmetric factors, the hash table's edge, and evidence with a
large heterogeneous cluster.  Plain Python and NumPy.  No test functions: tests/test_colour_host.py (CPU) and
tests/test_gpu_colour.py (MI355X) use it."""
import itertools
import math

import numpy as np

HUBS = (63, 64, 65, 127, 128, 129, 300)
N_ISOLATED = 5                   # small variables of ``ragged`` that are kept out of every factor ...
N_SINGLE = 5                     # ... and that get exactly one incidence


def _build(scopes, V, var_value=None):
    """``build_flat`` of a list of scopes with one potential row (refinement never reads the potentials)"""
    from lhvi import potentials as P
    from lhvi.flat import build_flat
    from lhvi.graph import Domain
    dom = Domain((-50, 50), continuous=True, integral_points=np.linspace(-50, 50, 8))
    fac_ptr = np.zeros(len(scopes) + 1, dtype=np.int32)
    np.cumsum([len(s) for s in scopes], out=fac_ptr[1:])
    edge_var = np.fromiter((v for s in scopes for v in s), dtype=np.int32, count=int(fac_ptr[-1]))
    value = np.full(V, np.nan) if var_value is None else np.asarray(var_value, dtype=np.float64)
    return build_flat(fac_ptr, edge_var, np.zeros(len(scopes), dtype=np.int32), [(P.POT_X2, [1.0, 4.0])], value,
                      np.zeros(V, dtype=np.int32), [dom])


def scopes_of(flat):
    return [flat.edge_var[flat.fac_ptr[f]:flat.fac_ptr[f + 1]].tolist() for f in range(flat.F)]


def ragged(seed, hubs=HUBS, n_small=3000, n_fac=4000, n_rv0=3, n_f0=4, twins=True):
    """(flat, symmetric, rv_color0, f_color0).  Variable h < len(hubs) has exactly hubs[h] incidences, from factors of arity 1 to 6
    of which about a fifth list the hub twice; `n_fac` random factors of arity 1 to 6 over the small variables (drawn with
    replacement: scopes repeat variables); the last N_ISOLATED small variables have no factor, the N_SINGLE before them one
    incidence each.  The symmetric flag is a function of the initial factor colour (``f0 % 2``), as in every real input, where a
    colour class shares one potential: with independent flags the partition would depend on how colours are numbered.
    `twins`: variable len(hubs) + h is a twin of hub h -- every factor of the hub has a copy with the same initial colour in which
    the twin takes the hub's place, at another place in the factor order.  Swapping the two is an automorphism, so hub and twin
    share a colour after every half round, while their rows list the same factor colours in different orders: a hub whose sum
    loses or repeats a term leaves its twin (alone, a hub of a degree no other variable has is a cluster of one whatever its
    fingerprint)."""
    rng = np.random.default_rng(seed)
    H = len(hubs)
    first_small = 2 * H if twins else H
    V = first_small + n_small
    free_hi = V - N_ISOLATED - N_SINGLE              # small variables the random draws may use: [first_small, free_hi)
    assert free_hi - first_small >= 1
    small = lambda n: rng.integers(first_small, free_hi, n).tolist()
    scopes, twin_of = [], []                         # twin_of[i]: the factor whose initial colour factor i takes, or -1
    for h, need in enumerate(hubs):
        while need > 0:
            a = int(rng.integers(1, 7))
            times = 2 if (a >= 2 and need >= 2 and rng.random() < 0.2) else 1
            scope = small(a)
            for p in rng.choice(a, size=times, replace=False):
                scope[int(p)] = h
            scopes.append(scope)
            twin_of.append(-1)
            if twins:
                scopes.append([H + h if v == h else v for v in scope])
                twin_of.append(len(scopes) - 2)
            need -= times
    for _ in range(n_fac):
        scopes.append(small(int(rng.integers(1, 7))))
    for v in range(free_hi, free_hi + N_SINGLE):
        scope = small(int(rng.integers(1, 4)))
        scope[int(rng.integers(0, len(scope)))] = v
        scopes.append(scope)
    twin_of += [-1] * (len(scopes) - len(twin_of))
    rv0 = rng.integers(0, n_rv0, V).astype(np.int32)
    f0 = rng.integers(0, n_f0, len(scopes)).astype(np.int32)
    rv0[:min(n_rv0, V)] = np.arange(min(n_rv0, V))   # every colour id in use: the ids stay dense
    f0[:min(n_f0, f0.size)] = np.arange(min(n_f0, f0.size))
    if twins:
        rv0[H:2 * H] = rv0[:H]
        tw = np.array(twin_of)
        f0[tw >= 0] = f0[tw[tw >= 0]]
    order = rng.permutation(len(scopes))
    return _build([scopes[i] for i in order], V), (f0[order] % 2).astype(np.uint8), rv0, f0[order]


def single():
    """one variable with one unary factor"""
    return _build([[0]], 1), np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)


def copies(flat, sym, rv0, f0, c=3, seed=0):
    """(flat, symmetric, rv_color0, f_color0, vperm, fperm): `c` disjoint copies of the graph under independent random permutations
    of all variable ids and all factor ids, the scopes of the symmetric factors shuffled.  ``vperm[k, v]`` / ``fperm[k, f]`` is
    the id of variable v / factor f of the base graph in copy k."""
    rng = np.random.default_rng(seed)
    vperm = rng.permutation(c * flat.V).reshape(c, flat.V)
    fperm = rng.permutation(c * flat.F).reshape(c, flat.F)
    base = scopes_of(flat)
    scopes = [None] * (c * flat.F)
    for k in range(c):
        for f, s in enumerate(base):
            s = vperm[k, s].tolist()
            if sym[f]:
                s = [s[i] for i in rng.permutation(len(s))]
            scopes[fperm[k, f]] = s
    rv_c, f_c = np.zeros(c * flat.V, dtype=np.int32), np.zeros(c * flat.F, dtype=np.int32)
    sym_c, val = np.zeros(c * flat.F, dtype=np.uint8), np.full(c * flat.V, np.nan)
    for k in range(c):
        rv_c[vperm[k]], f_c[fperm[k]], sym_c[fperm[k]], val[vperm[k]] = rv0, f0, sym, flat.var_value
    return _build(scopes, c * flat.V, val), sym_c, rv_c, f_c, vperm, fperm


# ---- the sort network of the symmetric factors -------------------------------------------------------------------------------
def sort_multisets(a):
    """multisets of `a` variable colours (ascending tuples): all distinct, one colour twice, and the latter with its largest colour
    raised by one -- two factors over 'repeated' and 'top' differ in the LAST entry of their sorted tuples only"""
    repeated = (0, 0) + tuple(range(1, a - 1))
    return {'distinct': tuple(range(a)), 'repeated': repeated, 'top': repeated[:-1] + (repeated[-1] + 1,)}


def sort_network_case(a, symmetric, multisets=('distinct',)):
    """(flat, symmetric flags, rv_color0, f_color0, expected number of factor colours after one factor half round).  All factors
    share one initial colour; their scopes are every distinct permutation of each named multiset of `a` variable colours
    (``sort_multisets``).  Two variables share each initial colour and the scopes alternate between them, so a repeated colour is
    sometimes one variable twice and sometimes two variables.  All factors symmetric: one colour per multiset; none symmetric: one
    per distinct colour tuple."""
    table = sort_multisets(a)
    tuples = []
    for name in multisets:
        tuples += sorted(set(itertools.permutations(table[name])))
    n_colors = max(max(t) for t in tuples) + 1
    scopes = [[2 * col + (i + p) % 2 for p, col in enumerate(t)] for i, t in enumerate(tuples)]
    rv0 = np.repeat(np.arange(n_colors, dtype=np.int32), 2)
    flat = _build(scopes, 2 * n_colors)
    expected = len(set(multisets)) if symmetric else len(set(tuples))
    for name in multisets:
        m = table[name]
        assert len(set(itertools.permutations(m))) == math.factorial(a) // math.prod(math.factorial(m.count(x)) for x in set(m))
    return flat, np.full(flat.F, 1 if symmetric else 0, dtype=np.uint8), rv0, np.zeros(flat.F, dtype=np.int32), expected


# ---- the hash table's edge ---------------------------------------------------------------------------------------------------
MAX_DISTINCT = 524288            # csrc/color.hip: TABLE_SLOTS / 2 distinct keys fit the table of a half round


def all_distinct(V):
    """V variables, each with a unary factor of its own, every initial variable colour distinct and one factor colour: both half
    rounds see V distinct keys, and the partition they must return is the identity"""
    return (_build(np.arange(V).reshape(V, 1).tolist(), V), np.zeros(V, dtype=np.uint8), np.arange(V, dtype=np.int32),
            np.zeros(V, dtype=np.int32))


# ---- graphs with evidence for the lifting reductions -------------------------------------------------------------------------
POOL = (-3.5, 0.25, 7.0)
BIG = (1e16, 1.0, -1e16)         # a running sum of these shows its order in the leading digits: (1e16 + 1) - 1e16 = 0


def _big_values(n, rng):
    vals = np.tile(np.array(BIG), n // 3 + 1)[:n]
    extra = rng.random(n) < 0.3
    vals[extra] = np.round(rng.uniform(-30, 30, int(extra.sum())), 3)
    vals[:3] = BIG
    return vals


RGM_C, RGM_B = 65, 63            # ``synth.rgm_flat``: market degree B + 1 = 64, revenue and recession degree C = 65


def rgm_hub_case():
    """the RGM template at variable degrees 64 and 65 with the evidence of ``synth.rgm_flat`` (a fifth of the atoms, three values)"""
    from lhvi import synth
    return synth.rgm_flat(RGM_C, RGM_B, n_values=3, evidence_ratio=0.2)


def rgm_lift_case(seed=0):
    """(flat, symmetric, rv_color0, f_color0, big): ``rgm_hub_case``'s graph with evidence that is a function of (c mod 4, b mod 3):
    markets with c % 4 == 0 and revenues with b % 3 == 0 observed from POOL, and the loss atoms of (c % 4 == 1, b % 3 == 1) observed
    with values that differ inside ONE initial colour `big` (coarse evidence: ``is_split_cont_evidence=False``) -- colour passing
    keeps them together, a cluster of 17 * 21 members whose evidence value is a running sum over +-1e16."""
    from lhvi import synth
    C, B = RGM_C, RGM_B
    flat, sym, _, f0 = synth.rgm_flat(C, B, n_values=0, evidence_ratio=0.0)
    rng = np.random.default_rng(seed)
    market, loss, revenue = 1, 1 + C, 1 + C + C * B
    val, rv0 = np.full(flat.V, np.nan), np.zeros(flat.V, dtype=np.int32)
    c, b = np.arange(C), np.arange(B)
    mo, ro = c[c % 4 == 0], b[b % 3 == 0]
    val[market + mo], rv0[market + mo] = np.array(POOL)[(mo // 4) % 3], 1 + (mo // 4) % 3
    val[revenue + ro], rv0[revenue + ro] = np.array(POOL)[(ro // 3) % 3], 1 + (ro // 3) % 3
    block = (loss + c[c % 4 == 1][:, None] * B + b[b % 3 == 1][None, :]).ravel()
    val[block], rv0[block] = _big_values(block.size, rng), 4
    val[0], rv0[0] = POOL[1], 2                      # the recession atom: an observed cluster of one
    flat.var_value = val
    return flat, sym, rv0, f0, 4


def copies_lift_case(seed=0):
    """(flat, symmetric, rv_color0, f_color0, big): three copies of a ragged graph with more variables than factors, with evidence:
    a fifth of the variables observed from POOL (initial colour = old colour and value), and the variables without a factor whose
    old colour is 0 observed with values that differ inside ONE initial colour `big` -- variables without a factor are never told
    apart, a cluster of some 450 members whose evidence value is a running sum over +-1e16."""
    flat, sym, rv0, f0 = ragged(seed, n_small=4000, n_fac=1500)
    flat, sym, rv0, f0, _, _ = copies(flat, sym, rv0, f0, c=3, seed=seed + 1)
    rng = np.random.default_rng(seed + 2)
    code = np.where(rng.random(flat.V) < 0.2, 1 + rng.integers(0, 3, flat.V), 0)
    val = np.where(code > 0, np.array((np.nan,) + POOL)[code], np.nan)
    block = np.flatnonzero((np.diff(flat.var_ptr) == 0) & (rv0 == 0))
    code[block], val[block] = 4, _big_values(block.size, rng)
    flat.var_value = val
    _, rv_e = np.unique(rv0.astype(np.int64) * 5 + code, return_inverse=True)
    big = int(rv_e[block[0]])
    return flat, sym, rv_e.astype(np.int32), f0, big


# ---- wave-level shapes of the two lifting kernels ----------------------------------------------------------------------------
SEG_LENGTHS = (0, 1, 3, 255, 256, 257, 511, 512, 513, 1000)
SEG_SHORT = (0, 1, 3, 255)       # below SEG_LONG = 256: summed by the segment's own thread


def segment_case(seed=0):
    """(values, lengths) for ``lifting.segment_sums``.  Wavefronts of 64 segments: three that hold long runs (256 and more entries,
    streamed through LDS by the whole wavefront) at lanes 0 and 63 -- every long length of SEG_LENGTHS once -- and short runs
    between them; one with every length of SEG_LENGTHS at random lanes; one that is all short; and a last partial wavefront of 37
    segments that ends in a long run.  The values are (1e16, 1.0, -1e16) triples, every run starting at another phase, and a few
    random values: any other order of the additions changes the leading digits."""
    rng = np.random.default_rng(seed)
    waves = []
    for first, last in ((256, 1000), (257, 511), (512, 513)):
        w = rng.choice(SEG_SHORT, 64)
        w[0], w[63] = first, last
        waves.append(w)
    w = rng.choice(SEG_LENGTHS, 64)
    w[rng.permutation(64)[:len(SEG_LENGTHS)]] = SEG_LENGTHS
    waves.append(w)
    waves.append(rng.choice(SEG_SHORT, 64))
    w = rng.choice(SEG_SHORT, 37)
    w[36] = 257
    waves.append(w)
    lengths = np.concatenate(waves).astype(np.int64)
    n = int(lengths.sum())
    values = np.tile(np.array(BIG), n // 3 + 1)[:n]
    extra = rng.random(n) < 0.1
    values[extra] = rng.uniform(-30, 30, int(extra.sum()))
    return values, lengths


def first_member_cases():
    """(name, colours, number of colours) for ``lifting.first_members`` at n = 63, 64, 65 and 257: 64 distinct colours in one
    wavefront, one colour everywhere, colours descending, and a colour whose only members are the last lane of one wavefront and
    the first lane of the next"""
    out = []
    for n in (63, 64, 65, 257):
        i = np.arange(n)
        out.append(('distinct64_n%d' % n, i % 64, 64))
        out.append(('one_n%d' % n, np.zeros(n, dtype=np.int64), 1))
        out.append(('descending_n%d' % n, n - 1 - i, n))
        if n > 64:
            col = np.where(i < 64, i, i - 1)         # items 63 and 64 share colour 63
            col[65:] = 64 + (i[65:] % 7)
            out.append(('straddle_n%d' % n, col, int(col.max()) + 1))
    return out
