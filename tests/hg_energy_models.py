"""Models and NumPy restatements of the joint-energy / joint-MAP tests (csrc/hg_energy.hip, docs/kernels_hg_energy.md), shared
by tests/test_hg_energy_host.py (the host twins) and tests/test_gpu_hg_energy.py (the device).

The reference for an energy is ``numpy_energy``: ``eval_joint_assignment_energy`` restated on the factor objects (not on the
flat descriptors the kernel reads) in ``np.longdouble``, returning e_ref and T = sum |term| over all
n_terms = sum_f (nc^2 + nc + 1) + n_tab terms.  The bound ``|e - e_ref| <= 2 n_terms * 1.1e-16 * T`` is recursive summation
(n_terms u T to first order) plus two roundings per product P x_a x_j: derived, not measured.
"""
import numpy as np

import exact_models as em
from lhvi import exact
from lhvi.potentials import LogHybridQuadratic, LogQuadratic, LogTable

U = 1.1e-16
S_LIST = (1, 63, 64, 65, 130)
SENTINEL = -12345.6789
ENERGY_MODELS = ('nc1', 'deep_scope', 'wide_states', 'nc7', 'nc64', 'disc_chain', 'gauss_only')
FIXTURES = {'ref_hybrid2': 3, 'ref_mln0': 3, 'rand_3_2': 0, 'rand_8_8': 426, 'rand_8_8_ev': 30}    # joint MAP configuration
MIN_GAP = {'ref_hybrid2': 0.1, 'ref_mln0': 0.1, 'rand_3_2': 1.78, 'rand_8_8': 0.435, 'rand_8_8_ev': 0.834}


# ---- models ------------------------------------------------------------------------------------------------------------------
def disc_chain(ns, Nd=40, seed=201):
    """discrete only: Nd binary variables, a chain of pair tables (every second one in the scope order (i + 1, i)) and a unary
    table on the first and the last variable.  2^40 configurations: never enumerated"""
    rng = np.random.RandomState(seed)
    Vd = [ns.RV(domain=ns.Domain(values=(0, 1), continuous=False)) for _ in range(Nd)]
    factors = [ns.F(nb=(Vd[0],), log_potential_fun=ns.LogTable(rng.randn(2)))]
    for i in range(Nd - 1):
        nb = (Vd[i], Vd[i + 1]) if i % 2 == 0 else (Vd[i + 1], Vd[i])
        factors.append(ns.F(nb=nb, log_potential_fun=ns.LogTable(rng.randn(2, 2))))
    factors.append(ns.F(nb=(Vd[-1],), log_potential_fun=ns.LogTable(rng.randn(2))))
    return em._pack(Vd, factors)


def gauss_only(ns, seed=202):
    """Gaussian only: Nd = 0, M = 1, Nc = 3: a dense quadratic in the scope order (2, 0, 1) and a unary one"""
    rng = np.random.RandomState(seed)
    Vc = [ns.RV(domain=ns.Domain(values=em.CDOM, continuous=True)) for _ in range(3)]
    B = rng.randn(3, 3) / np.sqrt(3)
    factors = [ns.F(nb=(Vc[2], Vc[0], Vc[1]), log_potential_fun=ns.LogQuadratic(A=-0.5 * (B @ B.T + np.eye(3)), b=rng.randn(3), c=0.3)),
               ns.F(nb=(Vc[1],), log_potential_fun=ns.LogQuadratic(A=-(0.5 + rng.rand(1, 1)), b=rng.randn(1), c=0.))]
    return em._pack(Vc, factors)


def peak_vs_mass(ns):
    """one binary d, one continuous x on (-10, 10), one hybrid factor: J = (100, 0.01), energies at the means (0, -1), so the
    joint MAP is d = 0, while log p~ = 1/2 log(2 pi / J) + c = (-1.384, 2.222) and ``disc_table`` peaks at d = 1: the narrow
    peak is the higher one, the wide one holds the mass"""
    d = ns.RV(domain=ns.Domain(values=(0, 1), continuous=False))
    x = ns.RV(domain=ns.Domain(values=(-10, 10), continuous=True))
    lp = ns.LogHybridQuadratic(A=np.array([[[-50.]], [[-0.005]]]), b=np.zeros((2, 1)), c=np.array([0., -1.]))
    return em._pack([d, x], [ns.F(nb=(d, x), log_potential_fun=lp)])


def peak_vs_mass2(ns, seed=203):
    """the seeded two-variable version: dstates (2, 3), Nc = 3, one hybrid factor over all five variables whose blocks are
    -1/2 s W with W = B B^T + I per state and s = 100 / 0.01 by the first variable's state; its constants favour the narrow
    states by 1.5 and separate the second variable's states by 0.5; two tables of small entries.  The mass term
    -1/2 log det J differs by 3 log(10^4) / 2 = 13.8 the other way.  tests/test_hg_energy_host.py proves what the seed delivers."""
    rng = np.random.RandomState(seed)
    d0 = ns.RV(domain=ns.Domain(values=(0, 1), continuous=False))
    d1 = ns.RV(domain=ns.Domain(values=(0, 1, 2), continuous=False))
    Vc = [ns.RV(domain=ns.Domain(values=em.CDOM, continuous=True)) for _ in range(3)]
    A, b, c = np.empty((2, 3, 3, 3)), np.empty((2, 3, 3)), np.empty((2, 3))
    for i, scale in enumerate((100., 0.01)):
        for j in range(3):
            B = rng.randn(3, 3) / np.sqrt(3)
            A[i, j] = -0.5 * scale * (B @ B.T + np.eye(3))
            b[i, j] = 0.1 * np.sqrt(scale) * rng.randn(3)
            c[i, j] = -1.5 * i - 0.5 * j + 0.02 * rng.randn()
    factors = [ns.F(nb=(d0, d1, Vc[0], Vc[1], Vc[2]), log_potential_fun=ns.LogHybridQuadratic(A=A, b=b, c=c)),
               ns.F(nb=(d1, d0), log_potential_fun=ns.LogTable(0.02 * rng.randn(3, 2))),
               ns.F(nb=(d1,), log_potential_fun=ns.LogTable(0.02 * rng.randn(3)))]
    return em._pack([d0, d1] + Vc, factors)


def tie_model(ns):
    """dstates (2, 2): the second variable appears only in a unary table of zeros, so configurations 2k and 2k + 1 have
    bit-identical energies; the first variable's state 1 is the better one (the joint MAP is configuration 2, not 0)"""
    d0, d1 = (ns.RV(domain=ns.Domain(values=(0, 1), continuous=False)) for _ in range(2))
    x = ns.RV(domain=ns.Domain(values=(-10, 10), continuous=True))
    lp = ns.LogHybridQuadratic(A=np.array([[[-0.7]], [[-1.3]]]), b=np.array([[0.3], [-0.9]]), c=np.array([0.1, 0.45]))
    factors = [ns.F(nb=(d0, x), log_potential_fun=lp), ns.F(nb=(d1,), log_potential_fun=ns.LogTable(np.zeros(2))),
               ns.F(nb=(d0,), log_potential_fun=ns.LogTable(np.array([0.2, 0.25])))]
    return em._pack([d0, d1, x], factors)


EXTRA = {'disc_chain': disc_chain, 'gauss_only': gauss_only, 'peak_vs_mass': peak_vs_mass, 'peak_vs_mass2': peak_vs_mass2,
         'tie_model': tie_model}
REDUCTION = {177147: (3,) * 11, 531441: (3,) * 12}


def build(name):
    """the model `name` (this module's, else exact_models') with its indices set, and its flat form"""
    ns = em.local_ns()
    if name in EXTRA:
        model = EXTRA[name](ns)
    elif name in REDUCTION:
        model = em.reduction_model(ns, list(REDUCTION[name]))
    else:
        model = em.build(name, **({'hand': True} if name == 'ref_mln0' else {}))
    em.set_indices(model)
    flat = exact.flatten_factors(model['factors'], [rv.dstates for rv in model['Vd']], len(model['Vc']))
    return model, flat


def solver(name):
    """(model, ExactHybridGaussian over it); exact_models.solver for its names (evidence applied, MLN potentials converted)"""
    if name not in EXTRA and name not in REDUCTION:
        return em.solver(name)
    model, _ = build(name)
    return model, exact.ExactHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc'])


# ---- rows ----------------------------------------------------------------------------------------------------------------------
def digits(flat, cfgs):
    """[S, Nd] int32 digits of the configuration indices (dstride / dstates)"""
    cfgs = np.asarray(cfgs, dtype=np.int64).reshape(-1)
    if flat.Nd == 0:
        return np.zeros((cfgs.size, 0), dtype=np.int32)
    return ((cfgs[:, None] // flat.dstride[None, :]) % flat.dstates[None, :].astype(np.int64)).astype(np.int32)


def rows(model, flat, S, seed, cfg_begin=None):
    """S assignments: the configurations cfg_begin .. cfg_begin + S, or seeded ones (all of [0, M) in turn when M <= S); x_c is
    the configuration's conditional mean in the even rows (the host's, lhvi_exact_config_host) and a seeded uniform point of
    the domain in the odd ones.  Returns (cfgs [S], x_d [S, Nd] int32, x_c [S, Nc])."""
    rng = np.random.RandomState(seed)
    if cfg_begin is not None:
        cfgs = cfg_begin + np.arange(S, dtype=np.int64)
        assert cfgs[-1] < flat.M
    elif flat.M <= S:
        cfgs = np.arange(S, dtype=np.int64) % flat.M
    else:
        cfgs = rng.randint(0, flat.M, size=S).astype(np.int64)
    lo = np.array([rv.domain.values[0] for rv in model['Vc']], dtype=np.float64)
    hi = np.array([rv.domain.values[1] for rv in model['Vc']], dtype=np.float64)
    x_c = lo + (hi - lo) * rng.rand(S, flat.Nc)
    if flat.Nc:
        for s in range(0, S, 2):
            x_c[s] = exact.config_host(flat, int(cfgs[s]))[1]
    return cfgs, digits(flat, cfgs), np.ascontiguousarray(x_c)


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def numpy_energy(factors, x_d, x_c):
    """eval_joint_assignment_energy of the rows (x_d [S, Nd] state indices, x_c [S, Nc]) on factor objects carrying
    log_potential_fun / disc_nb_idx / cont_nb_idx, vectorised over the rows, in np.longdouble.
    Returns (e_ref [S] float64, T [S] = sum |term|, n_terms)."""
    ld = np.longdouble
    S = len(x_d)
    xc = np.asarray(x_c, dtype=np.float64).reshape(S, -1).astype(ld)
    e, T, n_terms = np.zeros(S, dtype=ld), np.zeros(S, dtype=ld), 0

    def add(term):
        nonlocal e, T, n_terms
        e = e + term
        T = T + np.abs(term)
        n_terms += 1

    for f in factors:
        lp = f.log_potential_fun
        sel = tuple(np.asarray(x_d)[:, i] for i in f.disc_nb_idx)
        if isinstance(lp, LogTable):
            add(np.asarray(lp.table, dtype=np.float64)[sel].astype(ld) * np.ones(S, dtype=ld))
            continue
        assert isinstance(lp, (LogQuadratic, LogHybridQuadratic))
        sc = list(f.cont_nb_idx)
        nc = len(sc)
        A, b, c = (np.asarray(a, dtype=np.float64) for a in (lp.A, lp.b, lp.c))
        if isinstance(lp, LogHybridQuadratic):
            A, b, c = A[sel], b[sel], c[sel]
        A = np.broadcast_to(A.reshape((-1, nc, nc)), (S, nc, nc)).astype(ld)
        b = np.broadcast_to(b.reshape((-1, nc)), (S, nc)).astype(ld)
        c = np.broadcast_to(c.reshape(-1), (S,)).astype(ld)
        for i in range(nc):
            for j in range(nc):
                add(A[:, i, j] * xc[:, sc[i]] * xc[:, sc[j]])
        for i in range(nc):
            add(b[:, i] * xc[:, sc[i]])
        add(c)
    return e.astype(np.float64), T.astype(np.float64), n_terms


def bound(T, n_terms):
    return 2 * n_terms * U * np.asarray(T)


def assert_within_bound(got, factors, x_d, x_c, what, offset=0.0):
    """|got - (e_ref + offset)| <= bound per row (offset: the solver's log_const, one more addition: counted as a term); prints
    the largest error next to its bound"""
    e_ref, T, n_terms = numpy_energy(factors, x_d, x_c)
    if offset:
        e_ref, T, n_terms = e_ref + offset, T + abs(offset), n_terms + 1
    err, bd = np.abs(np.asarray(got) - e_ref), bound(T, n_terms)
    worst = int(np.argmax(err - bd))
    print('%s: %d rows, %d terms, largest error %.3g (bound %.3g at that row)' % (what, len(err), n_terms, err.max(),
                                                                                  bd[int(np.argmax(err))]))
    assert (err <= bd).all(), '%s: row %d is off by %.3g, bound %.3g' % (what, worst, err[worst], bd[worst])
    return float(err.max())


# ---- the arg-max's definition ----------------------------------------------------------------------------------------------------
def argmax_definition(v):
    """plain Python: the smallest index attaining the maximum over the non-NaN entries ((-1, NaN) when there is none)"""
    best, where = None, -1
    for i, x in enumerate(v):
        x = float(x)
        if x != x:
            continue
        if where < 0 or x > best:
            best, where = x, i
    return where, (float('nan') if where < 0 else best)


def argmax_cases(n):
    """{pattern: array [n]}: the patterns the arg-max can get wrong.  First-stage slices are contiguous runs of ceil(n / parts)
    entries, parts = min(1024, ceil(n / 256)): duplicates are placed both far apart and next to each other."""
    rng = np.random.RandomState(n % 9973)
    base = rng.randn(n)
    base[base > 2.5] = 2.5                  # keeps the planted maximum of 3 the only one
    out = {}
    far = base.copy()
    far[[n // 3, n - 1 - n // 7, n // 2]] = 3.0                                       # in different slices (one slice when n is small)
    out['duplicates_far'] = far
    near = base.copy()
    lo = min(n - 1, n // 2)
    near[lo:min(n, lo + 3)] = 3.0                                                    # inside one slice, neighbouring threads
    out['duplicates_near'] = near
    first, last = base.copy(), base.copy()
    first[0] = 3.0
    last[n - 1] = 3.0
    out['max_first'], out['max_last'] = first, last
    out['all_equal'] = np.full(n, 1.25)
    out['all_neg_inf'] = np.full(n, -np.inf)
    nan_near = base.copy()
    k = n // 2
    nan_near[k] = 3.0
    nan_near[max(0, k - 1):k] = np.nan
    nan_near[k + 1:k + 2] = np.nan
    nan_near[:min(k, 5)] = np.nan                                                     # before the maximum, the first entries too
    out['nan_neighbours'] = nan_near
    out['all_nan'] = np.full(n, np.nan)
    zeros = np.full(n, -1.0)
    zeros[n // 2:] = 0.0
    zeros[n // 2::2] = -0.0                                                           # -0 first, then +0: they tie, the first wins
    out['signed_zeros'] = zeros
    nan_then_inf = np.full(n, np.nan)
    nan_then_inf[n - 1] = -np.inf                                                     # -inf beats nothing but NaN
    out['nan_then_neg_inf'] = nan_then_inf
    return out


ARGMAX_N = (1, 63, 64, 65, 257, 2 ** 18 + 1)


# ---- the identity of the recorded results ----------------------------------------------------------------------------------------
def golden_energies(gold):
    """energy(cfg) = log table + logZ - Nc/2 log 2 pi - 1/2 log det Sig from a full fixture's table, logZ and covs_tril"""
    Nc = gold['means'].shape[1]
    i, j = np.tril_indices(Nc)
    out = np.zeros(len(gold['cfg']))
    for row in range(len(out)):
        Sig = np.zeros((Nc, Nc))
        Sig[i, j] = gold['covs_tril'][row]
        Sig[j, i] = gold['covs_tril'][row]
        out[row] = np.log(gold['table'][row]) + gold['logZ'] - Nc / 2 * np.log(2 * np.pi) - 0.5 * np.linalg.slogdet(Sig)[1]
    return out
