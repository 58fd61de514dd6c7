"""Generators and NumPy restatements for the mixture-belief tests (lhvi/mixture.py, csrc/mixture.hip).

The restatements say in NumPy what the NumPy half of the reference's osi/mixture_beliefs.py (:505-746) and
osi/utils.py:66-98 compute; tests/golden/mixture_*.npz (scripts/capture_mixture.py) pin them to the reference itself.  They
take a dtype, so that the same code in np.longdouble is the yardstick of the kernels' rounding error.

A case is a dict: w [K], Mu / Var [Nc, K], Pi (list of [K, states]), bds [2, Nc], obs (row indices, repeats allowed), X [M, N_o]
(values / state indices, NaN = not observed in that row).  Rows: continuous 0 .. Nc - 1, then the discrete ones."""
import numpy as np

U = 1.1e-16                     # unit roundoff of fp64, rounded up
KS = (1, 3, 5, 8, 33)
NOS = (0, 1, 63, 64, 65)        # no evidence, one variable, one tile less one, one tile, one tile plus one
NOS_TWO_TILES = (129,)          # two tiles plus one
MS = (1, 5)                     # 5 = one more than a group of LHVI_MIX_ROWS = 4 evidence rows
NC, ND2, ND5 = 5, 3, 3          # rows of a condition case: 5 continuous, 3 of two states, 3 of five (Dmax padding)


def condition_case(K, N_o, M, seed=0, holes=True):
    """Observed sets mixing continuous rows and discrete rows of 2 and 5 states through an index list with repeats; NaN holes
    different per row; for K > 1 the last component sits 400 away with variance 0.01 on every continuous row, so its
    conditional weight underflows to 0 wherever a continuous variable is observed."""
    rng = np.random.RandomState(1000 * K + 10 * N_o + seed)
    w = rng.dirichlet(2 * np.ones(K))
    Mu = rng.uniform(-3, 3, (NC, K))
    Var = 10 ** rng.uniform(-1, 1, (NC, K))
    if K > 1:
        Mu[:, K - 1] += 400
        Var[:, K - 1] = 0.01
    Pi = [rng.dirichlet(2 * np.ones(s), K) for s in [2] * ND2 + [5] * ND5]
    V = NC + ND2 + ND5
    obs = rng.randint(0, V, N_o)
    X = np.empty((M, N_o))
    for j, v in enumerate(obs):
        X[:, j] = rng.uniform(-3, 3, M) if v < NC else rng.randint(0, Pi[v - NC].shape[1], M)
    if holes and N_o:
        X[rng.rand(M, N_o) < 0.25] = np.nan
    return dict(w=w, Mu=Mu, Var=Var, Pi=Pi, bds=np.array([[-10.] * NC, [10.] * NC]), obs=obs, X=X)


def belief_of(case, normaliser='gaussian'):
    from lhvi.mixture import MixtureBelief
    return MixtureBelief(case['w'], case['Mu'], case['Var'], case['Pi'], case['bds'], normaliser=normaliser)


def _pi_const(T):
    return 4 * np.arctan(T(1))


def row_terms(case, v, x, dtype=np.float64, normaliser='gaussian'):
    """log q_vk(x) of row v at the values / state indices x [P]: (terms [P, K], the summed magnitudes of a term's parts)"""
    T = dtype
    Nc = len(case['Mu'])
    x = np.asarray(x)
    if v < Nc:
        mu, var = case['Mu'][v].astype(T), case['Var'][v].astype(T)
        var_inv = 1 / var
        q = -T(0.5) * (x.astype(T)[:, None] - mu[None, :]) ** 2 * var_inv[None, :]
        if normaliser == 'vi':
            c = -np.log(T(2.506628274631) * var)
            cm = np.abs(c)
        else:
            c = -T(0.5) * np.log(2 * _pi_const(T)) + T(0.5) * np.log(var_inv)
            cm = T(0.5) * np.log(2 * _pi_const(T)) + np.abs(T(0.5) * np.log(var_inv))
        return c[None, :] + q, cm[None, :] + np.abs(q)
    lpi = np.log(case['Pi'][v - Nc].astype(T))
    t = lpi[:, np.asarray(x, dtype=np.int64)].T
    return t, np.abs(t)


def restate_condition(case, X=None, obs=None, dtype=np.float64, normaliser='gaussian'):
    """_calc_marg_comp_log_prob, calc_marg_log_prob and calc_cond_mixture_weights (:596-690), with NaN = not observed:
    dict(comp [M, K], logp [M], logcw [M, K] = log of the conditional weights, mag [M, K] = sum over the observed variables of
    the magnitudes of the parts of each term, which the error bounds are stated in)"""
    T = dtype
    X = case['X'] if X is None else X
    obs = case['obs'] if obs is None else obs
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    K = len(case['w'])
    comp, mag = np.zeros((X.shape[0], K), dtype=T), np.zeros((X.shape[0], K), dtype=T)
    for j, v in enumerate(obs):
        seen = ~np.isnan(X[:, j])
        t, m = row_terms(case, int(v), np.where(seen, X[:, j], 0), T, normaliser)
        comp += np.where(seen[:, None], t, 0)
        mag += np.where(seen[:, None], m, 0)
    with np.errstate(divide='ignore'):
        lw = np.log(case['w'].astype(T))
    t = lw[None, :] + comp
    mx = t.max(axis=1)
    logp = mx + np.log(np.exp(t - mx[:, None]).sum(axis=1))
    return dict(comp=comp, logp=logp, logcw=t - logp[:, None], mag=mag, lw=lw, t=t, mx=mx, n_obs=len(obs))


def condition_bounds(r):
    """Absolute error bounds of the fp64 kernels (docs/kernels_mixture.md, "Error bounds"), from a longdouble restatement `r`:
    comp, logp, log condw."""
    K = r['comp'].shape[1]
    n_o = r['n_obs']
    e_comp = (n_o + 8) * U * r['mag']
    e_t = e_comp + 3 * U * (np.abs(r['lw'])[None, :] + np.abs(r['comp']))
    cw = np.exp(r['logcw'])
    e_logp = (cw * e_t).sum(axis=1) + U * (2 * K + 8 + np.abs(r['logp']) + np.abs(r['mx']))
    e_logcw = e_t + e_logp[:, None] + 4 * U * (1 + np.abs(r['logcw']))
    return tuple(np.asarray(e, dtype=np.float64) for e in (e_comp, e_logp, e_logcw))


def restate_log_belief(case, r, query, x, dtype=np.float64, normaliser='gaussian'):
    """log sum_k condw[m, k] q_qk(x[q, p]) [M, N_q, P] from the restated conditioning `r`, and its error bound given the
    bound e_logcw [M, K] on the log weights (None: no bound)"""
    T = dtype
    out = np.empty((r['logcw'].shape[0], len(query), x.shape[1]), dtype=T)
    bound = np.empty(out.shape)
    K = r['logcw'].shape[1]
    e_logcw = r.get('e_logcw')
    for j, v in enumerate(query):
        t, m = row_terms(case, int(v), x[j], T, normaliser)             # [P, K]
        s = r['logcw'][:, None, :] + t[None, :, :]                         # [M, P, K]
        mx = s.max(axis=2)
        out[:, j, :] = mx + np.log(np.exp(s - mx[:, :, None]).sum(axis=2))
        if e_logcw is not None:
            resp = np.exp(s - out[:, j, :, None])
            e = (resp * (e_logcw[:, None, :] + 8 * U * m[None, :, :])).sum(axis=2)
            bound[:, j, :] = e + U * (2 * K + 8 + np.abs(out[:, j, :]) + np.abs(mx))
    return out, bound


def drv_belief_map(w, pi):
    """(:693-708) for a weight vector or [M, K] weights: the first state of largest w @ pi, and that probability per row"""
    p = np.atleast_2d(w) @ pi
    s = np.argmax(p, axis=1)
    best = p[np.arange(len(s)), s]
    gap = best - np.sort(p, axis=1)[:, -2] if p.shape[1] > 1 else np.full(len(s), np.inf)
    return (s, best, gap) if np.ndim(w) > 1 else (int(s[0]), float(best[0]), float(gap[0]))


def gm_log_pdf(x, w, mu, var):
    from scipy.special import logsumexp
    var_inv = 1 / var
    comp = -0.5 * np.log(2 * np.pi) + 0.5 * np.log(var_inv) - 0.5 * (x - mu) ** 2 * var_inv
    with np.errstate(divide='ignore'):
        return logsumexp(np.log(w) + comp)


def scalar_gm_mode(w, mu, var, bds):
    """get_scalar_gm_mode (osi/utils.py:66-98): SciPy's bounded ``minimize`` on the negative log density from every distinct
    component mean, the lowest result kept.  Returns (x, log density there, every start's (x, log density))."""
    from scipy.optimize import minimize
    runs = []
    for m in set(mu):                                       # (the reference's order of starts: it decides an exact tie)
        r = minimize(lambda x: -gm_log_pdf(x, w, mu, var), x0=m, bounds=[tuple(bds)])
        runs.append((float(r.x[0]), -float(r.fun)))
    best = max(runs, key=lambda r: r[1])
    return best[0], best[1], runs


def ambiguous(runs, x_tol=1e-3, f_tol=1e-3):
    """another of the reference's starts ends more than x_tol away in x with a log density within f_tol of the best"""
    best = max(runs, key=lambda r: r[1])
    return any(abs(x - best[0]) > x_tol and best[1] - f <= f_tol for x, f in runs)


def mode_case(seed):
    """The generator of the marginal-MAP tests: K uniform in 1..8, means U(-12, 12), variances 10^U(-2, 2), log weights = log of
    a flat Dirichlet draw plus N(0, 3) noise, renormalised; bounds (-10, 10), so that some modes sit on a bound."""
    rng = np.random.RandomState(seed)
    K = rng.randint(1, 9)
    mu = rng.uniform(-12, 12, K)
    var = 10 ** rng.uniform(-2, 2, K)
    lw = np.log(rng.dirichlet(np.ones(K))) + 3 * rng.randn(K)
    w = np.exp(lw - lw.max())
    return w / w.sum(), mu, var, (-10., 10.)


def mode_groups(n_cases, seed0=0, n_disc=4, K_of=None):
    """`n_cases` draws of ``mode_case`` (seeds seed0 ..) as batched problems, one belief per K.  A belief holds, per case j of
    its K, a query row (the case's means and variances) and an observed row o_j with unit variances and means
    sqrt(2 (max_k L_jk - L_jk)), L_j the case's log weights; its prior weights are uniform.  Evidence row j observes o_j = 0 and
    nothing else, so ``condition`` returns softmax(L_j): the case's weights, as conditional ones.  `n_disc` discrete query rows
    of 2 .. 5 states are appended.  Yields dicts: the belief's arrays, obs, X [n, n], query (continuous, then discrete), and
    the cases (w, mu, var, bds) in row order."""
    cases = [mode_case(seed0 + i) if K_of is None else mode_case_K(seed0 + i, K_of) for i in range(n_cases)]
    for K in sorted({len(c[0]) for c in cases}):
        grp = [c for c in cases if len(c[0]) == K]
        n = len(grp)
        rng = np.random.RandomState(9000 + K)
        Mu, Var = np.empty((2 * n, K)), np.ones((2 * n, K))
        for j, (w, mu, var, _) in enumerate(grp):
            L = np.log(w)
            Mu[j], Var[j] = mu, var
            Mu[n + j] = np.sqrt(2 * (L.max() - L))
        Pi = [rng.dirichlet(np.ones(s), K) for s in rng.randint(2, 6, n_disc)]
        X = np.full((n, n), np.nan)
        X[np.arange(n), np.arange(n)] = 0.0
        yield dict(w=np.full(K, 1.0 / K), Mu=Mu, Var=Var, Pi=Pi, bds=np.array([[-10.] * (2 * n), [10.] * (2 * n)]),
                   obs=n + np.arange(n), X=X, query=np.concatenate([np.arange(n), 2 * n + np.arange(n_disc)]), cases=grp,
                   n_disc=n_disc)


def mode_case_K(seed, K):
    """``mode_case`` with a given K (the K = 65 case: a second trip of the lane loop at 64 lanes)"""
    rng = np.random.RandomState(seed)
    mu = rng.uniform(-12, 12, K)
    var = 10 ** rng.uniform(-2, 2, K)
    lw = np.log(rng.dirichlet(np.ones(K))) + 3 * rng.randn(K)
    w = np.exp(lw - lw.max())
    return w / w.sum(), mu, var, (-10., 10.)


# ---- the checks shared by the CPU suite (host twins) and the GPU suite (kernels) ----------------------------------------------
def new_worst():
    """largest error seen, in units of its bound"""
    return dict(comp=0.0, logp=0.0, logcw=0.0, belief=0.0)


def check_condition(belief, case, run, worst):
    """`run(X, obs)` -> (comp, logp, condw) of the code under test; asserts the bounds, returns the longdouble restatement"""
    X, obs = case['X'], case['obs']
    comp, logp, condw = run(X, obs)
    r = restate_condition(case, dtype=np.longdouble)
    e_comp, e_logp, e_logcw = condition_bounds(r)
    r['e_logcw'] = e_logcw
    if len(obs) == 0:
        assert (comp == 0).all()
    d = np.abs(np.asarray(comp - r['comp'], dtype=np.float64))
    assert (d <= e_comp).all(), (d / np.maximum(e_comp, 1e-300)).max()
    worst['comp'] = max(worst['comp'], float((d[e_comp > 0] / e_comp[e_comp > 0]).max()) if (e_comp > 0).any() else 0)
    d = np.abs(np.asarray(logp - r['logp'], dtype=np.float64))
    assert (d <= e_logp).all(), (d / e_logp).max()
    worst['logp'] = max(worst['logp'], float((d / e_logp).max()))
    ref = np.asarray(r['logcw'], dtype=np.float64)
    live = ref > -700
    assert (condw[ref < -760] == 0).all() and (condw[live] > 0).all()
    d = np.abs(np.log(condw[live]) - ref[live])
    assert (d <= e_logcw[live] + U).all(), (d / e_logcw[live]).max()       # (+ u: the log taken by this check itself)
    worst['logcw'] = max(worst['logcw'], float((d / e_logcw[live]).max()))
    np.testing.assert_allclose(condw.sum(axis=1), 1.0, rtol=0, atol=1e-13)
    return r


def belief_points(case):
    """query rows (every row, one of them twice) and 3 points per row: values inside and outside the bounds / state indices"""
    rng = np.random.RandomState(5)
    query = np.array(list(range(NC + ND2 + ND5)) + [2])
    x = np.empty((query.size, 3))
    for j, v in enumerate(query):
        x[j] = rng.uniform(-4, 4, 3) if v < NC else rng.randint(0, case['Pi'][v - NC].shape[1], 3)
    x[-1] = x[2]
    return query, x


def check_log_belief(case, r, got, query, x, worst):
    want, bound = restate_log_belief(case, r, query, x, dtype=np.longdouble)
    d = np.abs(np.asarray(got - want, dtype=np.float64))
    assert (d <= bound).all(), (d / bound).max()
    worst['belief'] = max(worst['belief'], float((d / bound).max()))


def check_modes(grp, x, f, condw, stats):
    """criteria of the marginal-MAP test for the diagonal (evidence row j, query row j) of one group"""
    n = len(grp['cases'])
    for j, (w, mu, var, bds) in enumerate(grp['cases']):
        np.testing.assert_allclose(condw[j], w, rtol=1e-12, atol=0)           # the generator's weights, as conditional ones
        xr, fr, runs = scalar_gm_mode(condw[j], mu, var, bds)
        f_at = gm_log_pdf(x[j, j], condw[j], mu, var)
        assert abs(f_at - f[j, j]) <= 1e-12 * max(1, abs(f_at))
        stats['cases'] += 1
        stats['lower'] = max(stats['lower'], fr - f_at)
        assert f_at >= fr - 1e-9, (j, f_at, fr)
        if ambiguous(runs):
            stats['ambiguous'] += 1
        else:
            stats['far'] = max(stats['far'], abs(x[j, j] - xr))
            assert abs(x[j, j] - xr) <= 1e-4, (j, x[j, j], xr)
    Nc = 2 * n
    for m in range(n):
        for d in range(grp['n_disc']):
            s, p, gap = drv_belief_map(condw[m], grp['Pi'][d])
            assert gap >= 1e-9
            assert x[m, n + d] == s and abs(f[m, n + d] - p) <= 4 * U * len(w) * p
    return Nc




# ---- joint MAP (joint_map_from_belief_params :771-867 with get_multivar_gm_mode, osi/utils.py:101-161) ----------------------
JOINT_SHAPES = ((6, 5, 3, 2), (0, 7, 4, 2), (9, 0, 5, 3), (3, 1, 8, 5), (40, 33, 5, 2), (12, 70, 2, 4))     # (Nd, Nc, K, S)


def joint_case(shape, seed=0):
    """w ~ Dirichlet(2); Mu = base + offsets, base ~ U(-2.5, 2.5) per variable, offsets N(0, 0.6) 2 / sqrt(Nc) per component;
    Var = 10^U(-0.3, 0.5); Pi rows ~ Dirichlet(40 b_n / sqrt(Nd) + 0.5), b_n ~ Dirichlet(3); bounds +-3"""
    Nd, Nc, K, S = shape
    rng = np.random.RandomState(100 + seed + 7 * Nd + 13 * Nc + K)
    w = rng.dirichlet(2 * np.ones(K))
    Mu = Var = Pi = bds = None
    if Nc:
        Mu = rng.uniform(-2.5, 2.5, (Nc, 1)) + 0.6 * rng.randn(Nc, K) * 2 / np.sqrt(Nc)
        Var = 10 ** rng.uniform(-0.3, 0.5, (Nc, K))
        bds = np.array([[-3.] * Nc, [3.] * Nc])
    if Nd:
        Pi = np.stack([rng.dirichlet(40 * rng.dirichlet(3 * np.ones(S)) / np.sqrt(Nd) + 0.5, K) for _ in range(Nd)])
    return dict(w=w, Mu=Mu, Var=Var, Pi=Pi, bds=bds, shape=tuple(shape))


def restate_gm_ascent(log_w, MuT, Var_invT, consts, bds, x, gamma=0.05, grad_lr=0.01, grad_its=500, tol=1e-7):
    """one start of get_multivar_gm_mode: projected gradient ascent with Polyak averaging; (best x, best objective).
    MuT, Var_invT: [K, N]; consts [K]."""
    from scipy.special import logsumexp
    best_obj = prev_obj = -np.inf
    best_x, step = x, grad_lr
    for _ in range(grad_its):
        comp = consts - 0.5 * np.sum((x - MuT) ** 2 * Var_invT, axis=1)
        obj = logsumexp(log_w + comp)
        resp = np.exp(log_w + comp - obj)
        if obj > best_obj:
            best_x, best_obj = x, obj
        if obj <= prev_obj:                           # no improvement: back to the best point, half the step; the
            x = best_x                                # responsibilities stay those of the rejected point
            step *= 0.5
        dx = resp @ ((MuT - x) * Var_invT)
        x = gamma * x + (1 - gamma) * np.clip(x + dx * step, a_min=bds[0], a_max=bds[1])
        with np.errstate(invalid='ignore', divide='ignore'):
            if np.linalg.norm(dx) < tol or np.abs((obj - prev_obj) / prev_obj) < tol:     # (NaN, hence false, the first time)
                break
        prev_obj = obj
    return best_x, best_obj


def restate_joint_map(case, coord_its=100, **kw):
    """joint_map_from_belief_params, every start kept: dict(xd, xc: the winner's; xds [K, Nd], xcs [K, Nc], objs [K])"""
    from scipy.special import logsumexp
    w, Pi, Mu, Var, bds = (case[k] for k in ('w', 'Pi', 'Mu', 'Var', 'bds'))
    K, lw = len(w), np.log(w)
    xds = xcs = None
    if Pi is not None:
        Nd = len(Pi)
        lPi = [np.log(np.asarray(p)) for p in Pi]
        xds = np.stack([np.argmax(np.asarray(p), axis=-1) for p in Pi], axis=1)          # [K, Nd]
    if Mu is not None:
        Nc = len(Mu)
        MuT, Var_invT = Mu.T, 1 / Var.T
        consts = -0.5 * Nc * np.log(2 * np.pi) + 0.5 * np.sum(np.log(Var_invT), axis=1)
        xcs = np.array(MuT)
    objs = np.empty(K)
    for k in range(K):
        if Pi is not None:
            xd = xds[k]
            xd_lp = np.sum(np.stack([lPi[n][:, xd[n]] for n in range(Nd)], axis=1), axis=1)
        xc = xcs[k].copy() if Mu is not None else None
        best_obj, best_xc = -np.inf, None
        for _ in range(coord_its):
            if Mu is not None:
                xc, obj = restate_gm_ascent(lw + xd_lp if Pi is not None else lw, MuT, Var_invT, consts, bds, xc, **kw)
            if Pi is not None:
                if Mu is not None:
                    var_inv = 1 / Var.T
                    xc_lp = np.sum(-0.5 * np.log(2 * np.pi) + 0.5 * np.log(var_inv) - 0.5 * (xc - Mu.T) ** 2 * var_inv, axis=1)
                else:
                    xc_lp = 0
                tmp = lw + xc_lp
                for n in range(Nd):
                    xd_lp -= lPi[n][:, xd[n]]
                    cand = logsumexp(tmp + (xd_lp + lPi[n].T), axis=-1)
                    xd[n] = np.argmax(cand)
                    obj = cand[xd[n]]
                    xd_lp += lPi[n][:, xd[n]]
            if obj > best_obj:
                best_obj, best_xc = obj, xc                     # (the reference's best_xd aliases xd: the last sweep's is returned)
        if Mu is not None:
            xcs[k] = best_xc
        objs[k] = best_obj
    i = int(np.argmax(objs))
    return dict(xd=None if xds is None else xds[i], xc=None if xcs is None else xcs[i], xds=xds, xcs=xcs, objs=objs)


def joint_log_density(case, xd, xc):
    """log sum_k w_k prod_n pi_nk[xd_n] prod_n N(xc_n; mu_nk, var_nk) in longdouble"""
    T = np.longdouble
    t = np.log(case['w'].astype(T))
    if case['Pi'] is not None:
        for n, p in enumerate(case['Pi']):
            t = t + np.log(np.asarray(p, dtype=T)[:, int(xd[n])])
    if case['Mu'] is not None:
        mu, var = case['Mu'].astype(T), case['Var'].astype(T)
        t = t + np.sum(-T(0.5) * np.log(2 * _pi_const(T) * var) - T(0.5) * (np.asarray(xc, dtype=T)[:, None] - mu) ** 2 / var, axis=0)
    return float(t.max() + np.log(np.exp(t - t.max()).sum()))


def joint_case_mixed_states(seed=0):
    """discrete variables of 2, 5, 3 and 4 states (the reference assumes shared dstates; the restatement and the kernel do not)"""
    rng = np.random.RandomState(31 + seed)
    K, Nc = 3, 3
    Pi = [rng.dirichlet(2 * np.ones(s), K) for s in (2, 5, 3, 4)]
    Mu = rng.uniform(-2.5, 2.5, (Nc, 1)) + 0.6 * rng.randn(Nc, K) * 2 / np.sqrt(Nc)
    return dict(w=rng.dirichlet(2 * np.ones(K)), Mu=Mu, Var=10 ** rng.uniform(-0.3, 0.5, (Nc, K)), Pi=Pi,
                bds=np.array([[-3.] * Nc, [3.] * Nc]), shape=(4, Nc, K, 0))


_JOINT = {}


def joint_reference(shape):
    """(case, restated joint MAP with every start) of a shape of JOINT_SHAPES or 'mixed', computed once per process.  Asserts
    that the ascent is exercised: some start's xc ends at least 1e-3 from where it started."""
    if shape not in _JOINT:
        case = joint_case_mixed_states() if shape == 'mixed' else joint_case(shape)
        with np.errstate(all='ignore'):
            r = restate_joint_map(case)
        if case['Mu'] is not None:
            r['moved'] = float(np.abs(r['xcs'] - case['Mu'].T).max())
            assert r['moved'] >= 1e-3, (shape, r['moved'])
        _JOINT[shape] = (case, r)
    return _JOINT[shape]


def check_joint(shape, got):
    """criteria of the joint-MAP tests: xd equal, xc within 1e-9, joint log density within 1e-9; per start too"""
    case, want = joint_reference(shape)
    if want['xds'] is not None:
        np.testing.assert_array_equal(got['xds'], want['xds'])
        np.testing.assert_array_equal(got['xd'], want['xd'])
    if want['xcs'] is not None:
        np.testing.assert_allclose(got['xcs'], want['xcs'], rtol=0, atol=1e-9)
        np.testing.assert_allclose(got['xc'], want['xc'], rtol=0, atol=1e-9)
    np.testing.assert_allclose(got['objs'], want['objs'], rtol=0, atol=1e-9)
    K = len(case['w'])
    for k in range(K):
        a = joint_log_density(case, None if got['xds'] is None or not got['xds'].size else got['xds'][k],
                              None if want['xcs'] is None else got['xcs'][k])
        b = joint_log_density(case, None if want['xds'] is None else want['xds'][k], None if want['xcs'] is None else want['xcs'][k])
        assert abs(a - b) <= 1e-9, (k, a, b)
