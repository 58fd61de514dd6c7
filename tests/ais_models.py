"""Shared by the CPU and GPU tests of the annealed importance sampler (docs/kernels_ais.md): the settings of the deterministic
comparison, the injected draws, the NumPy restatement of one annealing run that is their yardstick, the device generator
restated from the doc's counter layout, and the models and step counts of the statistical tests.

The restatement assembles J, b, c and the table sum of the current x_d with this package's potential classes, tempers them
(J_beta = beta J + (1 - beta) tau0 I, b_beta, c_beta), takes ``np.linalg.cholesky`` for log det and |L^-1 b|^2, draws
x_c = mu + solve(L.T, z), forms the reduced tables by ``get_table_params_given_x_c`` and sweeps with the categorical rule of
``gibbs_models.restate`` on beta * lprobs.  Like that restatement it asserts that every injected uniform is at least MARGIN away
from every cumulative probability it is compared with; DRAW_SEED was checked on the CPU to satisfy that for every chain of
every model."""
import numpy as np

import exact_models as em
import gibbs_models as gm
from lhvi.potentials import LogTable

CHAINS, SWEEPS = 8, 2
BETAS = np.array([0., .05, .2, .5, .8, .95, 1.])
TAU0 = 1.7
MARGIN = gm.MARGIN
DRAW_SEED = 2029
DET_HOST = ('ref_hybrid2', 'rand_3_2', 'rand_8_8', 'pure_disc', 'no_disc')
DET_SHAPES = ('wide_states', 'deep_scope', 'nc1', 'nc7', 'nc33', 'nc64')

# the statistical tests: model -> steps, chosen by the protocol of docs/kernels_ais.md (scripts/ais_protocol.py, no GPU)
STAT_CHAINS = 4096
STAT_STEPS = {'ref_hybrid2': 4, 'ref_mln0': 1, 'rand_3_2': 16, 'rand_8_8': 64, 'rand_8_8_ev': 32, 'wide_states': 8, 'rand_12_16': 64}
BEYOND = (40, 8, 5)             # exact_models.rand_model(Nd, Nc, seed): no exact value
BEYOND_STEPS = 512


def mu0_of(Nc):
    """the base mean of the deterministic tests: not 0"""
    return 0.3 * np.cos(1.0 + np.arange(Nc))


def draws(model, chains=CHAINS, T=len(BETAS) - 1, its=SWEEPS, seed=DRAW_SEED):
    """(x_d0 [chains, Nd], z [T, chains, Nc], u [T, chains, its, Nd])"""
    return gm.draws(model, chains, T, its, seed)


def collapsed_mass(model, x_d, beta, tau0, mu0):
    """(log m_beta(x_d), L_beta, b_beta) by NumPy"""
    factors, Nc = model['factors'], len(model['Vc'])
    _, _, hyb_f = gm.split_factors(factors)
    A, b, c, ts = np.zeros((Nc, Nc)), np.zeros(Nc), 0.0, 0.0
    for f in factors:
        lp = f.log_potential_fun
        xd = tuple(x_d[i] for i in f.disc_nb_idx)
        if isinstance(lp, LogTable):
            ts += float(np.asarray(lp.table)[xd])
            continue
        if f in hyb_f:
            A_, b_, c_ = lp.get_quadratic_params_given_x_d(xd)
        else:
            A_, b_, c_ = np.asarray(lp.A).reshape(len(f.cont_nb_idx), -1), np.asarray(lp.b).reshape(-1), float(np.asarray(lp.c))
        sc = list(f.cont_nb_idx)
        A[np.ix_(sc, sc)] += A_
        b[sc] += b_
        c += float(c_)
    g = (1.0 - beta) * tau0
    Jb = beta * -(A + A.T) + g * np.eye(Nc)
    bb = beta * b + g * mu0
    cb = beta * c - 0.5 * g * float(mu0 @ mu0)
    if Nc == 0:
        return beta * ts + cb, np.zeros((0, 0)), bb
    assert np.linalg.cond(Jb) <= 500
    L = np.linalg.cholesky(Jb)
    y = np.linalg.solve(L, bb)
    return beta * ts + cb + 0.5 * Nc * np.log(2 * np.pi) - np.log(np.diag(L)).sum() + 0.5 * float(y @ y), L, bb


def restate_ais(model, x_d, betas, tau0, mu0, z, u, margin=MARGIN):
    """one chain: x_d [Nd], z [T, Nc], u [T, its, Nd] -> (final x_d, logw, the increments [T], smallest distance of a uniform
    from a cumulative probability)"""
    factors, dstates, Nc = model['factors'], model['dstates'], len(model['Vc'])
    Nd, T = len(dstates), len(betas) - 1
    its = u.shape[1]
    _, disc_f, hyb_f = gm.split_factors(factors)
    tables = [np.asarray(f.log_potential_fun.table) for f in disc_f]
    scopes = [f.disc_nb_idx for f in disc_f] + [f.disc_nb_idx for f in hyb_f]
    nbrs = [[j for j, sc in enumerate(scopes) if n in sc] for n in range(Nd)]
    x_d = np.array(x_d, dtype=int)
    mu0 = np.asarray(mu0, dtype=np.float64)
    inc, closest = np.zeros(T), np.inf
    for t in range(T):
        lm0, _, _ = collapsed_mass(model, x_d, betas[t], tau0, mu0)
        lm1, L, bb = collapsed_mass(model, x_d, betas[t + 1], tau0, mu0)
        inc[t] = lm1 - lm0
        if t == T - 1:
            break
        beta = betas[t + 1]
        x_c = np.zeros(0)
        if Nc:
            x_c = np.linalg.solve(L @ L.T, bb) + np.linalg.solve(L.T, z[t])
        cond = tables + gm.reduced_tables(hyb_f, x_c)
        for s in range(its):
            for n in range(Nd):
                lprobs = np.zeros(dstates[n])
                for j in nbrs[n]:
                    lprobs += cond[j][tuple(slice(None) if i == n else x_d[i] for i in scopes[j])]
                lprobs = beta * lprobs
                m = lprobs.max()
                probs = np.exp(lprobs - (m + np.log(np.exp(lprobs - m).sum())))
                cum = np.cumsum(probs)
                closest = min(closest, np.abs(u[t, s, n] - cum[:-1]).min() if len(cum) > 1 else np.inf)
                hit = np.flatnonzero(u[t, s, n] <= cum)
                x_d[n] = hit[0] if hit.size else dstates[n] - 1
    assert closest >= margin, 'an injected uniform is %.3g from a cumulative probability' % closest
    return x_d.astype(np.int32), float(inc.sum()), inc, closest


_RESTATED = {}


def restated(name):
    """(model, x0, z, u, x_d [CHAINS, Nd], logw [CHAINS]) of the deterministic comparison, computed once per model"""
    if name not in _RESTATED:
        model = gm.build(name)
        x0, z, u = draws(model)
        mu0 = mu0_of(len(model['Vc']))
        out = [restate_ais(model, x0[c], BETAS, TAU0, mu0, z[:, c], u[:, c]) for c in range(CHAINS)]
        _RESTATED[name] = (model, x0, z, u, np.array([o[0] for o in out]).reshape(CHAINS, -1), np.array([o[1] for o in out]))
    return _RESTATED[name]


def assert_matches(name, x_d, logw, what=''):
    """the deterministic pass condition: final x_d equal, logw within 1e-9 relative to max(1, |logw|)"""
    _, _, _, _, want_x, want_lw = restated(name)
    assert np.array_equal(np.asarray(x_d).reshape(want_x.shape), want_x), '%s %s: x_d differs' % (name, what)
    err = np.abs(np.asarray(logw) - want_lw) / np.maximum(1.0, np.abs(want_lw))
    assert err.max() <= 1e-9, '%s %s: logw off by %.3g relative to max(1, |logw|)' % (name, what, err.max())


# ---- the device generator, restated from docs/kernels_ais.md ("Random numbers") ------------------------------------------------
TAG_NORMAL, TAG_UNIFORM = (int.from_bytes(t, 'big') for t in (b'AISZ', b'AISU'))


def philox_normals(seed, chains, T, Nc):
    """z [T, chains, Nc]: counter (chain, step, r // 2, AISZ); Box-Muller as in gibbs_models.philox_normals"""
    t, ch, r = np.meshgrid(np.arange(T), np.arange(chains), np.arange(Nc), indexing='ij')
    u0, u1 = gm.uniform2(ch, t, r // 2, TAG_NORMAL, seed)
    rad, ang = np.sqrt(-2.0 * np.log(1.0 - u0)), 6.283185307179586 * u1
    return np.where(r % 2 == 1, rad * np.sin(ang), rad * np.cos(ang))


def philox_uniforms(seed, chains, T, its, Nd):
    """u [T, chains, its, Nd]: draw index (sweep * Nd + variable) // 2 with AISU, the first uniform for an even index"""
    t, ch, sw, n = np.meshgrid(np.arange(T), np.arange(chains), np.arange(its), np.arange(Nd), indexing='ij')
    idx = sw * Nd + n
    u0, u1 = gm.uniform2(ch, t, idx // 2, TAG_UNIFORM, seed)
    return np.where(idx % 2 == 1, u1, u0)


# ---- the statistical tests ---------------------------------------------------------------------------------------------------
def stat_solver(name):
    """(GibbsHybridGaussian over the model with its evidence applied, exact log Z): the golden fixture's logZ, or for
    wide_states the log-sum-exp of exact_models.enumerate_numpy"""
    from lhvi.gibbs import GibbsHybridGaussian
    model = em.build(name)
    for p, v in model['evidence'].items():
        model['rvs'][p].value = v
    s = GibbsHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc'])
    if name in em.SHAPE_SPECS:
        em.set_indices(model)
        logp = em.enumerate_numpy(model)[0]
        return s, float(logp.max() + np.log(np.exp(logp - logp.max()).sum()))
    return s, float(em.load_golden(name)['logZ'])


def beyond_solver():
    from lhvi.gibbs import GibbsHybridGaussian
    model = em.rand_model(em.local_ns(), *BEYOND)
    return GibbsHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc'])


def z_score(logw, logZ0, logZ_exact):
    """(mean(w~) - 1) / (std(w~) / sqrt(C)) with w~ = exp(logw + log Z0 - log Z)"""
    w = np.exp(np.asarray(logw) + logZ0 - logZ_exact)
    return float((w.mean() - 1.0) / (w.std(ddof=1) / np.sqrt(w.size)))
