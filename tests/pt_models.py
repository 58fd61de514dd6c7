"""Shared by the CPU and GPU tests of the tempered block Gibbs sampler (docs/kernels_pt.md): the model ``two_wells``, the settings
of the deterministic comparison, the injected draws, the NumPy restatement of one ladder that is their yardstick, the device
generator restated from the doc's counter layout, and the expected values and z scores of the statistical tests.

The restatement is written from the sampler's description, not from csrc/pt.hpp: per iteration every replica takes the
collapsed mass of its digits at its beta (``ais_models.collapsed_mass``: ``np.linalg.cholesky`` of J_beta), draws
x_c = mu + solve(L.T, z), forms the reduced tables and sweeps with the categorical rule of ``gibbs_models.restate`` on
beta * lprobs; replica R - 1 is recorded from iteration num_burnin on; then, when (it + 1) % swap_every == 0, the pairs
(r, r + 1), r = s mod 2, s mod 2 + 2, ... of swap round s = it // swap_every exchange their digits iff
log(1 - u) <= la.  It asserts every sweep uniform at least MARGIN from every cumulative probability it is compared with and every
|log(1 - u) - la| >= MARGIN max(1, |la|), so that a difference in the last bits cannot change a state or a decision; DRAW_SEED
was checked on the CPU to satisfy both for every ladder of every model, schedule and swap_every of the tests."""
import numpy as np

import ais_models as am
import exact_models as em
import gibbs_models as gm
from lhvi.graph import F, RV, Domain
from lhvi.potentials import LogHybridQuadratic, LogQuadratic, LogTable

LADDERS, ITERS, SWEEPS, BURNIN = 4, 7, 2, 2
TAU0 = 1.7
MARGIN = gm.MARGIN
DRAW_SEED = 2030
DET_MODELS = ('ref_hybrid2', 'rand_3_2', 'rand_8_8', 'pure_disc', 'no_disc', 'two_wells')
DET_SHAPES = ('wide_states', 'deep_scope', 'nc1', 'nc7', 'nc33', 'scratch_tables')
LADDER_BETAS = {1: [1.], 2: [.5, 1.], 3: [0., .4, 1.], 5: [0., .2, .5, .8, 1.], 8: list(np.linspace(0., 1., 8))}
SWAP_EVERY = (1, 2)
mu0_of = am.mu0_of

WELLS, WELL_S, WELL_T = (3., -3.), 1.0, (0.8, -0.5, 0.3)
TWO_WELLS_P1 = (0.644941, 0.634000, 0.634856)           # P(d_i = 1) by exact_models.enumerate_numpy


def two_wells():
    """three binary d_i, three continuous x_i: d_i selects the well of x_i, -s (x_i - well[d_i])^2; a table [0, t_i] on d_i, a
    weak unary on x_i and a coupling of neighbours.  Given x_i in a well, flipping d_i costs exp(-s (a - b)^2) = exp(-36)."""
    db, dc = Domain((0, 1)), Domain((-10, 10), continuous=True)
    Vd, Vc = [RV(db) for _ in range(3)], [RV(dc) for _ in range(3)]
    a, b = WELLS
    factors = []
    for i in range(3):
        factors.append(F(nb=(Vd[i], Vc[i]), log_potential_fun=LogHybridQuadratic(
            A=np.array([[[-WELL_S]], [[-WELL_S]]]), b=np.array([[2 * WELL_S * a], [2 * WELL_S * b]]),
            c=np.array([-WELL_S * a * a, -WELL_S * b * b]))))
        factors.append(F(nb=(Vd[i],), log_potential_fun=LogTable(np.array([0., WELL_T[i]]))))
        factors.append(F(nb=(Vc[i],), log_potential_fun=LogQuadratic(np.array([[-0.05]]), np.zeros(1), 0.)))
    for i in range(2):
        factors.append(F(nb=(Vc[i], Vc[i + 1]), log_potential_fun=LogQuadratic(-0.15 * np.array([[1., -1.], [-1., 1.]]), np.zeros(2), 0.)))
    return dict(rvs=Vd + Vc, factors=factors, Vd=Vd, Vc=Vc, evidence={})


_BUILT = {}


def build(name):
    """the model dict of gibbs_models.build (two_wells: this module's), built once"""
    if name not in _BUILT:
        _BUILT[name] = gm.finish(two_wells()) if name == 'two_wells' else gm.build(name)
    return _BUILT[name]


def draws(model, R, ladders=LADDERS, iters=ITERS, its=SWEEPS, seed=DRAW_SEED):
    """(x_d0 [ladders, R, Nd], z [iters, ladders * R, Nc], u [iters, ladders * R, its, Nd], usw [iters, ladders, max(R - 1, 1)])"""
    x0, z, u = gm.draws(model, ladders * R, iters, its, seed)
    usw = np.random.RandomState(seed + 1).rand(iters, ladders, max(R - 1, 1))
    return x0.reshape(ladders, R, -1), z, u, usw


def transition(model, x_d, beta, L, bb, z, u):
    """one block Gibbs iteration at beta from the factor of J_beta: (x_c, the new x_d, the smallest distance of a uniform from a
    cumulative probability)"""
    factors, dstates, Nc = model['factors'], model['dstates'], len(model['Vc'])
    Nd = len(dstates)
    _, disc_f, hyb_f = gm.split_factors(factors)
    tables = [np.asarray(f.log_potential_fun.table) for f in disc_f]
    scopes = [f.disc_nb_idx for f in disc_f] + [f.disc_nb_idx for f in hyb_f]
    nbrs = [[j for j, sc in enumerate(scopes) if n in sc] for n in range(Nd)]
    x_d, closest = np.array(x_d, dtype=int), np.inf
    x_c = np.linalg.solve(L @ L.T, bb) + np.linalg.solve(L.T, z) if Nc else np.zeros(0)
    cond = tables + gm.reduced_tables(hyb_f, x_c)
    for s in range(u.shape[0]):
        for n in range(Nd):
            lprobs = np.zeros(dstates[n])
            for j in nbrs[n]:
                lprobs += cond[j][tuple(slice(None) if i == n else x_d[i] for i in scopes[j])]
            lprobs = beta * lprobs
            m = lprobs.max()
            cum = np.cumsum(np.exp(lprobs - (m + np.log(np.exp(lprobs - m).sum()))))
            closest = min(closest, np.abs(u[s, n] - cum[:-1]).min() if len(cum) > 1 else np.inf)
            hit = np.flatnonzero(u[s, n] <= cum)
            x_d[n] = hit[0] if hit.size else dstates[n] - 1
    return x_c, x_d, closest


def restate_pt(model, x_d, betas, tau0, mu0, z, u, usw, num_burnin=BURNIN, swap_every=1, margin=MARGIN):
    """one ladder: x_d [R, Nd], z [iters, R, Nc], u [iters, R, its, Nd], usw [iters, max(R - 1, 1)] -> dict of disc
    [kept, Nd], cont [kept, Nc], counts, sum1, sum2 (lower triangle, row-major), x_d [R, Nd], swap_try / swap_acc [R - 1],
    la (every log ratio, in order) and accepted (the list of accepted (iteration, pair))"""
    dstates, Nc = model['dstates'], len(model['Vc'])
    betas = np.asarray(betas, dtype=np.float64)
    R, iters = len(betas), len(usw)
    x = [np.array(row, dtype=int) for row in np.asarray(x_d).reshape(R, -1)]
    off = np.concatenate([[0], np.cumsum(dstates)]).astype(int)
    out = dict(disc=[], cont=[], counts=np.zeros(off[-1], dtype=np.int32), sum1=np.zeros(Nc), sum2=np.zeros(Nc * (Nc + 1) // 2),
               swap_try=np.zeros(R - 1, dtype=np.int32), swap_acc=np.zeros(R - 1, dtype=np.int32), la=[], accepted=[])
    mu0 = np.asarray(mu0, dtype=np.float64)
    lm = lambda d, beta: am.collapsed_mass(model, d, beta, tau0, mu0)                   # noqa: E731
    ti, tj = np.tril_indices(Nc)
    closest, gap = np.inf, np.inf
    for it in range(iters):
        for r in range(R):
            _, L, bb = lm(x[r], betas[r])
            x_c, x[r], c = transition(model, x[r], betas[r], L, bb, z[it, r], u[it, r])
            closest = min(closest, c)
        if it >= num_burnin:
            out['disc'].append(x[R - 1].copy())
            out['cont'].append(x_c.copy())
            for n, k in enumerate(x[R - 1]):
                out['counts'][off[n] + k] += 1
            out['sum1'] += x_c
            out['sum2'] += x_c[ti] * x_c[tj]
        if swap_every > 0 and (it + 1) % swap_every == 0:
            s = it // swap_every
            for r in range(s % 2, R - 1, 2):
                la = lm(x[r + 1], betas[r])[0] + lm(x[r], betas[r + 1])[0] - lm(x[r], betas[r])[0] - lm(x[r + 1], betas[r + 1])[0]
                lu = np.log(1.0 - usw[it, r])
                gap = min(gap, abs(lu - la) / max(1.0, abs(la)))
                out['la'].append(la)
                out['swap_try'][r] += 1
                if lu <= la:
                    out['swap_acc'][r] += 1
                    out['accepted'].append((it, r))
                    x[r], x[r + 1] = x[r + 1], x[r]
    assert closest >= margin, 'an injected uniform is %.3g from a cumulative probability' % closest
    assert gap >= margin, 'a swap uniform is %.3g (relative) from its log ratio' % gap
    kept = len(out['disc'])
    out['disc'] = np.array(out['disc'], dtype=np.int32).reshape(kept, len(dstates))
    out['cont'] = np.array(out['cont']).reshape(kept, Nc)
    out['x_d'] = np.array(x, dtype=np.int32).reshape(R, len(dstates))
    return out


_RESTATED = {}


def restated(name, R, swap_every=1, betas=None):
    """(model, x0, z, u, usw, [restate_pt of every ladder]) of the deterministic comparison, computed once per case"""
    key = (name, R, swap_every, None if betas is None else tuple(betas))
    if key not in _RESTATED:
        model = build(name)
        x0, z, u, usw = draws(model, R)
        b = LADDER_BETAS[R] if betas is None else betas
        mu0 = mu0_of(len(model['Vc']))
        z4, u4 = z.reshape(ITERS, LADDERS, R, -1), u.reshape(ITERS, LADDERS, R, u.shape[2], -1)
        _RESTATED[key] = (model, x0, z, u, usw, [restate_pt(model, x0[l], b, TAU0, mu0, z4[:, l], u4[:, l], usw[:, l],
                                                            swap_every=swap_every) for l in range(LADDERS)])
    return _RESTATED[key]


FIELDS_EQUAL = ('disc', 'x_d', 'swap_try', 'swap_acc', 'counts')
FIELDS_CLOSE = ('cont', 'sum1', 'sum2')


def assert_matches(want, got, what=''):
    """the deterministic pass condition of one ladder: kept discrete samples, final x_d of every replica, counts and both swap
    counters equal; continuous samples and accumulators rtol 1e-9 / atol 1e-12.  got: a mapping or namespace of arrays"""
    get = (lambda k: got[k]) if isinstance(got, dict) else (lambda k: getattr(got, k))
    for k in FIELDS_EQUAL:
        np.testing.assert_array_equal(np.asarray(get(k)).reshape(want[k].shape), want[k], err_msg='%s: %s' % (what, k))
    for k in FIELDS_CLOSE:
        np.testing.assert_allclose(np.asarray(get(k)).reshape(want[k].shape), want[k], rtol=1e-9, atol=1e-12, err_msg='%s: %s' % (what, k))


# ---- the device generator, restated from docs/kernels_pt.md ("Random numbers") -------------------------------------------------
TAG_NORMAL, TAG_UNIFORM, TAG_SWAP = (int.from_bytes(t, 'big') for t in (b'PTNZ', b'PTUF', b'PTSW'))


def philox_normals(seed, ladders, R, iters, Nc):
    """z [iters, ladders * R, Nc]: counter (ladder * R + r, iteration, i // 2, PTNZ); Box-Muller as in gibbs_models"""
    it, ch, i = np.meshgrid(np.arange(iters), np.arange(ladders * R), np.arange(Nc), indexing='ij')
    u0, u1 = gm.uniform2(ch, it, i // 2, TAG_NORMAL, seed)
    rad, ang = np.sqrt(-2.0 * np.log(1.0 - u0)), 6.283185307179586 * u1
    return np.where(i % 2 == 1, rad * np.sin(ang), rad * np.cos(ang))


def philox_uniforms(seed, ladders, R, iters, its, Nd):
    """u [iters, ladders * R, its, Nd]: draw index (sweep * Nd + variable) // 2 with PTUF, the first uniform for an even index"""
    it, ch, sw, n = np.meshgrid(np.arange(iters), np.arange(ladders * R), np.arange(its), np.arange(Nd), indexing='ij')
    idx = sw * Nd + n
    u0, u1 = gm.uniform2(ch, it, idx // 2, TAG_UNIFORM, seed)
    return np.where(idx % 2 == 1, u1, u0)


def philox_swaps(seed, ladders, R, iters):
    """usw [iters, ladders, max(R - 1, 1)]: the first uniform of counter (ladder, iteration, pair, PTSW)"""
    it, l, p = np.meshgrid(np.arange(iters), np.arange(ladders), np.arange(max(R - 1, 1)), indexing='ij')
    return gm.uniform2(l, it, p, TAG_SWAP, seed)[0]


# ---- the statistical tests ---------------------------------------------------------------------------------------------------
STAT = dict(ladders=1024, num_burnin=100, num_samples=100, disc_block_its=1)
STAT_FIXTURES = ('ref_hybrid2', 'rand_8_8')             # at 4 replicas, against tests/golden/exact_*.npz
Z_BOUND = 4.5


def expected_of(name):
    """(discrete marginals concatenated, E[x_c], E[x_i x_j] lower triangle by rows): two_wells by exact_models.enumerate_numpy,
    the fixture models from the reference's recorded exact results (test_gpu_gibbs.expected_of)"""
    if name == 'two_wells':
        model = build(name)
        logp, mu, sig, _ = em.enumerate_numpy(model)
        t = np.exp(logp - logp.max())
        t /= t.sum()
        joint = t.reshape(model['dstates'])
        marg = np.concatenate([joint.sum(axis=tuple(a for a in range(joint.ndim) if a != n)) for n in range(joint.ndim)])
    else:
        g = em.load_golden(name)
        t, mu, marg = g['table'], g['means'], g['marg']
    i, j = np.tril_indices(mu.shape[1])
    sig_tril = sig[:, i, j] if name == 'two_wells' else g['covs_tril']
    return marg, t @ mu, t @ (sig_tril + mu[:, i] * mu[:, j])


def z_scores(counts, sum1, sum2, num_samples, want):
    """|grand mean - expected| / (std of the per-ladder means / sqrt(ladders)) of every quantity of ``expected_of``, in its
    order, from per-ladder accumulators [ladders, ...]"""
    got = np.concatenate([counts, sum1, sum2], axis=1) / float(num_samples)
    want = np.concatenate(want)
    assert got.shape[1] == want.size
    return np.abs(got.mean(axis=0) - want) / (got.std(axis=0, ddof=1) / np.sqrt(got.shape[0]))
