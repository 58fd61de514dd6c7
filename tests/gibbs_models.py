"""Shared by the CPU and GPU tests of the block Gibbs sampler: the models of the deterministic comparison, the injected draws,
and the NumPy restatement of gibbs/hybrid_gaussian_mrf.py::block_gibbs_sample :216-263 that is their yardstick.

The restatement fixes x_c = mu + solve(L.T, z) with L the Cholesky factor of J = -2A, the conditional tables by the formula of
LogHybridQuadratic.get_table_params_given_x_c, and the sweep of disc_mrf.gibbs_sample_one with the categorical rule of
disc_mrf_sampler.pyx (softmax as exp(v - (m + log(sum))), the first state with u <= cumulative sum).  It asserts that every
injected uniform is at least MARGIN away from every cumulative probability it is compared with, so that a difference in the
last bits of a probability cannot change a state; DRAW_SEED was checked on the CPU to satisfy that for every chain of every
model.

``philox_normals`` / ``philox_uniforms`` / ``philox_init`` restate the device generator from the counter layout written down in
docs/kernels_gibbs.md ("Random numbers"), independently of csrc/gibbs.hpp."""
import numpy as np

import exact_models as em
from lhvi import exact, gibbs
from lhvi.graph import F, RV, Domain
from lhvi.potentials import LogHybridQuadratic, LogQuadratic, LogTable

DET_MODELS = ('ref_hybrid2', 'rand_3_2', 'rand_8_8', 'pure_disc', 'no_disc',
              'wide_states', 'deep_scope', 'nc1', 'nc7', 'nc33', 'nc64')    # exact_models.SHAPE_SPECS: shapes the fixtures lack
CHAINS, ITERS, ITS, BURNIN = 8, 6, 3, 2
MARGIN = 1e-9
DRAW_SEED = 2026


def pure_disc():
    """Nc = 0: five variables (2, 3, 2, 4, 2 states), a unary table on each and five tables of arity 2 - 3"""
    rng = np.random.RandomState(21)
    Vd = [RV(Domain(tuple(range(d)))) for d in (2, 3, 2, 4, 2)]
    scopes = [(0,), (1,), (2,), (3,), (4,), (0, 1), (1, 2), (3, 2), (4, 0, 3), (1, 3)]
    factors = [F(nb=tuple(Vd[i] for i in sc), log_potential_fun=LogTable(rng.randn(*[Vd[i].dstates for i in sc]))) for sc in scopes]
    return dict(rvs=list(Vd), factors=factors, Vd=Vd, Vc=[], evidence={})


def no_disc():
    """Nd = 0: five continuous variables, the Gaussian draw alone; one LogHybridQuadratic without a discrete axis, which counts
    as a continuous factor"""
    rng = np.random.RandomState(22)
    Vc = [RV(Domain((-10, 10), continuous=True)) for _ in range(5)]
    factors = [F(nb=(rv,), log_potential_fun=LogQuadratic(-(0.5 + rng.rand(1, 1)), rng.randn(1), 0.)) for rv in Vc]
    for i, j in ((0, 1), (1, 2), (2, 3), (3, 4), (4, 0)):
        a = rng.randn()
        factors.append(F(nb=(Vc[i], Vc[j]), log_potential_fun=LogQuadratic(-0.3 * np.array([[a * a, -a], [-a, 1.]]), np.zeros(2), 0.)))
    factors.append(F(nb=(Vc[2],), log_potential_fun=LogHybridQuadratic(np.array([[-0.25]]), np.array([0.5]), np.array(0.1))))
    return dict(rvs=list(Vc), factors=factors, Vd=[], Vc=Vc, evidence={})


def not_pd():
    """two binary variables, two continuous: J is indefinite wherever d1 = 1 (tests/test_exact_host.py::not_pd_model)"""
    db, dc = Domain((0, 1)), Domain((-10, 10), continuous=True)
    d0, d1, x, y = RV(db), RV(db), RV(dc), RV(dc)
    factors = [F(nb=(x, y), log_potential_fun=LogQuadratic(-0.5 * np.array([[1., -1.], [-1., 1.]]), np.zeros(2), 0.)),
               F(nb=(d1, x), log_potential_fun=LogHybridQuadratic(np.array([[[-0.5]], [[0.25]]]), np.zeros((2, 1)), np.zeros(2))),
               F(nb=(d0,), log_potential_fun=LogTable(np.array([0.1, 0.2])))]
    return dict(rvs=[d0, d1, x, y], factors=factors, Vd=[d0, d1], Vc=[x, y], evidence={})


def build(name):
    """model dict with disc_nb_idx / cont_nb_idx set, plus dstates and the GibbsModel"""
    model = {'pure_disc': pure_disc, 'no_disc': no_disc, 'not_pd': not_pd}[name]() if name in ('pure_disc', 'no_disc', 'not_pd') \
        else em.build(name)
    return finish(model)


def finish(model):
    em.set_indices(model)
    model['dstates'] = [rv.dstates for rv in model['Vd']]
    model['gm'] = gibbs.GibbsModel(exact.flatten_factors(model['factors'], model['dstates'], len(model['Vc'])))
    return model


def draws(model, chains=CHAINS, iters=ITERS, its=ITS, seed=DRAW_SEED):
    """(x_d0 [chains, Nd], z [iters, chains, Nc], u [iters, chains, its, Nd]) of the deterministic tests"""
    rng = np.random.RandomState(seed)
    Nd, Nc = len(model['Vd']), len(model['Vc'])
    its = 1 if Nd == 1 else its
    x0 = np.stack([rng.randint(0, d, size=chains) for d in model['dstates']], axis=1).astype(np.int32) if Nd else \
        np.zeros((chains, 0), dtype=np.int32)
    return x0, rng.randn(iters, chains, Nc), rng.rand(iters, chains, its, Nd)


def split_factors(factors):
    """(continuous, discrete, strictly hybrid) factors, each in factor order"""
    cont_f, disc_f, hyb_f = [], [], []
    for f in factors:
        lp = f.log_potential_fun
        if isinstance(lp, LogQuadratic) or (isinstance(lp, LogHybridQuadratic) and np.ndim(lp.c) == 0):
            cont_f.append(f)
        elif isinstance(lp, LogHybridQuadratic):
            hyb_f.append(f)
        else:
            disc_f.append(f)
    return cont_f, disc_f, hyb_f


def reduced_tables(hyb_f, x_c):
    """the log table of every strictly hybrid factor at x_c, shaped by the factor's own discrete scope"""
    return [np.asarray(f.log_potential_fun.get_table_params_given_x_c(x_c[list(f.cont_nb_idx)])) for f in hyb_f]


def restate(model, x_d, z, u, num_burnin=0, margin=MARGIN):
    """one chain: x_d [Nd], z [iters, Nc], u [iters, its, Nd] -> (disc [iters - num_burnin, Nd], cont [.., Nc], smallest
    distance of a uniform from a cumulative probability)"""
    factors, dstates, Nc = model['factors'], model['dstates'], len(model['Vc'])
    Nd = len(dstates)
    iters, its = u.shape[0], u.shape[1]
    cont_f, disc_f, hyb_f = split_factors(factors)
    tables = [np.asarray(f.log_potential_fun.table) for f in disc_f]
    scopes = [f.disc_nb_idx for f in disc_f] + [f.disc_nb_idx for f in hyb_f]
    nbrs = [[j for j, sc in enumerate(scopes) if n in sc] for n in range(Nd)]
    x_d = np.array(x_d, dtype=int)
    disc, cont, closest = [], [], np.inf
    for it in range(iters):
        A, b = np.zeros((Nc, Nc)), np.zeros(Nc)
        for f in factors:
            lp = f.log_potential_fun
            if isinstance(lp, LogTable):
                continue
            if f in hyb_f:
                A_, b_, _ = lp.get_quadratic_params_given_x_d(tuple(x_d[i] for i in f.disc_nb_idx))
            else:
                A_, b_ = np.asarray(lp.A).reshape(len(f.cont_nb_idx), -1), np.asarray(lp.b).reshape(-1)
            sc = list(f.cont_nb_idx)
            A[np.ix_(sc, sc)] += A_
            b[sc] += b_
        x_c = np.zeros(0)
        if Nc:
            J = -2. * A
            assert np.linalg.cond(J) <= 500
            L = np.linalg.cholesky(J)
            x_c = np.linalg.solve(J, b) + np.linalg.solve(L.T, z[it])
        cond = tables + reduced_tables(hyb_f, x_c)
        for s in range(its):
            for n in range(Nd):
                lprobs = np.zeros(dstates[n])
                for j in nbrs[n]:
                    lprobs += cond[j][tuple(slice(None) if i == n else x_d[i] for i in scopes[j])]
                m = lprobs.max()
                probs = np.exp(lprobs - (m + np.log(np.exp(lprobs - m).sum())))
                cum = np.cumsum(probs)
                closest = min(closest, np.abs(u[it, s, n] - cum[:-1]).min() if len(cum) > 1 else np.inf)
                hit = np.flatnonzero(u[it, s, n] <= cum)
                x_d[n] = hit[0] if hit.size else dstates[n] - 1
        if it >= num_burnin:
            disc.append(x_d.copy())
            cont.append(x_c.copy())
    assert closest >= margin, 'an injected uniform is %.3g from a cumulative probability' % closest
    return np.array(disc).reshape(len(disc), Nd), np.array(cont).reshape(len(cont), Nc), closest


# ---- the device generator, restated from docs/kernels_gibbs.md ---------------------------------------------------------------------
TAG_NORMAL, TAG_UNIFORM, TAG_INIT = (int.from_bytes(t, 'big') for t in (b'GBNZ', b'GBUF', b'GBXI'))


def philox4(c0, c1, c2, c3, seed):
    """Philox4x32-10 on uint64 arrays holding 32-bit counter words; key = (low, high) word of the seed"""
    m32 = np.uint64(0xffffffff)
    c = [np.asarray(a, dtype=np.uint64) & m32 for a in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(seed) & 0xffffffff, (int(seed) >> 32) & 0xffffffff
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xffffffff, (k1 + 0xBB67AE85) & 0xffffffff
    return c


def uniform2(a, b, draw, tag, seed):
    """the two 53-bit uniforms in [0, 1) of counter (a, b, draw, tag): words (0, 1) and (2, 3), high word first"""
    c = philox4(a, b, draw, tag, seed)
    r0, r1 = (c[0] << np.uint64(32)) | c[1], (c[2] << np.uint64(32)) | c[3]
    return (r0 >> np.uint64(11)).astype(np.float64) * 2.0 ** -53, (r1 >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def philox_normals(seed, chains, iters, Nc):
    """z [iters, chains, Nc]: counter (chain, iteration, r // 2, GBNZ); Box-Muller radius sqrt(-2 log(1 - u0)), angle 2 pi u1,
    cosine for even r, sine for odd r"""
    it, ch, r = np.meshgrid(np.arange(iters), np.arange(chains), np.arange(Nc), indexing='ij')
    u0, u1 = uniform2(ch, it, r // 2, TAG_NORMAL, seed)
    rad, ang = np.sqrt(-2.0 * np.log(1.0 - u0)), 6.283185307179586 * u1
    return np.where(r % 2 == 1, rad * np.sin(ang), rad * np.cos(ang))


def philox_uniforms(seed, chains, iters, its, Nd):
    """u [iters, chains, its, Nd]: draw index (sweep * Nd + variable) // 2 with GBUF, the first uniform for an even index"""
    it, ch, sw, n = np.meshgrid(np.arange(iters), np.arange(chains), np.arange(its), np.arange(Nd), indexing='ij')
    idx = sw * Nd + n
    u0, u1 = uniform2(ch, it, idx // 2, TAG_UNIFORM, seed)
    return np.where(idx % 2 == 1, u1, u0)


def philox_init(seed, chains, dstates):
    """x_d [chains, Nd] of gibbs_init_kernel: counter (chain, variable, 0, GBXI), state floor(u0 d) capped at d - 1"""
    ch, n = np.meshgrid(np.arange(chains), np.arange(len(dstates)), indexing='ij')
    u0, _ = uniform2(ch, n, 0, TAG_INIT, seed)
    d = np.asarray(dstates)[None, :]
    return np.minimum((u0 * d).astype(np.int64), d - 1).astype(np.int32)
