"""The statistical tests of the Rao-Blackwellised marginals (tests/test_gpu_gibbs_rb.py) run ahead on the CPU: the per-chain host
code (lhvi_gibbs_chain_host, lhvi_gibbs_rb_disc_host, lhvi_exact_config_at_host) with NumPy draws at the tests' settings (4096
chains, burn-in 50, 50 kept, 10 sweeps) on three seeds.  Prints, per model and seed, the largest z = |grand mean - expected| /
(standard error over chains) of the RB discrete marginals, E[x_i], E[x_i^2] and (rand_8_8) the RB density at the test's five points, and
whether every configuration occurs among the kept samples (the precondition of the KL inequality).  docs/kernels_gibbs_rb.md
records the output; a quantity enters the GPU tests only if it stayed below 3.5 on all three seeds.

usage: python scripts/gibbs_rb_host_check.py [model ...]      (no GPU is touched)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'lifted-hybrid-variational-inference_amd'), os.path.join(ROOT, 'tests')]

import exact_models as em                                                               # noqa: E402
from lhvi import exact, gibbs                                                           # noqa: E402

CHAINS, BURNIN, KEPT, SWEEPS = 4096, 50, 50, 10
SEEDS = (1, 2, 3)
MODELS = ('ref_hybrid2', 'ref_mln0', 'rand_3_2', 'rand_8_8', 'rand_8_8_ev', 'wide_states')


def expected(name, solver):
    """(discrete marginals, E[x_i], E[x_i^2], table [M], means [M, Nc], variances [M, Nc])"""
    if name == 'wide_states':
        model = em.build(name)
        em.set_indices(model)
        logp, mu, sig, _ = em.enumerate_numpy(model)
        t = np.exp(logp - logp.max())
        t /= t.sum()
        joint = t.reshape(9, 5, 2)
        marg = np.concatenate([joint.sum(axis=(1, 2)), joint.sum(axis=(0, 2)), joint.sum(axis=(0, 1))])
        var = sig[:, np.arange(3), np.arange(3)]
    else:
        g = em.load_golden(name)
        t, mu, marg = g['table'], g['means'], g['marg']
        i, j = np.tril_indices(mu.shape[1])
        var = g['covs_tril'][:, i == j]
    return marg, t @ mu, t @ (var + mu * mu), t, mu, var


def run(name, seed):
    model, solver = em.solver(name)
    s = gibbs.GibbsHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc'])
    gm = s.model
    ex = gm.ex
    Nd, Nc = ex.Nd, ex.Nc
    rng = np.random.RandomState(seed)
    iters = BURNIN + KEPT
    disc, cont, prob = np.zeros((CHAINS, KEPT, Nd), dtype=np.int32), np.zeros((CHAINS, KEPT, Nc)), np.zeros((CHAINS, gm.n_states))
    for c in range(CHAINS):
        x0 = [rng.randint(d) for d in ex.dstates]
        r = gibbs.chain_host(gm, x0, rng.randn(iters, Nc), rng.rand(iters, SWEEPS, Nd), SWEEPS, BURNIN, KEPT)
        disc[c], cont[c] = r.disc, r.cont
        prob[c] = gibbs.rb_disc_host(gm, r.disc, r.cont) / KEPT
    rows, inverse, counts = np.unique(disc.reshape(-1, Nd), axis=0, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(CHAINS, KEPT)
    comp = [exact.config_at_host(ex, row) for row in rows]
    means, vars_ = np.array([c[1] for c in comp]), np.array([c[2] for c in comp])
    marg, m1, m2, table, mu, var = expected(name, solver)

    def z_of(per_chain, want):
        se = per_chain.std(axis=0, ddof=1) / np.sqrt(CHAINS)
        diff = np.abs(per_chain.mean(axis=0) - want)
        ok = se > 1e-9
        return float((diff[ok] / se[ok]).max()) if ok.any() else 0.0
    out = dict(disc=z_of(prob, marg), mean=z_of(means[inverse].mean(axis=1), m1),
               second=z_of((vars_ + means ** 2)[inverse].mean(axis=1), m2), U=len(rows), M=len(table))
    if name == 'rand_8_8':
        worst = 0.0
        for i, rv in enumerate(s.Vc):
            sd = np.sqrt(m2[i] - m1[i] ** 2)
            x = m1[i] + sd * np.linspace(-2, 2, 5)            # the test's five points: the exact marginal's mean +- 2 sd
            dens = lambda w_, m_, v_: (w_[..., None] * np.exp(-0.5 * (x - m_[..., None]) ** 2 / v_[..., None])      # noqa: E731
                                       / np.sqrt(2 * np.pi * v_[..., None]))
            want = dens(table, mu[:, i], var[:, i]).sum(axis=0)
            grid = np.linspace(rv.domain.values[0], rv.domain.values[1], 2001)
            peak = (table[:, None] * np.exp(-0.5 * (grid - mu[:, i][:, None]) ** 2 / var[:, i][:, None])
                    / np.sqrt(2 * np.pi * var[:, i][:, None])).sum(axis=0).max()
            keep = want >= 1e-3 * peak
            per = dens(np.ones((CHAINS, KEPT)), means[:, i][inverse], vars_[:, i][inverse]).mean(axis=1)
            se = per.std(axis=0, ddof=1) / np.sqrt(CHAINS)
            worst = max(worst, float((np.abs(per.mean(axis=0) - want) / se)[keep].max()))
            assert keep.sum() >= 3, (i, keep)
        out['density'] = worst
    return out


if __name__ == '__main__':
    for name in (sys.argv[1:] or MODELS):
        for seed in SEEDS:
            r = run(name, seed)
            print('%-12s seed %d: max z discrete %.2f, mean %.2f, second %.2f%s; U = %d of M = %d configurations%s'
                  % (name, seed, r['disc'], r['mean'], r['second'], ', density %.2f' % r['density'] if 'density' in r else '',
                     r['U'], r['M'], ' (all occur)' if r['U'] == r['M'] else ''), flush=True)
