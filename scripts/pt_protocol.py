"""The protocol that qualifies the models and quantities of the statistical tests of the tempered sampler
(tests/test_gpu_pt.py), run ahead on the CPU: the per-ladder host code (lhvi_pt_ladder_host) with NumPy draws at exactly the
tests' settings (1024 ladders, burn-in 100, 100 kept, one sweep, swaps every iteration; two_wells: 8 replicas, base mean 0 and
precision 0.1; the fixture models: 4 replicas, the default base) on three seeds.  Per quantity
z = |grand mean - expected| / (std of the per-ladder means / sqrt(ladders)); a group of quantities (discrete marginals, E[x_i],
E[x_i x_j]) stays in the test only if its largest z over the three seeds is below 3.5.  docs/kernels_pt.md records the output.

usage: python scripts/pt_protocol.py [--procs N] [model ...]      (no GPU is touched)"""
import multiprocessing as mp
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'lifted-hybrid-variational-inference_amd'), os.path.join(ROOT, 'tests')]

import pt_models as pm                                                                  # noqa: E402
from lhvi import pt                                                                     # noqa: E402

SEEDS, ZMAX = (1, 2, 3), 3.5
MODELS = ('two_wells',) + pm.STAT_FIXTURES
S = pm.STAT


def setting(name):
    """(replicas, base mean, base precision) of the test of `name`"""
    return (8, None, 0.1) if name == 'two_wells' else (4, None, None)


def chunk(args):
    """the accumulators and swap counters of ladders [lo, hi) of (model, seed): every ladder's draws from a NumPy stream of its own"""
    name, seed, lo, hi = args
    gm = pm.build(name)['gm']
    ex = gm.ex
    R, mu0, tau0 = setting(name)
    betas = pt.schedule(R)
    iters = S['num_burnin'] + S['num_samples']
    rows = []
    for l in range(lo, hi):
        rng = np.random.RandomState([seed, l])
        x0 = np.stack([rng.randint(d, size=R) for d in ex.dstates], axis=1)
        r = pt.ladder_host(gm, x0, betas, tau0, mu0, S['disc_block_its'], S['num_burnin'], S['num_samples'], 1,
                           z=rng.randn(iters, R, ex.Nc), u=rng.rand(iters, R, 1, ex.Nd), usw=rng.rand(iters, R - 1))
        rows.append(np.concatenate([r.counts, r.sum1, r.sum2, r.swap_try, r.swap_acc]))
    return np.array(rows)


def main(argv):
    procs = min(16, os.cpu_count() or 1)
    while argv and argv[0].startswith('--'):
        if argv[0] == '--procs':
            procs = int(argv[1])
        argv = argv[2:]
    L = S['ladders']
    edges = np.linspace(0, L, 4 * procs + 1).astype(int)
    with mp.Pool(procs) as pool:
        for name in (argv or MODELS):
            want = pm.expected_of(name)
            n = [w.size for w in want]
            R = setting(name)[0]
            worst = np.zeros(3)
            for seed in SEEDS:
                acc = np.concatenate(pool.map(chunk, [(name, seed, int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]))
                q = sum(n)
                z = pm.z_scores(acc[:, :n[0]], acc[:, n[0]:n[0] + n[1]], acc[:, n[0] + n[1]:q], S['num_samples'], want)
                zs = np.array([z[:n[0]].max(), z[n[0]:n[0] + n[1]].max(), z[n[0] + n[1]:].max()])
                worst = np.maximum(worst, zs)
                tried, accd = acc[:, q:q + R - 1].sum(axis=0), acc[:, q + R - 1:].sum(axis=0)
                print('%-12s seed %d: max z discrete %.2f, E[x] %.2f, E[xx] %.2f; swap rates %s'
                      % (name, seed, zs[0], zs[1], zs[2], ' '.join('%.3f' % v for v in accd / tried)), flush=True)
            print('%-12s -> %s' % (name, ', '.join('%s %s' % (g, 'qualifies' if w < ZMAX else 'does NOT qualify (z >= %.1f)' % ZMAX)
                                                    for g, w in zip(('discrete', 'E[x]', 'E[xx]'), worst))), flush=True)


if __name__ == '__main__':
    main(sys.argv[1:])
