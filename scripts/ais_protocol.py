"""The protocol that chooses the number of annealing steps of the statistical tests (tests/test_gpu_ais.py), run ahead on the
CPU: the per-chain host code (lhvi_ais_chain_host) with NumPy draws at the tests' settings (4096 chains, one sweep, the default
base: mean 0, precision 1, linear schedule) on three seeds.  Per model: the smallest power of two T <= 1024 at which the
standard deviation of the log weights is at most 0.5 on all three seeds; the model qualifies if the largest |z| of the three is
below 3.5, z = (mean(w~) - 1) / (std(w~) / sqrt(C)), w~ = exp(logw + log Z0 - log Z).  The model without an exact value
(rand_model(40, 8, 5)) reports the spread and the three estimates instead.  docs/kernels_ais.md records the output and
tests/ais_models.py::STAT_STEPS the chosen T.

usage: python scripts/ais_protocol.py [--procs N] [--first T] [model ...]      (no GPU is touched)"""
import multiprocessing as mp
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'lifted-hybrid-variational-inference_amd'), os.path.join(ROOT, 'tests')]

import ais_models as am                                                                 # noqa: E402
import exact_models as em                                                               # noqa: E402
from lhvi import ais                                                                    # noqa: E402

CHAINS, SEEDS, CAP, SPREAD, ZMAX = am.STAT_CHAINS, (1, 2, 3), 1024, 0.5, 3.5
MODELS = em.FULL + ('wide_states', 'rand_12_16', 'beyond')
_GM = {}


def model_of(name):
    if name not in _GM:
        _GM[name] = (am.beyond_solver(), None) if name == 'beyond' else am.stat_solver(name)
    return _GM[name]


def chunk(args):
    """log weights of chains [lo, hi) of (model, T, seed): every chain's draws from a NumPy stream of its own"""
    name, T, seed, lo, hi = args
    gm = model_of(name)[0].model
    ex = gm.ex
    betas = ais.schedule(T)
    out = np.zeros(hi - lo)
    for c in range(lo, hi):
        rng = np.random.RandomState([seed, c, T])
        x0 = [rng.randint(d) for d in ex.dstates]
        out[c - lo] = ais.chain_host(gm, x0, betas, 1.0, None, 1, z=rng.randn(T, ex.Nc), u=rng.rand(T, 1, ex.Nd)).logw
    return out


def run(pool, procs, name, T, seed):
    edges = np.linspace(0, CHAINS, 4 * procs + 1).astype(int)
    return np.concatenate(pool.map(chunk, [(name, T, seed, int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]))


def main(argv):
    procs, first = min(16, os.cpu_count() or 1), 1
    while argv and argv[0].startswith('--'):
        if argv[0] == '--procs':
            procs = int(argv[1])
        elif argv[0] == '--first':
            first = int(argv[1])
        argv = argv[2:]
    with mp.Pool(procs) as pool:
        for name in (argv or MODELS):
            solver, logZ = model_of(name)
            gm = solver.model
            logZ0 = ais.log_z0(gm.ex.dstates, gm.ex.Nc, 1.0) + solver.log_const
            T = first
            while True:
                lw = [run(pool, procs, name, T, seed) for seed in SEEDS]
                sd = [float(w.std(ddof=1)) for w in lw]
                est = [ais.estimates(ais.reduce_numpy(w), CHAINS, logZ0) for w in lw]
                line = '%-12s T = %4d: std(logw) %s' % (name, T, ' / '.join('%.3f' % s for s in sd))
                if logZ is None:
                    line += '; logZ %s' % ' / '.join('%.3f +- %.3f' % (e.logZ, e.stderr) for e in est)
                else:
                    z = [am.z_score(w, logZ0, logZ) for w in lw]
                    line += '; z %s; lower - logZ %s' % (' / '.join('%+.2f' % v for v in z),
                                                       ' / '.join('%+.3f (se %.3f)' % (e.lower - logZ, e.lower_stderr) for e in est))
                print(line, flush=True)
                if max(sd) <= SPREAD:
                    ok = logZ is None or max(abs(v) for v in z) < ZMAX
                    print('%-12s -> T = %d, %s' % (name, T, 'qualifies' if ok else 'does NOT qualify (|z| >= %.1f)' % ZMAX), flush=True)
                    break
                if T >= CAP:
                    print('%-12s -> spread above %.1f at the cap of %d steps: left out' % (name, SPREAD, CAP), flush=True)
                    break
                T *= 2


if __name__ == '__main__':
    main(sys.argv[1:])
