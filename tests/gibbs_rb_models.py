"""Shared by the CPU and GPU tests of the Rao-Blackwellised marginals of the block Gibbs sampler (docs/kernels_gibbs_rb.md): the
NumPy restatement of the conditional probabilities p(x_n = k | x_d,-n, x_c), built on gibbs_models.reduced_tables /
split_factors (the yardstick of the sampler's own sweep), the rows of digits of the configs_at comparison, and the kept samples
of the existing deterministic run that the tests feed back."""
import numpy as np

import exact_models as em
import gibbs_models as gmod
from lhvi import gibbs

ENUMERABLE = tuple(n for n in gmod.DET_MODELS if n not in ('pure_disc',))     # Nc > 0: no_disc has one configuration
DISC_MODELS = tuple(n for n in gmod.DET_MODELS if n != 'no_disc')            # Nd > 0
ROW_SEED = 2027


def shuffled_rows(dstates, seed=ROW_SEED):
    """(cfg [M + 3], rows [M + 3, Nd] int32): the digits of all configurations in a seeded shuffle, the first three rows repeated
    at the end (a model with fewer than three configurations repeats what it has)"""
    M = int(np.prod(dstates)) if len(dstates) else 1
    cfg = np.random.RandomState(seed).permutation(M)
    cfg = np.concatenate([cfg, cfg[:3]])
    rows = np.stack(np.unravel_index(cfg, tuple(dstates)), axis=1) if len(dstates) else np.zeros((len(cfg), 0))
    return cfg, np.ascontiguousarray(rows, dtype=np.int32)


def cond_probs(model, x_d, x_c):
    """[sum dstates]: p(x_n = k | x_d,-n, x_c) of every discrete variable n, variable-major: the log tables of n's table
    factors, then the reduced tables of its strictly hybrid factors at x_c, with the other digits at x_d, and the softmax of
    disc_mrf_sampler.pyx, exp(v - (m + log(sum)))"""
    dstates = model['dstates']
    _, disc_f, hyb_f = gmod.split_factors(model['factors'])
    cond = [np.asarray(f.log_potential_fun.table) for f in disc_f] + gmod.reduced_tables(hyb_f, np.asarray(x_c, dtype=np.float64))
    scopes = [f.disc_nb_idx for f in disc_f] + [f.disc_nb_idx for f in hyb_f]
    out = []
    for n in range(len(dstates)):
        lprobs = np.zeros(dstates[n])
        for t, sc in zip(cond, scopes):
            if n in sc:
                lprobs = lprobs + t[tuple(slice(None) if i == n else x_d[i] for i in sc)]
        m = lprobs.max()
        out.append(np.exp(lprobs - (m + np.log(np.exp(lprobs - m).sum()))))
    return np.concatenate(out) if out else np.zeros(0)


def prob_sum(model, disc, cont):
    """one chain: disc [S, Nd], cont [S, Nc] -> the sum of cond_probs over the samples, in sample order"""
    total = np.zeros(int(np.sum(model['dstates'])))
    for x_d, x_c in zip(disc, cont):
        total += cond_probs(model, x_d, x_c)
    return total


def kept_samples(model):
    """(disc [CHAINS, kept, Nd] int32, cont [CHAINS, kept, Nc]) of the existing deterministic run (8 chains, 6 iterations, 3
    sweeps, burn-in 2, injected draws), through the sampler's host twin"""
    x0, z, u = gmod.draws(model)
    kept = gmod.ITERS - gmod.BURNIN
    runs = [gibbs.chain_host(model['gm'], x0[c], z[:, c], u[:, c], gmod.ITS, gmod.BURNIN, kept) for c in range(gmod.CHAINS)]
    return np.stack([r.disc for r in runs]), np.stack([r.cont for r in runs])


def nd1_model():
    """one ternary or binary discrete variable, three continuous (the model of the sampler's one-sweep test)"""
    model = em.rand_model(em.local_ns(), 1, 3, 7)
    return gmod.finish(model)


def build(name):
    return nd1_model() if name == 'nd1' else gmod.build(name)


def m0_model():
    """40 discrete variables, 1.6e15 configurations: past any enumeration (the tests also pass its struct with M = 0 and no
    dstride, the form of a model with more than 2^63 configurations)"""
    return gmod.finish(em.rand_model(em.local_ns(), 40, 8, 5))


def m0_rows(model, n=64, seed=ROW_SEED):
    rng = np.random.RandomState(seed)
    return np.stack([rng.randint(0, d, size=n) for d in model['dstates']], axis=1).astype(np.int32)
