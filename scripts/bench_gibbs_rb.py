"""Time of the Rao-Blackwellised marginals of the Gibbs baseline (rb_marginals(), rb_disc_marginals(); docs/kernels_gibbs_rb.md)
next to fit_marginals(3) on the same kept samples, and the quality of both against the exact marginals.
Writes profiles/gibbs_rb_bench.json.

Timing: the models and settings of scripts/bench_gibbs.py (rand_8_8, rand_12_16, rand_model(64, 32); 4096 chains, 40 outer
iterations of 10 discrete sweeps, the second 20 kept) with keep_samples=True.  Each call by device events on the launch stream,
2 warm-ups, 7 repeats, median and min / max (docs/measurement.md); every call includes its own plumbing (torch.unique for
rb_marginals, the download of the per-chain sums for rb_disc_marginals).  U, the number of distinct discrete states among the
kept samples = components of a Rao-Blackwellised mixture, is reported.  No ratio is asserted.

Quality: for rand_8_8 and ref_hybrid2 at the same settings, the mean over the continuous variables of KL(exact || rb) and of
KL(exact || fit_marginals(3)).

Usage: python scripts/bench_gibbs_rb.py [--out profiles/gibbs_rb_bench.json] [--chains 4096] [--iters 40]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'lifted-hybrid-variational-inference_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

ITS = 10
K = 3


def timed(call, repeats=7, warmup=2):
    import torch
    ms = []
    for i in range(warmup + repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        call()
        t1.record()
        t1.synchronize()
        if i >= warmup:
            ms.append(float(t0.elapsed_time(t1)))
    return {'ms_median': float(np.median(ms)), 'ms_min': min(ms), 'ms_max': max(ms)}


def sampler(model, chains, iters, seed=1):
    from lhvi import gibbs
    s = gibbs.GibbsHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc'])
    return s.run(chains=chains, num_burnin=iters // 2, num_samples=iters - iters // 2, disc_block_its=ITS, seed=seed, keep_samples=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gibbs_rb_bench.json'))
    ap.add_argument('--chains', type=int, default=4096)
    ap.add_argument('--iters', type=int, default=40)
    args = ap.parse_args()
    import exact_models as em
    from lhvi import exact
    out = {'chains': args.chains, 'iterations': args.iters, 'kept': args.iters - args.iters // 2, 'disc_block_its': ITS, 'K': K,
           'cases': [], 'quality': []}
    for name, model in (('rand_8_8', em.build('rand_8_8')), ('rand_12_16', em.build('rand_12_16')),
                        ('rand_64_32', em.rand_model(em.local_ns(), 64, 32, 1))):
        s = sampler(model, args.chains, args.iters)

        def disc():
            s._rb_prob = None           # rb_disc_marginals() keeps its result for the run: time the launch every repeat
            s.rb_disc_marginals()
        row = {'name': name, 'Nd': len(s.Vd), 'Nc': len(s.Vc), 'samples': s.chains * s.num_samples, 'lanes': s._run.lanes,
               'tables_in_lds': s._run.in_lds, 'rb_marginals': timed(s.rb_marginals), 'rb_disc_marginals': timed(disc),
               'fit_marginals_3': timed(lambda: s.fit_marginals(K)), 'U': int(s.rb.rows.shape[0])}
        out['cases'].append(row)
        print(json.dumps(row), flush=True)
    for name in ('rand_8_8', 'ref_hybrid2'):
        model = em.build(name)
        s = sampler(model, args.chains, args.iters)
        ex = exact.ExactHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc']).run()
        p = ex.marginals()
        kl_rb = p.kl(s.rb_marginals()).cpu().numpy()
        kl_fit = p.kl(s.fit_marginals(K)).cpu().numpy()
        row = {'name': name, 'M': int(ex.model.M), 'U': int(s.rb.rows.shape[0]), 'kl_exact_rb_mean': float(kl_rb.mean()),
               'kl_exact_fit3_mean': float(kl_fit.mean()), 'kl_exact_rb': kl_rb.tolist(), 'kl_exact_fit3': kl_fit.tolist()}
        out['quality'].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
