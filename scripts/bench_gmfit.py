"""Time of ``GibbsHybridGaussian.fit_marginals(K=3)`` (lhvi/gmfit.py, csrc/gmfit.hip) on the kept samples of 4096 chains x 100
samples at Nc = 8 and Nc = 64, next to the path it replaces on the same samples: the device-to-host copy of the samples plus
Nc calls of ``gibbs.fit_scalar_gm_from_samples`` (scikit-learn).  Writes profiles/gmfit_bench.json.

Models: rand_8_8 of tests/exact_models.py and rand_model(8, 64) (Nd = 8, Nc = 64).  Device times are device events around the
call (the transposed copy, the launch, the read-back of the flags), 2 warm-up calls, 7 repeats, median and min / max; the
launch alone is timed the same way on the already transposed samples, and the sampler's own run once for scale.  The
scikit-learn path is a host clock around the copy and the fits, once.  The library under test is the one ``LHVI_LIB`` names
(default: csrc/liblhvi.so); ``--label`` goes into the output, which is how a build with another LHVI_GMFIT_BLOCK is told
apart.

``--launch-ks 2,5,16`` also times the launch alone at those K with a fixed number of iterations (``tol=0, max_iter=10``: the same
work for every build), which is what the choice of the workgroup size was measured on beyond K = 3.

Usage: python scripts/bench_gmfit.py [--out profiles/gmfit_bench.json] [--label block256] [--skip-sklearn] [--chains 4096]
                                     [--launch-ks 2,5,16]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'lifted-hybrid-variational-inference_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

K = 3


def timed(fn, repeats=7, warmup=2):
    import torch
    ms = []
    for i in range(warmup + repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        t1.synchronize()
        if i >= warmup:
            ms.append(float(t0.elapsed_time(t1)))
    return {'ms_median': float(np.median(ms)), 'ms_min': min(ms), 'ms_max': max(ms)}, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gmfit_bench.json'))
    ap.add_argument('--label', default='block256')
    ap.add_argument('--chains', type=int, default=4096)
    ap.add_argument('--samples', type=int, default=100)
    ap.add_argument('--skip-sklearn', action='store_true')
    ap.add_argument('--launch-ks', default='')
    args = ap.parse_args()
    import exact_models as em
    from lhvi import _abi, gibbs, gmfit
    out = {'label': args.label, 'library': _abi.LIB_PATH, 'chains': args.chains, 'num_samples': args.samples, 'K': K, 'cases': []}
    for name, model in (('rand_8_8', em.build('rand_8_8')), ('rand_8_64', em.rand_model(em.local_ns(), 8, 64, 1))):
        s = gibbs.GibbsHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc'])
        run = dict(chains=args.chains, num_burnin=20, num_samples=args.samples, disc_block_its=10, seed=7, keep_samples=True)
        t_run, _ = timed(lambda: s.run(**run), repeats=1, warmup=1)
        Nc, n = len(s.Vc), args.chains * args.samples
        t_fit, fit = timed(lambda: s.fit_marginals(K))
        x = s._run.cont.reshape(n, Nc).t().contiguous()
        t_launch, direct = timed(lambda: gmfit.fit_scalar_gms(x, K))
        n_iter = fit.n_iter.cpu().numpy()
        row = {'name': name, 'Nc': Nc, 'samples_per_variable': n, 'sampler_run_ms': t_run['ms_median'], 'fit_marginals': t_fit,
               'fit_scalar_gms_on_transposed_samples': t_launch, 'n_iter': n_iter.tolist(),
               'converged': int(fit.converged.sum().item()), 'lower_bound_mean': float(fit.lower_bound.mean().item())}
        for k in [int(v) for v in args.launch_ks.split(',') if v]:
            row.setdefault('launch_10_iterations_ms', {})['K%d' % k] = timed(
                lambda: gmfit.fit_scalar_gms(x, k, tol=0.0, max_iter=10), repeats=5, warmup=1)[0]
        if not args.skip_sklearn:
            t = time.perf_counter()
            host = s._run.cont.cpu().numpy().reshape(n, Nc)
            t_copy = time.perf_counter() - t
            fits = [gibbs.fit_scalar_gm_from_samples(host[:, i], K) for i in range(Nc)]
            t_all = time.perf_counter() - t
            lbs = [float(np.mean(gmfit.ScalarMixtures(w[None], mu[None], var[None], host=True).log_pdf(host[::64, i])))
                   for i, (w, mu, var) in enumerate(fits)]
            row['device_fit_mean_log_density_on_every_64th_sample'] = float(np.mean(
                [np.mean(gmfit.ScalarMixtures(*(a[None] for a in direct.params(i)), host=True).log_pdf(host[::64, i]))
                 for i in range(Nc)]))
            row['replaced_path'] = {'copy_ms': 1e3 * t_copy, 'copy_and_sklearn_fits_ms': 1e3 * t_all,
                                    'mean_log_density_on_every_64th_sample': float(np.mean(lbs))}
            row['fit_marginals_speedup_over_replaced_path'] = 1e3 * t_all / t_fit['ms_median']
        out['cases'].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
