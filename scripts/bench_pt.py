"""Ladder-iterations per second of the tempered block Gibbs sampler (lhvi/pt.py) per (replicas, lanes), next to the host twin
(lhvi_pt_ladder_host: the same per-ladder code on one CPU thread) timed in the same run, and next to the plain sampler
(lhvi_gibbs_run) at ladders * replicas chains of the same model, sweeps and iterations.  Writes profiles/pt_bench.json.

Models: two_wells of tests/pt_models.py, rand_8_8 and rand_12_16 of tests/exact_models.py.  1024 ladders, 64 iterations (none
kept apart from the accumulators), one discrete sweep an iteration, swaps every iteration, the linear ladder, the default base.
Times: the launches of one run by device events, 2 warm-up runs, 7 repeats, median and min / max.  The ratio
``chain_iterations_vs_gibbs`` is (ladders * replicas * iterations / s of the tempered run) / (chain-iterations / s of the plain
run): a replica factors three times an iteration where a plain chain factors once.

Usage: python scripts/bench_pt.py [--out profiles/pt_bench.json] [--ladders 1024] [--iters 64]
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

ITS = 1
HOST_LADDERS = 8
REPLICAS = (2, 4, 8)
LANES = (1, 2, 4, 8, 16, 32)


def time_host(gm, R, iters):
    """seconds of HOST_LADDERS ladders of the host twin drawing from the Philox stream, 3 runs"""
    from lhvi import pt
    betas = pt.schedule(R)
    x0 = np.zeros((R, gm.ex.Nd), dtype=np.int32)
    out = []
    for _ in range(3):
        t = time.perf_counter()
        for l in range(HOST_LADDERS):
            pt.ladder_host(gm, x0, betas, 1.0, None, ITS, 0, iters, 1, seed=1, ladder=l)
        out.append(time.perf_counter() - t)
    return out


def timed(make, repeats=7, warmup=2):
    import torch
    ms = []
    for i in range(warmup + repeats):
        r = make(1 + i)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        r.run()
        t1.record()
        t1.synchronize()
        if i >= warmup:
            ms.append(float(t0.elapsed_time(t1)))
    return ms, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pt_bench.json'))
    ap.add_argument('--ladders', type=int, default=1024)
    ap.add_argument('--iters', type=int, default=64)
    args = ap.parse_args()
    import pt_models as pm
    from lhvi import _abi, gibbs, pt
    out = {'ladders': args.ladders, 'iters': args.iters, 'disc_block_its': ITS, 'swap_every': 1, 'host_ladders': HOST_LADDERS, 'cases': []}
    for name in ('two_wells', 'rand_8_8', 'rand_12_16'):
        gm = pm.build(name)['gm']
        Nc, Nd = gm.ex.Nc, gm.ex.Nd
        for R in REPLICAS:
            betas = pt.schedule(R)
            t_host = time_host(gm, R, args.iters)
            ms, g = timed(lambda seed: gibbs._Chains(gm, args.ladders * R, 0, args.iters, ITS, seed))
            gibbs_rate = args.ladders * R * args.iters / (float(np.median(ms)) * 1e-3)
            row = {'name': name, 'Nd': Nd, 'Nc': Nc, 'replicas': R, 'host_s': t_host,
                   'host_ladder_iterations_per_s': HOST_LADDERS * args.iters / min(t_host),
                   'gibbs': {'chains': args.ladders * R, 'lanes': g.lanes, 'ms_median': float(np.median(ms)), 'ms_min': min(ms),
                             'ms_max': max(ms), 'chain_iterations_per_s': gibbs_rate},
                   'launches': {}}
            for lanes in LANES:
                lds = int(_abi.lib().lhvi_pt_lds_bytes(Nc, Nd, gm.max_states, R, lanes))
                if lds == 0 or lds > gibbs.LDS_LIMIT:
                    row['launches']['lanes_%d' % lanes] = {'skipped': 'a workgroup needs %d bytes of LDS or more than 256 threads' % lds}
                    continue
                ms, r = timed(lambda seed: pt._Ladders(gm, args.ladders, betas, 1.0, np.zeros(Nc), 0, args.iters, ITS, 1, seed, lanes=lanes))
                med = float(np.median(ms))
                rate = args.ladders * args.iters / (med * 1e-3)
                row['launches']['lanes_%d' % lanes] = {'ms_median': med, 'ms_min': min(ms), 'ms_max': max(ms), 'tables_in_lds': r.in_lds,
                                                       'ladder_iterations_per_s': rate,
                                                       'chain_iterations_vs_gibbs': rate * R / gibbs_rate}
            done = {k: v for k, v in row['launches'].items() if 'ms_median' in v}
            row['best_lanes'] = min(done, key=lambda k: done[k]['ms_median'])
            row['speedup_over_host_thread_at_best'] = done[row['best_lanes']]['ladder_iterations_per_s'] / row['host_ladder_iterations_per_s']
            out['cases'].append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
