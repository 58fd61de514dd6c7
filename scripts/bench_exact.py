"""Configurations per second of the exact hybrid-Gaussian baseline (lhvi/exact.py) next to a batched NumPy restatement timed
in the same run, and as a fraction of the fp64 vector roof.  Writes profiles/exact_bench.json.

Sizes: (a) the reference's own 4-variable models (gibbs/test_hybrid2.py, osi/hybrid_mln_test_0.py); (b) 20 736 configurations,
Nc = 16 (rand_12_16 of tests/exact_models.py); (c) 2^20 binary configurations, Nc = 32, keep_cov = False.  For (b) also the
one-wavefront-per-configuration launch (lanes = 64) against the packed one.  Times: the enumeration kernel chain
(configurations, normalisation, marginals) by device events, 3 warm-up runs, 10 repeats, median and min / max; the flops
counted are Nc^3 / 3 (factorisation) + Nc^3 / 3 (inverse factor) + 3 Nc^2 (solves, inverse diagonal) per configuration.

Usage: python scripts/bench_exact.py [--out profiles/exact_bench.json] [--skip-large]
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

FP64_VECTOR_ROOF = 78.6e12       # MI355X fp64 vector peak, flop/s


def numpy_batched(model, rows):
    """the same enumeration in NumPy on `rows` configurations: assemble J and b per configuration (vectorised over the
    configurations, factor by factor), np.linalg.cholesky on the stack, triangular inverse, means, variances, log p~"""
    Nc, n = model.Nc, rows.size
    dig = (rows[:, None] // model.dstride[None, :]) % model.dstates[None, :] if model.Nd else np.zeros((n, 0), dtype=np.int64)
    A, b, c = np.zeros((n, Nc, Nc)), np.zeros((n, Nc)), np.zeros(n)
    for f in range(model.n_quad):
        rec = model.quad_desc[model.quad_ptr[f]:model.quad_ptr[f + 1]]
        nd, nc, off = int(rec[0]), int(rec[1]), int(rec[2])
        loc = np.zeros(n, dtype=np.int64)
        for a in range(nd):
            loc += dig[:, rec[3 + 2 * a]] * int(rec[4 + 2 * a])
        w = nc * nc + nc + 1
        P = model.quad_par[off + loc[:, None] * w + np.arange(w)[None, :]]
        sc = rec[3 + 2 * nd:]
        A[:, sc[:, None], sc[None, :]] += P[:, :nc * nc].reshape(n, nc, nc)
        b[:, sc] += P[:, nc * nc:nc * nc + nc]
        c += P[:, -1]
    t = np.zeros(n)
    for f in range(model.n_tab):
        rec = model.tab_desc[model.tab_ptr[f]:model.tab_ptr[f + 1]]
        loc = np.zeros(n, dtype=np.int64)
        for a in range(int(rec[0])):
            loc += dig[:, rec[2 + 2 * a]] * int(rec[3 + 2 * a])
        t += model.tab_par[int(rec[1]) + loc]
    J = -(A + np.swapaxes(A, 1, 2))
    L = np.linalg.cholesky(J)
    X = np.linalg.solve(L, np.broadcast_to(np.eye(Nc), J.shape))
    y = np.einsum('nij,nj->ni', X, b)
    mu = np.einsum('nji,nj->ni', X, y)
    var = (X * X).sum(axis=1)
    logdet = 2 * np.log(np.diagonal(L, axis1=1, axis2=2)).sum(axis=1)
    return t + c + Nc / 2 * np.log(2 * np.pi) - 0.5 * logdet + 0.5 * (mu * b).sum(axis=1), mu, var


def time_device(model, keep_cov, lanes, repeats=10, warmup=3):
    import torch
    from lhvi import exact
    ms = []
    for i in range(warmup + repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        r = exact._DeviceRun(model, keep_cov=keep_cov, lanes=lanes)
        t1.record()
        t1.synchronize()
        if i >= warmup:
            ms.append(float(t0.elapsed_time(t1)))
        del r
    return ms


def time_numpy(model, cap=1 << 16, repeats=3):
    rows = np.arange(min(model.M, cap), dtype=np.int64)
    best = []
    for _ in range(repeats):
        t = time.perf_counter()
        numpy_batched(model, rows)
        best.append(time.perf_counter() - t)
    return rows.size, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'exact_bench.json'))
    ap.add_argument('--skip-large', action='store_true')
    args = ap.parse_args()
    import exact_models as em
    from lhvi import exact
    from test_gpu_exact import big_model
    cases = []
    for name in ('ref_hybrid2', 'ref_mln0', 'rand_12_16'):
        _, s = em.solver(name)
        cases.append((name, s.model, True))
    if not args.skip_large:
        factors, Vd, Vc = big_model(20, 32)
        cases.append(('binary_20_32', exact.ExactHybridGaussian(factors=factors, Vd=Vd, Vc=Vc).model, False))
    out = {'fp64_vector_roof_flops': FP64_VECTOR_ROOF, 'threads_numpy': int(os.environ.get('OMP_NUM_THREADS', 0)) or None, 'cases': []}
    for name, model, keep_cov in cases:
        Nc, M = model.Nc, model.M
        flops = M * (2 * Nc ** 3 / 3 + 3 * Nc ** 2)
        n_np, t_np = time_numpy(model)
        row = {'name': name, 'configurations': M, 'Nc': Nc, 'keep_cov': keep_cov, 'flops_counted': flops,
               'numpy_configurations': n_np, 'numpy_s': t_np, 'numpy_cfg_per_s': n_np / min(t_np), 'launches': {}}
        for lanes in sorted({exact.default_lanes(Nc), 64}):
            ms = time_device(model, keep_cov, lanes)
            med = float(np.median(ms))
            row['launches']['lanes_%d' % lanes] = {
                'ms_median': med, 'ms_min': min(ms), 'ms_max': max(ms), 'cfg_per_s': M / (med * 1e-3),
                'fraction_of_fp64_vector_roof': flops / (med * 1e-3) / FP64_VECTOR_ROOF}
        cases_row = row['launches']['lanes_%d' % exact.default_lanes(Nc)]
        row['speedup_over_numpy'] = cases_row['cfg_per_s'] / row['numpy_cfg_per_s']
        out['cases'].append(row)
        print(json.dumps(row))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
