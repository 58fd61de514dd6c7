"""Time of the exact Gaussian solver (lhvi/gauss_exact.py: blocked dense fp64 Cholesky, X = L^-1, moments) next to the NumPy
``inv`` route of the reference and ``torch.linalg.cholesky`` timed in the same run, and as a fraction of the fp64 vector roof.
Writes profiles/gauss_exact_bench.json.

Sizes: N = 1 029 (the RGM with the evidence of tests/golden/gauss_exact_rgm4.npz, assembled from its factors) and synthetic
diagonally dominant N = 4 096 and 16 384 (dense A through get_gaussian_mean_params_from_quadratic_params' path).  Times: device
events around assembly (or packing), factorisation, and inverse + moments separately; 2 warm-up runs, 5 repeats, median and
min / max.  Flops counted: N^3 / 3 for the factor and N^3 / 3 for X.  The NumPy route (J = -2A, inv, Sig b) runs on the threads
the environment gives NumPy (OMP_NUM_THREADS, recorded in the output as threads_numpy).

Usage: python scripts/bench_gauss_exact.py [--out profiles/gauss_exact_bench.json] [--sizes 4096,16384] [--no-numpy-above N]
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
WARMUP, REPEATS = 2, 5


def synthetic(N, seed=0):
    """A = -J / 2 of a banded, strictly diagonally dominant J (cond(J) < 10) and a random b"""
    rng = np.random.default_rng(seed)
    J = np.zeros((N, N))
    idx = np.arange(N)
    for off in (1, 7, 64, 65):
        v = rng.uniform(-0.2, 0.2, size=N - off)
        J[idx[off:], idx[:-off]] = v
        J[idx[:-off], idx[off:]] = v
    J[idx, idx] = 2.0 + rng.uniform(0, 1, size=N)
    return -0.5 * J, rng.normal(size=N)


def summarise(rows):
    out = {}
    for k in rows[0]:
        v = [r[k] for r in rows]
        out[k] = {'median': float(np.median(v)), 'min': float(min(v)), 'max': float(max(v))}
    return out


def time_runs(run):
    import torch
    rows = []
    for i in range(WARMUP + REPEATS):
        t = {}
        run(t)
        torch.cuda.synchronize()
        if i >= WARMUP:
            rows.append(t)
    return summarise(rows)


def time_torch_cholesky(J):
    import torch
    try:
        ms = []
        for i in range(WARMUP + REPEATS):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            torch.linalg.cholesky(J)
            t1.record()
            t1.synchronize()
            if i >= WARMUP:
                ms.append(float(t0.elapsed_time(t1)))
        return {'median': float(np.median(ms)), 'min': min(ms), 'max': max(ms)}
    except Exception as exc:            # this torch build may lack the solver backend
        return {'unavailable': str(exc)[:200]}


def time_numpy(A, b, repeats=2):
    best = []
    for _ in range(repeats):
        t = time.perf_counter()
        Sig = np.linalg.inv(-2.0 * A)
        Sig @ b
        best.append(time.perf_counter() - t)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gauss_exact_bench.json'))
    ap.add_argument('--sizes', default='4096,16384')
    ap.add_argument('--no-numpy-above', type=int, default=1 << 30)
    args = ap.parse_args()
    import gauss_exact_models as gm
    from lhvi import _abi, gauss_exact
    torch = _abi.require_gpu()
    out = {'fp64_vector_roof_flops': FP64_VECTOR_ROOF, 'threads_numpy': int(os.environ.get('OMP_NUM_THREADS', 0)) or None,
           'warmup': WARMUP, 'repeats': REPEATS, 'cases': []}
    ex, _, _ = gm.rgm_solver(4)
    A4, b4, _ = ex.joint_quadratic()
    cases = [('rgm4', ex.N, lambda t: ex.run(times=t), A4, b4)]
    for N in [int(s) for s in args.sizes.split(',') if s]:
        A, b = synthetic(N)
        Ad, bd = _abi.to_dev(A), _abi.to_dev(b)
        cases.append(('synthetic_%d' % N, N, (lambda Ad, bd: lambda t: gauss_exact.mean_params_from_quadratic(Ad, bd, True, times=t))(Ad, bd), A, b))
    for name, N, run, A, b in cases:
        ms = time_runs(run)
        flops = N ** 3 / 3
        row = {'name': name, 'N': N, 'flops_factor': flops, 'flops_inverse': flops, 'device_ms': ms,
               'factor_fraction_of_fp64_vector_roof': flops / (ms['factor_ms']['median'] * 1e-3) / FP64_VECTOR_ROOF,
               'inverse_fraction_of_fp64_vector_roof': flops / (ms['inverse_moments_ms']['median'] * 1e-3) / FP64_VECTOR_ROOF}
        Jd = _abi.to_dev(-2.0 * A)
        row['torch_linalg_cholesky_ms'] = time_torch_cholesky(Jd)
        del Jd
        if N <= args.no_numpy_above:
            row['numpy_inv_s'] = time_numpy(A, b, repeats=2 if N <= 8192 else 1)
        out['cases'].append(row)
        print(json.dumps(row))
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
