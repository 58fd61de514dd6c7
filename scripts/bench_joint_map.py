"""Time of the exact joint MAP (``ExactHybridGaussian.config_energies`` + the first-index arg-max, lhvi/hg_energy.py) next to the
same run's ``run()`` (the enumeration, whose code this measurement does not touch) and to the NumPy restatement timed in the
same run.  Writes profiles/joint_map_bench.json.

Sizes: rand_12_16 of tests/exact_models.py (M = 20 736, Nc = 16) and reduction_model at M = 531 441 (Nc = 1; three launches of
the 2^18 chunk).  Times by device events, 3 warm-up runs, 10 repeats, median and min / max.  The energy kernel's algorithmic
bytes are the 8 M Nc of the means it reads plus the 8 M it writes (the model's parameters stay in cache), priced against the
8 TB/s HBM roof as docs/measurement.md does.

Usage: python scripts/bench_joint_map.py [--out profiles/joint_map_bench.json]
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

HBM_ROOF = 8e12                 # MI355X, bytes/s


def events(fn, repeats=10, warmup=3):
    import torch
    ms = []
    for i in range(warmup + repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        if i >= warmup:
            ms.append(float(t0.elapsed_time(t1)))
    return {'ms_median': float(np.median(ms)), 'ms_min': min(ms), 'ms_max': max(ms)}


def numpy_joint_map(model, means):
    """the restatement in float64, vectorised over the configurations on the flat model: energies, then np.argmax"""
    M, dig = model.M, None
    rows = np.arange(M, dtype=np.int64)
    dig = (rows[:, None] // model.dstride[None, :]) % model.dstates[None, :] if model.Nd else np.zeros((M, 0), dtype=np.int64)
    e = np.zeros(M)
    for f in range(model.n_quad):
        rec = model.quad_desc[model.quad_ptr[f]:model.quad_ptr[f + 1]]
        nd, nc, off = int(rec[0]), int(rec[1]), int(rec[2])
        loc = np.zeros(M, dtype=np.int64)
        for a in range(nd):
            loc += dig[:, rec[3 + 2 * a]] * int(rec[4 + 2 * a])
        w = nc * nc + nc + 1
        P = model.quad_par[off + loc[:, None] * w + np.arange(w)[None, :]]
        x = means[:, rec[3 + 2 * nd:]]
        e += np.einsum('nij,ni,nj->n', P[:, :nc * nc].reshape(M, nc, nc), x, x) + (P[:, nc * nc:nc * nc + nc] * x).sum(axis=1) + P[:, -1]
    for f in range(model.n_tab):
        rec = model.tab_desc[model.tab_ptr[f]:model.tab_ptr[f + 1]]
        loc = np.zeros(M, dtype=np.int64)
        for a in range(int(rec[0])):
            loc += dig[:, rec[2 + 2 * a]] * int(rec[3 + 2 * a])
        e += model.tab_par[int(rec[1]) + loc]
    return int(np.argmax(e)), e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'joint_map_bench.json'))
    args = ap.parse_args()
    import torch
    import exact_models as em
    from lhvi import exact, hg_energy
    cases = [('rand_12_16', em.solver('rand_12_16')[1])]
    model = em.reduction_model(em.local_ns(), [3] * 12)
    cases.append(('reduction_3^12', exact.ExactHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc'])))
    out = {'hbm_roof_bytes_per_s': HBM_ROOF, 'threads_numpy': int(os.environ.get('OMP_NUM_THREADS', 0)) or None, 'cases': []}
    for name, s in cases:
        M, Nc = s.model.M, s.model.Nc
        run = events(lambda: exact._DeviceRun(s.model, keep_cov=False))
        r = exact._DeviceRun(s.model, keep_cov=False)

        def joint_map():
            r._energies = None
            return hg_energy.argmax_first(r.config_energies())

        def energies_only():
            r._energies = None
            r.config_energies()
        jm, en = events(joint_map), events(energies_only)
        index = int(joint_map()[0].item())
        means = r.means.cpu().numpy()
        t_np = []
        for _ in range(3):
            t = time.perf_counter()
            np_index, np_e = numpy_joint_map(s.model, means)
            t_np.append(time.perf_counter() - t)
        dev_e = r.config_energies().cpu().numpy()
        bytes_alg = 8 * M * Nc + 8 * M
        row = {'name': name, 'configurations': M, 'Nc': Nc, 'launches_of_the_energy_kernel': -(-M // exact.CHUNK),
               'run': run, 'config_energies_plus_argmax': jm, 'config_energies': en,
               'joint_map_fraction_of_run': jm['ms_median'] / run['ms_median'],
               'energy_algorithmic_bytes': bytes_alg,
               'energy_fraction_of_hbm_roof': bytes_alg / (en['ms_median'] * 1e-3) / HBM_ROOF,
               'numpy_s': t_np, 'speedup_over_numpy': min(t_np) / (jm['ms_median'] * 1e-3),
               'index': index, 'numpy_index': np_index, 'max_abs_difference_to_numpy': float(np.abs(dev_e - np_e).max())}
        out['cases'].append(row)
        print(json.dumps(row))
        del r
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
