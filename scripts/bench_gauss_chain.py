"""Time of the block-tridiagonal Gaussian solver (lhvi/gauss_chain.py, csrc/gauss_chain.hip) on Kalman models
(A = 0.9 I + 0.3 randn / sqrt(n), q = 0.7, r = 0.4, 40 % missing observations), next to the dense ``ExactGaussian`` and 20 sweeps of
``GaBP`` on the same systems in the same process where the dense solver fits.  Writes profiles/gauss_chain_bench.json.

Cases (B, n, M): (1, 30, 19 999) the 12 M-factor chain of docs/widened_rows.md -- one workgroup, so this is what the missing
parallelism in time costs; (64, 30, 199) a batch of short chains; (5, 76, 19) the tree fixture's shape (the two-tile path).
Times: device events around ``lhvi_gauss_chain_solve`` alone (inputs, workspace and results already on the device), with and
without the covariances; 2 warm-up runs, 5 repeats, median and min / max.  The dense solver and GaBP take one system at a time
and their host set-up is long, so they are timed on the first ``--dense-systems`` systems of a case (default 1) and reported
per system.

With ``--segments`` the partitioned solve (``lhvi_gauss_chain_part_solve``) is timed next to the serial one in the same process, the
dense solver and GaBP are left out, and the result goes to profiles/gauss_chain_part_bench.json.  ``--segments sweep`` takes each
case's own list (the long chain: 64, 128, 256, 512), ``--segments 64,128`` that list for every case.  Per S: the solve with and
without the covariances, a serial solve of S - 1 blocks (the reduced chain's share), the distance from the serial moments, and
r = (t_part - t_reduced) / (ceil(M / S) t_serial / M): the cost of a block in stages 1 and 3 over a serial block
(``gauss_chain.SEGMENT_COST_RATIO``).

Usage: python scripts/bench_gauss_chain.py [--out profiles/gauss_chain_bench.json] [--cases 0,1,2] [--dense-systems 1]
                                           [--segments sweep|S,S,...]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'lifted-hybrid-variational-inference_amd'))

WARMUP, REPEATS = 2, 5
CASES = [dict(name='single long chain', B=1, n=30, M=19999, dense=False, segments=(64, 128, 256, 512)),
         dict(name='batch of short chains', B=64, n=30, M=199, dense=True, segments=(4, 12)),
         dict(name='tree fixture shape', B=5, n=76, M=19, dense=True, segments=(4, 10))]


def models(B, n, M, seed=0):
    from lhvi.graph import Domain
    from lhvi.kalman import MISSING, KalmanFilter
    rng = np.random.default_rng(seed)
    dom = Domain((-4, 4), continuous=True, integral_points=np.linspace(-4, 4, 30))
    data = rng.normal(size=(n, M + 1))
    data[:, 1:][rng.random((n, M)) < 0.4] = MISSING
    kfs = []
    for _ in range(B):
        A = 0.9 * np.eye(n) + 0.3 * rng.normal(size=(n, n)) / np.sqrt(n)
        kfs.append(KalmanFilter(dom, A, 0.7, np.diag(rng.uniform(0.5, 1.5, size=n)), 0.4))
    return kfs, data


def stats(v):
    return {'median': float(np.median(v)), 'min': float(min(v)), 'max': float(max(v))}


def timed(fn):
    """device-event milliseconds of fn() over the repeats"""
    import torch
    ms = []
    for i in range(WARMUP + REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= WARMUP:
            ms.append(a.elapsed_time(b))
    return stats(ms)


def chain_times(kfs, data, M, n, segments=()):
    import torch
    from lhvi import _abi
    B = len(kfs)
    parts = [kf.block_tridiagonal(M + 1, data) for kf in kfs]
    D, O, h = (_abi.to_dev(np.stack([p[i] for p in parts])) for i in range(3))
    l, new = _abi.lib(), lambda *s: torch.empty(*s, dtype=torch.float64, device='cuda')
    ws = new(int(l.lhvi_gauss_chain_ws_doubles(B, M, n)))
    mu, var, logdet, cov, cross = new(B, M, n), new(B, M, n), new(B), new(B, M, n, n), new(B, M - 1, n, n)
    bad = torch.empty(B, 2, dtype=torch.int32, device='cuda')

    def run(keep):
        _abi.check(l.lhvi_gauss_chain_solve(B, M, n, _abi.ptr(D), _abi.ptr(O), _abi.ptr(h), _abi.ptr(ws), _abi.ptr(mu), _abi.ptr(var),
                                            _abi.ptr(cov) if keep else None, _abi.ptr(cross) if keep else None, _abi.ptr(logdet),
                                            _abi.ptr(bad), _abi.stream_ptr()))
    out = {'solve_ms': timed(lambda: run(False)), 'solve_keep_cov_ms': timed(lambda: run(True)),
           'workspace_bytes': int(ws.numel()) * 8}
    assert int(bad.max().item()) == -1
    smu, svar = mu.cpu().numpy(), var.cpu().numpy()
    if segments:
        from lhvi import gauss_chain
        out['auto_segments'] = gauss_chain.auto_segments(B, M, n)
        out['partitioned'] = []
    for S in segments:
        pws = new(int(l.lhvi_gauss_chain_part_ws_doubles(B, M, n, S)))

        def part(keep):
            _abi.check(l.lhvi_gauss_chain_part_solve(B, M, n, S, _abi.ptr(D), _abi.ptr(O), _abi.ptr(h), _abi.ptr(pws), _abi.ptr(mu),
                                                     _abi.ptr(var), _abi.ptr(cov) if keep else None, _abi.ptr(cross) if keep else None,
                                                     _abi.ptr(logdet), _abi.ptr(bad), _abi.stream_ptr()))
        Se = int(gauss_chain.segment_bounds(M, S)[0])
        row = {'S': S, 'S_eff': Se, 'solve_ms': timed(lambda: part(False)), 'solve_keep_cov_ms': timed(lambda: part(True)),
               'workspace_bytes': int(pws.numel()) * 8}
        assert int(bad.max().item()) == -1
        row['vs_serial_max_dmu'] = float(np.abs(mu.cpu().numpy() - smu).max())
        row['vs_serial_max_rel_dvar'] = float(np.abs(var.cpu().numpy() / svar - 1).max())
        if Se > 1:                                     # the reduced chain's share: a serial solve of S_eff - 1 blocks, covariances kept
            R = Se - 1
            row['reduced_chain_ms'] = timed(lambda: _abi.check(l.lhvi_gauss_chain_solve(
                B, R, n, _abi.ptr(D), _abi.ptr(O), _abi.ptr(h), _abi.ptr(ws), _abi.ptr(mu), _abi.ptr(var), _abi.ptr(cov),
                _abi.ptr(cross), _abi.ptr(logdet), _abi.ptr(bad), _abi.stream_ptr())))
            per_block = out['solve_ms']['median'] / M
            row['r'] = (row['solve_ms']['median'] - row['reduced_chain_ms']['median']) / (-(-M // Se) * per_block)
        row['speedup'] = out['solve_ms']['median'] / row['solve_ms']['median']
        out['partitioned'].append(row)
        del pws
    return out, smu, svar


def dense_and_gabp(kf, data, M, mu, var):
    """one system through ExactGaussian and GaBP(20): their times and their distance from the chain solve's moments"""
    from lhvi.gabp import GaBP
    from lhvi.gauss_exact import ExactGaussian
    flat, state_id = kf.grounded_flat(M + 1, data)
    ex = ExactGaussian(flat)
    rows = []
    for i in range(WARMUP + REPEATS):
        t = {}
        ex.run(times=t)
        if i >= WARMUP:
            rows.append(sum(t.values()))
    em, ev = ex.mu_var
    bp = GaBP(flat)
    gabp = timed(lambda: bp.run(20))
    bp = GaBP(flat)                                   # a fresh run for the comparison: exactly 20 sweeps
    bp.run(20)
    mv = bp._state['mv'].cpu().numpy()[state_id[1:]]
    return {'dense_ms': stats(rows), 'gabp20_ms': gabp,
            'chain_vs_dense_max_dmu': float(np.abs(em[state_id[1:]] - mu).max()),
            'chain_vs_dense_max_rel_dvar': float(np.abs(ev[state_id[1:]] / var - 1).max()),
            'gabp20_vs_chain_max_dmu': float(np.abs(mv[..., 0] - mu).max()),
            'gabp20_vs_chain_max_rel_dvar': float(np.abs(mv[..., 1] / var - 1).max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--cases', default='0,1,2')
    ap.add_argument('--dense-systems', type=int, default=1)
    ap.add_argument('--segments', default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, 'profiles', 'gauss_chain_part_bench.json' if args.segments else 'gauss_chain_bench.json')
    import torch
    result = {'device': torch.cuda.get_device_name(0), 'warmup': WARMUP, 'repeats': REPEATS, 'cases': []}
    for c in (CASES[int(i)] for i in args.cases.split(',')):
        kfs, data = models(c['B'], c['n'], c['M'])
        row = {k: c[k] for k in ('name', 'B', 'n', 'M')}
        segments = () if not args.segments else c['segments'] if args.segments == 'sweep' else tuple(int(x) for x in args.segments.split(','))
        times, mu, var = chain_times(kfs, data, c['M'], c['n'], segments)
        row.update(times)
        if c['dense'] and not segments:
            row['per_system'] = [dense_and_gabp(kfs[b], data, c['M'], mu[b], var[b]) for b in range(min(args.dense_systems, c['B']))]
        print(json.dumps(row), flush=True)
        result['cases'].append(row)
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
