"""Conditional queries on a mixture belief (lhvi/mixture.py): the three entry points on held-out evidence rows against every
query variable and the joint MAP, next to the NumPy restatements of the reference's functions (tests/mixture_models.py) timed in the same run on
16 threads over slices of the evidence rows.  Writes profiles/mixture_bench.json.

Belief: K components over 600 continuous rows and 400 discrete rows of 2 .. 5 states.  Evidence: M = 4096 rows over N_o = 800
observed variables, a fifth of the entries NaN; N_q = 200 query variables (half continuous); P = 30 points per query.
Times: the launches of one call by device events, 2 warm-up calls, 7 repeats, median and min / max.

lhvi_mix_condition is reported in algorithmic bytes, 24 K N_o per group of LHVI_MIX_ROWS evidence rows (the records) plus
8 N_o per row (the evidence), as a fraction of the 8 TB/s HBM roof of docs/measurement.md.

Usage: python scripts/bench_mixture.py [--out profiles/mixture_bench.json] [--rows 4096] [--K 8 32]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'lifted-hybrid-variational-inference_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

THREADS = 16
HBM_ROOF = 8e12
NC, ND, N_O, N_Q, P = 600, 400, 800, 200, 30


def make_case(K, M, seed=0):
    rng = np.random.RandomState(seed)
    w = rng.dirichlet(2 * np.ones(K))
    Mu, Var = rng.uniform(-3, 3, (NC, K)), 10 ** rng.uniform(-0.5, 1, (NC, K))
    Pi = [rng.dirichlet(2 * np.ones(s), K) for s in rng.randint(2, 6, ND)]
    obs = rng.permutation(np.concatenate([rng.choice(NC, 500, replace=False), NC + rng.choice(ND, 300, replace=False)]))
    X = np.empty((M, N_O))
    for j, v in enumerate(obs):
        X[:, j] = rng.uniform(-3, 3, M) if v < NC else rng.randint(0, Pi[v - NC].shape[1], M)
    X[rng.rand(M, N_O) < 0.2] = np.nan
    rest = np.setdiff1d(np.arange(NC + ND), obs)
    query = np.concatenate([rest[rest < NC][:N_Q // 2], rest[rest >= NC][:N_Q // 2]])
    assert obs.size == N_O and query.size == N_Q
    return dict(w=w, Mu=Mu, Var=Var, Pi=Pi, bds=np.array([[-10.] * NC, [10.] * NC]), obs=obs, X=X, query=query)


def timed(fn, repeats=7, warmup=2):
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


def time_numpy(case, rows, repeats=2):
    """the restated calc_cond_mixture_weights / calc_marg_log_prob on `rows` evidence rows, 16 threads over slices of them"""
    import mixture_models as mm
    per = (rows + THREADS - 1) // THREADS
    parts = [case['X'][i:i + per] for i in range(0, rows, per)]
    out = []
    with ThreadPoolExecutor(THREADS) as pool:
        for _ in range(repeats):
            t = time.perf_counter()
            list(pool.map(lambda x: mm.restate_condition(case, X=x), parts))
            out.append(time.perf_counter() - t)
    return out


def time_scipy_modes(case, condw, pairs=64):
    """get_scalar_gm_mode restated with SciPy's bounded minimize, per (evidence row, continuous query) pair"""
    import mixture_models as mm
    cont = [v for v in case['query'] if v < NC]
    t = time.perf_counter()
    for i in range(pairs):
        v = cont[i % len(cont)]
        mm.scalar_gm_mode(condw[i % len(condw)], case['Mu'][v], case['Var'][v], case['bds'][:, v])
    return (time.perf_counter() - t) / pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mixture_bench.json'))
    ap.add_argument('--rows', type=int, default=4096)
    ap.add_argument('--K', type=int, nargs='+', default=[8, 32])
    ap.add_argument('--numpy-rows', type=int, default=512)
    args = ap.parse_args()
    import mixture_models as mm
    from lhvi import _abi
    from lhvi.mixture import _p, default_lanes
    _abi.require_gpu()
    l, M = _abi.lib(), args.rows
    out = {'rows': M, 'n_obs': N_O, 'n_query': N_Q, 'points': P, 'threads_numpy': THREADS, 'cases': []}
    for K in args.K:
        case = make_case(K, M)
        belief = mm.belief_of(case)
        side = belief._side(False)
        X, obs, query = side.put(case['X']), side.put(case['obs'], np.int32), side.put(case['query'], np.int32)
        ws = side.empty((int(l.lhvi_mix_condition_ws_doubles(M, N_O, K)),))
        comp, logp, condw = side.empty((M, K)), side.empty((M,)), side.empty((M, K))
        lo, hi = side.lo[query.long()].contiguous(), side.hi[query.long()].contiguous()
        xq, fq = side.empty((M, N_Q)), side.empty((M, N_Q))
        pts = np.tile(np.linspace(-3, 3, P), (N_Q, 1))
        pts[N_Q // 2:] = np.arange(P) % 2
        pts, lb = side.put(pts), side.empty((M, N_Q, P))
        st = _abi.stream_ptr()

        def condition():
            _abi.check(l.lhvi_mix_condition(side.struct, M, N_O, _p(obs), _p(X), _p(ws), _p(comp), _p(logp), _p(condw), st))

        def marginal_map(lanes):
            _abi.check(l.lhvi_mix_marginal_map(side.struct, M, _p(condw), N_Q, _p(query), _p(lo), _p(hi), 0, None, None, None,
                                               lanes, 100, _p(xq), _p(fq), st))

        def log_belief():
            _abi.check(l.lhvi_mix_log_belief(side.struct, M, _p(condw), N_Q, _p(query), P, _p(pts), _p(lb), st))
        row = {'K': K, 'condition': timed(condition)}
        groups = (M + _abi.MIX_ROWS - 1) // _abi.MIX_ROWS
        nbytes = groups * 24 * K * N_O + M * 8 * N_O
        row['condition']['algorithmic_bytes'] = nbytes
        row['condition']['fraction_of_hbm_roof'] = nbytes / (row['condition']['ms_median'] * 1e-3) / HBM_ROOF
        row['condition']['rows_per_s'] = M / (row['condition']['ms_median'] * 1e-3)
        t_np = time_numpy(case, args.numpy_rows)
        row['numpy_condition'] = {'rows': args.numpy_rows, 's': t_np, 'rows_per_s': args.numpy_rows / min(t_np)}
        row['condition']['speedup_over_numpy'] = row['condition']['rows_per_s'] / row['numpy_condition']['rows_per_s']
        row['marginal_map'] = {}
        for lanes in sorted({1, default_lanes(K), 64}):
            t = timed(lambda: marginal_map(lanes))
            t['pairs_per_s'] = M * N_Q / (t['ms_median'] * 1e-3)
            row['marginal_map']['lanes_%d' % lanes] = t
        row['default_lanes'] = default_lanes(K)
        per_pair = time_scipy_modes(case, condw[:64].cpu().numpy())
        row['scipy_mode'] = {'s_per_continuous_pair': per_pair, 'pairs_per_s_one_thread': 1 / per_pair}
        row['log_belief'] = timed(log_belief)
        row['log_belief']['points_per_s'] = M * N_Q * P / (row['log_belief']['ms_median'] * 1e-3)
        out['cases'].append(row)
        print(json.dumps(row), flush=True)
    # joint MAP: the kernel (one workgroup per start, host clock around a call that ends in the copy of its results) against the
    # NumPy restatement of joint_map_from_belief_params on one thread (the reference is one process)
    import torch
    out['joint_map'] = []
    for shape in ((40, 33, 5, 2), (130, 70, 2, 4)):
        case = mm.joint_case(shape)
        belief = mm.belief_of(case)
        belief.joint_map()
        ts = []
        for _ in range(5):
            torch.cuda.synchronize()
            t = time.perf_counter()
            belief.joint_map()
            ts.append(time.perf_counter() - t)
        t = time.perf_counter()
        with np.errstate(all='ignore'):
            mm.restate_joint_map(case)
        row = {'shape': shape, 'device_s_median': float(np.median(ts)), 'device_s_min': min(ts), 'device_s_max': max(ts),
               'numpy_s': time.perf_counter() - t}
        out['joint_map'].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
