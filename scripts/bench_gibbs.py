"""Chain-iterations per second of the block Gibbs sampler (lhvi/gibbs.py) for every `lanes` value, next to a NumPy restatement
of the same chains (vectorised over chains, 16 threads over slices of them) timed in the same run.
Writes profiles/gibbs_bench.json.

Models: rand_8_8 and rand_12_16 of tests/exact_models.py, and rand_model(64, 32) (Nd = 64, Nc = 32; enumeration impossible).
4096 chains, 40 outer iterations of 10 discrete sweeps, accumulators only.  Times: the launches of one run by device events,
2 warm-up runs, 7 repeats, median and min / max.

Usage: python scripts/bench_gibbs.py [--out profiles/gibbs_bench.json] [--chains 4096] [--iters 40]
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

ITS = 10
THREADS = 16


def _local(rec, nd, x, skip=None):
    """local index of a descriptor's discrete scope at the states x [n, Nd], variable `skip` left out; its stride"""
    loc, stride = np.zeros(x.shape[0], dtype=np.int64), 0
    for a in range(nd):
        v, s = int(rec[2 * a]), int(rec[2 * a + 1])
        if v == skip:
            stride = s
        else:
            loc += x[:, v] * s
    return loc, stride


def numpy_chains(gm, chains, iters, its, seed):
    """`chains` chains of the sampler in NumPy, every step vectorised over the chains: batched Cholesky and triangular solves,
    the reduced tables by einsum, the sweep variable by variable.  Returns the state counts and sum x_c."""
    ex = gm.ex
    Nd, Nc, n = ex.Nd, ex.Nc, chains
    rng = np.random.RandomState(seed)
    x = np.stack([rng.randint(0, d, size=n) for d in ex.dstates], axis=1) if Nd else np.zeros((n, 0), dtype=np.int64)
    quads = []
    for f in range(ex.n_quad):
        rec = ex.quad_desc[ex.quad_ptr[f]:ex.quad_ptr[f + 1]]
        nd, nc, off = int(rec[0]), int(rec[1]), int(rec[2])
        quads.append((rec[3:3 + 2 * nd], nd, nc, off, rec[3 + 2 * nd:]))
    tabs = []
    for f in range(ex.n_tab):
        rec = ex.tab_desc[ex.tab_ptr[f]:ex.tab_ptr[f + 1]]
        tabs.append((rec[2:], int(rec[0]), int(rec[1])))
    counts, sum1 = np.zeros((n, gm.n_states)), np.zeros((n, Nc))
    rows = np.arange(n)
    for _ in range(iters):
        A, b = np.zeros((n, Nc, Nc)), np.zeros((n, Nc))
        for scope, nd, nc, off, sc in quads:
            w = nc * nc + nc + 1
            P = ex.quad_par[off + _local(scope, nd, x)[0][:, None] * w + np.arange(w)[None, :]]
            A[:, sc[:, None], sc[None, :]] += P[:, :nc * nc].reshape(n, nc, nc)
            b[:, sc] += P[:, nc * nc:nc * nc + nc]
        L = np.linalg.cholesky(-(A + np.swapaxes(A, 1, 2)))
        y = np.linalg.solve(L, b[:, :, None])[:, :, 0]
        xc = np.linalg.solve(np.swapaxes(L, 1, 2), (y + rng.randn(n, Nc))[:, :, None])[:, :, 0]
        red = []
        for h in range(gm.n_hyb):
            scope, nd, nc, off, sc = quads[gm.hyb_quad[h]]
            w, K = nc * nc + nc + 1, int(gm.hyb_off[h + 1] - gm.hyb_off[h])
            P = ex.quad_par[off:off + K * w].reshape(K, w)
            xs = xc[:, sc]
            red.append(np.einsum('kab,na,nb->nk', P[:, :nc * nc].reshape(K, nc, nc), xs, xs) + xs @ P[:, nc * nc:nc * nc + nc].T
                       + P[:, -1][None, :])
        for _s in range(its):
            for v in range(Nd):
                d = int(ex.dstates[v])
                lp = np.zeros((n, d))
                for e in range(gm.vt_ptr[v], gm.vt_ptr[v + 1]):
                    scope, nd, off = tabs[gm.vt_fac[e]]
                    loc, st = _local(scope, nd, x, v)
                    lp += ex.tab_par[off + loc[:, None] + np.arange(d)[None, :] * st]
                for e in range(gm.vh_ptr[v], gm.vh_ptr[v + 1]):
                    h = gm.vh_fac[e]
                    loc, st = _local(quads[gm.hyb_quad[h]][0], quads[gm.hyb_quad[h]][1], x, v)
                    lp += red[h][rows[:, None], loc[:, None] + np.arange(d)[None, :] * st]
                m = lp.max(axis=1, keepdims=True)
                cum = np.cumsum(np.exp(lp - (m + np.log(np.exp(lp - m).sum(axis=1, keepdims=True)))), axis=1)
                x[:, v] = np.minimum((rng.rand(n, 1) > cum).sum(axis=1), d - 1)
        for v in range(Nd):
            counts[rows, gm.dstate_off[v] + x[:, v]] += 1
        sum1 += xc
    return counts, sum1


def time_numpy(gm, chains, iters, repeats=2):
    per = (chains + THREADS - 1) // THREADS
    sizes = [min(per, chains - i) for i in range(0, chains, per)]
    best = []
    with ThreadPoolExecutor(THREADS) as pool:
        for _ in range(repeats):
            t = time.perf_counter()
            list(pool.map(lambda a: numpy_chains(gm, a[1], iters, ITS, a[0]), enumerate(sizes)))
            best.append(time.perf_counter() - t)
    return best


def time_device(gm, chains, iters, lanes, repeats=7, warmup=2):
    import torch
    from lhvi import gibbs
    ms = []
    for i in range(warmup + repeats):
        r = gibbs._Chains(gm, chains, iters // 2, iters - iters // 2, ITS, 1 + i, lanes=lanes)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        r.run()
        t1.record()
        t1.synchronize()
        if i >= warmup:
            ms.append(float(t0.elapsed_time(t1)))
    return ms, r.in_lds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gibbs_bench.json'))
    ap.add_argument('--chains', type=int, default=4096)
    ap.add_argument('--iters', type=int, default=40)
    ap.add_argument('--numpy-iters', type=int, default=4)
    args = ap.parse_args()
    import exact_models as em
    from lhvi import _abi, exact, gibbs
    cases = []
    for name, model in (('rand_8_8', em.build('rand_8_8')), ('rand_12_16', em.build('rand_12_16')),
                        ('rand_64_32', em.rand_model(em.local_ns(), 64, 32, 1))):
        em.set_indices(model)
        cases.append((name, gibbs.GibbsModel(exact.flatten_factors(model['factors'], [rv.dstates for rv in model['Vd']],
                                                                   len(model['Vc'])))))
    out = {'chains': args.chains, 'iterations': args.iters, 'disc_block_its': ITS, 'threads_numpy': THREADS, 'cases': []}
    for name, gm in cases:
        work = args.chains * args.iters
        t_np = time_numpy(gm, args.chains, args.numpy_iters)
        row = {'name': name, 'Nd': gm.ex.Nd, 'Nc': gm.ex.Nc, 'table_doubles': gm.table_doubles, 'numpy_iterations': args.numpy_iters,
               'numpy_s': t_np, 'numpy_chain_its_per_s': args.chains * args.numpy_iters / min(t_np),
               'default_lanes': gibbs.default_lanes(gm.ex.Nc), 'launches': {}}
        for lanes in (1, 2, 4, 8, 16, 32, 64):
            lds = int(_abi.lib().lhvi_gibbs_lds_bytes(gm.ex.Nc, gm.ex.Nd, gm.max_states, lanes))
            if lds > gibbs.LDS_LIMIT:
                row['launches']['lanes_%d' % lanes] = {'skipped': 'a workgroup needs %d bytes of LDS' % lds}
                continue
            ms, in_lds = time_device(gm, args.chains, args.iters, lanes)
            med = float(np.median(ms))
            row['launches']['lanes_%d' % lanes] = {'ms_median': med, 'ms_min': min(ms), 'ms_max': max(ms), 'tables_in_lds': in_lds,
                                                   'chain_its_per_s': work / (med * 1e-3)}
        timed = {k: v for k, v in row['launches'].items() if 'ms_median' in v}
        row['best_lanes'] = min(timed, key=lambda k: timed[k]['ms_median'])
        row['speedup_over_numpy_at_best'] = timed[row['best_lanes']]['chain_its_per_s'] / row['numpy_chain_its_per_s']
        out['cases'].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
