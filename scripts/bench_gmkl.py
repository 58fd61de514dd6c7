"""Times of ``lhvi.gmkl.kl_scalar_mixtures`` on the device at two shapes -- R = 2 000 rows of (Kp, Kq) = (4 096, 3), the exact
baseline against a K = 3 solver, and R = 100 000 rows of (3, 3) -- and of the reference's host route
(``utils.kl_continuous_logpdf`` with ``points``) on a subsample of the rows over 16 worker processes, scaled linearly.

    python3 scripts/bench_gmkl.py [out.json]          # docs/kernels_gmkl.md, profiles/gmkl_bench.json
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'lifted-hybrid-variational-inference_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import numpy as np


def make(R, Kp, Kq, seed):
    rng = np.random.default_rng(seed)
    def side(K, vlo, vhi):
        w = rng.gamma(2.0, size=(R, K))
        w /= w.sum(axis=1, keepdims=True)
        return w, rng.uniform(-10, 10, (R, K)), np.exp(rng.uniform(np.log(vlo), np.log(vhi), (R, K)))
    return side(Kp, 0.05, 9.0), side(Kq, 0.05, 9.0)


def host_row(args):
    import gmkl_models as gm
    from lhvi import utils
    p, q = args
    L, U, P, _ = gm.plan(p, -np.inf, np.inf)
    mu = p[1]
    pts = np.sort(mu[(mu > L) & (mu < U)])
    t = time.perf_counter()
    val = utils.kl_continuous_logpdf(lambda x: float(gm.log_mixture(x, *p)[0]), lambda x: float(gm.log_mixture(x, *q)[0]), L, U,
                                     points=pts, limit=max(400, 2 * (pts.size + 2)))
    return val, time.perf_counter() - t


def main():
    out = {}
    from concurrent.futures import ProcessPoolExecutor
    import multiprocessing as mp
    cases = {'exact_vs_k3': (2000, 4096, 3, 16), 'k3_vs_k3': (100000, 3, 3, 48)}
    data = {name: make(R, Kp, Kq, 7) for name, (R, Kp, Kq, _) in cases.items()}
    # ---- the host route first (no process has the GPU open yet): 16 worker processes over a subsample
    host_vals = {}
    with ProcessPoolExecutor(16, mp_context=mp.get_context('spawn')) as ex:
        list(ex.map(host_row, [(tuple(t[0] for t in data['k3_vs_k3'][0]), tuple(t[0] for t in data['k3_vs_k3'][1]))] * 16))    # start the workers
        for name, (R, Kp, Kq, n_sub) in cases.items():
            p, q = data[name]
            rows = [(tuple(t[r] for t in p), tuple(t[r] for t in q)) for r in range(n_sub)]
            t = time.perf_counter()
            res = list(ex.map(host_row, rows))
            wall = time.perf_counter() - t
            host_vals[name] = np.array([v for v, _ in res])
            out[name] = dict(R=R, Kp=Kp, Kq=Kq, host_subsample_rows=n_sub, host_subsample_wall_s=wall,
                             host_row_s_mean=float(np.mean([s for _, s in res])), host_scaled_to_R_s=wall * R / n_sub)
            print(name, 'host', out[name], flush=True)
    # ---- the device
    import torch
    from lhvi import _abi, gmkl
    for name, (R, Kp, Kq, n_sub) in cases.items():
        p, q = data[name]
        pd, qd = tuple(_abi.to_dev(t) for t in p), tuple(_abi.to_dev(t) for t in q)
        kl, info = gmkl.kl_scalar_mixtures(pd, qd, info=True)
        torch.cuda.synchronize()
        reps = 5
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            gmkl.kl_scalar_mixtures(pd, qd, info=True)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / reps
        t = time.perf_counter()
        for _ in range(reps):
            gmkl.kl_scalar_mixtures(pd, qd, info=True)
        torch.cuda.synchronize()
        wall_ms = (time.perf_counter() - t) / reps * 1e3
        ne = info['neval'].cpu().numpy().astype(np.int64)
        st = info['status'].cpu().numpy()
        klh = kl.cpu().numpy()
        evals = int(ne.sum())
        d = out[name]
        d.update(device_ms=ms, device_wall_ms=wall_ms, evals=evals, evals_per_row_mean=float(ne.mean()), evals_per_row_max=int(ne.max()),
                 evals_per_s=evals / (ms * 1e-3), exps_per_s=evals * (Kp + Kq) / (ms * 1e-3), status_nonzero=int((st != 0).sum()),
                 max_abs_diff_to_host_subsample=float(np.max(np.abs(klh[:n_sub] - host_vals[name]))),
                 speedup_vs_host_scaled=d['host_scaled_to_R_s'] / (ms * 1e-3))
        print(name, 'device', d, flush=True)
    if len(sys.argv) > 1:
        json.dump(out, open(sys.argv[1], 'w'), indent=1)


if __name__ == '__main__':
    main()
