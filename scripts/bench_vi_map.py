"""The variational MAP query: host scipy (one minimize per row, the reference's call) against lhvi_vi_map_bfgs (one launch).

  python scripts/bench_vi_map.py loglik [--out F]   (a) robot-mapping C2FVarInference.run(n, log_fe=False), K = 2: wall seconds
                                                        per logged update with map_mode 'scipy' (small n) and 'device', same process
  python scripts/bench_vi_map.py kernel [--out F]   (b) lhvi_vi_map_bfgs on 1 M hidden continuous rows, K = 2 and K = 5 (run it
                                                        under rocprofv3 --kernel-trace --stats for the kernel time), and the host
                                                        scipy cost per row on a 2 000-row sample of the same parameters
One JSON object per line, appended to --out (default profiles/r06_vi_map.jsonl).
"""
import argparse
import gzip
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'lifted-hybrid-variational-inference_amd')]
import numpy as np  # noqa: E402
import torch  # noqa: E402


def robot_flat():
    from lhvi import generators
    rec = json.load(gzip.open(os.path.join(ROOT, 'tests', 'golden', 'grounding.json.gz'), 'rt'))['robot_mapping']
    data = {tuple(k): v for k, v in rec['evidence']}
    return generators.robot_mapping().ground_flat(data)[0]


def c2f_owner(K, mode):
    from lhvi import c2fvi
    owner = c2fvi.VarInference.__new__(c2fvi.VarInference)
    owner._init_common(K, 3)
    owner.map_mode = mode
    return owner


def loglik(out):
    from lhvi import c2fvi
    flat = robot_flat()
    K = 2
    opts = dict(k_mean_k=2, k_mean_its=10, update_obs_its=10, output_its=0, min_obs_var=0, gaussian_obs=True, kmeans_member_order=None)
    runs = {}
    for mode, n, log_map in (('device', 10, True), ('scipy', 10, True), ('device', 30, True), ('device', 30, False)):
        owner = c2f_owner(K, mode)
        o = dict(opts, log_map_likelihood=log_map)
        np.random.seed(0)
        c2fvi.run_c2fvi_flat(flat, c2fvi._DeviceEngine(owner), K, 10, 0.2, o)           # warm-up (code objects, caches)
        np.random.seed(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = c2fvi.run_c2fvi_flat(flat, c2fvi._DeviceEngine(owner), K, n, 0.2, o)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        st = res['stage']
        rec = dict(part='a', model='robot-mapping HMLN', K=K, map_mode=mode if log_map else None, log_fe=not log_map, updates=n,
                   ground_vars=int(flat.V), lifted_rows_last_round=int(st.flat.V),
                   hidden_cont_rows_last_round=int((st.flat.var_hidden & st.flat.var_cont).sum()),
                   wall_s=wall, s_per_update=wall / n, log_last=float(res['fe_log'][-1]))
        runs[(mode, n, log_map)] = res['fe_log']
        print(json.dumps(rec))
        out.write(json.dumps(rec) + '\n')
    same = np.allclose(runs[('device', 10, True)], runs[('scipy', 10, True)], rtol=1e-9, atol=1e-9)
    rec = dict(part='a', check='device and scipy logs of the first 10 updates agree (rtol 1e-9)', value=bool(same))
    print(json.dumps(rec))
    out.write(json.dumps(rec) + '\n')


def isolated_flat(V):
    """V hidden continuous rows without neighbours (a unary X2 prior each), built on arrays"""
    from lhvi import synth
    return synth.random_gaussian_mrf(V=V, deg=0, seed=0, evidence_ratio=0.0)


def sample_params(rng, V, K):
    w_tau = rng.random(K) * 4
    eta = np.empty((V, K, 2))
    eta[:, :, 0] = rng.normal(0, 5, (V, K))
    eta[:, :, 1] = 10 ** rng.uniform(-3, 2.5, (V, K))
    return w_tau, eta


def kernel(out, V):
    from lhvi.vi import VarInference
    from scipy.optimize import minimize
    flat = isolated_flat(V)
    rng = np.random.default_rng(0)
    for K in (2, 5):
        vi = VarInference(None, K, 3)
        vi._setup_flat(flat)
        w_tau, eta = sample_params(rng, flat.V, K)
        vi._upload_params(w_tau, eta, np.zeros((flat.V, K, 1)))
        vi.map_rows_device()                                        # warm-up
        walls = []
        for _ in range(5):
            vi._cache = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            x, (f, nit, status) = vi.map_rows_device(info=True)
            walls.append(time.perf_counter() - t0)
        hid = flat.var_hidden & flat.var_cont
        # host: the reference's call on a 2 000-row sample of the same rows
        rows = np.flatnonzero(hid)[:2000]
        t0 = time.perf_counter()
        for v in rows:
            p = {m: vi._row_belief(v, m) for m in vi._host('eta_c')[v][:, 0]}
            x0 = max(p.keys(), key=lambda k: p[k])
            minimize(lambda val, v=v: -vi._row_belief(v, val), x0=np.array([x0]), options={'disp': False})
        host = (time.perf_counter() - t0) / rows.size
        rec = dict(part='b', K=K, rows=int(hid.sum()), launch_wall_ms_incl_readback=[round(1e3 * w, 3) for w in walls],
                   nit_mean=float(nit[hid].mean()), nit_max=int(nit[hid].max()),
                   status_counts={str(s): int(c) for s, c in zip(*np.unique(status[hid], return_counts=True))},
                   host_scipy_ms_per_row=1e3 * host, host_sample_rows=int(rows.size),
                   host_scipy_s_for_all_rows_extrapolated=host * int(hid.sum()))
        print(json.dumps(rec))
        out.write(json.dumps(rec) + '\n')
        del vi


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('part', choices=('loglik', 'kernel'))
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r06_vi_map.jsonl'))
    ap.add_argument('--rows', type=int, default=1 << 20)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    with open(a.out, 'a') as fh:
        loglik(fh) if a.part == 'loglik' else kernel(fh, a.rows)
