"""Time per update of nonparametric variational inference (lhvi_npvi_run) next to the mixture VI step (lhvi_vi_adam_run) on the same
graph, K and T, in one process: the 1.0 M-factor ground RGM of scripts/bench_configs.py (`vi_ground`) at (K, T) = (1, 3), (2, 3),
(4, 3), and the scaled cfg-3 HMLN (`vi_scaled`) at K = 2.  Not the contract benchmark (that is bench.py).  Writes
profiles/npvi_bench.json and prints one JSON line per measurement; docs/kernels_npvi.md quotes the numbers.

    python scripts/bench_npvi.py [--updates 20] [--copies 286] [--out profiles/npvi_bench.json] [--small]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'lifted-hybrid-variational-inference_amd')]
import numpy as np
import torch
from lhvi import synth
from lhvi.npvi import NPVI
from lhvi.vi import VarInference


def timed(fn, updates, reps=3):
    """median device time per update over `reps` windows of `updates` updates (events around the enqueued loop), after a warm-up"""
    fn(2)
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn(updates)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / updates)
    return float(np.median(times)), [float(t) for t in times]


def measure(label, flat, K, T, updates):
    base = dict(model=label, rvs=int(flat.V), factors=int(flat.F), edges=int(flat.E), hidden=int(flat.var_hidden.sum()), K=K, T=T,
                updates_per_window=updates)
    s = NPVI(flat, K, T, seed=0)
    s._ensure_dev()
    log = torch.zeros(updates, dtype=torch.float64, device=s.dg.device)
    t_npvi, w_npvi = timed(lambda n: s._enqueue(n, 0.05, 0, log), updates)
    obj = float(log[updates - 1].item())
    kernel = 'interpreter' if s.dg.p.interpreted or s.max_arity > 3 else ('lean, 8 slots' if s.max_slots <= 8 else 'lean, 24 slots')
    del s, log
    torch.cuda.empty_cache()

    vi = VarInference(None, K, T)
    vi._setup_flat(flat)
    np.random.seed(0)
    vi.init_param()
    vi.is_log, vi.log_fe = False, False
    vi.alpha, vi.b1, vi.b2, vi.eps, vi.t = 0.05, 0.9, 0.999, 1e-8, 0
    t_vi, w_vi = timed(vi.ADAM_update, updates)
    split = dict(zip(('cc', 'tiny', 'grp3', 'grp6', 'rest3', 'rest6'), vi._fac_counts))
    del vi
    torch.cuda.empty_cache()
    return dict(base, npvi_ms_per_update=t_npvi, npvi_windows_ms=w_npvi, npvi_factor_kernel=kernel, npvi_obj_last=obj,
                vi_ms_per_update=t_vi, vi_windows_ms=w_vi, vi_kernel_split=split, npvi_over_vi=t_npvi / t_vi)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--updates', type=int, default=20)
    ap.add_argument('--copies', type=int, default=286)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'npvi_bench.json'))
    ap.add_argument('--small', action='store_true', help='a rehearsal at toy sizes (the numbers mean nothing)')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_npvi.py needs a GPU'
    C_, B_, copies = (1000, 500, args.copies) if not args.small else (20, 10, 1)
    rgm = synth.rgm_flat(C=C_, B=B_, n_values=0, evidence_ratio=0.1, seed=0)[0]
    results = []
    for K in (1, 2, 4):
        results.append(measure('RGM C=%d B=%d ground (Gaussian pairwise)' % (C_, B_), rgm, K, 3, args.updates))
        print(json.dumps(results[-1]), flush=True)
    del rgm
    hmln = synth.paper_popularity_copies(copies, 300, 10, seed=0, points=20)
    results.append(measure('scaled cfg 3: %d x paper-popularity 300 x 10' % copies, hmln, 2, 3, args.updates))
    print(json.dumps(results[-1]), flush=True)
    if not args.small:
        with open(args.out, 'w') as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), results=results), f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
