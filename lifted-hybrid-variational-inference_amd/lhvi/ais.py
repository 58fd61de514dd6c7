"""Annealed importance sampling (Neal 2001) for ``log Z`` of a hybrid Gaussian MRF as many independent annealing runs on the
device (``csrc/ais.hip``; the estimator is written down in docs/kernels_ais.md).

The path runs from the base ``f0 = exp(-tau0 / 2 |x_c - mu0|^2)`` (x_d uniform, ``log Z0`` exact) to the model along
``f_beta = p~^beta f0^(1 - beta)``.  Because x_c | x_d is Gaussian, the importance weights live on the collapsed space of x_d
and are built from the chain's Cholesky factor alone; the block Gibbs transition of ``csrc/gibbs.hpp`` is the invariant kernel.

The public entry points are ``GibbsHybridGaussian.log_partition``, ``HybridGaussianSampler.log_partition`` and
``gibbs.ais_log_partition``; this module holds what they share.  There is no CPU path: without a GPU ``log_partition`` raises
``LhviError`` (``chain_host`` runs one chain through the device's code on the CPU for the tests).

Out of scope: reverse AIS and bridge sampling, adaptive schedules, weighted-sample marginals from the final states, and the
``log Z`` of ``FlatGraph`` models.
"""
from __future__ import annotations

import math
import types

import numpy as np

from . import _abi
from .gibbs import _block_its, _check_host, _check_states, _dev_ptr, _host_ptr, _Run, _seed

STEPS_PER_LAUNCH = 256          # annealing steps of one launch
REDUCE_OUT, REDUCE_WS = 9, 8192  # LHVI_AIS_REDUCE_OUT, LHVI_AIS_REDUCE_WS


def schedule(steps=None, betas=None):
    """the schedule as a float64 array [T + 1]: ``betas`` checked (from 0 to 1, never decreasing), or the linear one"""
    if betas is None:
        steps = int(steps)
        if steps < 1:
            raise ValueError('steps must be positive')
        return np.linspace(0.0, 1.0, steps + 1)
    b = np.ascontiguousarray(betas, dtype=np.float64).reshape(-1)
    if b.size < 2 or b[0] != 0.0 or b[-1] != 1.0:
        raise ValueError('betas must run from 0 to 1')
    if not np.all(np.diff(b) >= 0.0):              # NaN fails here too
        raise ValueError('betas must not decrease')
    return b


def base(Nc, base_mean=None, base_prec=None):
    """(mu0 [Nc], tau0) of the base distribution: mean 0 and precision 1 unless given"""
    mu0 = np.zeros(Nc) if base_mean is None else np.ascontiguousarray(base_mean, dtype=np.float64).reshape(-1)
    if mu0.shape != (Nc,) or not np.all(np.isfinite(mu0)):
        raise ValueError('base_mean must hold %d finite numbers' % Nc)
    tau0 = 1.0 if base_prec is None else float(base_prec)
    if not (tau0 > 0.0 and math.isfinite(tau0)):
        raise ValueError('base_prec must be positive')
    return mu0, tau0


def log_z0(dstates, Nc, tau0):
    """the base's normaliser: sum_n log dstates[n] + Nc / 2 log(2 pi / tau0)"""
    return float(sum(math.log(int(d)) for d in dstates) + 0.5 * Nc * math.log(2.0 * math.pi / tau0))


def chain_host(gm, x_d, betas, tau0, mu0, disc_block_its=1, z=None, u=None, seed=0, chain=0, t_begin=0, t_end=None, logw=0.0):
    """steps [t_begin, t_end) of one chain on the CPU through the device's code (``lhvi_ais_chain_host``), with injected draws
    z [T, Nc] and u [T, its, Nd] or, when both are None, the Philox stream of chain ``chain`` under ``seed``.  Returns a
    namespace: x_d [Nd], logw."""
    ex = gm.ex
    Nd, Nc = ex.Nd, ex.Nc
    betas = schedule(betas=betas)
    T = betas.size - 1
    its = _block_its(Nd, disc_block_its)
    t_end = T if t_end is None else int(t_end)
    mu0, tau0 = base(Nc, mu0, tau0)
    if z is not None or u is not None:
        z = np.ascontiguousarray(np.zeros((T, Nc)) if z is None else z, dtype=np.float64)
        u = np.ascontiguousarray(np.zeros((T, its, Nd)) if u is None else u, dtype=np.float64)
        z, u = z.reshape(len(z), Nc), u.reshape(len(u), its, Nd)
        if (Nc and z.shape[0] < T) or (Nd and its and u.shape[0] < T):
            raise ValueError('fewer injected draws than steps')
    s = gm.host_struct(its, 0, 0, seed)
    r = types.SimpleNamespace(x_d=np.array(x_d, dtype=np.int32).reshape(Nd))
    _check_states('x_d', r.x_d, ex.dstates)
    lw = np.array([logw], dtype=np.float64)
    p = _host_ptr
    _check_host(_abi.lib().lhvi_ais_chain_host(s, int(chain), T, betas.ctypes.data, int(t_begin), t_end, tau0, p(mu0), p(r.x_d),
                                               lw.ctypes.data, p(z), p(u)), r.x_d)
    r.logw = float(lw[0])
    return r


class _AisChains(_Run):
    """`chains` annealing runs on the device.  After ``run()``: x_d [chains, Nd] and logw [chains] as device tensors.
    z / u: injected draws (host arrays [T, chains, Nc] / [T, chains, its, Nd]) for the tests; tables: 'lds' / 'global' forces
    where the reduced tables live (default: LDS when the workspace fits)."""

    LDS_BYTES = 'lhvi_ais_lds_bytes'
    NOUNS = ('chain', 'step')
    PER_LAUNCH = ('steps_per_launch', STEPS_PER_LAUNCH)
    ZERO_FILL_MISSING = True        # like the host twin: a test injects the stream it is about

    def __init__(self, gm, chains, betas, tau0, mu0, disc_block_its, seed, lanes=None, init_x_d=None, z=None, u=None, tables=None):
        chains = int(chains)
        if chains < 1:
            raise ValueError('chains >= 1 is required')
        self.T = betas.size - 1
        super().__init__(gm, chains, self.T, disc_block_its, seed, lanes, tables, init_x_d, dict(z=z, u=u))
        self.tau0 = float(tau0)
        self.betas = _abi.to_dev(betas)
        self.mu0 = _abi.to_dev(mu0 if gm.ex.Nc else np.zeros(1))

    def _device_bytes(self, keep_samples):
        return None                 # a state and a weight per chain: never checked against the free memory (kept as it was)

    def _alloc_outputs(self, torch, dev, keep_samples):
        self.logw = torch.zeros(self.chains, dtype=torch.float64, device=dev)

    def _streams(self):
        return ('z', (self.chains, self.gm.ex.Nc)), ('u', (self.chains, self.its, self.gm.ex.Nd))

    def advance(self, t_end):
        p = _dev_ptr
        _abi.check(_abi.lib().lhvi_ais_run(self.s, self.chains, self.T, _abi.ptr(self.betas), self.done, int(t_end), self.lanes,
                                           self.tau0, _abi.ptr(self.mu0), p(self.x_d), _abi.ptr(self.logw), p(self.z), p(self.u),
                                           _abi.ptr(self.bad), _abi.stream_ptr()))
        self.done = int(t_end)


def reduce(logw):
    """the nine sums of ``lhvi_ais_reduce`` over a device tensor logw [chains], as a host array"""
    torch = _abi.require_gpu()
    if logw.dim() != 1 or logw.dtype != torch.float64 or not logw.is_contiguous() or logw.numel() < 1:
        raise ValueError('logw must be a contiguous float64 tensor [chains]')
    out = torch.empty(REDUCE_OUT, dtype=torch.float64, device=logw.device)
    ws = torch.empty(REDUCE_WS, dtype=torch.float64, device=logw.device)
    _abi.check(_abi.lib().lhvi_ais_reduce(int(logw.numel()), _abi.ptr(logw), _abi.ptr(out), _abi.ptr(ws), _abi.stream_ptr()))
    return out.cpu().numpy()


def estimates(sums, chains, logZ0, log_const=0.0):
    """the estimates from the sums of ``reduce`` (or ``reduce_numpy``): namespace logZ, stderr, ess, lower, lower_stderr, obj.
    With mx = max logw, d = logw - mx, S1 = sum exp(d), S2 = sum exp(2 d), D1 = sum d, D2 = sum d^2 and C chains:
    logZ = log Z0 + mx + log(S1 / C); stderr = std(w / mean w) / sqrt(C) = sqrt((C S2 / S1^2 - 1) / C) (delta method);
    ess = S1^2 / (C S2), the effective sample fraction; lower = log Z0 + mean(logw) with the standard error of that mean."""
    Cn = float(chains)
    mx, S1, S2, D1, D2 = (float(sums[i]) for i in (4, 5, 6, 7, 8))
    off = float(logZ0) + float(log_const)
    logZ = off + mx + math.log(S1 / Cn)
    stderr = math.sqrt(max(Cn * S2 / (S1 * S1) - 1.0, 0.0) / Cn)
    lower = off + mx + D1 / Cn
    lower_stderr = math.sqrt(max(D2 - D1 * D1 / Cn, 0.0) / (Cn - 1.0) / Cn) if chains > 1 else float('nan')
    return types.SimpleNamespace(logZ=logZ, stderr=stderr, ess=S1 * S1 / (Cn * S2), lower=lower, lower_stderr=lower_stderr,
                                 obj=-logZ)


def reduce_numpy(logw):
    """``lhvi_ais_reduce`` restated in NumPy (any order of summation), for host-side use of ``estimates``"""
    lw = np.asarray(logw, dtype=np.float64).reshape(-1)
    mx = lw.max()
    d = lw - mx
    S1, S2 = np.exp(d).sum(), np.exp(2.0 * d).sum()
    return np.array([mx + np.log(S1), 2.0 * mx + np.log(S2), lw.sum(), (lw * lw).sum(), mx, S1, S2, d.sum(), (d * d).sum()])


def log_partition(gm, chains=4096, steps=256, betas=None, disc_block_its=1, seed=0, base_mean=None, base_prec=None, lanes=None,
                  steps_per_launch=None, log_const=0.0, init_x_d=None, z=None, u=None, tables=None):
    """the annealed importance sampling estimate of ``log Z`` of the ``GibbsModel`` gm (plus ``log_const``): the record of
    ``estimates`` with logZ0, betas, chains, steps, base_mean, base_prec, the device tensors log_weights [chains] and
    x_d [chains, Nd] (the final states), and run (the ``_AisChains`` that holds the model on the device)"""
    betas = schedule(steps, betas)
    mu0, tau0 = base(gm.ex.Nc, base_mean, base_prec)
    run = _AisChains(gm, chains, betas, tau0, mu0, disc_block_its, _seed(seed), lanes=lanes, init_x_d=init_x_d, z=z, u=u,
                     tables=tables).run(steps_per_launch)
    logZ0 = log_z0(gm.ex.dstates, gm.ex.Nc, tau0)
    r = estimates(reduce(run.logw), run.chains, logZ0, log_const)
    r.logZ0, r.betas, r.chains, r.steps, r.base_mean, r.base_prec = logZ0, betas, run.chains, run.T, mu0, tau0
    r.log_weights, r.x_d, r.lanes, r.run = run.logw, run.x_d, run.lanes, run
    return r
