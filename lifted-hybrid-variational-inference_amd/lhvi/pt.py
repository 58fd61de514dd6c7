"""Parallel tempering (replica exchange) for the block Gibbs sampler of a hybrid Gaussian MRF as many independent ladders on the
device (``csrc/pt.hip``; the sampler is written down in docs/kernels_pt.md).

A ladder is ``R`` replicas at ``betas[0] <= ... <= betas[R - 1] = 1`` on the path of the annealed importance sampler,
``f_beta = p~^beta f0^(1 - beta)`` with the base ``f0 = exp(-tau0 / 2 |x_c - mu0|^2)`` (x_d uniform).  Every replica makes block
Gibbs transitions at its own beta; every ``swap_every`` iterations adjacent replicas propose to exchange their discrete states,
accepted by the ratio of the collapsed masses ``m_beta(x_d)`` (x_c integrated out).  Only the ``beta = 1`` replica is recorded,
in the layout of the plain sampler with ``chains`` read as ``ladders``.

The public entry points are ``GibbsHybridGaussian.run_tempered``, ``HybridGaussianSampler.tempered_gibbs_sample`` and
``gibbs.tempered_gibbs_sample``; this module holds what they share.  There is no CPU path: without a GPU they raise ``LhviError``
(``ladder_host`` runs one ladder through the device's code on the CPU for the tests).

Out of scope: adaptive ladders, round-trip statistics, reuse of factors across the swap, more than 64 KiB of LDS per ladder, and
tempering for ``FlatGraph`` models.
"""
from __future__ import annotations

import types

import numpy as np

from . import _abi
from .ais import base
from .gibbs import MAX_BLOCK, _block_its, _Chains, _check_host, _check_states, _dev_ptr, _host_ptr, _Run, output_bytes, place  # noqa: F401


def schedule(replicas=None, betas=None):
    """the ladder as a float64 array [R]: ``betas`` checked (never decreasing, betas[0] >= 0, the last one 1), or
    ``linspace(0, 1, replicas)`` (``[1.]`` for one replica)"""
    if betas is None:
        R = int(replicas)
        if R < 1:
            raise ValueError('replicas must be positive')
        return np.linspace(0.0, 1.0, R) if R > 1 else np.ones(1)
    b = np.ascontiguousarray(betas, dtype=np.float64).reshape(-1)
    if b.size < 1 or b[-1] != 1.0:
        raise ValueError('betas must end at 1')
    if not b[0] >= 0.0:
        raise ValueError('betas must not be negative')
    if not np.all(np.diff(b) >= 0.0):              # NaN fails here too
        raise ValueError('betas must not decrease')
    return b


def _swap_every(swap_every):
    swap_every = int(swap_every)
    if swap_every < 0:
        raise ValueError('swap_every must not be negative')
    return swap_every


def ladder_host(gm, x_d, betas, tau0, mu0, disc_block_its, num_burnin, num_samples, swap_every=1, z=None, u=None, usw=None, seed=0,
                ladder=0, it_begin=0, it_end=None, state=None):
    """iterations [it_begin, it_end) of one ladder on the CPU through the device's code (``lhvi_pt_ladder_host``), with injected
    draws z [iters, R, Nc], u [iters, R, its, Nd] and usw [iters, max(R - 1, 1)] or, when all are None, the Philox stream of
    ladder ``ladder`` under ``seed``.  Returns a namespace: x_d [R, Nd], disc [num_samples, Nd], cont [num_samples, Nc], counts,
    sum1, sum2, swap_try [R - 1], swap_acc [R - 1].  ``state``: the namespace of an earlier call, to go on from (its x_d is
    used when ``x_d`` is None)."""
    ex = gm.ex
    Nd, Nc = ex.Nd, ex.Nc
    betas = schedule(betas=betas)
    R = betas.size
    its = _block_its(Nd, disc_block_its)
    swap_every = _swap_every(swap_every)
    iters = num_burnin + num_samples
    it_end = iters if it_end is None else int(it_end)
    mu0, tau0 = base(Nc, mu0, tau0)
    if z is not None or u is not None or usw is not None:
        z = np.ascontiguousarray(np.zeros((iters, R, Nc)) if z is None else z, dtype=np.float64)
        u = np.ascontiguousarray(np.zeros((iters, R, its, Nd)) if u is None else u, dtype=np.float64)
        usw = np.ascontiguousarray(np.zeros((iters, max(R - 1, 1))) if usw is None else usw, dtype=np.float64)
        z, u, usw = z.reshape(len(z), R, Nc), u.reshape(len(u), R, its, Nd), usw.reshape(len(usw), max(R - 1, 1))
        if (Nc and z.shape[0] < it_end) or (Nd and its and u.shape[0] < it_end) or usw.shape[0] < it_end:
            raise ValueError('fewer injected draws than iterations')
    s = gm.host_struct(its, num_burnin, num_samples, seed)
    if state is None:
        r = types.SimpleNamespace(
            disc=np.zeros((num_samples, Nd), dtype=np.int32), cont=np.zeros((num_samples, Nc)),
            counts=np.zeros(gm.n_states, dtype=np.int32), sum1=np.zeros(Nc), sum2=np.zeros(Nc * (Nc + 1) // 2),
            swap_try=np.zeros(R - 1, dtype=np.int32), swap_acc=np.zeros(R - 1, dtype=np.int32))
    else:
        r = types.SimpleNamespace(**{k: np.array(v) for k, v in vars(state).items()})
    if x_d is not None or state is None:
        rows = np.asarray(x_d, dtype=np.int32)
        r.x_d = np.array(np.broadcast_to(rows.reshape(rows.size // Nd if Nd else 1, Nd), (R, Nd)), order='C')      # a copy
    _check_states('x_d', r.x_d, ex.dstates)
    p = _host_ptr
    rc = _abi.lib().lhvi_pt_ladder_host(s, int(ladder), R, betas.ctypes.data, int(it_begin), it_end, swap_every, tau0, p(mu0),
                                        p(r.x_d), p(z), p(u), p(usw), p(r.disc), p(r.cont), p(r.counts), p(r.sum1), p(r.sum2),
                                        p(r.swap_try), p(r.swap_acc))
    _check_host(rc, _failed_state(gm, r.x_d) if rc == _abi.E_NOT_PD else None)
    return r


def _failed_state(gm, x_d):
    """the state to name when a ladder died: that of the hottest-to-coldest first replica whose J = -2A is not positive definite
    (a J_beta that fails has such a J behind it), the beta = 1 replica's when none is found"""
    from .exact import config_at_host
    x_d = np.asarray(x_d).reshape(-1, gm.ex.Nd)
    for row in x_d[::-1]:
        try:
            config_at_host(gm.ex, row)
        except ValueError:
            return row
    return x_d[-1]


class _Ladders(_Chains):
    """`ladders` ladders of R replicas on the device.  After ``run()`` the fields of ``_Chains`` with ``chains = ladders`` (the
    outputs of the beta = 1 replica), x_d [ladders, R, Nd], and swap_try / swap_acc [ladders, R - 1].  z / u / usw: injected draws
    (host arrays [iters, ladders * R, Nc] / [iters, ladders * R, its, Nd] / [iters, ladders, max(R - 1, 1)]) for the tests;
    tables: 'lds' / 'global' forces where the reduced tables live (default: LDS when the workgroup fits)."""

    LDS_BYTES = 'lhvi_pt_lds_bytes'
    NOUNS = ('ladder', 'iteration')
    ZERO_FILL_MISSING = True        # like the host twin: a test injects the stream it is about
    PLACEHOLDER = True              # a stream that is not read still has to be there when another is injected: the kernel
                                    # takes one non-null stream for "all are injected" and tests each pointer alone

    def __init__(self, gm, ladders, betas, tau0, mu0, num_burnin, num_samples, disc_block_its, swap_every, seed, keep_samples=False,
                 lanes=None, init_x_d=None, z=None, u=None, usw=None, tables=None):
        ladders, num_burnin, num_samples = int(ladders), int(num_burnin), int(num_samples)
        if ladders < 1 or num_burnin < 0 or num_samples < 0:
            raise ValueError('ladders >= 1, num_burnin >= 0 and num_samples >= 0 are required')
        self.ladders, self.R = ladders, int(betas.size)
        # (not _Chains.__init__: that is the plain sampler's arguments; _Chains lends the outputs and rb_disc)
        _Run.__init__(self, gm, ladders, num_burnin + num_samples, disc_block_its, seed, lanes, tables, init_x_d,
                      dict(z=z, u=u, usw=usw), num_burnin, num_samples, keep_samples, self.R)
        self.swap_every = _swap_every(swap_every)
        self.tau0, self.betas_host = float(tau0), betas
        self.betas = _abi.to_dev(betas)
        self.mu0 = _abi.to_dev(mu0 if gm.ex.Nc else np.zeros(1))

    def _device_bytes(self, keep_samples):
        return (output_bytes(self.gm, self.ladders, self.num_samples, keep_samples)
                + 4 * self.ladders * (self.R * self.gm.ex.Nd + 2 * self.R),
                '%d ladders of %d replicas and %d kept samples' % (self.ladders, self.R, self.num_samples))

    def _alloc_outputs(self, torch, dev, keep_samples):
        super()._alloc_outputs(torch, dev, keep_samples)
        self.swap_try = torch.zeros(self.ladders, self.R - 1, dtype=torch.int32, device=dev)
        self.swap_acc = torch.zeros(self.ladders, self.R - 1, dtype=torch.int32, device=dev)

    def _streams(self):
        n, Nd, Nc = self.ladders * self.R, self.gm.ex.Nd, self.gm.ex.Nc
        return ('z', (n, Nc)), ('u', (n, self.its, Nd)), ('usw', (self.ladders, max(self.R - 1, 1)))

    def advance(self, it_end):
        p = _dev_ptr
        _abi.check(_abi.lib().lhvi_pt_run(self.s, self.ladders, self.R, _abi.ptr(self.betas), self.done, int(it_end), self.swap_every,
                                          self.lanes, self.tau0, _abi.ptr(self.mu0), p(self.x_d), p(self.z), p(self.u), p(self.usw),
                                          p(self.disc), p(self.cont), p(self.counts), p(self.sum1), p(self.sum2), p(self.swap_try),
                                          p(self.swap_acc), _abi.ptr(self.bad), _abi.stream_ptr()))
        self.done = int(it_end)

    def rb_disc(self, s_begin=0, s_end=None, prob_sum=None, lanes=None):
        """``_Chains.rb_disc`` over the beta = 1 replica's kept samples; lanes default to the plain sampler's choice (a ladder's
        lanes are sized for R replicas a workgroup) with the tables where the ladder's are (one chain of 64 lanes fits where a
        ladder did, so this never refuses)"""
        if lanes is None:
            gm = self.gm
            lanes = place(_abi.lib().lhvi_gibbs_lds_bytes, gm.ex.Nc, gm.ex.Nd, gm.max_states, gm.table_doubles,
                          tables='lds' if self.in_lds else 'global')[0]
        return super().rb_disc(s_begin, s_end, prob_sum, lanes)

    def _bad_state(self, ladder):
        return _failed_state(self.gm, self.x_d[ladder].cpu().numpy())

    def swap_counts(self):
        """(tried [R - 1], accepted [R - 1]) summed over the ladders, as int64 host arrays"""
        return (self.swap_try.sum(dim=0, dtype=_abi._torch().int64).cpu().numpy(),
                self.swap_acc.sum(dim=0, dtype=_abi._torch().int64).cpu().numpy())


def run(gm, ladders=1024, replicas=8, betas=None, num_burnin=100, num_samples=100, disc_block_its=1, swap_every=1, seed=0,
        keep_samples=False, lanes=None, its_per_launch=None, base_mean=None, base_prec=None, init_x_d=None, z=None, u=None, usw=None,
        tables=None):
    """the finished ``_Ladders`` of the ``GibbsModel`` gm: the arguments of ``GibbsHybridGaussian.run_tempered``, the base mean 0
    and precision 1 unless given"""
    from .gibbs import _seed
    betas = schedule(replicas, betas)
    mu0, tau0 = base(gm.ex.Nc, base_mean, base_prec)
    return _Ladders(gm, ladders, betas, tau0, mu0, num_burnin, num_samples, disc_block_its, _swap_every(swap_every), _seed(seed),
                    keep_samples, lanes, init_x_d=init_x_d, z=z, u=u, usw=usw, tables=tables).run(its_per_launch)
