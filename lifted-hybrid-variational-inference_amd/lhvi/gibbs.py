"""Block Gibbs sampling in a hybrid Gaussian MRF (API of ``gibbs/hybrid_gaussian_mrf.py``, the sampling half, and of
``gibbs/disc_mrf.py``) as many independent chains on the device (``csrc/gibbs.hip``).

``block_gibbs_sample``, ``HybridGaussianSampler`` and ``gibbs_sample`` keep the reference's names, argument order and return
shapes, with one more keyword ``chains``; ``GibbsHybridGaussian`` is the solver-shaped form (evidence, automatic conversion of
potentials, marginals with standard errors over chains, R-hat).  The model is the flat model of the exact baseline
(``exact.flatten_factors``) plus the variable-to-factor lists of the discrete sweep (``GibbsModel``).  There is no CPU path:
without a GPU the calls raise ``LhviError`` (``chain_host`` runs one chain with injected draws through the device's code for
the tests).

Deliberate differences (docs/kernels_gibbs.md): x_c is drawn as ``mu + L^-T z`` from the Cholesky factor of J instead of
``np.random.multivariate_normal`` (SVD of the covariance); the random numbers are a counter-based Philox stream instead of
``drand48`` / NumPy's generator; ``HybridGaussianSampler.map`` of a discrete variable works.  ``GibbsHybridGaussian`` fits the
mixtures of all continuous variables to the kept samples on the device (``fit_marginals``, ``lhvi/gmfit.py``);
``fit_scalar_gm_from_samples`` and ``HybridGaussianSampler.map`` keep calling scikit-learn like the reference.

Beyond the reference (docs/kernels_gibbs_rb.md): ``GibbsHybridGaussian.rb_marginals()`` / ``rb_disc_marginals()`` /
``rb_moments()`` and ``rao_blackwell=True`` of ``map`` / ``map_all`` / ``belief`` average the exact conditionals
``p(x_c | x_d)`` and ``p(x_n | x_d,-n, x_c)`` over the kept samples (``csrc/gibbs_rb.hip``); ``rb_disc_host`` runs one chain of
the latter through the device's code on the CPU.  ``GibbsHybridGaussian.log_partition()``,
``HybridGaussianSampler.log_partition()`` and ``ais_log_partition`` estimate ``log Z`` by annealed importance sampling
(``csrc/ais.hip``, ``lhvi/ais.py``, docs/kernels_ais.md): the ``obj = -logZ`` the reference's Gibbs baseline leaves as a TODO.
``GibbsHybridGaussian.run_tempered()``, ``HybridGaussianSampler.tempered_gibbs_sample()`` and ``tempered_gibbs_sample`` run the
sampler as ladders of replicas along the same path that exchange their discrete states (parallel tempering, ``csrc/pt.hip``,
``lhvi/pt.py``, docs/kernels_pt.md), for models whose discrete variables select the well a continuous variable sits in.
"""
from __future__ import annotations

import ctypes as C
import os
import types

import numpy as np

from . import _abi, hg_energy
from . import exact as _exact
from .exact import MAX_NC, ExactHybridGaussian, ExactModel, _Factor, flatten_factors, joint_map_dict
from .potentials import LogTable

LDS_LIMIT = 64 * 1024
ITS_PER_LAUNCH = 256            # outer iterations of one launch
MAX_BLOCK = 256                 # threads of a workgroup: the replicas of a ladder times their lanes may not exceed it


# ---- host: flat model -> sampler model ----------------------------------------------------------------------------------------------
class GibbsModel:
    """the lists of ``lhvi_gibbs_t`` (include/lhvi.h) beyond its ``lhvi_exact_t``, in host arrays, derived from the descriptors
    of an ``ExactModel``"""

    FIELDS = ('dstate_off', 'vt_ptr', 'vt_fac', 'vh_ptr', 'vh_fac', 'hyb_quad', 'hyb_off')

    def __init__(self, ex):
        self.ex = ex
        Nd = ex.Nd
        vt, vh = [[] for _ in range(Nd)], [[] for _ in range(Nd)]
        hyb_quad, hyb_off = [], [0]
        for f in range(ex.n_quad):              # a LogHybridQuadratic without a discrete axis counts as continuous (:186-190)
            rec = ex.quad_desc[ex.quad_ptr[f]:ex.quad_ptr[f + 1]]
            nd = int(rec[0])
            if nd == 0:
                continue
            scope = [int(v) for v in rec[3:3 + 2 * nd:2]]
            for v in scope:
                vh[v].append(len(hyb_quad))
            hyb_quad.append(f)
            hyb_off.append(hyb_off[-1] + int(np.prod(ex.dstates[scope], dtype=np.int64)))
        for f in range(ex.n_tab):
            rec = ex.tab_desc[ex.tab_ptr[f]:ex.tab_ptr[f + 1]]
            for v in rec[2:2 + 2 * int(rec[0]):2]:
                vt[int(v)].append(f)
        if hyb_off[-1] >= 2 ** 31:
            raise ValueError('the reduced tables of the hybrid factors exceed 32-bit offsets')
        i32 = lambda a: np.asarray(a, dtype=np.int32).reshape(-1)                       # noqa: E731
        self.dstate_off = i32(np.concatenate([[0], np.cumsum(ex.dstates)]))
        self.vt_ptr = i32(np.concatenate([[0], np.cumsum([len(l) for l in vt])]))
        self.vt_fac = i32([f for l in vt for f in l])
        self.vh_ptr = i32(np.concatenate([[0], np.cumsum([len(l) for l in vh])]))
        self.vh_fac = i32([h for l in vh for h in l])
        self.hyb_quad, self.hyb_off = i32(hyb_quad), i32(hyb_off)
        self.n_hyb, self.table_doubles = len(hyb_quad), int(hyb_off[-1])
        self.max_states = int(ex.dstates.max()) if Nd else 1
        self.n_states = int(ex.dstates.sum())

    def struct(self, ptr_of, disc_block_its, num_burnin, num_samples, seed, table_scratch=None):
        s = _abi.GibbsStruct()
        s.ex = self.ex.struct(ptr_of)
        for name in self.FIELDS:
            setattr(s, name, ptr_of(name))
        s.n_hyb, s.table_doubles, s.max_states = self.n_hyb, self.table_doubles, self.max_states
        s.table_scratch = table_scratch
        s.disc_block_its, s.num_burnin, s.num_samples = int(disc_block_its), int(num_burnin), int(num_samples)
        s.seed = int(seed) & (2 ** 64 - 1)
        return s

    def arrays(self):
        out = {n: getattr(self.ex, n) for n in ExactModel.FIELDS}
        out.update({n: getattr(self, n) for n in self.FIELDS})
        return out

    def host_struct(self, disc_block_its, num_burnin, num_samples, seed):
        """``struct`` over the host arrays, which it keeps alive (``ExactModel.host_struct``): the model of a host twin"""
        arrs = {n: np.ascontiguousarray(a) for n, a in self.arrays().items()}
        s = self.struct(lambda n: C.c_void_p(arrs[n].ctypes.data if arrs[n].size else 0), disc_block_its, num_burnin, num_samples,
                        seed)
        s._keep = arrs
        return s


def _block_its(Nd, disc_block_its):
    """one sweep samples p(x_d | x_c) exactly when there is one discrete variable (:167-168)"""
    if disc_block_its < 0:
        raise ValueError('disc_block_its must not be negative')
    return 1 if Nd == 1 else int(disc_block_its)


def _not_pd_message(state):
    return 'the precision matrix J = -2A is not positive definite at the discrete state %r' % (tuple(int(s) for s in state),)


def _host_ptr(a):
    """the address of a host array for a twin's call (None: no array, or an empty one)"""
    return a.ctypes.data if a is not None and a.size else None


def _dev_ptr(t):
    """the address of a device tensor for a launch (None: no tensor, or an empty one)"""
    return _abi.ptr(t) if t is not None and t.numel() else None


def _check_states(what, x, dstates):
    """x [..., Nd]: every digit inside its variable's range"""
    if x.size and (x.min() < 0 or (x >= np.asarray(dstates)).any()):
        raise ValueError('%s holds a state outside its variable\'s range' % what)


def _check_host(rc, state):
    """the return code of a host twin: ``LHVI_E_NOT_PD`` names the discrete state it happened at"""
    if rc == _abi.E_NOT_PD:
        raise ValueError(_not_pd_message(state))
    _abi.check(rc)


def chain_host(gm, x_d, z, u, disc_block_its, num_burnin, num_samples, it_begin=0, it_end=None):
    """one chain on the CPU through the device's code (``lhvi_gibbs_chain_host``) with injected draws z [iters, Nc] and
    u [iters, its, Nd].  Returns a namespace: disc [num_samples, Nd], cont [num_samples, Nc], counts, sum1, sum2, x_d."""
    ex = gm.ex
    Nd, Nc = ex.Nd, ex.Nc
    its = _block_its(Nd, disc_block_its)
    it_end = num_burnin + num_samples if it_end is None else it_end
    z = np.ascontiguousarray(z, dtype=np.float64).reshape(len(z), Nc)
    u = np.ascontiguousarray(u, dtype=np.float64).reshape(len(u), its, Nd)
    if (Nc and z.shape[0] < it_end) or (Nd and its and u.shape[0] < it_end):
        raise ValueError('fewer injected draws than iterations')
    s = gm.host_struct(its, num_burnin, num_samples, 0)
    r = types.SimpleNamespace(
        disc=np.zeros((num_samples, Nd), dtype=np.int32), cont=np.zeros((num_samples, Nc)),
        counts=np.zeros(gm.n_states, dtype=np.int32), sum1=np.zeros(Nc), sum2=np.zeros(Nc * (Nc + 1) // 2),
        x_d=np.array(x_d, dtype=np.int32).reshape(Nd))
    _check_states('x_d', r.x_d, ex.dstates)
    p = _host_ptr
    _check_host(_abi.lib().lhvi_gibbs_chain_host(s, int(it_begin), int(it_end), p(r.x_d), p(z), p(u), p(r.disc), p(r.cont),
                                                 p(r.counts), p(r.sum1), p(r.sum2)), r.x_d)
    return r


def rb_disc_host(gm, disc, cont, s_begin=0, s_end=None, prob_sum=None):
    """one chain's Rao-Blackwellised probability sums on the CPU through the device's code (``lhvi_gibbs_rb_disc_host``):
    disc [num_samples, Nd], cont [num_samples, Nc] -> prob_sum [sum dstates], the sum over the samples [s_begin, s_end) of
    p(x_n = k | x_d,-n, x_c), added to ``prob_sum`` when one is given (a run split over calls)"""
    ex = gm.ex
    Nd, Nc = ex.Nd, ex.Nc
    num_samples = len(disc)
    disc = np.ascontiguousarray(disc, dtype=np.int32).reshape(num_samples, Nd)
    cont = np.ascontiguousarray(cont, dtype=np.float64).reshape(num_samples, Nc)
    s_end = num_samples if s_end is None else int(s_end)
    _check_states('disc', disc, ex.dstates)
    s = gm.host_struct(1, 0, num_samples, 0)
    out = np.zeros(gm.n_states) if prob_sum is None else np.ascontiguousarray(prob_sum, dtype=np.float64).reshape(gm.n_states)
    p = _host_ptr
    _abi.check(_abi.lib().lhvi_gibbs_rb_disc_host(s, int(s_begin), s_end, p(disc), p(cont), p(out)))
    return out


# ---- device ------------------------------------------------------------------------------------------------------------------
def default_lanes(Nc):
    """lanes per chain: the smallest power of two >= Nc / 2, at least 4 (docs/kernels_gibbs.md, "Lanes")"""
    lanes = 4
    while 2 * lanes < min(Nc, 64):
        lanes *= 2
    return lanes


def place(lds_bytes, Nc, Nd, max_states, table_doubles, lanes=None, tables=None, R=None):
    """(lanes, in_lds) of a run: the lanes of a chain and whether its reduced tables live in LDS.  ``lds_bytes``: the sampler's
    ``lhvi_*_lds_bytes`` (a host function of the library: this needs no device); ``tables``: 'lds' / 'global' forces the place;
    ``R``: the replicas of a ladder, None for the plain and the annealed sampler.  Without ``lanes`` a chain gets
    ``default_lanes(Nc)``: doubled while a workgroup of chains is over 64 KiB (sized with the tables in LDS only when they are
    forced there), or halved while the R replicas of a ladder exceed a workgroup's threads and never grown (the tables leave LDS
    before a ladder is refused).  Raises ``ValueError`` for lanes that are no power of two up to 64 and for a workgroup that is
    still too large."""
    shape = () if R is None else (R,)
    lds_of = lambda lanes, in_lds: int(lds_bytes(Nc, Nd, max_states + (table_doubles if in_lds else 0), *shape, lanes))  # noqa: E731
    if R is not None and R > MAX_BLOCK:
        raise ValueError('%d replicas exceed the %d threads of a workgroup' % (R, MAX_BLOCK))
    if lanes is None and R is None:
        lanes = default_lanes(Nc)
        while lanes < 64 and lds_of(lanes, tables == 'lds') > LDS_LIMIT:
            lanes *= 2
    elif lanes is None:
        lanes = default_lanes(Nc)
        while lanes > 1 and R * lanes > MAX_BLOCK:
            lanes //= 2
    lanes = int(lanes)
    if lanes < 1 or lanes > 64 or lanes & (lanes - 1):
        raise ValueError('lanes must be a power of two up to 64')
    if R is not None and R * lanes > MAX_BLOCK:
        raise ValueError('%d replicas of %d lanes exceed the %d threads of a workgroup' % (R, lanes, MAX_BLOCK))
    in_lds = lds_of(lanes, True) <= LDS_LIMIT if tables is None else tables == 'lds'
    if lds_of(lanes, in_lds) > LDS_LIMIT:
        raise ValueError('a workgroup of %d %s needs %d bytes of LDS, more than %d'
                         % (((64 // lanes, 'chains') if R is None else (R, 'replicas')) + (lds_of(lanes, in_lds), LDS_LIMIT)))
    return lanes, in_lds


def output_bytes(gm, chains, num_samples, keep_samples):
    """device bytes of the outputs of a run: the state, the accumulators (, the samples)"""
    Nd, Nc = gm.ex.Nd, gm.ex.Nc
    n = 4 * chains * (Nd + gm.n_states) + 8 * chains * (Nc + Nc * (Nc + 1) // 2)
    return n + (chains * num_samples * (4 * Nd + 8 * Nc) if keep_samples else 0)


class _Run:
    """The run layer under the plain, the annealed and the tempered sampler: `units` chains (or ladders of R replicas, a chain
    each) of ``gm`` on the device.  It decides the lanes and the place of the reduced tables (``place``, before a device is asked
    for), uploads the model (``t``, ``scratch``, ``s``), starts the states ``x_d`` (given, or drawn on the device), uploads the
    injected draws, and runs ``total`` iterations in launches of ``advance``, which a subclass supplies with what else differs:

    LDS_BYTES   its ``lhvi_*_lds_bytes``
    NOUNS       what an error message calls a unit and an iteration
    PER_LAUNCH  the name and the default of ``run``'s argument
    _device_bytes / _alloc_outputs / _streams / _bad_state   (below)"""

    LDS_BYTES = None
    NOUNS = ('chain', 'iteration')
    PER_LAUNCH = ('its_per_launch', ITS_PER_LAUNCH)
    # An injected stream that is missing while another is given: zeros in its place, or (the plain sampler, which takes both
    # streams or neither; kept for compatibility) the error of converting None.
    ZERO_FILL_MISSING = False
    # An injected stream nothing reads (no x_c, no sweep): no pointer, or a placeholder of one double.
    PLACEHOLDER = False

    def __init__(self, gm, units, total, disc_block_its, seed, lanes, tables, init_x_d, draws, num_burnin=0, num_samples=0,
                 keep_samples=False, R=None):
        ex = gm.ex
        Nd, Nc = ex.Nd, ex.Nc
        if Nc > MAX_NC:
            raise ValueError('Nc = %d continuous variables exceed LHVI_EXACT_MAX_NC = %d' % (Nc, MAX_NC))
        l = _abi.lib()
        its = _block_its(Nd, disc_block_its)
        lanes, in_lds = place(getattr(l, self.LDS_BYTES), Nc, Nd, gm.max_states, gm.table_doubles, lanes, tables, R)
        torch = _abi.require_gpu()
        chains = units * (1 if R is None else R)
        scratch_rows = 0 if in_lds else (chains + 63) // 64 * 64       # rb_disc pads its chains to 64
        self.gm, self.chains, self.lanes, self.in_lds, self.its, self.total = gm, units, lanes, in_lds, its, total
        self.num_burnin, self.num_samples = num_burnin, num_samples
        need = self._device_bytes(keep_samples)
        if need is not None:
            need, what = need[0] + 8 * scratch_rows * gm.table_doubles, need[1]
            free = int(torch.cuda.mem_get_info()[0])
            if need > free:
                raise MemoryError('%s (Nd = %d, Nc = %d) need %d bytes of device memory, %d are free' % (what, Nd, Nc, need, free))
        self.t = t = _abi.upload({n: (a if a.size else np.zeros(1, dtype=a.dtype)) for n, a in gm.arrays().items()})
        dev = t['dstates'].device
        self.scratch = None if in_lds else torch.empty(scratch_rows, max(gm.table_doubles, 1), dtype=torch.float64, device=dev)
        self.s = gm.struct(lambda n: _abi.ptr(t[n]), its, num_burnin, num_samples, seed, _abi.ptr(self.scratch))
        if init_x_d is not None:
            init = np.asarray(init_x_d, dtype=np.int64)
            init = np.broadcast_to(init.reshape(init.size // max(Nd, 1) if Nd else 1, Nd), (chains, Nd))
            _check_states('init_x_d', init, ex.dstates)
            x_d = _abi.to_dev(np.ascontiguousarray(init, dtype=np.int32))
        else:
            x_d = torch.zeros(chains, Nd, dtype=torch.int32, device=dev)
            _abi.check(l.lhvi_gibbs_init(self.s, chains, _abi.ptr(x_d) if Nd else None, _abi.stream_ptr()))
        self.x_d = x_d if R is None else x_d.reshape(units, R, Nd)
        self._alloc_outputs(torch, dev, keep_samples)
        streams = self._streams()
        for name, _ in streams:
            setattr(self, name, None)
        if any(draws[name] is not None for name, _ in streams):
            given = []
            for name, shape in streams:
                a = np.zeros((total,) + shape) if draws[name] is None and self.ZERO_FILL_MISSING else draws[name]
                given.append(np.ascontiguousarray(a, dtype=np.float64))
            given = [a.reshape((len(a),) + shape) for a, (_, shape) in zip(given, streams)]
            if any(a.shape[0] < total for a in given if all(a.shape[1:])):          # (a stream with an empty row is not read)
                raise ValueError('fewer injected draws than %ss' % self.NOUNS[1])
            for a, (name, _) in zip(given, streams):
                setattr(self, name, _abi.to_dev(a) if a.size else _abi.to_dev(np.zeros(1)) if self.PLACEHOLDER else None)
        self.bad = torch.full((1,), -1, dtype=torch.int64, device=dev)          # UINT64_MAX
        self.done = 0

    def _device_bytes(self, keep_samples):
        """(the device bytes of the outputs, how the error names the run), or None for no check against the free memory"""
        raise NotImplementedError

    def _alloc_outputs(self, torch, dev, keep_samples):
        raise NotImplementedError

    def _streams(self):
        """((attribute, the shape of one iteration's row), ...) of the injected draws"""
        raise NotImplementedError

    def advance(self, end):
        """iterations [done, end) in one launch"""
        raise NotImplementedError

    def _bad_state(self, unit):
        """the discrete state an error names for a unit whose precision matrix was not positive definite"""
        return self.x_d[unit].cpu().numpy()

    def run(self, per_launch=None):
        step = self.PER_LAUNCH[1] if per_launch is None else int(per_launch)
        if step < 1:
            raise ValueError('%s must be positive' % self.PER_LAUNCH[0])
        while self.done < self.total:
            self.advance(min(self.total, self.done + step))
        self.check()
        return self

    def check(self):
        first = int(self.bad.item())
        if first != -1:
            unit = (first & (2 ** 64 - 1)) >> 32
            raise ValueError(_not_pd_message(self._bad_state(unit)) + ' (%s %d, %s %d)'
                             % (self.NOUNS[0], unit, self.NOUNS[1], first & 0xffffffff))


class _Chains(_Run):
    """`chains` chains on the device.  After ``run()``: x_d [chains, Nd], counts [chains, sum dstates], sum1 [chains, Nc],
    sum2 [chains, Nc (Nc + 1) / 2] and, with keep_samples, disc [chains, num_samples, Nd] / cont [chains, num_samples, Nc]
    as device tensors.  z / u: injected draws (host arrays [iters, chains, Nc] / [iters, chains, its, Nd]) for the tests;
    tables: 'lds' / 'global' forces where the reduced tables live (default: LDS when the workspace fits)."""

    LDS_BYTES = 'lhvi_gibbs_lds_bytes'

    def __init__(self, gm, chains, num_burnin, num_samples, disc_block_its, seed, keep_samples=False, lanes=None, init_x_d=None,
                 z=None, u=None, tables=None):
        chains, num_burnin, num_samples = int(chains), int(num_burnin), int(num_samples)
        if chains < 1 or num_burnin < 0 or num_samples < 0:
            raise ValueError('chains >= 1, num_burnin >= 0 and num_samples >= 0 are required')
        super().__init__(gm, chains, num_burnin + num_samples, disc_block_its, seed, lanes, tables, init_x_d, dict(z=z, u=u),
                         num_burnin, num_samples, keep_samples)

    def _device_bytes(self, keep_samples):
        return (output_bytes(self.gm, self.chains, self.num_samples, keep_samples),
                '%d chains of %d kept samples' % (self.chains, self.num_samples))

    def _alloc_outputs(self, torch, dev, keep_samples):
        gm, n, S = self.gm, self.chains, self.num_samples
        Nd, Nc = gm.ex.Nd, gm.ex.Nc
        f64, i32 = torch.float64, torch.int32
        self.counts = torch.zeros(n, gm.n_states, dtype=i32, device=dev)
        self.sum1 = torch.zeros(n, Nc, dtype=f64, device=dev)
        self.sum2 = torch.zeros(n, Nc * (Nc + 1) // 2, dtype=f64, device=dev)
        self.disc = torch.zeros(n, S, Nd, dtype=i32, device=dev) if keep_samples else None
        self.cont = torch.zeros(n, S, Nc, dtype=f64, device=dev) if keep_samples else None

    def _streams(self):
        return ('z', (self.chains, self.gm.ex.Nc)), ('u', (self.chains, self.its, self.gm.ex.Nd))

    def advance(self, it_end):
        p = _dev_ptr
        _abi.check(_abi.lib().lhvi_gibbs_run(self.s, self.chains, self.done, int(it_end), self.lanes, p(self.x_d), p(self.z),
                                             p(self.u), p(self.disc), p(self.cont), p(self.counts), p(self.sum1), p(self.sum2),
                                             _abi.ptr(self.bad), _abi.stream_ptr()))
        self.done = int(it_end)

    def rb_disc(self, s_begin=0, s_end=None, prob_sum=None, lanes=None):
        """prob_sum [chains, sum dstates] (device tensor, zeros when not given) += the conditional probabilities
        p(x_n = k | x_d,-n, x_c) of the kept samples [s_begin, s_end) of every chain (``lhvi_gibbs_rb_disc``), one launch.
        lanes: lanes per chain (default: the run's); the reduced tables live where the run's do.  Needs keep_samples."""
        if self.disc is None:
            raise RuntimeError('rb_disc needs the kept samples')
        torch = _abi._torch()
        if prob_sum is None:
            prob_sum = torch.zeros(self.chains, max(self.gm.n_states, 1), dtype=torch.float64, device=self.x_d.device)
        if prob_sum.shape != (self.chains, max(self.gm.n_states, 1)) or prob_sum.dtype != torch.float64 or not prob_sum.is_contiguous():
            raise ValueError('prob_sum must be a contiguous float64 tensor [chains, sum dstates]')
        _abi.check(_abi.lib().lhvi_gibbs_rb_disc(self.s, self.chains, int(s_begin), self.num_samples if s_end is None else int(s_end),
                                                 self.lanes if lanes is None else int(lanes), _dev_ptr(self.disc), _dev_ptr(self.cont),
                                                 _abi.ptr(prob_sum), _abi.stream_ptr()))
        return prob_sum


def _seed(seed):
    return int.from_bytes(os.urandom(8), 'little') if seed is None else int(seed)


def _sample(gm, num_burnin, num_samples, init_x_d, disc_block_its, seed, chains, lanes=None):
    """(disc [chains * num_samples, Nd] int64, cont [chains * num_samples, Nc], run): the kept samples, chain-major"""
    run = _Chains(gm, chains, num_burnin, num_samples, disc_block_its, _seed(seed), keep_samples=True, lanes=lanes,
                  init_x_d=init_x_d).run()
    n = run.chains * run.num_samples
    return run.disc.cpu().numpy().reshape(n, gm.ex.Nd).astype(np.int64), run.cont.cpu().numpy().reshape(n, gm.ex.Nc), run


# ---- the reference's functions -----------------------------------------------------------------------------------------------
def block_gibbs_sample(factors, Vd, Vc, num_burnin, num_samples, init_x_d=None, disc_block_its=100, seed=None, chains=1):
    """``hybrid_gaussian_mrf.block_gibbs_sample`` (:145-265): (disc_samples [num_samples, Nd] int, cont_samples
    [num_samples, Nc]).  Reads ``factor.log_potential_fun`` and ``factor.disc_nb_idx / cont_nb_idx`` like ``convert_to_bn``.
    chains > 1: that many independent chains, their kept samples concatenated chain-major ([chains * num_samples, ...])."""
    gm = GibbsModel(flatten_factors(factors, [rv.dstates for rv in Vd], len(Vc)))
    disc, cont, _ = _sample(gm, num_burnin, num_samples, init_x_d, disc_block_its, seed, chains)
    return disc, cont


_LOG_PARTITION_DOC = """Annealed importance sampling (Neal 2001) along ``p~^beta f0^(1 - beta)`` from the base
    ``f0 = exp(-base_prec / 2 |x_c - base_mean|^2)`` (x_d uniform) with x_c integrated out in closed form (docs/kernels_ais.md):
    ``chains`` independent runs of ``steps`` steps (``betas``: a schedule of its own from 0 to 1, never decreasing; default
    ``linspace(0, 1, steps + 1)``), each step followed by one block Gibbs transition with ``disc_block_its`` sweeps.  Returns a
    record: ``logZ`` (log of the mean weight), ``stderr`` (delta method), ``ess`` (effective sample fraction), ``lower``
    (log Z0 + mean log weight: its expectation is at most log Z, the number to hold against an ELBO) with ``lower_stderr``,
    ``obj`` = -logZ, and the device tensors ``log_weights`` [chains] and ``x_d`` [chains, Nd] (the final states).  A poor base
    raises the variance of the weights and never biases the estimate of Z."""


def ais_log_partition(factors, Vd, Vc, chains=4096, steps=256, betas=None, disc_block_its=1, seed=0, base_mean=None,
                      base_prec=None, lanes=None, steps_per_launch=None):
    """``log Z`` of the hybrid Gaussian MRF that ``block_gibbs_sample`` samples (same reading of the factors).  Base mean 0 and
    precision 1 unless given."""
    from . import ais
    gm = GibbsModel(flatten_factors(factors, [rv.dstates for rv in Vd], len(Vc)))
    return ais.log_partition(gm, chains, steps, betas, disc_block_its, seed, base_mean, base_prec, lanes, steps_per_launch)


ais_log_partition.__doc__ += '\n\n    ' + _LOG_PARTITION_DOC


_TEMPERED_DOC = """Parallel tempering (docs/kernels_pt.md): ``ladders`` independent ladders of replicas at ``betas`` (never
    decreasing, not negative, the last one 1; default ``linspace(0, 1, replicas)``) along ``p~^beta f0^(1 - beta)`` with the base
    ``f0 = exp(-base_prec / 2 |x_c - base_mean|^2)`` (x_d uniform).  Every replica makes one block Gibbs transition per iteration
    with ``disc_block_its`` sweeps; every ``swap_every`` iterations (0: never) adjacent replicas, even and odd pairs in turn,
    propose to exchange their discrete states.  Only the ``beta = 1`` replica is kept, before the swap."""


def tempered_gibbs_sample(factors, Vd, Vc, num_burnin, num_samples, betas=None, replicas=8, ladders=1, disc_block_its=1, swap_every=1,
                          seed=None, base_mean=None, base_prec=None, lanes=None, its_per_launch=None):
    """what ``block_gibbs_sample`` returns, from the ``beta = 1`` replicas of ``ladders`` ladders, ladder-major
    ([ladders * num_samples, ...]).  Base mean 0 and precision 1 unless given."""
    from . import pt
    gm = GibbsModel(flatten_factors(factors, [rv.dstates for rv in Vd], len(Vc)))
    run = pt.run(gm, ladders, replicas, betas, num_burnin, num_samples, disc_block_its, swap_every, seed, True, lanes, its_per_launch,
                 base_mean, base_prec)
    n = run.chains * run.num_samples
    return run.disc.cpu().numpy().reshape(n, gm.ex.Nd).astype(np.int64), run.cont.cpu().numpy().reshape(n, gm.ex.Nc)


tempered_gibbs_sample.__doc__ += '\n\n    ' + _TEMPERED_DOC


def get_disc_marg_table_from_samples(samples, dstates):
    """``sampling_utils.get_disc_marg_table_from_samples``: the joint relative frequencies [v1..vN] of samples [S, N]"""
    samples = np.asarray(samples)
    counts = np.zeros(list(dstates), dtype=np.int64)
    np.add.at(counts, tuple(samples[:, n] for n in range(samples.shape[1])), 1)
    return counts / samples.shape[0]


def fit_scalar_gm_from_samples(samples, K):
    """``sampling_utils.fit_scalar_gm_from_samples``: (weights, means, variances) of a K-component mixture fitted by
    scikit-learn"""
    from sklearn import mixture
    clf = mixture.GaussianMixture(n_components=K, covariance_type='diag')
    clf.fit(np.asarray(samples, dtype=np.float64).reshape(-1, 1))
    return clf.weights_, np.ravel(clf.means_), np.ravel(clf.covariances_)


def fit_scalar_gms_from_samples(samples, K, **fit_args):
    """the batched sibling of ``fit_scalar_gm_from_samples``: a K-component mixture fitted to every column of ``samples``
    [S, N] (an array or a device tensor, laid out like the reference's ``cont_samples``) in one launch.  Returns the
    ``gmfit.ScalarMixtures`` of the N columns; ``fit_args``: the keywords of ``gmfit.fit_scalar_gms``."""
    from .gmfit import fit_scalar_gms
    if isinstance(samples, np.ndarray) or not hasattr(samples, 'data_ptr'):
        samples = np.asarray(samples, dtype=np.float64)
        if samples.ndim != 2:
            raise ValueError('samples must be [S, N]')
        return fit_scalar_gms(np.ascontiguousarray(samples.T), K, **fit_args)
    if samples.dim() != 2:
        raise ValueError('samples must be [S, N]')
    return fit_scalar_gms(samples.t().contiguous(), K, **fit_args)


class HybridGaussianSampler:
    """``hybrid_gaussian_mrf.HybridGaussianSampler`` (:268-302)"""

    def __init__(self, factors, Vd, Vc, Vd_idx, Vc_idx):
        self.factors, self.Vd, self.Vc, self.Vd_idx, self.Vc_idx = factors, Vd, Vc, Vd_idx, Vc_idx
        self.dstates = [rv.dstates for rv in Vd]

    def block_gibbs_sample(self, num_burnin, num_samples, init_x_d=None, disc_block_its=100, seed=None, chains=1):
        self.disc_samples, self.cont_samples = block_gibbs_sample(self.factors, self.Vd, self.Vc, num_burnin, num_samples,
                                                                  init_x_d, disc_block_its, seed, chains=chains)
        self.sampled_disc_marginal_table = get_disc_marg_table_from_samples(self.disc_samples, self.dstates)

    def tempered_gibbs_sample(self, num_burnin, num_samples, betas=None, replicas=8, ladders=1, disc_block_its=1, swap_every=1,
                              seed=None, base_mean=None, base_prec=None, lanes=None, its_per_launch=None):
        """``block_gibbs_sample`` by parallel tempering: sets ``disc_samples``, ``cont_samples`` and
        ``sampled_disc_marginal_table`` from the ``beta = 1`` replicas."""
        self.disc_samples, self.cont_samples = tempered_gibbs_sample(self.factors, self.Vd, self.Vc, num_burnin, num_samples, betas,
                                                                     replicas, ladders, disc_block_its, swap_every, seed, base_mean,
                                                                     base_prec, lanes, its_per_launch)
        self.sampled_disc_marginal_table = get_disc_marg_table_from_samples(self.disc_samples, self.dstates)

    tempered_gibbs_sample.__doc__ += '\n\n        ' + _TEMPERED_DOC

    def map(self, rv, num_gm_components_for_crv=1):
        """discrete: the argmax of the variable's sampled marginal (the reference's line :296 passes ``Vd_idx`` where an index
        belongs and cannot run).  Continuous: the mode of a K-component mixture fitted to the samples; K = 1 is the sample
        mean clipped to the domain."""
        from .exact import get_drv_marg_map, get_rv_marg_map_from_bn_params
        if rv in self.Vd_idx:
            return get_drv_marg_map(self.sampled_disc_marginal_table, self.Vd_idx[rv])
        x = self.cont_samples[:, self.Vc_idx[rv]]
        if num_gm_components_for_crv == 1:
            return float(min(max(x.mean(), rv.values[0]), rv.values[1]))
        w, mu, var = fit_scalar_gm_from_samples(x, num_gm_components_for_crv)
        return get_rv_marg_map_from_bn_params(w, mu[:, None], var[:, None, None], {}, {rv: 0}, rv)

    def log_partition(self, chains=4096, steps=256, betas=None, disc_block_its=1, seed=0, base_mean=None, base_prec=None,
                      lanes=None, steps_per_launch=None):
        """``ais_log_partition`` of the sampler's model (the reference leaves ``obj = -logZ`` of its Gibbs baseline as a TODO,
        ``osi/hybrid_mln_experiment.py:304``).  After ``block_gibbs_sample`` the base defaults to the sample means and the
        reciprocal of the mean sample variance of ``cont_samples``; before it, to mean 0 and precision 1."""
        cont = getattr(self, 'cont_samples', None)
        if cont is not None and len(self.Vc) and len(cont) > 1:
            cont = np.asarray(cont, dtype=np.float64)
            base_mean = cont.mean(axis=0) if base_mean is None else base_mean
            base_prec = 1.0 / float(cont.var(axis=0).mean()) if base_prec is None else base_prec
        return ais_log_partition(self.factors, self.Vd, self.Vc, chains, steps, betas, disc_block_its, seed, base_mean, base_prec,
                                 lanes, steps_per_launch)

    log_partition.__doc__ += '\n\n        ' + _LOG_PARTITION_DOC

    def joint_map(self):
        """the sample of largest joint log potential among ``disc_samples`` / ``cont_samples`` (the reference leaves this as a
        TODO, ``osi/hybrid_mln_experiment.py:306``): the host arrays go to the device, one launch evaluates every sample, the
        first one wins on ties.  A dict: config (state indices), xd (domain values), xc, energy, sample (its row)."""
        model = flatten_factors(self.factors, self.dstates, len(self.Vc))
        disc = np.asarray(self.disc_samples)
        _check_states('disc_samples', disc, self.dstates)
        t = _abi.upload({n: (a if a.size else np.zeros(1, dtype=a.dtype)) for n, a in ((n, getattr(model, n)) for n in ExactModel.FIELDS)})
        e = hg_energy.energies(model.struct(lambda n: _abi.ptr(t[n])), x_d=_abi.to_dev(disc.astype(np.int32)),
                               x_c=_abi.to_dev(np.asarray(self.cont_samples, dtype=np.float64)))
        index, value = hg_energy.argmax_first(e)
        row = int(index.item())
        if row < 0:
            raise ValueError('no sample has a finite energy')
        config = tuple(int(k) for k in disc[row])
        return dict(config=config, xd=tuple(rv.domain.values[k] for rv, k in zip(self.Vd, config)),
                    xc=np.array(self.cont_samples[row], dtype=np.float64), energy=float(value.item()), sample=row)


def gibbs_sample(lpot_tables, scopes, nbr_factor_ids, dstates, x, num_burnin, num_samples, seed=None, chains=1):
    """``disc_mrf.gibbs_sample``: samples [num_samples, N] of a discrete MRF of log tables, one sweep per sample, from the
    state x (which ends as the last state when chains = 1, like the reference's).  nbr_factor_ids is checked against the
    scopes; the kernel adds a variable's tables in factor order."""
    N = len(dstates)
    for n in range(N):
        if sorted(nbr_factor_ids[n]) != [j for j, sc in enumerate(scopes) if n in sc]:
            raise ValueError('nbr_factor_ids[%d] does not list the factors whose scope holds variable %d' % (n, n))
    factors = [_Factor('table %d' % j, LogTable(np.asarray(t, dtype=np.float64)), tuple(int(i) for i in sc), ())
               for j, (t, sc) in enumerate(zip(lpot_tables, scopes))]
    gm = GibbsModel(flatten_factors(factors, list(dstates), 0))
    disc, _, run = _sample(gm, num_burnin, num_samples, np.asarray(x), 1, seed, chains)
    if chains == 1 and isinstance(x, np.ndarray):
        x[:] = run.x_d[0].cpu().numpy()
    return disc


# ---- the solver-shaped class ---------------------------------------------------------------------------------------------------
class GibbsHybridGaussian:
    """Sampled marginals of a hybrid Gaussian MRF from many independent block Gibbs chains.  ``GibbsHybridGaussian(g)`` or
    ``GibbsHybridGaussian(factors=, Vd=, Vc=)``; variables with ``rv.value`` set are evidence, potentials are converted as in
    ``ExactHybridGaussian``.  After ``run()``: ``disc_marginals()``, ``moments()``, ``rhat()``, ``map`` / ``map_all`` /
    ``belief``, and with ``keep_samples`` ``disc_samples`` [chains, num_samples, Nd] / ``cont_samples`` and
    ``fit_marginals(K)``: the mixtures of the continuous variables fitted to the kept samples on the device,
    ``sample_energies()`` / ``joint_map()``: the joint log potential of every kept sample and the best of them, and the
    Rao-Blackwellised estimates ``rb_marginals()`` / ``rb_disc_marginals()`` / ``rb_moments()`` and ``map`` / ``map_all`` /
    ``belief`` with ``rao_blackwell=True``: the exact conditionals p(x_c | x_d) and p(x_n | x_d,-n, x_c) averaged over the kept
    samples (docs/kernels_gibbs_rb.md)."""

    def __init__(self, g=None, factors=None, Vd=None, Vc=None):
        if g is None and (factors is None or Vd is None or Vc is None):
            raise ValueError('GibbsHybridGaussian needs a graph, or factors=, Vd= and Vc=')
        ex = ExactHybridGaussian(g=g, factors=factors, Vd=Vd, Vc=Vc)           # the flattening, evidence included
        self.rvs, self.Vd, self.Vc, self.Vd_idx, self.Vc_idx = ex.rvs, ex.Vd, ex.Vc, ex.Vd_idx, ex.Vc_idx
        self.dstates, self.factors, self.log_const = ex.dstates, ex.factors, ex.log_const
        self.model = GibbsModel(ex.model)
        self._run = None
        self.marginals, self._fits = None, {}
        self.rb, self._rb_prob, self._rb_run, self._rb_maps = None, None, None, None

    def run(self, chains=1024, num_burnin=100, num_samples=100, disc_block_its=100, seed=0, keep_samples=False, lanes=None,
            its_per_launch=None, init_x_d=None):
        if num_samples < 1:
            raise ValueError('num_samples must be positive')
        return self._adopt(_Chains(self.model, chains, num_burnin, num_samples, disc_block_its, _seed(seed), keep_samples, lanes,
                                   init_x_d=init_x_d).run(its_per_launch), keep_samples)

    def _adopt(self, r, keep_samples):
        """the state a finished run leaves"""
        self._run = r
        self.chains, self.num_samples = r.chains, r.num_samples
        self.marginals, self._fits = None, {}           # fits of an earlier run's samples
        self._energies = None
        self.rb, self._rb_prob, self._rb_run, self._rb_maps = None, None, None, None
        self.counts = r.counts.cpu().numpy()
        self.sum1, self.sum2 = r.sum1.cpu().numpy(), r.sum2.cpu().numpy()
        self.disc_samples = r.disc.cpu().numpy() if keep_samples else None
        self.cont_samples = r.cont.cpu().numpy() if keep_samples else None
        return self

    def run_tempered(self, ladders=1024, replicas=8, betas=None, num_burnin=100, num_samples=100, disc_block_its=1, swap_every=1,
                     seed=0, keep_samples=False, lanes=None, its_per_launch=None, base_mean=None, base_prec=None):
        """``run()`` by parallel tempering: afterwards the object is in the state ``run(chains=ladders)`` leaves, filled from the
        ``beta = 1`` replica of every ladder, so every read-out works unchanged; ``swap_rates()`` / ``swap_counts()`` say how the
        ladder exchanged.  The base defaults to ``log_partition``'s: the moments of an earlier run, else mean 0 and precision 1."""
        from . import pt
        if num_samples < 1:
            raise ValueError('num_samples must be positive')
        base_mean, base_prec = self._default_base(base_mean, base_prec)
        return self._adopt(pt.run(self.model, ladders, replicas, betas, num_burnin, num_samples, disc_block_its, swap_every, seed,
                                  keep_samples, lanes, its_per_launch, base_mean, base_prec), keep_samples)

    run_tempered.__doc__ += '\n\n        ' + _TEMPERED_DOC

    def swap_counts(self):
        """(tried [R - 1], accepted [R - 1]): the swaps of every adjacent pair of replicas summed over the ladders of the last
        ``run_tempered``"""
        r = self._need_run()
        if not hasattr(r, 'swap_try'):
            raise RuntimeError('swap_counts needs run_tempered()')
        return r.swap_counts()

    def swap_rates(self):
        """[R - 1]: the accepted fraction of the proposed swaps per adjacent pair (NaN where none was proposed)"""
        tried, acc = self.swap_counts()
        with np.errstate(divide='ignore', invalid='ignore'):
            return acc / tried.astype(np.float64)

    def _default_base(self, base_mean, base_prec):
        """after a run the base defaults to ``moments()``: the sample means and the reciprocal of the mean marginal variance"""
        Nc = len(self.Vc)
        if self._run is not None and Nc and (base_mean is None or base_prec is None):
            mo = self.moments()
            var = float(np.diag(mo.cov).mean())
            base_mean = mo.mean if base_mean is None else base_mean
            if base_prec is None and var > 0.0 and np.isfinite(var):
                base_prec = 1.0 / var
        return base_mean, base_prec

    def _need_run(self):
        if self._run is None:
            raise RuntimeError('call run() first')
        return self._run

    def _stderr(self, per_chain):
        if self.chains < 2:
            return np.full(per_chain.shape[1:], np.nan)
        return per_chain.std(axis=0, ddof=1) / np.sqrt(self.chains)

    def disc_marginals(self):
        """per discrete variable (marginal [states], standard error [states]): the grand mean of the chains' relative
        frequencies and the standard error of that mean over chains"""
        self._need_run()
        freq = self.counts / float(self.num_samples)
        mean, se = freq.mean(axis=0), self._stderr(freq)
        off = self.model.dstate_off
        return [(mean[off[i]:off[i + 1]], se[off[i]:off[i + 1]]) for i in range(len(self.Vd))]

    def moments(self):
        """namespace: mean [Nc] = E[x_c], second [Nc, Nc] = E[x_c x_c^T], cov = second - mean mean^T, and the standard errors
        over chains mean_se, second_se"""
        self._need_run()
        Nc = len(self.Vc)
        i, j = np.tril_indices(Nc)
        m1, m2 = self.sum1 / float(self.num_samples), self.sum2 / float(self.num_samples)

        def full(v):
            out = np.zeros((Nc, Nc))
            out[i, j] = out[j, i] = v
            return out
        mean, second = m1.mean(axis=0), full(m2.mean(axis=0))
        return types.SimpleNamespace(mean=mean, second=second, cov=second - np.outer(mean, mean), mean_se=self._stderr(m1),
                                     second_se=full(self._stderr(m2)))

    def rhat(self):
        """Gelman-Rubin potential scale reduction from the per-chain accumulators: namespace disc (list of [states] arrays, one
        per discrete variable: the state's indicator), cont [Nc], max (NaN entries, a state no chain left or entered, skipped)"""
        self._need_run()
        S, Nc = float(self.num_samples), len(self.Vc)
        if self.chains < 2 or S < 2:
            raise ValueError('rhat needs at least two chains and two kept samples')

        def psr(means, within):
            W = within.mean(axis=0)
            B_over_n = means.var(axis=0, ddof=1)
            with np.errstate(divide='ignore', invalid='ignore'):
                return np.sqrt(((S - 1) / S * W + B_over_n) / W)
        p = self.counts / S
        rd = psr(p, p * (1 - p) * S / (S - 1))
        diag = np.arange(Nc) * (np.arange(Nc) + 1) // 2 + np.arange(Nc)
        m1 = self.sum1 / S
        rc = psr(m1, (self.sum2[:, diag] / S - m1 * m1) * S / (S - 1))
        off = self.model.dstate_off
        both = np.concatenate([rd, rc])
        return types.SimpleNamespace(disc=[rd[off[i]:off[i + 1]] for i in range(len(self.Vd))], cont=rc,
                                     max=float(np.nanmax(both)) if both.size and not np.isnan(both).all() else float('nan'))

    def fit_marginals(self, K, **fit_args):
        """Fit a K-component Gaussian mixture to the kept samples of every continuous variable in one launch
        (``gmfit.fit_scalar_gms`` on the device tensor of the samples, transposed to [Nc, chains * num_samples]: they do not
        visit the host).  Returns the ``gmfit.ScalarMixtures`` in ``Vc`` order and keeps it as ``self.marginals``, which
        ``belief`` of a continuous variable reads.  Needs ``run(keep_samples=True)``."""
        from .gmfit import fit_scalar_gms
        r = self._need_run()
        if r.cont is None:
            raise RuntimeError('fit_marginals needs the kept samples: call run(keep_samples=True)')
        Nc = len(self.Vc)
        if Nc == 0:
            raise ValueError('the model has no continuous variable')
        x = r.cont.reshape(r.chains * r.num_samples, Nc).t().contiguous()
        self.marginals = fit_scalar_gms(x, K, **fit_args)
        if not fit_args:
            self._fits[int(K)] = self.marginals
        return self.marginals

    # ---- Rao-Blackwellised estimates (docs/kernels_gibbs_rb.md) ---------------------------------------------------------------
    def _need_samples(self, what):
        r = self._need_run()
        if r.disc is None:
            raise RuntimeError('%s needs the kept samples: call run(keep_samples=True)' % what)
        return r

    def rb_marginals(self, chunk=None):
        """The Rao-Blackwellised marginals of the continuous variables: ``p(x_i) ~ (1 / S) sum_s N(x_i; mu_i(x_d^s),
        Sig_ii(x_d^s))`` over the kept discrete samples, with no K and no EM.  The distinct rows of the kept ``disc`` samples
        (``torch.unique`` on the device tensor, lexicographic order) go through ``lhvi_exact_configs_at``; a component per distinct
        row, its weight the row's share of the samples.  Returns the ``gmfit.ScalarMixtures`` [Nc, U] in ``Vc`` order, the shape
        of ``ExactHybridGaussian.marginals()``, and keeps ``self.rb``: a namespace of rows [U, Nd], counts [U], inverse
        [chains, num_samples], means / vars [U, Nc] (device tensors) and mixtures.  ``self.marginals`` (the fitted mixtures) is
        left alone.  Needs ``run(keep_samples=True)``."""
        from .gmfit import ScalarMixtures
        r = self._need_samples('rb_marginals')
        Nd, Nc = len(self.Vd), len(self.Vc)
        if Nc == 0:
            raise ValueError('the model has no continuous variable')
        torch = _abi._torch()
        total = r.chains * r.num_samples
        if Nd:
            rows, inverse, counts = torch.unique(r.disc.reshape(total, Nd), dim=0, return_inverse=True, return_counts=True)
        else:
            dev = r.disc.device
            rows = torch.zeros(1, 0, dtype=torch.int32, device=dev)
            inverse = torch.zeros(total, dtype=torch.int64, device=dev)
            counts = torch.full((1,), total, dtype=torch.int64, device=dev)
        rows = rows.to(torch.int32).contiguous()
        _, means, vars_ = _exact.configs_at(self.model.ex, r.s.ex, rows, chunk=_exact.CHUNK if chunk is None else chunk)
        U = int(rows.shape[0])
        weights = counts.to(torch.float64) / float(total)
        mixtures = ScalarMixtures(weights[None, :].expand(Nc, U), means.t(), vars_.t())
        self.rb = types.SimpleNamespace(rows=rows, counts=counts, inverse=inverse.reshape(r.chains, r.num_samples), means=means,
                                        vars=vars_, weights=weights, mixtures=mixtures)
        self._rb_run = self._rb_maps = None
        return mixtures

    def _rb_probs(self):
        """[chains, sum dstates] host array: per chain the mean over its kept samples of p(x_n = k | x_d,-n, x_c)
        (``lhvi_gibbs_rb_disc``, one launch over all chains; computed once per run)"""
        r = self._need_samples('rb_disc_marginals')
        if self._rb_prob is None:
            self._rb_prob = r.rb_disc().cpu().numpy()[:, :self.model.n_states] / float(r.num_samples)
        return self._rb_prob

    def rb_disc_marginals(self):
        """``disc_marginals()`` with the state counts replaced by the conditional probabilities
        ``p(x_n = k | x_d,-n, x_c)`` averaged over the kept samples: per discrete variable (marginal [states], standard error over
        chains [states]).  Needs ``run(keep_samples=True)``."""
        prob = self._rb_probs()
        mean, se = prob.mean(axis=0), self._stderr(prob)
        off = self.model.dstate_off
        return [(mean[off[i]:off[i + 1]], se[off[i]:off[i + 1]]) for i in range(len(self.Vd))]

    def rb_moments(self):
        """namespace: mean [Nc] = E[x_c] and second_diag [Nc] = E[x_i^2] from the conditional means and variances of the kept
        discrete samples (the per-chain means of ``rb.means[inverse]`` and of ``(rb.vars + rb.means^2)[inverse]``), and their
        standard errors over chains mean_se, second_diag_se.  Cross moments stay with ``moments()``.  Needs
        ``run(keep_samples=True)``; calls ``rb_marginals()`` when it has not run."""
        self._need_samples('rb_moments')
        if self.rb is None:
            self.rb_marginals()
        rb = self.rb
        m1 = rb.means[rb.inverse].mean(dim=1).cpu().numpy()
        m2 = (rb.vars + rb.means * rb.means)[rb.inverse].mean(dim=1).cpu().numpy()
        return types.SimpleNamespace(mean=m1.mean(axis=0), second_diag=m2.mean(axis=0), mean_se=self._stderr(m1),
                                     second_diag_se=self._stderr(m2))

    def _rb_mixture_run(self):
        """the Rao-Blackwellised mixtures behind the exact baseline's mixture kernels (lhvi_exact_mix_prepare / _mixture /
        _map_polish)"""
        self._need_samples('the Rao-Blackwellised mixture')
        if self.rb is None:
            self.rb_marginals()
        if self._rb_run is None:
            self._rb_run = _exact.mixture_run(self.rb.weights, self.rb.means, self.rb.vars)
        return self._rb_run

    def _rb_cont_maps(self):
        if self._rb_maps is None:
            bds = self._bds()
            x, lf = self._rb_mixture_run().cont_map(bds[0], bds[1])
            self._rb_maps = (x.cpu().numpy(), lf.cpu().numpy())
        return self._rb_maps

    def sample_energies(self):
        """[chains, num_samples] device tensor: the joint log potential of every kept sample with the evidence in place
        (``log_const`` included, like ``ExactHybridGaussian.config_energies``), one launch over all of them.  Needs
        ``run(keep_samples=True)``."""
        r = self._need_run()
        if r.disc is None:
            raise RuntimeError('sample_energies needs the kept samples: call run(keep_samples=True)')
        if self._energies is None:
            S, Nd, Nc = r.chains * r.num_samples, len(self.Vd), len(self.Vc)
            e = hg_energy.energies(r.s.ex, x_d=r.disc.reshape(S, Nd), x_c=r.cont.reshape(S, Nc))
            self._energies = (e + self.log_const).reshape(r.chains, r.num_samples)
        return self._energies

    def joint_map(self):
        """the kept sample of largest joint log potential, the first in chain-major order on ties: the dict of
        ``ExactHybridGaussian.joint_map`` (index: the flat configuration index, None when the configurations cannot be
        numbered) plus chain and sample.  Only the winner's row is downloaded.  Needs ``run(keep_samples=True)``."""
        r = self._need_run()
        if r.disc is None:
            raise RuntimeError('joint_map needs the kept samples: call run(keep_samples=True)')
        index, value = hg_energy.argmax_first(self.sample_energies().reshape(-1))
        row = int(index.item())
        if row < 0:
            raise ValueError('no sample has a finite energy')
        chain, sample = divmod(row, r.num_samples)
        config = tuple(int(k) for k in r.disc[chain, sample].cpu().numpy())
        ex = self.model.ex
        flat = int(np.dot(np.asarray(config, dtype=object), ex.dstride.astype(object))) if ex.M else None
        return joint_map_dict(self, config, flat, r.cont[chain, sample].cpu().numpy(), float(value.item()), chain=chain,
                              sample=sample)

    def log_partition(self, chains=4096, steps=256, betas=None, disc_block_its=1, seed=0, base_mean=None, base_prec=None,
                      lanes=None, steps_per_launch=None):
        """``log Z`` of the model with the evidence in place (``log_const`` included): comparable with
        ``ExactHybridGaussian.logZ`` on the same evidence, and ``obj`` = -logZ is the column the reference's Gibbs baseline
        leaves empty.  Needs no ``run()``; after one, the base defaults to ``moments()``: the sample means and the reciprocal of
        the mean marginal variance.  Before it, to mean 0 and precision 1."""
        from . import ais
        base_mean, base_prec = self._default_base(base_mean, base_prec)
        return ais.log_partition(self.model, chains, steps, betas, disc_block_its, seed, base_mean, base_prec, lanes,
                                 steps_per_launch, log_const=self.log_const)

    log_partition.__doc__ += '\n\n        ' + _LOG_PARTITION_DOC

    def _bds(self):
        return np.array([[rv.domain.values[0] for rv in self.Vc], [rv.domain.values[1] for rv in self.Vc]], dtype=np.float64)

    def map(self, rv, num_gm_components_for_crv=1, rao_blackwell=False):
        """observed: its value; discrete: the state of largest sampled marginal; continuous: the sample mean clipped to the
        domain (the one-component fit of ``HybridGaussianSampler.map``) or, with ``num_gm_components_for_crv`` = K > 1, the
        mode inside the domain of the K-component mixture fitted to the kept samples on the device (``fit_marginals(K)``
        with its defaults, fitted once for all variables).  ``rao_blackwell``: the state of largest ``rb_disc_marginals()``; the
        mode inside the domain of the variable's Rao-Blackwellised mixture, by the exact baseline's candidate selection and
        Newton polish (K is not read)."""
        if rv.value is not None:
            return rv.value
        self._need_run()
        if rao_blackwell:
            if rv in self.Vd_idx:
                return rv.domain.values[int(np.argmax(self.rb_disc_marginals()[self.Vd_idx[rv]][0]))]
            return float(self._rb_cont_maps()[0][self.Vc_idx[rv]])
        if rv in self.Vd_idx:
            return rv.domain.values[int(np.argmax(self.disc_marginals()[self.Vd_idx[rv]][0]))]
        K = int(num_gm_components_for_crv)
        if K > 1:
            fit = self._fits[K] if K in self._fits else self.fit_marginals(K)
            return float(fit.modes(self._bds())[0][self.Vc_idx[rv]])
        mean = float(self.moments().mean[self.Vc_idx[rv]])
        return float(min(max(mean, rv.domain.values[0]), rv.domain.values[1]))

    def map_all(self, num_gm_components_for_crv=1, rao_blackwell=False):
        """``map`` of every variable of ``self.rvs`` as an array"""
        return np.array([float(self.map(rv, num_gm_components_for_crv, rao_blackwell)) for rv in self.rvs])

    def belief(self, x, rv, rao_blackwell=False):
        """sampled marginal probability of the state x of a discrete variable; for a continuous variable the density at x
        (a number or an array) of its mixture of the last ``fit_marginals`` call.  ``rao_blackwell``: the probability from
        ``rb_disc_marginals()``; the density of the variable's Rao-Blackwellised mixture (``lhvi_exact_mixture``)."""
        if rv.value is not None:
            return 1 if x == rv.value else 0
        self._need_run()
        if rao_blackwell:
            if rv in self.Vd_idx:
                vals = list(rv.domain.values)
                return float(self.rb_disc_marginals()[self.Vd_idx[rv]][0][vals.index(x)]) if x in vals else 0.0
            torch = _abi._torch()
            run = self._rb_mixture_run()
            xs = np.asarray(x, dtype=np.float64)
            pts = torch.zeros(len(self.Vc), xs.size, dtype=torch.float64, device=run.table.device)
            pts[self.Vc_idx[rv]] = _abi.to_dev(np.ascontiguousarray(xs.reshape(-1)))
            out = np.exp(run.mixture(pts)[self.Vc_idx[rv], :, 0].cpu().numpy()).reshape(xs.shape)
            return float(out) if xs.ndim == 0 else out
        if rv not in self.Vd_idx:
            if self.marginals is None:
                raise NotImplementedError('belief of a continuous variable is the density of its fitted mixture: call '
                                          'fit_marginals(K) first (or see moments())')
            xs = np.asarray(x, dtype=np.float64)
            out = self.marginals.pdf(xs.reshape(1, -1), rows=[self.Vc_idx[rv]])
            out = (out if isinstance(out, np.ndarray) else out.cpu().numpy()).reshape(xs.shape)
            return float(out) if xs.ndim == 0 else out
        vals = list(rv.domain.values)
        return float(self.disc_marginals()[self.Vd_idx[rv]][0][vals.index(x)]) if x in vals else 0.0
