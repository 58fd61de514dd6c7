"""Single-site Gibbs / slice sampling on any ground ``FlatGraph``: the sampled baseline for models the block sampler of
``lhvi/gibbs.py`` cannot take (any potential kind with a device encoding, any number of continuous variables).

``FlatGibbs(g).run(...)`` runs many independent chains on the device (``csrc/fgibbs.hip``): hidden discrete variables are drawn
from their exact conditional, hidden continuous ones by slice sampling with shrinkage inside their domain interval, the
variables of one colour of ``colour_variables`` in one launch.  ``HostChains`` / ``chain_host`` run the same code on the host,
one chain at a time in the sequential order (``lhvi_fgibbs_chain_host``).  docs/kernels_fgibbs.md has the semantics, the
layout of the draws and what single-site Gibbs cannot do (hard factors, strongly coupled Gaussians).
"""
from __future__ import annotations

import ctypes as C
import os
import types

import numpy as np

from . import _abi
from .flat import flatten
from .potentials import POT_GENERIC, POT_TABLE

MAX_STATES = _abi.FGIBBS_MAX_STATES
MAX_SHRINK = 510            # the draw pair index rides in the top byte of a Philox counter word
MAX_CHAINS = 1 << 24
TAG_SWEEP, TAG_INIT = 0x46475355, 0x46475849       # "FGSU", "FGXI"


# ---- schedule -------------------------------------------------------------------------------------------------------------------
def conflict_graph(flat):
    """(ptr [V + 1], nbr): per hidden variable the other hidden variables it shares a factor with, ascending, each once"""
    V = flat.V
    hid = np.isnan(flat.var_value)
    fp = flat.fac_ptr.astype(np.int64)
    arity = np.diff(fp)
    us, ws = [], []
    amax = int(arity.max()) if arity.size else 0
    for a in range(amax):
        for b in range(amax):
            if a == b:
                continue
            f = np.flatnonzero(arity > max(a, b))
            u, w = flat.edge_var[fp[f] + a], flat.edge_var[fp[f] + b]
            keep = hid[u] & hid[w] & (u != w)
            us.append(u[keep].astype(np.int64))
            ws.append(w[keep].astype(np.int64))
    if us:
        key = np.unique(np.concatenate(us) * max(V, 1) + np.concatenate(ws))
        u, w = key // max(V, 1), key % max(V, 1)
    else:
        u = w = np.zeros(0, dtype=np.int64)
    ptr = np.zeros(V + 1, dtype=np.int64)
    np.cumsum(np.bincount(u, minlength=V), out=ptr[1:])
    return ptr, w


def colour_variables(flat):
    """(colour [V] int32, n_colours): greedy colouring of the hidden variables in variable order -- a variable takes the smallest
    colour none of its earlier conflict neighbours holds, so no factor has two hidden variables of one colour and
    n_colours <= 1 + the largest conflict degree.  Observed variables: -1.  Pure host function."""
    flat = flatten(flat)
    ptr, nbr = conflict_graph(flat)
    colour = np.full(flat.V, -1, dtype=np.int32)
    hidden = np.flatnonzero(np.isnan(flat.var_value))
    deg = np.diff(ptr)
    # variables without a conflict take colour 0 at once; the others in order, each a small array operation
    colour[hidden[deg[hidden] == 0]] = 0
    for v in hidden[deg[hidden] > 0]:
        used = colour[nbr[ptr[v]:ptr[v + 1]]]
        used = used[used >= 0]
        if used.size == 0:
            colour[v] = 0
            continue
        seen = np.zeros(used.size + 1, dtype=bool)
        seen[used[used <= used.size]] = True
        colour[v] = int(np.argmin(seen))
    return colour, int(colour.max() + 1) if hidden.size else 0


def work_lists(flat, colour, n_colours, hub_degree):
    """(col_ptr, col_var, hub_ptr, hub_var): the hidden variables colour by colour in ascending id, and per colour those with
    more than hub_degree incident edges"""
    hidden = np.flatnonzero(colour >= 0)
    order = hidden[np.argsort(colour[hidden], kind='stable')]
    col_ptr = np.zeros(n_colours + 1, dtype=np.int32)
    np.cumsum(np.bincount(colour[hidden], minlength=n_colours), out=col_ptr[1:])
    deg = np.diff(flat.var_ptr)
    hubs = order[deg[order] > hub_degree]
    hub_ptr = np.zeros(n_colours + 1, dtype=np.int32)
    np.cumsum(np.bincount(colour[hubs], minlength=n_colours), out=hub_ptr[1:])
    return col_ptr, order.astype(np.int32), hub_ptr, hubs.astype(np.int32)


# ---- a run ----------------------------------------------------------------------------------------------------------------------
def _np_ptr(a):
    return C.c_void_p(0 if a is None else a.ctypes.data)


class _Run:
    """the arrays of `chains` chains, on the device or (host=True) in NumPy, and the struct over them"""

    def __init__(self, sampler, chains, num_burnin, num_samples, thin, seed, keep_vars, init_x, max_shrink, hub_degree, u, host):
        fl = sampler.flat
        chains, num_burnin, num_samples, thin = int(chains), int(num_burnin), int(num_samples), int(thin)
        max_shrink, hub_degree = int(max_shrink), int(hub_degree)
        if chains < 1 or num_burnin < 0 or num_samples < 0 or thin < 1:
            raise ValueError('chains >= 1, num_burnin >= 0, num_samples >= 0 and thin >= 1 are required')
        if chains > MAX_CHAINS:
            raise ValueError('at most %d chains a run' % MAX_CHAINS)
        if not 0 <= max_shrink <= MAX_SHRINK:
            raise ValueError('max_shrink must lie in 0 .. %d' % MAX_SHRINK)
        if hub_degree < 0:
            raise ValueError('hub_degree must not be negative')
        self.sampler, self.host = sampler, bool(host)
        self.chains, self.num_burnin, self.num_samples, self.thin = chains, num_burnin, num_samples, thin
        self.max_shrink, self.hub_degree, self.seed = max_shrink, hub_degree, int(seed) & ((1 << 64) - 1)
        self.iters = num_burnin + ((num_samples - 1) * thin + 1 if num_samples else 0)
        V = fl.V
        self.col_ptr, self.col_var, self.hub_ptr, self.hub_var = work_lists(fl, sampler.colour, sampler.n_colours, hub_degree)
        keep = sampler.var_ids(keep_vars)
        if keep.size and (~sampler.hidden[keep]).any():
            raise ValueError('keep_vars names an observed variable')
        if np.unique(keep).size != keep.size:
            raise ValueError('keep_vars names a variable twice')
        self.keep_vars = keep
        keep_row = np.full(V, -1, dtype=np.int32)
        keep_row[keep] = np.arange(keep.size, dtype=np.int32)
        host_arrays = dict(col_ptr=self.col_ptr, col_var=self.col_var if self.col_var.size else np.zeros(1, np.int32),
                           hub_ptr=self.hub_ptr, hub_var=self.hub_var if self.hub_var.size else np.zeros(1, np.int32),
                           cnt_off=sampler.cnt_off, keep_row=keep_row)
        if init_x is not None:
            init = np.asarray(init_x, dtype=np.float64)
            if init.size not in (V, chains * V):
                raise ValueError('init_x must be [V] or [chains, V]')
            init = np.array(np.broadcast_to(init.reshape(-1, V), (chains, V)), order='C')
            sampler.check_state(init)
            host_arrays['init_x'] = init
        if u is not None:
            u = np.ascontiguousarray(u, dtype=np.float64)
            if u.ndim != 4 or u.shape[1:] != (chains, V, 1 + max_shrink) or u.shape[0] < self.iters:
                raise ValueError('u must be [iterations >= %d, %d, %d, %d]' % (self.iters, chains, V, 1 + max_shrink))
            host_arrays['u'] = u
        n_states = max(sampler.n_states, 1)
        rows = max(int(keep.size), 1)
        if host:
            self.graph = sampler.host_graph()
            self.t = t = host_arrays
            ptr = _np_ptr
            z = lambda shape, dt: np.zeros(shape, dtype=dt)                               # noqa: E731
            i32, i64, f64 = np.int32, np.int64, np.float64
        else:
            torch = _abi.require_gpu()
            self.graph = sampler.device_graph()
            need = chains * (12 * V + 4 * n_states + 16 * V + 8 * rows * max(num_samples, 1) + 16)
            free = int(torch.cuda.mem_get_info()[0])
            if need > free:
                raise MemoryError('%d chains over %d variables need %d bytes of device memory, %d are free' % (chains, V, need, free))
            self.t = t = _abi.upload(host_arrays, self.graph.device)
            ptr = _abi.ptr
            dev = self.graph.device
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)                # noqa: E731
            i32, i64, f64 = torch.int32, torch.int64, torch.float64
        self.x, self.idx = z((max(V, 1), chains), f64), z((max(V, 1), chains), i32)
        self.counts = z((n_states, chains), i32)
        self.sum1, self.sum2 = z((max(V, 1), chains), f64), z((max(V, 1), chains), f64)
        self.samples = z((rows, chains * max(num_samples, 1)), f64) if keep.size else None
        self.stuck, self.capped, self.evals = z((chains,), i32), z((chains,), i32), z((chains,), i64)
        s = _abi.FgibbsStruct()
        s.n_colours = sampler.n_colours
        s.col_ptr, s.col_var, s.hub_ptr, s.hub_var = ptr(t['col_ptr']), ptr(t['col_var']), ptr(t['hub_ptr']), ptr(t['hub_var'])
        s.max_shrink, s.hub_degree, s.num_burnin, s.num_samples, s.thin, s.seed = (max_shrink, hub_degree, num_burnin, num_samples,
                                                                                   thin, self.seed)
        s.u, s.init_x = ptr(t.get('u')), ptr(t.get('init_x'))
        s.cnt_off, s.counts, s.sum1, s.sum2 = ptr(t['cnt_off']), ptr(self.counts), ptr(self.sum1), ptr(self.sum2)
        s.keep_row, s.samples = ptr(t['keep_row']), ptr(self.samples)
        s.stuck, s.capped, s.evals = ptr(self.stuck), ptr(self.capped), ptr(self.evals)
        self.s, self._ptr = s, ptr
        self.done = 0
        if not host:
            _abi.check(_abi.lib().lhvi_fgibbs_init(self.graph.g, s, chains, ptr(self.x), ptr(self.idx), _abi.stream_ptr()))
        self._initialised = not host

    def advance(self, it_end, threads=1):
        """iterations [done, it_end) of every chain: one call on the device (a launch per colour and iteration, in stream
        order); on the host chain after chain, `threads` chains at a time"""
        it_end = int(it_end)
        if it_end < self.done or it_end > self.iters:
            raise ValueError('it_end must lie in [%d, %d]' % (self.done, self.iters))
        l, g, p = _abi.lib(), self.graph.g, self.graph.p
        if not self.host:
            _abi.check(l.lhvi_fgibbs_run(g, p, self.s, self.chains, self.done, it_end, _np_ptr(self.col_ptr), _np_ptr(self.hub_ptr),
                                         self._ptr(self.x), self._ptr(self.idx), _abi.stream_ptr()))
        else:
            init = 0 if self._initialised else 1

            def one(c):
                return l.lhvi_fgibbs_chain_host(g, p, self.s, self.chains, int(c), init, self.done, it_end, self._ptr(self.x),
                                                self._ptr(self.idx))
            if threads > 1:
                from concurrent.futures import ThreadPoolExecutor
                with ThreadPoolExecutor(int(threads)) as pool:
                    rcs = list(pool.map(one, range(self.chains)))
            else:
                rcs = [one(c) for c in range(self.chains)]
            for rc in rcs:
                _abi.check(rc)
            self._initialised = True
        self.done = it_end
        return self

    def run(self, its_per_launch=None, threads=1):
        step = self.iters if its_per_launch is None else int(its_per_launch)
        if its_per_launch is not None and step < 1:
            raise ValueError('its_per_launch must be positive')
        if self.iters == 0:
            self.advance(0, threads)
        while self.done < self.iters:
            self.advance(min(self.iters, self.done + step), threads)
        return self

    def numpy(self, name):
        a = getattr(self, name)
        return None if a is None else (a if self.host else a.cpu().numpy())


class HostChains(_Run):
    """`chains` chains on the host through the device's code (``lhvi_fgibbs_chain_host``): the arrays of a device run as NumPy
    arrays (x, idx [V, chains]; counts; sum1, sum2; samples; stuck, capped, evals).  ``advance(it_end)`` / ``run()``."""

    def __init__(self, sampler, chains=1, num_burnin=0, num_samples=0, thin=1, seed=0, keep_vars=None, init_x=None, max_shrink=64,
                 u=None):
        _Run.__init__(self, sampler, chains, num_burnin, num_samples, thin, seed, keep_vars, init_x, max_shrink, _abi.HUB_DEGREE, u,
                      host=True)


def chain_host(sampler, threads=1, **kw):
    """``HostChains(sampler, **kw).run()``"""
    return HostChains(sampler, **kw).run(threads=threads)


# ---- the solver-shaped class ------------------------------------------------------------------------------------------------------
class FlatGibbs:
    """Sampled marginals of any ground model from many single-site Gibbs chains.  ``FlatGibbs(g)`` (an object graph) or
    ``FlatGibbs(None, flat=...)``.  After ``run()``: ``disc_marginals()``, ``moments()``, ``rhat()``, ``stats()``, ``map`` /
    ``map_all``, and with ``keep_vars`` ``fit_marginals(K)`` and ``belief`` of a kept continuous variable."""

    def __init__(self, g, flat=None):
        self.g = g
        if flat is None and g is None:
            raise ValueError('FlatGibbs needs a graph or flat=')
        self.flat = fl = flatten(flat if flat is not None else g, require_device_potentials=True)
        if (fl.pot_kind == POT_GENERIC).any():
            raise NotImplementedError('a potential has no device encoding (device_spec); FlatGibbs evaluates potentials on the device')
        if fl.lifted:
            raise NotImplementedError('FlatGibbs runs on ground graphs (edge_count / var_mult / fac_mult)')
        self.hidden = np.isnan(fl.var_value)
        cont = fl.dom_cont[fl.var_dom].astype(bool) if fl.V else np.zeros(0, dtype=bool)
        self.Vd_ids = np.flatnonzero(self.hidden & ~cont)
        self.Vc_ids = np.flatnonzero(self.hidden & cont)
        nst = fl.var_nstates if fl.V else np.zeros(0, dtype=np.int64)
        self.dstates = nst[self.Vd_ids].astype(np.int64)
        if self.dstates.size and self.dstates.max() > MAX_STATES:
            raise NotImplementedError('a hidden discrete variable has %d states, more than LHVI_FGIBBS_MAX_STATES = %d'
                                      % (int(self.dstates.max()), MAX_STATES))
        if self.dstates.size and self.dstates.min() < 1:
            raise ValueError('a hidden discrete variable has no state')
        lo, hi = fl.dom_lo[fl.var_dom[self.Vc_ids]], fl.dom_hi[fl.var_dom[self.Vc_ids]]
        if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
            raise ValueError('a hidden continuous variable has an infinite domain bound: the slice sampler shrinks from the domain interval')
        if (hi < lo).any():
            raise ValueError('a hidden continuous variable has an empty domain interval')
        self._check_evidence()
        self.dstate_off = np.zeros(self.Vd_ids.size + 1, dtype=np.int64)
        np.cumsum(self.dstates, out=self.dstate_off[1:])
        self.n_states = int(self.dstate_off[-1])
        self.cnt_off = np.full(fl.V, -1, dtype=np.int32)
        self.cnt_off[self.Vd_ids] = self.dstate_off[:-1]
        self.colour, self.n_colours = colour_variables(fl)
        self._dg = self._hg = None
        self._run = None
        self.marginals = None

    def _check_evidence(self):
        """a discrete variable observed off its states has no table index"""
        fl = self.flat
        obs = np.flatnonzero(~self.hidden & ~fl.dom_cont[fl.var_dom].astype(bool))
        off = [v for v in obs if fl.var_value[v] not in fl.dom_val[fl.dom_ptr[fl.var_dom[v]]:fl.dom_ptr[fl.var_dom[v] + 1]]]
        for v in off:
            for e in fl.var_edge[fl.var_ptr[v]:fl.var_ptr[v + 1]]:
                if fl.pot_kind[fl.fac_pot[fl.edge_fac[e]]] == POT_TABLE:
                    raise ValueError('variable %d is observed at %r, none of its states, and is an argument of a table' % (v, fl.var_value[v]))

    def check_state(self, x):
        """x [chains, V]: hidden discrete entries must be states, hidden continuous ones inside the domain"""
        fl = self.flat
        for v in self.Vd_ids:
            st = fl.dom_val[fl.dom_ptr[fl.var_dom[v]]:fl.dom_ptr[fl.var_dom[v] + 1]]
            if not np.isin(x[:, v], st).all():
                raise ValueError('init_x holds a value of variable %d that is none of its states' % v)
        d = fl.var_dom[self.Vc_ids]
        xc = x[:, self.Vc_ids]
        if xc.size and not ((xc >= fl.dom_lo[d][None, :]) & (xc <= fl.dom_hi[d][None, :])).all():
            raise ValueError('init_x holds a continuous value outside its domain')

    def var_ids(self, rvs):
        """variable ids of a list of ids / rv objects; 'cont': every hidden continuous variable; None: none"""
        if rvs is None:
            return np.zeros(0, dtype=np.int64)
        if isinstance(rvs, str):
            if rvs != 'cont':
                raise ValueError("keep_vars: a list of variables, 'cont' or None")
            return self.Vc_ids.astype(np.int64)
        out = np.array([v if isinstance(v, (int, np.integer)) else self.flat.var_index[v] for v in rvs], dtype=np.int64)
        if out.size and (out.min() < 0 or out.max() >= self.flat.V):
            raise ValueError('keep_vars names a variable outside the graph')
        return out

    def device_graph(self):
        if self._dg is None:
            self._dg = _abi.DeviceGraph(self.flat)
        return self._dg

    def host_graph(self):
        if self._hg is None:
            from .npvi import _HostGraph
            self._hg = _HostGraph(self.flat)
        return self._hg

    # ---- running ----------------------------------------------------------------------------------------------------------
    def run(self, chains=1024, num_burnin=100, num_samples=100, thin=1, seed=0, keep_vars=None, init_x=None, max_shrink=64,
            hub_degree=_abi.HUB_DEGREE, its_per_launch=None, u=None):
        """`chains` chains of num_burnin + (num_samples - 1) thin + 1 iterations; every thin-th iteration from num_burnin on is
        kept.  keep_vars: the variables whose kept samples stay on the device for ``fit_marginals`` (ids, rv objects or 'cont').
        init_x [V] or [chains, V]: the initial state; u: injected uniforms [iterations, chains, V, 1 + max_shrink] (tests)."""
        if num_samples < 1:
            raise ValueError('num_samples must be positive')
        seed = int.from_bytes(os.urandom(8), 'little') if seed is None else int(seed)
        r = _Run(self, chains, num_burnin, num_samples, thin, seed, keep_vars, init_x, max_shrink, hub_degree, u, host=False)
        return self.adopt(r.run(its_per_launch))

    def adopt(self, r):
        """the state a finished run (device or host) leaves"""
        self._run = r
        self.chains, self.num_samples = r.chains, r.num_samples
        self.marginals = None
        self.counts = r.numpy('counts')[:self.n_states].T.copy()                 # [chains, sum of states]
        self.sum1 = r.numpy('sum1')[self.Vc_ids].T.copy()                        # [chains, Nc]
        self.sum2 = r.numpy('sum2')[self.Vc_ids].T.copy()
        self.stuck, self.capped, self.evals = r.numpy('stuck'), r.numpy('capped'), r.numpy('evals')
        self.samples = r.samples
        return self

    def _need_run(self):
        if self._run is None:
            raise RuntimeError('call run() first')
        return self._run

    def _stderr(self, per_chain):
        if self.chains < 2:
            return np.full(per_chain.shape[1:], np.nan)
        return per_chain.std(axis=0, ddof=1) / np.sqrt(self.chains)

    # ---- read-outs (the definitions of GibbsHybridGaussian) ----------------------------------------------------------------------
    def disc_marginals(self):
        """per hidden discrete variable, in variable order (``Vd_ids``): (marginal [states], standard error over chains)"""
        self._need_run()
        freq = self.counts / float(self.num_samples)
        mean, se = freq.mean(axis=0), self._stderr(freq)
        off = self.dstate_off
        return [(mean[off[i]:off[i + 1]], se[off[i]:off[i + 1]]) for i in range(self.Vd_ids.size)]

    def moments(self):
        """namespace over the hidden continuous variables (``Vc_ids``): mean = E[x], second = E[x^2], var = second - mean^2, and
        the standard errors over chains mean_se, second_se"""
        self._need_run()
        m1, m2 = self.sum1 / float(self.num_samples), self.sum2 / float(self.num_samples)
        mean, second = m1.mean(axis=0), m2.mean(axis=0)
        return types.SimpleNamespace(mean=mean, second=second, var=second - mean * mean, mean_se=self._stderr(m1),
                                     second_se=self._stderr(m2))

    def rhat(self):
        """Gelman-Rubin potential scale reduction from the per-chain accumulators: namespace disc (a [states] array per discrete
        variable: the state's indicator), cont [Nc], max (NaN entries skipped)"""
        self._need_run()
        S = float(self.num_samples)
        if self.chains < 2 or S < 2:
            raise ValueError('rhat needs at least two chains and two kept samples')

        def psr(means, within):
            W = within.mean(axis=0)
            B_over_n = means.var(axis=0, ddof=1)
            with np.errstate(divide='ignore', invalid='ignore'):
                return np.sqrt(((S - 1) / S * W + B_over_n) / W)
        p = self.counts / S
        rd = psr(p, p * (1 - p) * S / (S - 1))
        m1 = self.sum1 / S
        rc = psr(m1, (self.sum2 / S - m1 * m1) * S / (S - 1))
        off = self.dstate_off
        both = np.concatenate([rd, rc])
        return types.SimpleNamespace(disc=[rd[off[i]:off[i + 1]] for i in range(self.Vd_ids.size)], cont=rc,
                                     max=float(np.nanmax(both)) if both.size and not np.isnan(both).all() else float('nan'))

    def stats(self):
        """dict: stuck / capped (totals over chains and iterations), evals (all evaluations of a conditional log density) and
        evals_per_slice_update (the mean over the continuous updates: a discrete update costs its number of states)"""
        r = self._need_run()
        total = int(self.evals.sum())
        disc = int(self.dstates.sum()) * r.done * r.chains
        n_slice = int(self.Vc_ids.size) * r.done * r.chains
        return dict(stuck=int(self.stuck.sum()), capped=int(self.capped.sum()), evals=total, iterations=r.done,
                    evals_per_slice_update=(total - disc) / n_slice if n_slice else float('nan'))

    def fit_marginals(self, K, **fit_args):
        """a K-component Gaussian mixture fitted to the kept samples of every variable of ``keep_vars``
        (``gmfit.fit_scalar_gms`` on the device tensor [rows, chains * num_samples]); kept as ``self.marginals``"""
        from .gmfit import fit_scalar_gms
        r = self._need_run()
        if r.samples is None:
            raise RuntimeError('fit_marginals needs kept samples: call run(keep_vars=...)')
        cont = self.flat.dom_cont[self.flat.var_dom[r.keep_vars]].astype(bool)
        if not cont.all():
            raise ValueError('keep_vars names a discrete variable: a Gaussian mixture is fitted to continuous ones')
        self.marginals = fit_scalar_gms(r.samples, K, **fit_args)
        return self.marginals

    def _vid(self, rv):
        return int(rv) if isinstance(rv, (int, np.integer)) else self.flat.var_index[rv]

    def map(self, rv):
        """observed: the value; discrete: the state of largest sampled marginal (first on ties); continuous: the sample mean
        clipped to the domain"""
        self._need_run()
        fl, v = self.flat, self._vid(rv)
        if not self.hidden[v]:
            return float(fl.var_value[v])
        d = fl.var_dom[v]
        if fl.dom_cont[d]:
            i = int(np.searchsorted(self.Vc_ids, v))
            return float(min(max(self.moments().mean[i], fl.dom_lo[d]), fl.dom_hi[d]))
        i = int(np.searchsorted(self.Vd_ids, v))
        return float(fl.dom_val[fl.dom_ptr[d] + int(np.argmax(self.disc_marginals()[i][0]))])

    def map_all(self):
        """[V]: ``map`` of every variable"""
        self._need_run()
        fl = self.flat
        out = fl.var_value.copy()
        d = fl.var_dom[self.Vc_ids]
        out[self.Vc_ids] = np.clip(self.moments().mean, fl.dom_lo[d], fl.dom_hi[d])
        for i, (m, _) in enumerate(self.disc_marginals()):
            v = self.Vd_ids[i]
            out[v] = fl.dom_val[fl.dom_ptr[fl.var_dom[v]] + int(np.argmax(m))]
        return out

    def belief(self, x, rv):
        """discrete: the sampled marginal of the state x (0 for a value that is no state); continuous: the density of the
        fitted mixture at x (after ``fit_marginals``; the variable must be one of ``keep_vars``)"""
        r = self._need_run()
        fl, v = self.flat, self._vid(rv)
        if not self.hidden[v]:
            return 1.0 if x == fl.var_value[v] else 0.0
        d = fl.var_dom[v]
        if not fl.dom_cont[d]:
            i = int(np.searchsorted(self.Vd_ids, v))
            st = np.flatnonzero(fl.dom_val[fl.dom_ptr[d]:fl.dom_ptr[d + 1]] == x)
            return float(self.disc_marginals()[i][0][st[0]]) if st.size else 0.0
        if self.marginals is None:
            raise RuntimeError('belief of a continuous variable needs fit_marginals()')
        row = np.flatnonzero(r.keep_vars == v)
        if not row.size:
            raise ValueError('the variable is not one of keep_vars')
        out = self.marginals.pdf(np.atleast_1d(np.asarray(x, dtype=np.float64)).reshape(1, -1).copy(), rows=row)
        out = out if isinstance(out, np.ndarray) else out.cpu().numpy()
        return float(out[0, 0]) if np.ndim(x) == 0 else out[0]
