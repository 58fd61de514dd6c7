"""Nonparametric variational inference on the GPU: ``NPVI`` and ``LiftedNPVI`` (the reference's ``osi/NPVI.py``).

A K-component product mixture -- weights ``w = softmax(tau)``, a Gaussian ``(Mu, exp(lVar))`` per hidden continuous variable and
component, a categorical ``softmax(Rho)`` per hidden discrete one -- is fitted to the negative ELBO with the Jensen lower bound on
the mixture entropy (Gershman et al. 2012).  The expectation step, the entropy bound, their gradient and TensorFlow's Adam run as HIP
kernels (``csrc/npvi.hip``, docs/kernels_npvi.md); the fitted parameters live in the arrays ``VarInference`` uses (``w``, ``eta_c``
= (mu, var), ``eta_d``), so ``belief``, ``map_rows_device``, ``mixture_belief`` and ``MixtureBelief.from_solver`` read an NPVI fit
in place -- with normal component densities (``norm_pdf`` here, ``LHVI_VI_GAUSSIAN_PDF``, ``belief_normaliser = 'gaussian'``), not the
``exp(-u^2 / 2 var) / (2.5066 var)`` of ``VarInference.norm_pdf``: the queries answer for the mixture that was optimised.

Differences from the reference, all on purpose:

* evidence stays in the graph (a one-point axis with coefficient 1) instead of being conditioned away first;
* discrete variables may have different numbers of states (the reference's entropy bound asserts a common one);
* ``init_param(seed)`` draws with ``np.random.RandomState(seed)`` in this order: ``Rho ~ N(0, 1)`` [V, K, Dmax], ``Mu ~ U(lo, hi)``
  [V, K], ``lVar ~ U(log Var_bds)`` [V, K], ``tau = 0`` -- TensorFlow's random start is not reproduced;
* out of scope: ``isotropic_cov``, ``LiftedNPVI2``'s regulariser, ``init_grid``, the per-array mean-|gradient| records.

``run(..., host=True)`` and ``grad(host=True)`` go through the library's host twins (the device code with one lane): no GPU needed.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from .flat import FlatGraph, flatten
from .vi import _Variational, factor_lists


def _np_ptr(a):
    return C.c_void_p(0 if a is None else a.ctypes.data)


class _HostGraph:
    """``lhvi_graph_t`` / ``lhvi_pots_t`` over the FlatGraph's own host arrays (for the ``*_host`` entry points)"""

    def __init__(self, flat):
        pot_off, pot_param, interpreted = _abi.device_potentials(flat)
        c = lambda a, dt: np.ascontiguousarray(a, dtype=dt)
        self.keep = k = dict(
            fac_ptr=c(flat.fac_ptr, np.int32), edge_var=c(flat.edge_var, np.int32), edge_fac=c(flat.edge_fac, np.int32),
            var_ptr=c(flat.var_ptr, np.int32), var_edge=c(flat.var_edge, np.int32), fac_pot=c(flat.fac_pot, np.int32),
            var_value=c(flat.var_value, np.float64), var_dom=c(flat.var_dom, np.int32), dom_cont=c(flat.dom_cont, np.int32),
            dom_lo=c(flat.dom_lo, np.float64), dom_hi=c(flat.dom_hi, np.float64), dom_ptr=c(flat.dom_ptr, np.int32),
            dom_val=c(flat.dom_val if flat.dom_val.size else np.zeros(1), np.float64), pot_kind=c(flat.pot_kind, np.int32),
            pot_off=c(pot_off, np.int32), pot_param=c(pot_param if pot_param.size else np.zeros(1), np.float64))
        g = _abi.GraphStruct()
        g.V, g.F, g.E, g.nnz = flat.V, flat.F, flat.E, int(flat.var_edge.size)
        for name in ('fac_ptr', 'edge_var', 'edge_fac', 'var_ptr', 'var_edge', 'fac_pot', 'var_value', 'var_dom', 'dom_cont',
                     'dom_lo', 'dom_hi', 'dom_ptr', 'dom_val'):
            setattr(g, name, _np_ptr(k[name]))
        g.D, g.n_hubs = int(flat.dom_cont.size), 0
        self.g = g
        p = _abi.PotsStruct()
        p.P = int(flat.pot_kind.size)
        p.kind, p.off, p.param, p.interpreted = _np_ptr(k['pot_kind']), _np_ptr(k['pot_off']), _np_ptr(k['pot_param']), int(interpreted)
        self.p = p


class NPVI(_Variational):
    """``NPVI(g, K, T, Var_bds=None, seed=None)``: `g` an object graph or a ``FlatGraph``.  ``var_count`` / ``fac_count``: the
    sharing counts ([V] / [F]; default: the objects' ``sharing_count``, ones for a FlatGraph)."""

    _param_names = ('tau', 'theta_c', 'rho')
    belief_normaliser = 'gaussian'      # the components are normal densities: what MixtureBelief.from_solver and every query evaluate
    adam_eps = 1e-8                     # tf.train.AdamOptimizer's epsilon
    _stem = 'npvi'                      # the entry points are lhvi_<stem>_{workspace_bytes, grad, run, grad_host, run_host}
    _extra = ()                         # the solver's own [V] input arrays (attributes), after fac_count in grad, after the options in run

    @staticmethod
    def norm_pdf(x, eta):
        """the normal density of a component (``VarInference.norm_pdf`` divides by the variance instead: its own convention)"""
        u = x - eta[0]
        return np.e ** (-u * u * 0.5 / eta[1]) / (2.506628274631 * np.sqrt(eta[1]))

    def __init__(self, g, K, T, Var_bds=None, seed=None, var_count=None, fac_count=None):
        if not 1 <= int(K) <= _abi.NPVI_MAX_K:
            raise ValueError('K must be in 1 .. %d' % _abi.NPVI_MAX_K)
        if int(T) < 1:
            raise ValueError('T must be at least 1')
        self.g = g
        self._init_common(int(K), int(T))
        self.Var_bds = [5e-3, 10] if Var_bds is None else [float(Var_bds[0]), float(Var_bds[1])]
        if not 0 < self.Var_bds[0] <= self.Var_bds[1]:
            raise ValueError('Var_bds must be 0 < lo <= hi')
        self._set_flat(flatten(self._graph_like(), require_device_potentials=True), var_count, fac_count)
        self.t = 0
        self.init_param(seed)

    # ---- graph ------------------------------------------------------------------------------------------------------------
    def _graph_like(self):
        return self.g

    def _ground_graph(self):
        return self.g

    def _var_index(self, rv):
        return self.flat.var_index[rv]

    def _counts_of(self, flat, var_count, fac_count):
        def one(given, items, n):
            if given is not None:
                a = np.ascontiguousarray(given, dtype=np.float64)
                if a.shape != (n,):
                    raise ValueError('a count array has the wrong length')
                return a
            if items and len(items) == n:
                a = np.array([float(getattr(x, 'sharing_count', 1)) for x in items])
                return a if (a != 1).any() else None
            return None
        return one(var_count, flat.rvs, flat.V), one(fac_count, flat.factors, flat.F)

    def _set_flat(self, flat, var_count=None, fac_count=None):
        self.flat = flat
        hidden, cont = flat.var_hidden, flat.var_cont
        self._cont, self._disc = hidden & cont, hidden & ~cont
        self.Dmax = int(flat.var_nstates[self._disc].max()) if self._disc.any() else 1
        self._has_disc = bool(self._disc.any())
        self.max_arity = int(np.diff(flat.fac_ptr).max()) if flat.F else 0
        if self.max_arity > 6:
            raise ValueError('factors of more than 6 arguments are not supported')
        _, _, rec = factor_lists(flat, self.K, self.T, None, False)
        self._edge_axis = np.ascontiguousarray(rec if rec.size else np.zeros((1, 4), dtype=np.int32))
        slots = np.where(hidden[flat.edge_var], rec[:flat.E, 1] & 0xffff, 1) if flat.E else np.zeros(0, dtype=np.int64)
        csum = np.concatenate([[0], np.cumsum(slots)])
        per_fac = csum[flat.fac_ptr[1:]] - csum[flat.fac_ptr[:-1]]
        self.max_slots = int(per_fac.max()) if flat.F else 0
        if self.max_slots > _abi.NPVI_MAX_SLOTS:
            raise ValueError('a factor spans %d quadrature slots (T per continuous, #states per discrete hidden argument); '
                             'at most %d are supported' % (self.max_slots, _abi.NPVI_MAX_SLOTS))
        self.var_count, self.fac_count = self._counts_of(flat, var_count, fac_count)
        dom = flat.var_dom.astype(np.int64)
        self._mu_lo = np.where(self._cont, flat.dom_lo[dom], 0.0).astype(np.float64)
        self._mu_hi = np.where(self._cont, flat.dom_hi[dom], 0.0).astype(np.float64)
        nst = np.where(self._disc, flat.var_nstates, 0)
        self._mask_d = np.arange(self.Dmax)[None, :] < nst[:, None]
        self._hg = None
        self._dev = None

    # ---- parameters (host copies are the record; the device arrays are refreshed from them before a device call) -----------
    def init_param(self, seed=None):
        flat, K = self.flat, self.K
        rng = np.random.RandomState(seed)
        rho = rng.randn(flat.V, K, self.Dmax)
        mu = rng.uniform(self._mu_lo[:, None], self._mu_hi[:, None], size=(flat.V, K))
        lb = np.log(self.Var_bds)
        lvar = rng.uniform(lb[0], lb[1], size=(flat.V, K))
        self.set_params(np.zeros(K), mu, lvar, rho)

    def set_params(self, tau, Mu, lVar, Rho=None):
        """``tau`` [K], ``Mu`` / ``lVar`` [V, K] (rows of variables that are not hidden and continuous are ignored), ``Rho``
        [V, K, Dmax] (entries beyond a variable's states and rows of other variables are ignored)"""
        flat, K = self.flat, self.K
        tau = np.array(tau, dtype=np.float64).reshape(K)
        theta = np.zeros((flat.V, K, 2))
        theta[:, :, 0] = np.where(self._cont[:, None], np.asarray(Mu, dtype=np.float64).reshape(flat.V, K), 0.0)
        theta[:, :, 1] = np.where(self._cont[:, None], np.asarray(lVar, dtype=np.float64).reshape(flat.V, K), 0.0)
        rho = np.zeros((flat.V, K, self.Dmax))
        if Rho is not None:
            rho[:] = np.asarray(Rho, dtype=np.float64).reshape(flat.V, K, self.Dmax)
        rho *= self._mask_d[:, None, :]
        self._h = dict(tau=tau, theta_c=theta, rho=rho)
        for name in self._param_names:
            self._h['m_' + name] = np.zeros_like(self._h[name])
            self._h['s_' + name] = np.zeros_like(self._h[name])
        self.t = 0
        self._refresh_view()
        self._dirty = True

    def _refresh_view(self):
        h = self._h
        e = np.exp(h['tau'] - h['tau'].max())
        h['w'] = e / e.sum()
        h['eta_c'] = np.stack([h['theta_c'][:, :, 0], np.exp(h['theta_c'][:, :, 1])], axis=2)
        r = np.where(self._mask_d[:, None, :], h['rho'], -np.inf)
        with np.errstate(invalid='ignore'):
            ex = np.where(self._mask_d[:, None, :], np.exp(r - np.max(r, axis=2, keepdims=True, initial=-1e300)), 0.0)
        den = ex.sum(axis=2, keepdims=True)
        h['eta_d'] = np.where(den > 0, ex / np.where(den > 0, den, 1.0), 0.0)
        for name in ('w', 'eta_c', 'eta_d'):
            h[name] = np.ascontiguousarray(h[name])
        self._cache = {}

    def _host(self, name):
        return self._h[name]

    @property
    def w(self):
        return self._h['w']

    # ---- structs ----------------------------------------------------------------------------------------------------------
    def _host_struct(self):
        if self._hg is None:
            self._hg = _HostGraph(self.flat)
            self._hq = (np.ascontiguousarray(self.quad_x, dtype=np.float64), np.ascontiguousarray(self.quad_w, dtype=np.float64))
        h = self._h
        p = _abi.ViStruct()
        p.K, p.T, p.Dmax, p.quirks = self.K, self.T, self.Dmax, _abi.VI_GAUSSIAN_PDF
        p.gh_x, p.gh_w = _np_ptr(self._hq[0]), _np_ptr(self._hq[1])
        p.w, p.eta_c, p.eta_d, p.edge_axis = _np_ptr(h['w']), _np_ptr(h['eta_c']), _np_ptr(h['eta_d']), _np_ptr(self._edge_axis)
        return p

    def _ensure_dev(self):
        if self._dev is None:
            torch = _abi.require_gpu()
            self.dg = _abi.DeviceGraph(self.flat)
            d = dict(gh_x=_abi.to_dev(self.quad_x), gh_w=_abi.to_dev(self.quad_w), edge_axis=_abi.to_dev(self._edge_axis),
                     mu_lo=_abi.to_dev(self._mu_lo), mu_hi=_abi.to_dev(self._mu_hi), obj=self.dg.zeros(1),
                     var_count=None if self.var_count is None else _abi.to_dev(self.var_count),
                     fac_count=None if self.fac_count is None else _abi.to_dev(self.fac_count))
            for name, a in self._h.items():
                d[name] = _abi.to_dev(a)
            for name in self._extra:
                d[name] = _abi.to_dev(getattr(self, name))
            for name in self._param_names:
                d['g_' + name] = torch.zeros_like(d[name])
            self._dev = d
            ws_bytes = int(self._entry('workspace_bytes')(self.dg.g, self._struct()))
            d['ws'] = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=self.dg.device)
            d['ws_bytes'] = ws_bytes
            self._dirty = False
        elif self._dirty:
            for name, a in self._h.items():
                self._dev[name].copy_(_abi.to_dev(a))
            self._dirty = False
        return self._dev

    def _struct(self):
        d = self._dev
        p = _abi.ViStruct()
        p.K, p.T, p.Dmax, p.quirks = self.K, self.T, self.Dmax, _abi.VI_GAUSSIAN_PDF
        p.gh_x, p.gh_w, p.w = _abi.ptr(d['gh_x']), _abi.ptr(d['gh_w']), _abi.ptr(d['w'])
        p.eta_c, p.eta_d, p.edge_axis = _abi.ptr(d['eta_c']), _abi.ptr(d['eta_d']), _abi.ptr(d['edge_axis'])
        return p

    def _opt_struct(self, arrays, to_ptr, lr):
        o = _abi.NpviOptStruct()
        for field, name in (('tau', 'tau'), ('theta_c', 'theta_c'), ('rho', 'rho'), ('m_tau', 'm_tau'), ('s_tau', 's_tau'),
                            ('m_c', 'm_theta_c'), ('s_c', 's_theta_c'), ('m_rho', 'm_rho'), ('s_rho', 's_rho'), ('g_tau', 'g_tau'),
                            ('g_c', 'g_theta_c'), ('g_rho', 'g_rho'), ('obj', 'obj'), ('w', 'w'), ('eta_c', 'eta_c'),
                            ('eta_d', 'eta_d'), ('mu_lo', 'mu_lo'), ('mu_hi', 'mu_hi'), ('var_count', 'var_count'),
                            ('fac_count', 'fac_count')):
            setattr(o, field, to_ptr(arrays.get(name)))
        lb = np.log(self.Var_bds)
        o.lvar_lo, o.lvar_hi = float(lb[0]), float(lb[1])
        o.lr, o.b1, o.b2, o.eps, o.t = float(lr), 0.9, 0.999, float(self.adam_eps), int(self.t)
        o.max_slots, o.max_arity = int(self.max_slots), int(self.max_arity)
        return o

    def _download(self):
        d = self._dev
        for name in list(self._h):
            self._h[name] = np.ascontiguousarray(d[name].cpu().numpy())
        self._cache = {}

    def _entry(self, what):
        return getattr(_abi.lib(), 'lhvi_%s_%s' % (self._stem, what))

    # ---- objective and gradient -------------------------------------------------------------------------------------------
    def grad(self, host=False):
        """``(obj, g_tau [K], g_c [V, K, 2] = (d / d Mu, d / d lVar), g_rho [V, K, Dmax])``: the negative ELBO at the current
        parameters and the gradient of the reference's auxiliary objective"""
        flat, K = self.flat, self.K
        if host:
            out = dict(obj=np.zeros(1), g_tau=np.zeros(K), g_c=np.zeros((flat.V, K, 2)), g_rho=np.zeros((flat.V, K, self.Dmax)))
            p = self._host_struct()
            _abi.check(self._entry('grad_host')(self._hg.g, self._hg.p, p, _np_ptr(self.var_count), _np_ptr(self.fac_count),
                                                *[_np_ptr(getattr(self, name)) for name in self._extra], _np_ptr(out['obj']),
                                                _np_ptr(out['g_tau']), _np_ptr(out['g_c']), _np_ptr(out['g_rho'])))
            return float(out['obj'][0]), out['g_tau'], out['g_c'], out['g_rho']
        d = self._ensure_dev()
        _abi.check(self._entry('grad')(self.dg.g, self.dg.p, self._struct(), _abi.ptr(d['var_count']), _abi.ptr(d['fac_count']),
                                       *[_abi.ptr(d[name]) for name in self._extra], int(self.max_slots), int(self.max_arity),
                                       _abi.ptr(d['obj']), _abi.ptr(d['g_tau']), _abi.ptr(d['g_theta_c']), _abi.ptr(d['g_rho']),
                                       _abi.ptr(d['ws']), d['ws_bytes'], _abi.stream_ptr()))
        return (float(d['obj'].item()), d['g_tau'].cpu().numpy(), d['g_theta_c'].cpu().numpy(), d['g_rho'].cpu().numpy())

    # ---- optimisation -----------------------------------------------------------------------------------------------------
    def _enqueue(self, n, lr, fix_mix_its, log_dev):
        """enqueues `n` updates on the current stream, the objective before each into ``log_dev[:n]``; the host copies go stale"""
        d = self._ensure_dev()
        o = self._opt_struct(d, _abi.ptr, lr)
        _abi.check(self._entry('run')(self.dg.g, self.dg.p, self._struct(), C.byref(o), *[_abi.ptr(d[name]) for name in self._extra],
                                      n, fix_mix_its, _abi.ptr(log_dev), _abi.ptr(d['ws']), d['ws_bytes'], _abi.stream_ptr()))
        self.t += n

    def run(self, its=100, lr=5e-2, fix_mix_its=0, host=False):
        """NPVI.run (NPVI.py:184-319): `its` updates of TensorFlow's Adam from the current parameters (the Adam state continues
        across calls; ``set_params`` / ``init_param`` reset it).  ``fix_mix_its``: the mixture weights stay uniform during that many
        first updates ('all': every one).  Returns ``{'record': {'obj': [...]}, 'w', 'Mu', 'Var', 'Pi', 'Rho'}`` -- ``Mu`` / ``Var``
        [V, K] and ``Pi`` / ``Rho`` [V, K, Dmax] by row of the solver's graph (NaN / 0 where a row has no such parameter) -- and
        sets ``rv.belief_params`` on an object graph."""
        its = int(its)
        if its < 0:
            raise ValueError('its must not be negative')
        if fix_mix_its == 'all':
            fix_mix_its = its
        fix_mix_its = int(fix_mix_its)
        if host:
            log = np.zeros(max(its, 1))
            h = dict(self._h)
            h.update(obj=np.zeros(1), g_tau=np.zeros(self.K), g_theta_c=np.zeros_like(self._h['theta_c']),
                     g_rho=np.zeros_like(self._h['rho']), mu_lo=self._mu_lo, mu_hi=self._mu_hi, var_count=self.var_count,
                     fac_count=self.fac_count)
            p = self._host_struct()
            o = self._opt_struct(h, _np_ptr, lr)
            _abi.check(self._entry('run_host')(self._hg.g, self._hg.p, p, C.byref(o), *[_np_ptr(getattr(self, name)) for name in self._extra],
                                               its, fix_mix_its, _np_ptr(log)))
            self._dirty = True
            self._cache = {}
            self.t += its
        else:
            torch = _abi.require_gpu()
            self._ensure_dev()
            log_dev = torch.zeros(max(its, 1), dtype=torch.float64, device=self.dg.device)
            self._enqueue(its, lr, fix_mix_its, log_dev)
            log = log_dev.cpu().numpy()
            self._download()
        return self._result([float(x) for x in log[:its]])

    def _result(self, obj):
        h = self._h
        Mu = np.where(self._cont[:, None], h['eta_c'][:, :, 0], np.nan)
        Var = np.where(self._cont[:, None], h['eta_c'][:, :, 1], np.nan)
        self.params = dict(w=h['w'].copy(), Mu=Mu, Var=Var, Pi=h['eta_d'].copy(), Rho=h['rho'].copy())
        self._set_belief_params()
        return {'record': {'obj': obj}, **self.params}

    def _belief_params_of(self, v):
        if self._cont[v]:
            return {'mu': self._h['eta_c'][v, :, 0].copy(), 'var': self._h['eta_c'][v, :, 1].copy()}
        if self._disc[v]:
            return {'pi': self._h['eta_d'][v, :, :int(self.flat.var_nstates[v])].copy()}
        return None

    def _set_belief_params(self):
        for v, rv in enumerate(self.flat.rvs):
            bp = self._belief_params_of(v)
            if bp is not None:
                rv.belief_params = bp

    def map(self, obs_rvs, query_rv=None):
        """NPVI.map (NPVI.py:321-335): the marginal MAP value of ``query_rv`` given the ``.value`` of ``obs_rvs``, through
        ``lhvi.mixture.marginal_map``.  ``map(rv)`` with one argument is ``VarInference.map``."""
        if query_rv is None:
            return _Variational.map(self, obs_rvs)
        if query_rv.value is not None:
            return query_rv.value
        from .mixture import marginal_map
        X = np.array([v.value for v in obs_rvs], dtype=np.float64)
        return marginal_map(X=X, obs_rvs=obs_rvs, query_rv=query_rv, w=self._h['w'])

    def map_rows_device(self, *args, **kwargs):
        self._ensure_dev()
        return _Variational.map_rows_device(self, *args, **kwargs)

    def mixture_belief(self, normaliser='gaussian'):
        return _Variational.mixture_belief(self, normaliser)


class LiftedNPVI(NPVI):
    """``LiftedNPVI(g, K, T, ...)``: colour passing once, then NPVI on the cluster graph with the cluster sizes as sharing counts
    (NPVI.py:338-362).  `g`: a ground object graph (compressed here), a compressed graph, or a lifted ``FlatGraph``.  After
    ``run`` the members of a cluster carry its ``belief_params``."""

    def _graph_like(self):
        g = self.g
        if isinstance(g, FlatGraph):
            return g
        from .lifting import CompressedGraph
        if isinstance(g, CompressedGraph) or hasattr(g, 'lifted_flat'):
            return g
        self._ground = g
        cg = CompressedGraph(g)
        cg.run()
        self.cg = cg
        return cg

    def _ground_graph(self):
        return getattr(self, '_ground', self.g)

    def _counts_of(self, flat, var_count, fac_count):
        if var_count is None and fac_count is None and flat.lifted:
            return np.ascontiguousarray(flat.var_mult, dtype=np.float64), np.ascontiguousarray(flat.fac_mult, dtype=np.float64)
        return NPVI._counts_of(self, flat, var_count, fac_count)

    def _var_index(self, rv):
        c = getattr(rv, 'cluster', None)
        return self.flat.var_index[c if c in self.flat.var_index else rv]

    def _set_belief_params(self):
        for v, crv in enumerate(self.flat.rvs):
            bp = self._belief_params_of(v)
            if bp is None:
                continue
            crv.belief_params = bp
            for rv in getattr(crv, 'rvs', ()):
                rv.belief_params = bp
