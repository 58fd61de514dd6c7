"""Conditional queries on a fitted mixture belief, batched on the device (``csrc/mixture.hip``, docs/kernels_mixture.md).

``VarInference``, ``LiftedVarInference`` and ``C2FVarInference`` fit one mixture q(x) = sum_k w_k prod_i q_ik(x_i).  After the
fit every conditional query is a re-weighting of the K components (the "one-shot" of the reference's ``osi/``):
p(x_h | x_o) = sum_k w'_k prod q_ik(x_h), w' = softmax(log w + sum_{i in o} log q_ik(x_i)).  ``MixtureBelief`` answers such
queries for thousands of evidence rows against every query variable in a few launches; the functions below it are the NumPy
half of the reference's ``osi/mixture_beliefs.py`` (:505-867) over the same kernels, re-exported by
``compat/osi/mixture_beliefs.py``.

Variables are ROWS of the belief: int32 indices, repeats allowed.  Evidence is ``X [M, N_o]``: a value for a continuous row, a
state INDEX for a discrete row, NaN where the evidence row does not observe that variable.

Every method takes ``host=False``.  ``host=True`` runs the host twins (``lhvi_mix_*_host``: the device's code with one
"lane") on NumPy arrays and needs no GPU; it is what the CPU tests use.  Nothing switches to it by itself: without a GPU the
default raises ``LhviError``."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi

MAX_K = _abi.MIX_MAX_K
_NORMALISERS = {'gaussian': _abi.MIX_GAUSSIAN, 'vi': _abi.MIX_VI}


def _p(a):
    if a is None:
        return C.c_void_p(0)
    return C.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())


def default_lanes(K):
    """lanes per (evidence row, query) item of ``lhvi_mix_marginal_map``: the lanes take the K starts, so the smallest power of
    two >= K, at most a wavefront.  The answer does not depend on it."""
    lanes = 1
    while lanes < min(int(K), 64):
        lanes *= 2
    return lanes


class _Side:
    """the prepared belief on one side (host: NumPy arrays, device: torch tensors) and the C struct that points into it"""

    def __init__(self, host, w, eta_c, eta_d, nstates, lo, hi, K, Dmax, normaliser):
        self.host = host
        V = int(nstates.shape[0])
        has_d = eta_d is not None
        self.keep = (w, eta_c, eta_d, nstates)
        self.nstates, self.lo, self.hi = nstates, lo, hi
        self.logw = self.empty((K,))
        self.rec = self.empty((max(V, 1), K, 3))
        self.lpi = self.empty((max(V, 1), K, Dmax)) if has_d else None
        l = _abi.lib()
        args = (V, K, Dmax, normaliser, _p(w), _p(eta_c), _p(eta_d), _p(nstates), _p(self.logw), _p(self.rec), _p(self.lpi))
        if V:
            _abi.check(l.lhvi_mix_prepare_host(*args) if host else l.lhvi_mix_prepare(*args, _abi.stream_ptr()))
        s = _abi.MixStruct()
        s.V, s.K, s.Dmax = V, K, Dmax
        s.nstates, s.logw, s.rec, s.lpi, s.pi = _p(nstates), _p(self.logw), _p(self.rec), _p(self.lpi), _p(eta_d)
        self.struct = s

    def empty(self, shape, dtype=np.float64):
        if self.host:
            return np.empty(shape, dtype=dtype)
        torch = _abi.require_gpu()
        return torch.empty(tuple(shape), dtype=torch.int32 if dtype == np.int32 else torch.float64, device='cuda')

    def put(self, a, dtype=np.float64):
        if not isinstance(a, np.ndarray) and not self.host:
            return a.contiguous()                # a device tensor already
        a = np.ascontiguousarray(a, dtype=dtype)
        return a if self.host else _abi.to_dev(a)

    @staticmethod
    def numpy(a):
        return a if isinstance(a, np.ndarray) else a.cpu().numpy()


class MixtureBelief:
    """A mixture belief over ``Nc`` continuous rows (``Mu``, ``Var`` [Nc, K]; rows 0 .. Nc - 1) and ``Nd`` discrete rows (``Pi``:
    Nd arrays [K, states_n], or one array [Nd, K, S]; rows Nc .. Nc + Nd - 1) with weights ``w`` [K].  ``bds`` [2, Nc]: lower and
    upper bounds of the continuous rows (default: none).  ``normaliser``: 'gaussian' -- the component density is the normal
    density (``osi/mixture_beliefs.py:538``); 'vi' -- it is ``VarInference.norm_pdf``, which divides by the variance."""

    def __init__(self, w, Mu=None, Var=None, Pi=None, bds=None, normaliser='gaussian'):
        w = np.ascontiguousarray(w, dtype=np.float64).reshape(-1)
        K = int(w.size)
        Nc = 0 if Mu is None else len(Mu)
        Nd = 0 if Pi is None else len(Pi)
        self._check_K(K)
        eta_c = None
        if Nc:
            Mu, Var = np.asarray(Mu, dtype=np.float64), np.asarray(Var, dtype=np.float64)
            if Mu.shape != (Nc, K) or Var.shape != (Nc, K):
                raise ValueError('Mu and Var must be [Nc, K] = [%d, %d]' % (Nc, K))
            eta_c = np.zeros((Nc + Nd, K, 2))
            eta_c[:Nc, :, 0], eta_c[:Nc, :, 1] = Mu, Var
            eta_c[Nc:, :, 1] = 1.0
        nstates = np.zeros(Nc + Nd, dtype=np.int32)
        eta_d, Dmax = None, 1
        if Nd:
            pis = [np.asarray(p, dtype=np.float64) for p in Pi]
            if any(p.ndim != 2 or p.shape[0] != K or p.shape[1] < 1 for p in pis):
                raise ValueError('every Pi[n] must be [K, states] with K = %d' % K)
            nstates[Nc:] = [p.shape[1] for p in pis]
            Dmax = int(nstates.max())
            eta_d = np.zeros((Nc + Nd, K, Dmax))
            for n, p in enumerate(pis):
                eta_d[Nc + n, :, :p.shape[1]] = p
        lo, hi = np.full(Nc + Nd, -np.inf), np.full(Nc + Nd, np.inf)
        if bds is not None and Nc:
            bds = np.asarray(bds, dtype=np.float64)
            lo[:Nc], hi[:Nc] = bds[0], bds[1]
        self._init(K, Dmax, normaliser, dict(w=w, eta_c=eta_c, eta_d=eta_d, nstates=nstates, lo=lo, hi=hi), None)
        self.Nc, self.Nd = Nc, Nd

    @staticmethod
    def _check_K(K):
        if K < 1:
            raise ValueError('a mixture belief needs at least one component')
        if K > MAX_K:
            raise ValueError('K = %d mixture components: the mixture kernels serve K <= LHVI_MIX_MAX_K = %d' % (K, MAX_K))

    def _init(self, K, Dmax, normaliser, host_src, dev_src):
        if normaliser not in _NORMALISERS:
            raise ValueError("normaliser must be 'gaussian' or 'vi', not %r" % (normaliser,))
        self.K, self.Dmax, self.normaliser = int(K), int(Dmax), normaliser
        self._src = {True: host_src, False: dev_src}
        self._from_arrays = host_src is not None
        self._sides = {}
        self.values = {}            # row -> the state values of a discrete row (from_solver): answers are values, not indices
        self.row_value = None       # [V] the value of a row without parameters (evidence of the solver), NaN elsewhere
        self._row_of = None

    @classmethod
    def from_solver(cls, vi, normaliser=None):
        """The belief of a fitted ``VarInference`` / ``LiftedVarInference`` / ``C2FVarInference``: its device tensors are read in
        place (nothing is expanded: a lifted solver's rows are its clusters, and ``row(rv)`` goes through ``rv.cluster``).  Rows
        that were evidence when the solver ran have no parameters: naming one in ``obs`` raises ``ValueError``, as a query it
        returns its value.  ``normaliser`` defaults to the solver's ``belief_normaliser`` ('vi'; 'gaussian' for ``NPVI``).  With ``normaliser='vi'`` and no evidence ``log_belief_all`` is ``log vi.belief(x, rv)``.  The
        records are prepared now: call again after further updates of the solver."""
        if normaliser is None:                       # the density the solver fitted: VarInference's own, NPVI's normal one
            normaliser = getattr(vi, 'belief_normaliser', 'vi')
        if hasattr(vi, '_ensure_dev'):               # (a solver that keeps host copies: bring its device arrays up to date)
            vi._ensure_dev()
        if vi._dev is None:
            raise RuntimeError('the solver has no parameters yet: call init_param() or run() first')
        cls._check_K(vi.K)
        flat, d = vi.flat, vi._dev
        self = cls.__new__(cls)
        nstates = np.where(vi._cont, 0, np.where(vi._disc, flat.var_nstates, -1)).astype(np.int32)
        dom = flat.var_dom.astype(np.int64)
        lo = np.where(vi._cont, flat.dom_lo[dom], -np.inf).astype(np.float64)
        hi = np.where(vi._cont, flat.dom_hi[dom], np.inf).astype(np.float64)
        has_d = bool(vi._disc.any())
        dev = dict(w=d['w'], eta_c=d['eta_c'], eta_d=d['eta_d'] if has_d else None, nstates=_abi.to_dev(nstates),
                   lo=_abi.to_dev(lo), hi=_abi.to_dev(hi))
        self._init(vi.K, vi.Dmax if has_d else 1, normaliser, None, dev)
        self._host_meta = dict(nstates=nstates, lo=lo, hi=hi)
        self.Nc, self.Nd = int(vi._cont.sum()), int(vi._disc.sum())
        for v in np.flatnonzero(vi._disc):
            self.values[int(v)] = np.array(flat.dom_val[flat.dom_ptr[dom[v]]:flat.dom_ptr[dom[v] + 1]])
        self.row_value = np.where(nstates < 0, flat.var_value, np.nan)
        self._row_of = vi._var_index
        return self

    # ---- the two sides -----------------------------------------------------------------------------------------------------
    def _side(self, host):
        host = bool(host)
        if host not in self._sides:
            src = self._src[host]
            if src is None:
                other = self._src[not host]
                if host:
                    src = {k: (None if a is None else _Side.numpy(a)) for k, a in other.items()}
                    src['nstates'] = src['nstates'].astype(np.int32)
                else:
                    _abi.require_gpu()
                    src = {k: (None if a is None else _abi.to_dev(a)) for k, a in other.items()}
                self._src[host] = src
            self._sides[host] = _Side(host, src['w'], src['eta_c'], src['eta_d'], src['nstates'], src['lo'], src['hi'], self.K,
                                      self.Dmax, _NORMALISERS[self.normaliser])
        return self._sides[host]

    @property
    def nstates(self):
        """[V] 0: continuous row, > 0: states of a discrete row, < 0: a row without parameters"""
        meta = getattr(self, '_host_meta', None)
        return meta['nstates'] if meta is not None else self._src[True]['nstates']

    @property
    def V(self):
        return int(self.nstates.shape[0])

    def scalar_mixtures(self, rows=None, host=False):
        """The marginals of the continuous rows ``rows`` (default: every continuous row, in row order) as ``ScalarMixtures``
        [R, K]: the shared weights ``w`` for every row, the row's means and variances.  A belief read from a solver gives
        device tensors (nothing is downloaded), one built from arrays gives arrays; ``host``: whether the result's queries
        (``kl``, ``log_pdf``, ``modes``) run the host twins.  ``ValueError`` unless the normaliser is 'gaussian' (only then is
        a component the normal density) and for a row that is not continuous."""
        from .gmfit import ScalarMixtures
        if self.normaliser != 'gaussian':
            raise ValueError("scalar_mixtures needs the normaliser 'gaussian', not %r: the components of this belief are not "
                             'normal densities' % (self.normaliser,))
        nstates = self.nstates
        rows = np.flatnonzero(nstates == 0) if rows is None else self._rows(rows, 'rows')
        if rows.size and (nstates[rows] != 0).any():
            raise ValueError('rows names a row that is not continuous')
        src = self._src[self._from_arrays]             # the side the belief was built on (the other one is a lazy copy)
        w, eta_c = src['w'], src['eta_c']
        if eta_c is None:
            raise ValueError('the belief has no continuous rows')
        if self._from_arrays:
            mu, var = np.ascontiguousarray(eta_c[rows, :, 0]), np.ascontiguousarray(eta_c[rows, :, 1])
            return ScalarMixtures(np.broadcast_to(w, mu.shape), mu, var, host=host)
        if host:
            raise ValueError('host=True needs a belief built from arrays')
        idx = _abi.to_dev(rows.astype(np.int64), eta_c.device)
        mu, var = eta_c[idx, :, 0].contiguous(), eta_c[idx, :, 1].contiguous()
        return ScalarMixtures(w.reshape(1, -1).expand(mu.shape), mu, var)

    def row(self, rv):
        """the row of a variable of the solver's graph (``from_solver``): a lifted solver answers through ``rv.cluster``"""
        if self._row_of is None:
            raise RuntimeError('this belief was not built from a solver: variables are row indices')
        return int(self._row_of(rv))

    def _rows(self, rows, what):
        rows = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1))
        if rows.size and (rows.min() < 0 or rows.max() >= self.V):
            raise ValueError('%s names a row outside [0, %d)' % (what, self.V))
        return rows.astype(np.int32)

    def _evidence(self, X, obs):
        """(X [M, N_o] float64 on the host or a device tensor, obs int32 [N_o], single): validated"""
        obs = self._rows(obs, 'obs')
        ns = self.nstates[obs]
        if (ns < 0).any():
            raise ValueError('obs names row %d, which has no parameters (it was evidence when the solver ran)'
                             % int(obs[np.flatnonzero(ns < 0)[0]]))
        tensor = not isinstance(X, np.ndarray) and hasattr(X, 'data_ptr')
        Xh = X.detach().cpu().numpy() if tensor else np.asarray(X, dtype=np.float64)
        single = Xh.ndim == 1
        if single:
            Xh = Xh[None, :]
            X = X[None, :] if tensor else X
        if Xh.ndim != 2 or Xh.shape[1] != obs.size:
            raise ValueError('X must be [M, N_o] with N_o = %d observed rows' % obs.size)
        d = ns > 0
        if d.any():
            D = Xh[:, d]
            seen = ~np.isnan(D)
            bad = seen & ~((D == np.floor(D)) & (D >= 0) & (D < ns[d][None, :]))
            if bad.any():
                m, o = np.argwhere(bad)[0]
                raise ValueError('Discrete observations must be integers in [0, states): X[%d, %d] = %r for a row of %d states'
                                 % (m, np.flatnonzero(d)[o], float(D[m, o]), int(ns[d][o])))
        return (X if tensor else Xh), obs, single

    # ---- part 1: conditioning ----------------------------------------------------------------------------------------------
    def _condition(self, X, obs, host, want_comp=True):
        """(side, M, X, obs, comp, logp, condw) as arrays of the side"""
        X, obs, single = self._evidence(X, obs)
        side = self._side(host)
        M, n_obs = int(X.shape[0]), int(obs.size)
        Xs, obs_s = side.put(X), side.put(obs, np.int32)
        l = _abi.lib()
        ws = side.empty((max(int(l.lhvi_mix_condition_ws_doubles(M, n_obs, self.K)), 1),))
        comp = side.empty((M, self.K)) if want_comp else None
        logp, condw = side.empty((M,)), side.empty((M, self.K))
        args = (side.struct, M, n_obs, _p(obs_s), _p(Xs), _p(ws), _p(comp), _p(logp), _p(condw))
        _abi.check(l.lhvi_mix_condition_host(*args) if side.host else l.lhvi_mix_condition(*args, _abi.stream_ptr()))
        return side, M, Xs, obs, comp, logp, condw, single

    def condition(self, X, obs, host=False):
        """``(condw [M, K], logp [M])``: the conditional mixture weights (``calc_cond_mixture_weights`` :677-690) and the marginal
        log probability of the observation (``calc_marg_log_prob`` :663-674) of every evidence row.  A vector X gives a vector and
        a scalar."""
        side, _, _, _, _, logp, condw, single = self._condition(X, obs, host, want_comp=False)
        condw, logp = side.numpy(condw), side.numpy(logp)
        return (condw[0], logp[0]) if single else (condw, logp)

    def comp_log_prob(self, X, obs, host=False):
        """``comp [M, K] = sum_o log q_ok(X[m, o])`` (``_calc_marg_comp_log_prob`` :596-640)"""
        side, _, _, _, comp, _, _, single = self._condition(X, obs, host)
        comp = side.numpy(comp)
        return comp[0] if single else comp

    # ---- part 2: marginal MAP ----------------------------------------------------------------------------------------------
    def _map(self, side, M, condw, query, X=None, obs=None, lanes=None, max_iter=100):
        """(x, f) NumPy [M, N_q] under the weights condw [M, K] (an array of the side); discrete rows as state indices"""
        n_q = int(query.size)
        qptr = qidx = None
        n_obs = 0
        if obs is not None and obs.size:
            n_obs = int(obs.size)
            order = np.argsort(obs, kind='stable')
            so = obs[order]
            ptr = np.zeros(n_q + 1, dtype=np.int32)
            ptr[1:] = np.cumsum(np.searchsorted(so, query, 'right') - np.searchsorted(so, query, 'left'))
            idx = np.concatenate([order[np.searchsorted(so, q, 'left'):np.searchsorted(so, q, 'right')] for q in query] +
                                 [np.zeros(1, dtype=np.int64)]).astype(np.int32)
            qptr, qidx = side.put(ptr, np.int32), side.put(idx, np.int32)
        q_s = side.put(query, np.int32)
        lo = side.lo[q_s.astype(np.int64)] if side.host else side.lo[q_s.long()]
        hi = side.hi[q_s.astype(np.int64)] if side.host else side.hi[q_s.long()]
        lo, hi = side.put(lo), side.put(hi)
        x, f = side.empty((M, n_q)), side.empty((M, n_q))
        l = _abi.lib()
        head = (side.struct, M, _p(condw), n_q, _p(q_s), _p(lo), _p(hi), n_obs, _p(X if qptr is not None else None), _p(qptr),
                _p(qidx))
        if side.host:
            _abi.check(l.lhvi_mix_marginal_map_host(*head, int(max_iter), _p(x), _p(f)))
        else:
            _abi.check(l.lhvi_mix_marginal_map(*head, int(lanes or default_lanes(self.K)), int(max_iter), _p(x), _p(f),
                                               _abi.stream_ptr()))
        return side.numpy(x), side.numpy(f)

    def _finish_map(self, x, query):
        """state indices -> state values where the belief knows them; rows without parameters -> their value"""
        for j, v in enumerate(query):
            v = int(v)
            if v in self.values:
                col = x[:, j]
                ok = ~np.isnan(col)
                col[ok] = self.values[v][col[ok].astype(np.int64)]
            elif self.row_value is not None and self.nstates[v] < 0:
                x[:, j] = self.row_value[v]
        return x

    def marginal_map_all(self, X, obs, query, lanes=None, max_iter=100, host=False, info=False):
        """``[M, N_q]``: the marginal MAP value of every query row given every evidence row (``marginal_map`` :723-746 for every
        pair at once).  A discrete row answers with a state index (with its state VALUE when the belief came from a solver), a
        continuous row with the mode of its conditional mixture inside its bounds, a variable the evidence row observes with
        the observed value.  ``info=True`` also returns the probability (discrete) or log density (continuous) there."""
        side, M, Xs, obs, _, _, condw, single = self._condition(X, obs, host, want_comp=False)
        query = self._rows(query, 'query')
        x, f = self._map(side, M, condw, query, Xs, obs, lanes, max_iter)
        x = self._finish_map(x, query)
        if single:
            x, f = x[0], f[0]
        return (x, f) if info else x

    def map_weights(self, condw, query, lanes=None, max_iter=100, host=False):
        """``(x, f)`` [M, N_q] (discrete rows as state INDICES) under given conditional weights ``condw`` [M, K] or [K]: what
        ``drv_belief_map`` / ``crv_belief_map`` (:693-720) compute for one variable"""
        condw = np.asarray(condw, dtype=np.float64)
        single = condw.ndim == 1
        cw = condw[None, :] if single else condw
        if cw.shape[1] != self.K:
            raise ValueError('condw must have K = %d columns' % self.K)
        side = self._side(host)
        x, f = self._map(side, int(cw.shape[0]), side.put(cw), self._rows(query, 'query'), lanes=lanes, max_iter=max_iter)
        return (x[0], f[0]) if single else (x, f)

    # ---- part 3: log beliefs -----------------------------------------------------------------------------------------------
    def log_belief_all(self, X, obs, query, x, host=False):
        """``out [M, N_q, P] = log sum_k condw[m, k] q_qk(x[q, p])``: the conditional log belief of every query row at ``x``
        [N_q, P] (or [P], the same points for every query): values for a continuous row, state INDICES for a discrete one.
        Without evidence (``obs = []``, ``X`` of shape [M, 0]) it is the log of the fitted marginal belief."""
        side, M, _, _, _, _, condw, single = self._condition(X, obs, host, want_comp=False)
        query = self._rows(query, 'query')
        x = np.asarray(x, dtype=np.float64)
        if x.ndim == 1:
            x = np.broadcast_to(x, (query.size, x.size))
        if x.ndim != 2 or x.shape[0] != query.size:
            raise ValueError('x must be [N_q, P] or [P]')
        P = int(x.shape[1])
        out = side.empty((M, int(query.size), P))
        q_s, x_s = side.put(query, np.int32), side.put(x)       # (named: they must outlive the launch)
        args = (side.struct, M, _p(condw), int(query.size), _p(q_s), P, _p(x_s), _p(out))
        l = _abi.lib()
        _abi.check(l.lhvi_mix_log_belief_host(*args) if side.host else l.lhvi_mix_log_belief(*args, _abi.stream_ptr()))
        out = side.numpy(out)
        return out[0] if single else out

    # ---- part 4: joint MAP -------------------------------------------------------------------------------------------------
    def joint_map(self, rows=None, log_w=None, init_xs=None, coord_its=100, gamma=0.05, grad_lr=0.01, grad_its=500, tol=1e-7,
                  host=False):
        """Joint MAP of the rows ``rows`` (default: every row with parameters) under the fitted weights (or ``log_w``):
        ``joint_map_from_belief_params`` (:771-867) -- from every component k, coordinate ascent on the joint log density
        between the continuous block (``get_multivar_gm_mode`` from the previous point: projected gradient ascent with
        Polyak averaging ``gamma``, step ``grad_lr``, ``grad_its``, ``tol``) and one sweep over the discrete rows.  Returns a
        dict: ``xd`` (state indices) / ``xc`` of the start with the largest objective, in the order of the discrete /
        continuous rows of ``rows`` (None when there are none), and per start ``xds`` [S, Nd], ``xcs`` [S, Nc], ``objs`` [S],
        ``crows`` / ``drows``.  ``init_xs`` [S, Nc]: explicit continuous starts instead of the component means (with no
        discrete rows and ``coord_its=1`` this is ``get_multivar_gm_mode``)."""
        ns_all = self.nstates
        rows = np.flatnonzero(ns_all >= 0).astype(np.int32) if rows is None else self._rows(rows, 'rows')
        if (ns_all[rows] < 0).any():
            raise ValueError('rows names a row without parameters')
        crows, drows = rows[ns_all[rows] == 0], rows[ns_all[rows] > 0]
        Nc, Nd, K = int(crows.size), int(drows.size), self.K
        side = self._side(host)
        src = self._src[True] if self._src[True] is not None else {k: (None if a is None else _Side.numpy(a))
                                                                    for k, a in self._src[False].items()}
        if init_xs is not None:
            if Nd:
                raise ValueError('init_xs is for beliefs without discrete rows')
            x0 = np.ascontiguousarray(np.asarray(init_xs, dtype=np.float64).reshape(-1, Nc))
        else:
            x0 = np.ascontiguousarray(src['eta_c'][crows, :, 0].T) if Nc else np.zeros((K, 0))
        S = int(x0.shape[0])
        xd0 = np.zeros((S, Nd), dtype=np.int32)
        for n, v in enumerate(drows):
            xd0[:, n] = np.argmax(src['eta_d'][v, :, :ns_all[v]], axis=-1)
        if log_w is None:
            logw = side.logw
        else:
            logw = side.put(np.asarray(log_w, dtype=np.float64).reshape(K))
        lo = side.put(_Side.numpy(side.lo)[crows]) if side.host else side.lo[side.put(crows, np.int32).long()].contiguous()
        hi = side.put(_Side.numpy(side.hi)[crows]) if side.host else side.hi[side.put(crows, np.int32).long()].contiguous()
        c_s, d_s, x0_s, xd0_s = side.put(crows, np.int32), side.put(drows, np.int32), side.put(x0), side.put(xd0, np.int32)
        l = _abi.lib()
        ws = side.empty((max(int(l.lhvi_mix_joint_map_ws_doubles(K, Nc, Nd, self.Dmax, S)), 1),))
        xc, xd, objs = side.empty((S, max(Nc, 1))), side.empty((S, max(Nd, 1)), np.int32), side.empty((max(S, 1),))
        args = (side.struct, _p(logw), Nc, _p(c_s), _p(lo), _p(hi), Nd, _p(d_s), S, _p(x0_s), _p(xd0_s), int(coord_its),
                float(gamma), float(grad_lr), int(grad_its), float(tol), _p(ws), _p(xc), _p(xd), _p(objs))
        _abi.check(l.lhvi_mix_joint_map_host(*args) if side.host else l.lhvi_mix_joint_map(*args, _abi.stream_ptr()))
        xcs = side.numpy(xc).reshape(-1)[:S * Nc].reshape(S, Nc)
        xds = side.numpy(xd).reshape(-1)[:S * Nd].reshape(S, Nd)
        objs = side.numpy(objs)[:S]
        i = int(np.argmax(objs))
        return dict(xd=xds[i] if Nd else None, xc=xcs[i] if Nc else None, xds=xds, xcs=xcs, objs=objs, crows=crows, drows=drows)

    def set_belief_params(self, rvs):
        """``rv.belief_params`` = {'mu', 'var'} or {'pi'} of every hidden rv of ``rvs``, as the reference's per-call functions
        (``marginal_map``, ``calc_marg_log_prob`` with ``all_rvs_params=None``) read them"""
        src = self._src[True] or {k: (None if a is None else _Side.numpy(a)) for k, a in self._src[False].items()}
        for rv in rvs:
            v = self.row(rv) if self._row_of is not None else int(rv)
            ns = int(self.nstates[v])
            if ns == 0:
                rv.belief_params = {'mu': src['eta_c'][v, :, 0].copy(), 'var': src['eta_c'][v, :, 1].copy()}
            elif ns > 0:
                rv.belief_params = {'pi': src['eta_d'][v, :, :ns].copy()}


# ---- the NumPy half of osi/mixture_beliefs.py over the kernels ----------------------------------------------------------------
def eval_crvs_comp_log_prob(X, Mu, Var, backend=np):
    """(:521-539) component-wise log densities of N continuous variables, shape [K] + X.shape: slice n of ``X`` [N, ...] is
    evaluated under ``Mu[n]``, ``Var[n]`` ([N, K]).  Elementwise, on the host; the batched sum over observed variables is
    ``MixtureBelief.comp_log_prob``."""
    if backend is not np:
        raise NotImplementedError('the symbolic (TensorFlow) half of osi/mixture_beliefs.py is out of scope')
    X, Mu, Var = np.asarray(X), np.asarray(Mu), np.asarray(Var)
    if Mu.ndim != 2:
        raise ValueError('Mu and Var must be [N, K]')
    shape = Mu.shape[::-1] + (1,) * (X.ndim - 1)             # [K, N, 1, ...]: lines up with X for broadcasting
    mu, var_inv = Mu.T.reshape(shape), 1 / Var.T.reshape(shape)
    return -0.5 * np.log(2 * np.pi) + 0.5 * np.log(var_inv) - 0.5 * (X - mu) ** 2 * var_inv


def eval_drvs_comp_prob(X, Pi):
    """(:542-556) ``out[k, n, m] = Pi[n][k, X[n, m]]`` for integer ``X`` [N, M] and ``Pi[n]`` [K, states_n]"""
    X = np.asarray(X)
    return np.stack([np.asarray(Pi[n])[:, X[n]] for n in range(X.shape[0])], axis=1)


def get_obs_rvs_domain_types_and_params(obs_rvs, all_rvs_params=None, Vc_idx=None, Vd_idx=None):
    """(:559-593) ``(domain types, {'Mu', 'Var' [N_oc, K], 'Pi' [K x states] * N_od})`` of the observed rvs, in their order:
    rows of ``all_rvs_params`` through ``Vc_idx`` / ``Vd_idx`` when given, else the rvs' own ``belief_params``"""
    types = [rv.domain_type for rv in obs_rvs]
    crvs = [rv for rv, t in zip(obs_rvs, types) if t[0] == 'c']
    drvs = [rv for rv, t in zip(obs_rvs, types) if t[0] == 'd']
    params = {}
    if all_rvs_params is None:
        assert all(rv.belief_params for rv in obs_rvs), 'obs_rvs must have belief_params'
        if crvs:
            params['Mu'] = np.stack([rv.belief_params['mu'] for rv in crvs])
            params['Var'] = np.stack([rv.belief_params['var'] for rv in crvs])
        if drvs:
            params['Pi'] = [rv.belief_params['pi'] for rv in drvs]
        return types, params
    if crvs:
        assert Vc_idx is not None
        rows = [Vc_idx[rv] for rv in crvs]
        params['Mu'], params['Var'] = np.asarray(all_rvs_params['Mu'])[rows], np.asarray(all_rvs_params['Var'])[rows]
    if drvs:
        assert Vd_idx is not None
        params['Pi'] = [all_rvs_params['Pi'][Vd_idx[rv]] for rv in drvs]
    return types, params


def _obs_belief(obs_rvs_domain_types, obs_rvs_params, w=None, bds_of=None):
    """(belief over the observed variables, their rows in observation order); bds_of: {position: (lb, ub)} of continuous ones"""
    is_c = np.array([t[0] == 'c' for t in obs_rvs_domain_types], dtype=bool)
    Mu, Var, Pi = obs_rvs_params.get('Mu'), obs_rvs_params.get('Var'), obs_rvs_params.get('Pi')
    Nc = int(is_c.sum())
    K = np.asarray(Mu).shape[1] if Nc else np.asarray(Pi[0]).shape[0]
    rows = np.where(is_c, np.cumsum(is_c) - 1, Nc + np.cumsum(~is_c) - 1)
    bds = None
    if bds_of:
        bds = np.array([[-np.inf] * Nc, [np.inf] * Nc])
        for i, b in bds_of.items():
            bds[:, rows[i]] = b
    belief = MixtureBelief(np.full(K, 1.0 / K) if w is None else w, Mu if Nc else None, Var if Nc else None,
                           Pi if Nc < is_c.size else None, bds)
    return belief, rows


def _calc_marg_comp_log_prob(X, obs_rvs_domain_types, obs_rvs_params, host=False):
    """(:596-640) ``[M, K]`` (or ``[K]`` for a vector X): sum over the observed variables of the component log probabilities"""
    belief, rows = _obs_belief(obs_rvs_domain_types, obs_rvs_params)
    return belief.comp_log_prob(np.asarray(X, dtype=np.float64), rows, host=host)


def _obs_params(obs_rvs, all_rvs_params, g):
    if all_rvs_params is not None:
        assert g is not None
        return get_obs_rvs_domain_types_and_params(obs_rvs, all_rvs_params, g.Vc_idx, g.Vd_idx)
    return get_obs_rvs_domain_types_and_params(obs_rvs)


def calc_marg_comp_log_prob(X, obs_rvs, all_rvs_params=None, g=None):
    """(:643-660)"""
    return _calc_marg_comp_log_prob(X, *_obs_params(obs_rvs, all_rvs_params, g))


def calc_marg_log_prob(X, obs_rvs, w, all_rvs_params=None, g=None):
    """(:663-674) log p(x_o) of every evidence row"""
    belief, rows = _obs_belief(*_obs_params(obs_rvs, all_rvs_params, g), w=w)
    return belief.condition(np.asarray(X, dtype=np.float64), rows)[1]


def calc_cond_mixture_weights(X, obs_rvs, w, all_rvs_params=None, g=None):
    """(:677-690) the weights of the mixture conditioned on every evidence row, [M, K]"""
    belief, rows = _obs_belief(*_obs_params(obs_rvs, all_rvs_params, g), w=w)
    return belief.condition(np.asarray(X, dtype=np.float64), rows)[0]


def drv_belief_map(w, pi):
    """(:693-708) the first state of largest ``w @ pi`` and its probability; ``w`` [K], or [M, K] for M weight vectors at once
    (then M states and the M probabilities of those states: the reference indexes ``state_probs[:, map_states]``, the M x M
    matrix whose diagonal these are)"""
    w = np.asarray(w, dtype=np.float64)
    pi = np.asarray(pi, dtype=np.float64)
    x, f = MixtureBelief(np.full(pi.shape[0], 1.0 / pi.shape[0]), Pi=[pi]).map_weights(w, [0])
    if w.ndim == 1:
        return int(x[0]), float(f[0])
    return x[:, 0].astype(np.int64), f[:, 0]


def crv_belief_map(w, mu, var, bds):
    """(:711-720)"""
    from .utils import get_scalar_gm_mode
    return get_scalar_gm_mode(w, mu, var, bds)


def marginal_map(X, obs_rvs, query_rv, w):
    """(:723-746) the marginal MAP value of ``query_rv`` given one observation X of ``obs_rvs`` (their ``belief_params`` set).
    ``MixtureBelief.marginal_map_all`` is the batched form."""
    rvs = list(obs_rvs) + [query_rv]
    types, params = get_obs_rvs_domain_types_and_params(rvs)
    cont = query_rv.domain_type[0] == 'c'
    belief, rows = _obs_belief(types, params, w=w, bds_of={len(rvs) - 1: (query_rv.values[0], query_rv.values[1])} if cont else None)
    q = int(rows[-1])
    X = np.asarray(X, dtype=np.float64).reshape(1, -1) if obs_rvs else np.zeros((1, 0))
    out = belief.marginal_map_all(X, rows[:-1], [q])[0, 0]
    if query_rv.domain_type[0] == 'd':
        return query_rv.values[int(out)]
    return float(out)


def joint_map_from_belief_params(w, Pi=None, Mu=None, Var=None, bds=None, coord_its=100, **kwargs):
    """(:771-867) ``{'xd', 'xc'}``: the joint MAP configuration found by coordinate ascent from each of the K component modes.
    ``Pi`` [Nd, K, S] (or Nd arrays [K, states_n]: the states may differ per variable, where the reference assumes shared
    ones), ``Mu`` / ``Var`` [Nc, K], ``bds`` [2, Nc]; ``kwargs``: ``gamma``, ``grad_lr``, ``grad_its``, ``tol``, ``host``."""
    r = MixtureBelief(w, Mu, Var, Pi, bds).joint_map(coord_its=coord_its, **kwargs)
    return {'xd': r['xd'], 'xc': r['xc']}


def joint_map(rvs, Vd, Vc, Vd_idx, Vc_idx, params, **kwargs):
    """(:749-768) the joint MAP value of every rv of ``rvs`` from ``params`` = {'w', 'Mu', 'Var', 'Pi'}"""
    bds = np.array([[rv.values[0] for rv in Vc], [rv.values[1] for rv in Vc]], dtype=np.float64) if len(Vc) else None
    val = joint_map_from_belief_params(params['w'], params.get('Pi'), params.get('Mu'), params.get('Var'), bds, **kwargs)
    return np.array([val['xd'][Vd_idx[rv]] if rv.domain_type[0] == 'd' else val['xc'][Vc_idx[rv]] for rv in rvs], dtype=np.float64)
