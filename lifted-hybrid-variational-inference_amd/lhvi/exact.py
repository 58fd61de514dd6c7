"""Exact inference in a hybrid Gaussian MRF by enumerating the discrete states (API of ``gibbs/hybrid_gaussian_mrf.py``, the
enumeration half): ``p(x_d, x_c) = p(x_d) N(x_c; mu(x_d), Sig(x_d))``.

``convert_to_bn`` and the ``get_*`` helpers keep the reference's names, argument order and return shapes (NumPy arrays);
``ExactHybridGaussian`` is the solver-shaped form (evidence, automatic conversion of potentials, batched ``map_all`` /
``belief_all``, no full covariances unless asked).  The host flattens the factors once (``flatten_factors``); every
configuration is then one dense fp64 factorisation on the device (``csrc/exact.hip``).  There is no CPU path: without a GPU
the calls raise ``LhviError`` (``config_host`` runs single configurations through the device's code for the tests).
``configs_at`` / ``config_at_host`` are the same computation for explicit rows of discrete digits (``csrc/gibbs_rb.hip``): they
read neither ``M`` nor ``dstride`` and serve the Rao-Blackwellised marginals of ``lhvi/gibbs.py``.

Deliberate differences (docs/kernels_exact.md): the conditional Gaussian comes from a Cholesky factor of ``J = -(A + A^T)``
instead of ``np.linalg.inv(-2A)`` (equal for the symmetric ``A`` every potential class yields); a ``J`` that is not positive
definite raises ``ValueError`` where the reference returns garbage; the marginal MAP of a continuous variable polishes the
best component means by Newton's method instead of starting L-BFGS-B from every one.
"""
from __future__ import annotations

import ctypes as C
import itertools

import numpy as np

from . import _abi, expr, hg_energy
from .potentials import LogHybridQuadratic, LogQuadratic, LogTable
from .utils import get_conditional_quadratic

NotConditionallyQuadratic = expr.NotConditionallyQuadratic
MAX_NC = _abi.EXACT_MAX_NC
CHUNK = 1 << 18                 # configurations of one launch
MAX_CANDIDATES = 1 << 16        # component means map_all evaluates per variable (all of them up to this many)


# ---- host: factors -> flat model ---------------------------------------------------------------------------------------------
class ExactModel:
    """flat form of ``lhvi_exact_t`` (include/lhvi.h) in host arrays"""

    FIELDS = ('dstates', 'dstride', 'quad_ptr', 'quad_desc', 'quad_par', 'tab_ptr', 'tab_desc', 'tab_par')

    def __init__(self, dstates, Nc):
        self.Nd, self.Nc = len(dstates), int(Nc)
        self.dstates = np.asarray(dstates, dtype=np.int32).reshape(-1)
        M = int(np.prod(self.dstates, dtype=object)) if self.Nd else 1
        if M < 2 ** 63:
            self.M = M
            self.dstride = np.array([int(np.prod(self.dstates[i + 1:], dtype=object)) for i in range(self.Nd)], dtype=np.int64)
        else:       # too many configurations to number: only the sampler (lhvi/gibbs.py), which reads neither field, takes it
            self.M, self.dstride = 0, np.zeros(self.Nd, dtype=np.int64)
        self.n_quad = self.n_tab = 0

    def struct(self, ptr_of, keep=None):
        s = _abi.ExactStruct()
        s.Nd, s.Nc, s.M, s.n_quad, s.n_tab = self.Nd, self.Nc, self.M, self.n_quad, self.n_tab
        for name in self.FIELDS:
            setattr(s, name, ptr_of(name))
        return s

    def host_struct(self):
        arrs = {n: np.ascontiguousarray(getattr(self, n)) for n in self.FIELDS}
        s = self.struct(lambda n: C.c_void_p(arrs[n].ctypes.data if arrs[n].size else 0))
        s._keep = arrs
        return s


def _strides(dims):
    return [int(np.prod(dims[i + 1:], dtype=np.int64)) for i in range(len(dims))]


def flatten_factors(factors, dstates, Nc):
    """descriptors of ``factors`` in factor order (the reference's summation order).  Reads ``factor.log_potential_fun``
    (LogQuadratic / LogTable / LogHybridQuadratic) and ``factor.disc_nb_idx / cont_nb_idx`` like ``convert_to_bn`` (:34-49).
    A distinct log potential's parameters are stored once."""
    m = ExactModel(dstates, Nc)
    qdesc, qptr, qpar, qoff, qseen = [], [0], [], 0, {}
    tdesc, tptr, tpar, toff, tseen = [], [0], [], 0, {}
    for f in factors:
        lp = f.log_potential_fun
        dscope, cscope = tuple(int(i) for i in f.disc_nb_idx), tuple(int(i) for i in f.cont_nb_idx)
        if any(not 0 <= i < m.Nd for i in dscope) or any(not 0 <= i < m.Nc for i in cscope):
            raise ValueError('%s: scope index outside Vd / Vc' % f)
        if isinstance(lp, LogQuadratic):
            nc = len(cscope)
            A, b = np.asarray(lp.A, dtype=np.float64).reshape(nc, nc), np.asarray(lp.b, dtype=np.float64).reshape(nc)
            if id(lp) not in qseen:
                qseen[id(lp)] = qoff
                blk = np.concatenate([A.ravel(), b, [float(lp.c)]])
                qpar.append(blk)
                qoff += blk.size
            qdesc += [0, nc, qseen[id(lp)]] + list(cscope)
            qptr.append(len(qdesc))
        elif isinstance(lp, LogHybridQuadratic):
            nc = len(cscope)
            dims = [int(m.dstates[i]) for i in dscope]
            A, b, c = (np.asarray(a, dtype=np.float64) for a in (lp.A, lp.b, lp.c))
            if list(c.shape) != dims or list(A.shape) != dims + [nc, nc] or list(b.shape) != dims + [nc]:
                raise ValueError('%s: LogHybridQuadratic shapes %s / %s / %s do not match its scope' % (f, A.shape, b.shape, c.shape))
            if id(lp) not in qseen:
                qseen[id(lp)] = qoff
                L = int(np.prod(dims, dtype=np.int64))
                blk = np.concatenate([A.reshape(L, nc * nc), b.reshape(L, nc), c.reshape(L, 1)], axis=1).ravel()
                qpar.append(blk)
                qoff += blk.size
            qdesc += [len(dscope), nc, qseen[id(lp)]]
            for i, s in zip(dscope, _strides(dims)):
                qdesc += [i, s]
            qdesc += list(cscope)
            qptr.append(len(qdesc))
        elif isinstance(lp, LogTable):
            dims = [int(m.dstates[i]) for i in dscope]
            t = np.asarray(lp.table, dtype=np.float64)
            if list(t.shape) != dims or cscope:
                raise ValueError('%s: LogTable of shape %s does not match its scope' % (f, t.shape))
            if id(lp) not in tseen:
                tseen[id(lp)] = toff
                tpar.append(t.ravel())
                toff += t.size
            tdesc += [len(dscope), tseen[id(lp)]]
            for i, s in zip(dscope, _strides(dims)):
                tdesc += [i, s]
            tptr.append(len(tdesc))
        else:
            raise TypeError('%s: log_potential_fun must be a LogQuadratic, LogTable or LogHybridQuadratic, not %s'
                            % (f, type(lp).__name__))
    if max(qoff, toff) >= 2 ** 31:
        raise ValueError('potential parameters exceed the 32-bit offsets of the descriptors')
    m.n_quad, m.n_tab = len(qptr) - 1, len(tptr) - 1
    m.quad_ptr, m.quad_desc = np.array(qptr, dtype=np.int32), np.array(qdesc, dtype=np.int32)
    m.quad_par = np.concatenate(qpar) if qpar else np.zeros(0)
    m.tab_ptr, m.tab_desc = np.array(tptr, dtype=np.int32), np.array(tdesc, dtype=np.int32)
    m.tab_par = np.concatenate(tpar) if tpar else np.zeros(0)
    return m


def config_host(model, cfg, cov=False):
    """one configuration on the CPU through the device's code (``lhvi_exact_config_host``): (logp, mean, var, cov or None)"""
    logp, mean, var = np.zeros(1), np.zeros(max(model.Nc, 1)), np.zeros(max(model.Nc, 1))
    cv = np.zeros((model.Nc, model.Nc)) if cov else None
    s = model.host_struct()
    rc = _abi.lib().lhvi_exact_config_host(s, int(cfg), logp.ctypes.data, mean.ctypes.data, var.ctypes.data,
                                           cv.ctypes.data if cov and cv.size else None)
    if rc == _abi.E_NOT_PD:
        raise ValueError(_not_pd_message(model, int(cfg)))
    _abi.check(rc)
    return float(logp[0]), mean[:model.Nc], var[:model.Nc], cv


def _not_pd_message(model, cfg):
    states = tuple(int(s) for s in np.unravel_index(cfg, tuple(model.dstates))) if model.Nd else ()
    return 'the precision matrix J = -2A is not positive definite at the discrete configuration %r' % (states,)


# ---- host: potentials -> the three log-potential classes, evidence ----------------------------------------------------------------
def _mln_log_potential(f, pot):
    """MLNPotential -> LogTable / LogHybridQuadratic / LogQuadratic over the factor's HIDDEN arguments through
    ``expr.conditional_quadratic``; an observed argument enters as a one-state discrete argument of its value"""
    nb = list(f.nb)
    roles = []
    for rv in nb:
        if rv.value is not None:
            roles.append((float(rv.value),))
        else:
            roles.append(None if rv.domain.continuous else tuple(rv.domain.values))
    try:
        program = pot._program_for([rv.domain for rv in nb])
        dims, coef = expr.conditional_quadratic(program, roles)
    except (expr.NotConditionallyQuadratic, expr.FormulaNotTraceable) as exc:
        raise NotConditionallyQuadratic('%s: the MLN formula is not conditionally quadratic (%s)' % (f, exc))
    w = float(pot.w)
    coef = np.asarray(coef, dtype=np.float64).reshape(len(coef), 6)
    keep = [d for d, a in zip(dims, [a for a, r in enumerate(roles) if r is not None]) if nb[a].value is None]
    nc = sum(r is None for r in roles)
    if nc == 0:
        return LogTable(w * coef[:, 5].reshape(keep)) if keep else float(w * coef[0, 5])
    if nc == 1:
        A, b = w * coef[:, 0].reshape(keep + [1, 1]), w * coef[:, 3].reshape(keep + [1])
    else:
        A = w * np.stack([coef[:, 0], coef[:, 1] / 2, coef[:, 1] / 2, coef[:, 2]], axis=1).reshape(keep + [2, 2])
        b = w * coef[:, 3:5].reshape(keep + [2])
    c = w * coef[:, 5].reshape(keep)
    return LogHybridQuadratic(A, b, c) if keep else LogQuadratic(A, b, float(c))


def _state_index(rv):
    vals = list(rv.domain.values)
    if rv.value not in vals:
        raise ValueError('%s is observed at %r, which is none of its states' % (rv, rv.value))
    return vals.index(rv.value)


def _condition(f, lp):
    """``lp`` over f.nb restricted to the hidden arguments: a log potential of the three classes, or a float when every
    argument is observed"""
    nb = list(f.nb)
    if all(rv.value is None for rv in nb):
        return lp
    disc = [rv for rv in nb if not rv.domain.continuous]
    cont = [rv for rv in nb if rv.domain.continuous]
    obs_c = {i: float(rv.value) for i, rv in enumerate(cont) if rv.value is not None}
    if isinstance(lp, LogTable):
        t = np.asarray(lp.table)[tuple(_state_index(rv) if rv.value is not None else slice(None) for rv in disc)]
        return LogTable(t) if t.ndim else float(t)
    if isinstance(lp, LogQuadratic):
        A, b, c = get_conditional_quadratic(lp.A, np.asarray(lp.b), lp.c, obs_c) if obs_c else (lp.A, lp.b, lp.c)
        return LogQuadratic(A, b, c) if len(b) else float(c)
    if isinstance(lp, LogHybridQuadratic):
        sel = tuple(_state_index(rv) if rv.value is not None else slice(None) for rv in disc)
        A, b, c = np.asarray(lp.A)[sel], np.asarray(lp.b)[sel], np.asarray(lp.c)[sel]
        if obs_c:
            dims = list(c.shape)
            n_left = len(cont) - len(obs_c)
            A2, b2, c2 = np.zeros(dims + [n_left, n_left]), np.zeros(dims + [n_left]), np.zeros(dims)
            for idx in itertools.product(*[range(d) for d in dims]):
                A2[idx], b2[idx], c2[idx] = get_conditional_quadratic(A[idx], b[idx], c[idx], obs_c)
            A, b, c = A2, b2, c2
        if b.shape[-1] == 0:
            return LogTable(c) if c.ndim else float(c)
        return LogHybridQuadratic(A, b, c) if c.ndim else LogQuadratic(A, b, float(c))
    raise TypeError('%s: cannot condition a %s' % (f, type(lp).__name__))


def log_potential_of(f, cache=None):
    """the factor's log potential over its hidden arguments as LogQuadratic / LogTable / LogHybridQuadratic (or a float when all
    are observed): ``f.log_potential_fun`` if it is of these classes, else ``f.potential`` converted (``to_log_potential``; an
    MLNPotential through its conditional-quadratic view).  ``cache``: dict shared over the factors of a graph, so that factors
    sharing a potential and an evidence pattern share the result."""
    from .mln import MLNHardPotential, MLNPotential
    from .potentials import ImageEdgePotential, ImageNodePotential
    cache = {} if cache is None else cache
    lp, pot = f.log_potential_fun, f.potential
    src = lp if isinstance(lp, (LogQuadratic, LogTable, LogHybridQuadratic)) else pot
    key = (id(src), tuple((id(rv.domain), rv.value) for rv in f.nb))
    if key in cache:
        return cache[key][1]
    if src is pot:
        if isinstance(pot, (MLNHardPotential, ImageNodePotential, ImageEdgePotential)):
            raise NotImplementedError('%s: %s has no exact hybrid-Gaussian form' % (f, type(pot).__name__))
        if isinstance(pot, MLNPotential):
            out = _mln_log_potential(f, pot)
            cache[key] = (src, out)
            return out
        if pot is None or not hasattr(pot, 'to_log_potential'):
            raise NotImplementedError('%s: no log_potential_fun and no convertible potential' % f)
        lp = pot.to_log_potential()
        if not isinstance(lp, (LogQuadratic, LogTable, LogHybridQuadratic)):
            raise NotImplementedError('%s: %s has no exact hybrid-Gaussian form' % (f, type(pot).__name__))
    out = _condition(f, lp)
    cache[key] = (src, out)          # src kept alive: the key holds its id
    return out


class _Factor:
    """a conditioned factor as ``flatten_factors`` reads it"""

    def __init__(self, origin, lp, disc_nb_idx, cont_nb_idx):
        self.origin, self.log_potential_fun, self.disc_nb_idx, self.cont_nb_idx = origin, lp, disc_nb_idx, cont_nb_idx

    def __str__(self):
        return str(self.origin)


# ---- device ------------------------------------------------------------------------------------------------------------------
def default_lanes(Nc):
    """lanes per configuration of the packed launch: the smallest power of two >= Nc, at least 8"""
    lanes = 8
    while lanes < min(Nc, 64):
        lanes *= 2
    return lanes


def output_bytes(M, Nc, keep_cov):
    """device bytes of the outputs of a run: logp, table, means, variances (, covariances)"""
    return 8 * M * (2 + 2 * Nc + (Nc * Nc if keep_cov else 0))


class _DeviceRun:
    """the enumeration on the device: tensors logp / table [M], logZ [1], means / variances [M, Nc], covs or None, marg"""

    def __init__(self, model, keep_cov, lanes=None, chunk=CHUNK):
        torch = _abi.require_gpu()
        if model.M == 0:
            raise ValueError('the %d discrete variables have more joint states than can be enumerated' % model.Nd)
        if model.Nc > MAX_NC:
            raise ValueError('Nc = %d continuous variables exceed LHVI_EXACT_MAX_NC = %d' % (model.Nc, MAX_NC))
        need = output_bytes(model.M, model.Nc, keep_cov)
        free = int(torch.cuda.mem_get_info()[0])
        if need > free:
            raise MemoryError('%d configurations with Nc = %d%s need %d bytes of device memory for the outputs, %d are free'
                              % (model.M, model.Nc, ' and full covariances' if keep_cov else '', need, free))
        lanes = default_lanes(model.Nc) if lanes is None else int(lanes)
        l, st = _abi.lib(), _abi.stream_ptr()
        self.model, self.lanes = model, lanes
        arrs = {n: getattr(model, n) for n in ExactModel.FIELDS}
        self.t = t = _abi.upload({n: (a if a.size else np.zeros(1, dtype=a.dtype)) for n, a in arrs.items()})
        self.s = s = model.struct(lambda n: _abi.ptr(t[n]))
        dev = t['dstates'].device
        M, Nc = model.M, model.Nc
        f64 = torch.float64
        self.logp = torch.empty(M, dtype=f64, device=dev)
        # Nc = 0: the kernel stores no mean or variance, but the entry point wants real pointers (an empty view has none)
        means_buf = torch.empty(M, max(Nc, 1), dtype=f64, device=dev)
        vars_buf = torch.empty(M, max(Nc, 1), dtype=f64, device=dev)
        self.means, self.vars = means_buf[:, :Nc], vars_buf[:, :Nc]
        self.covs = torch.empty(M, Nc, Nc, dtype=f64, device=dev) if keep_cov else None
        bad = torch.full((1,), -1, dtype=torch.int64, device=dev)            # UINT64_MAX
        for b in range(0, M, int(chunk)):
            _abi.check(l.lhvi_exact_configs(s, b, min(int(chunk), M - b), lanes, _abi.ptr(self.logp), _abi.ptr(means_buf),
                                            _abi.ptr(vars_buf), _abi.ptr(self.covs) if keep_cov and Nc else None,
                                            _abi.ptr(bad), st))
        first = int(bad.item())
        if first != -1:
            raise ValueError(_not_pd_message(model, first))
        self.table = torch.empty(M, dtype=f64, device=dev)
        self.logZ = torch.empty(1, dtype=f64, device=dev)
        ws = torch.empty(2048, dtype=f64, device=dev)
        _abi.check(l.lhvi_exact_normalize(M, _abi.ptr(self.logp), _abi.ptr(self.table), _abi.ptr(self.logZ), _abi.ptr(ws), st))
        n_states = int(model.dstates.sum())
        self.marg = torch.empty(max(n_states, 1), dtype=f64, device=dev)[:n_states]
        _abi.check(l.lhvi_exact_marginals(s, n_states, _abi.ptr(self.table), _abi.ptr(self.marg), st))
        self._mix = None
        self._energies = None

    def config_energies(self):
        """[M] device tensor: the joint log potential of every configuration at its conditional mean (``lhvi_hg_energy`` on the
        run's means, a launch per chunk of the enumeration; computed once)"""
        if self._energies is None:
            torch = _abi._torch()
            M, Nc = self.model.M, self.model.Nc
            out = torch.empty(M, dtype=torch.float64, device=self.logp.device)
            for b in range(0, M, CHUNK):
                n = min(CHUNK, M - b)
                hg_energy.energies(self.s, cfg_range=(b, n), x_c=self.means[b:b + n] if Nc else None, out=out[b:b + n])
            self._energies = out
        return self._energies

    def joint_map(self):
        """(flat configuration index, its energy, its conditional mean [Nc] as an ndarray): the first arg-max of
        ``config_energies()``; only the winner's mean is downloaded"""
        index, value = hg_energy.argmax_first(self.config_energies())
        index = int(index.item())
        if index < 0:
            raise ValueError('every configuration\'s energy is NaN')
        return index, float(value.item()), self.means[index].cpu().numpy()

    def mix(self):
        if self._mix is None:
            torch = _abi._torch()
            M, Nc = self.model.M, self.model.Nc
            self._mix = torch.empty(Nc, M, 3, dtype=torch.float64, device=self.logp.device)
            _abi.check(_abi.lib().lhvi_exact_mix_prepare(Nc, M, _abi.ptr(self.table), _abi.ptr(self.means), _abi.ptr(self.vars),
                                                         _abi.ptr(self._mix), _abi.stream_ptr()))
        return self._mix

    def mixture(self, x):
        """x (Nc, m) device tensor -> (Nc, m, 3): log density, first and second derivative"""
        torch = _abi._torch()
        x = x.contiguous()
        out = torch.empty(x.shape[0], x.shape[1], 3, dtype=torch.float64, device=x.device)
        _abi.check(_abi.lib().lhvi_exact_mixture(self.model.Nc, self.model.M, _abi.ptr(self.mix()), x.shape[1], _abi.ptr(x),
                                                 _abi.ptr(out), _abi.stream_ptr()))
        return out

    def cont_map(self, lo, hi, max_starts=4096, max_iter=100):
        """marginal MAP of every continuous variable: (x [Nc], log density [Nc]) as device tensors"""
        torch = _abi._torch()
        M, Nc = self.model.M, self.model.Nc
        dev = self.logp.device
        cand, lo_d, hi_d = map_candidates(self.table, self.means, self.vars, lo, hi)
        dens = self.mixture(cand)[:, :, 0]
        S = int(min(cand.shape[1], max_starts))
        x = cand.gather(1, dens.topk(S, dim=1).indices).contiguous()
        vmin = self.vars.min(dim=0).values.contiguous()
        logf = torch.empty(Nc, S, dtype=torch.float64, device=dev)
        _abi.check(_abi.lib().lhvi_exact_map_polish(Nc, M, _abi.ptr(self.mix()), S, _abi.ptr(x), _abi.ptr(lo_d), _abi.ptr(hi_d),
                                                    _abi.ptr(vmin), int(max_iter), _abi.ptr(logf), _abi.stream_ptr()))
        best = logf.argmax(dim=1, keepdim=True)
        return x.gather(1, best)[:, 0], logf.gather(1, best)[:, 0]


def map_candidates(weights, means, vars, lo, hi):
    """the starting candidates of the marginal MAP of every variable of a mixture (weights [M], means / vars [M, Nc], device
    tensors; lo / hi [Nc] host arrays): every component mean up to MAX_CANDIDATES components, else the means of the components
    of largest peak density w_k / sqrt(var_kj), clipped to the domain.  Returns (cand [Nc, n], lo, hi on the device); shared by
    the exact baseline and the Rao-Blackwellised mixtures of the Gibbs baseline."""
    torch = _abi._torch()
    if means.shape[0] <= MAX_CANDIDATES:
        cand = means.t().contiguous()
    else:       # the components of largest peak density w_k / sqrt(var_kj)
        score = (weights[:, None] / torch.sqrt(vars)).t()
        cand = means.t().gather(1, score.topk(MAX_CANDIDATES, dim=1).indices).contiguous()
    lo_d, hi_d = _abi.to_dev(np.asarray(lo, dtype=np.float64)), _abi.to_dev(np.asarray(hi, dtype=np.float64))
    return torch.minimum(torch.maximum(cand, lo_d[:, None]), hi_d[:, None]), lo_d, hi_d


def config_at_host(model, x_d):
    """the conditional Gaussian of one row of digits on the CPU through the device's code (``lhvi_exact_config_at_host``):
    (logp, mean, var).  Serves a model with ``M = 0``."""
    row = np.ascontiguousarray(x_d, dtype=np.int32).reshape(model.Nd)
    if model.Nd and (row.min() < 0 or (row >= model.dstates).any()):
        raise ValueError('x_d holds a state outside its variable\'s range')
    logp, mean, var = np.zeros(1), np.zeros(max(model.Nc, 1)), np.zeros(max(model.Nc, 1))
    rc = _abi.lib().lhvi_exact_config_at_host(model.host_struct(), row.ctypes.data if row.size else None, logp.ctypes.data,
                                              mean.ctypes.data, var.ctypes.data)
    if rc == _abi.E_NOT_PD:
        raise ValueError('the precision matrix J = -2A is not positive definite at the discrete state %r'
                         % (tuple(int(k) for k in row),))
    _abi.check(rc)
    return float(logp[0]), mean[:model.Nc], var[:model.Nc]


def configs_at(model, s, rows, lanes=None, chunk=CHUNK):
    """the conditional Gaussians of explicit discrete states on the device (``lhvi_exact_configs_at``): rows [S, Nd] int32 device
    tensor, s the model's device struct.  Returns (logp [S], means [S, Nc], vars [S, Nc]) as device tensors, launched in chunks
    of ``chunk`` rows.  The digits are checked against ``model.dstates`` before the first launch; a row whose J is not positive
    definite raises ``ValueError`` naming the state; ``MemoryError`` with the byte count when the outputs do not fit."""
    torch = _abi.require_gpu()
    S, Nd, Nc = int(rows.shape[0]), model.Nd, model.Nc
    if rows.dim() != 2 or rows.shape[1] != Nd or rows.dtype != torch.int32:
        raise ValueError('rows must be an int32 tensor [S, %d]' % Nd)
    if Nc > MAX_NC:
        raise ValueError('Nc = %d continuous variables exceed LHVI_EXACT_MAX_NC = %d' % (Nc, MAX_NC))
    need = 8 * S * (1 + 2 * max(Nc, 1))
    free = int(torch.cuda.mem_get_info()[0])
    if need > free:
        raise MemoryError('%d discrete states with Nc = %d need %d bytes of device memory for the outputs, %d are free'
                          % (S, Nc, need, free))
    rows = rows.contiguous()
    if S and Nd:
        top = _abi.to_dev(np.asarray(model.dstates, dtype=np.int32))
        if bool(((rows < 0) | (rows >= top[None, :])).any().item()):
            raise ValueError('rows hold a state outside its variable\'s range')
    lanes = default_lanes(Nc) if lanes is None else int(lanes)
    dev, f64 = rows.device, torch.float64
    logp = torch.empty(S, dtype=f64, device=dev)
    means_buf = torch.empty(S, max(Nc, 1), dtype=f64, device=dev)       # real pointers at Nc = 0, as in _DeviceRun
    vars_buf = torch.empty(S, max(Nc, 1), dtype=f64, device=dev)
    bad = torch.full((1,), -1, dtype=torch.int64, device=dev)           # UINT64_MAX
    l, st = _abi.lib(), _abi.stream_ptr()
    for b in range(0, S, int(chunk)):
        n = min(int(chunk), S - b)
        _abi.check(l.lhvi_exact_configs_at(s, n, _abi.ptr(rows[b:]) if Nd else None, lanes, _abi.ptr(logp[b:]),
                                           _abi.ptr(means_buf[b:]), _abi.ptr(vars_buf[b:]), _abi.ptr(bad), st))
        first = int(bad.item())
        if first != -1:
            raise ValueError('the precision matrix J = -2A is not positive definite at the discrete state %r'
                             % (tuple(int(k) for k in rows[b + first].cpu().numpy()),))
    return logp, means_buf[:, :Nc], vars_buf[:, :Nc]


def mixture_run(weights, means, vars):
    """a ``_DeviceRun`` around given mixture parameters on the device (weights [M], means / vars [M, Nc]): its ``mixture`` and
    ``cont_map`` are the exact baseline's kernels on these components"""
    run = _DeviceRun.__new__(_DeviceRun)
    run.model = ExactModel([int(means.shape[0])], int(means.shape[1]))
    run.table = run.logp = weights.contiguous()
    run.means, run.vars = means.contiguous(), vars.contiguous()
    run._mix = None
    return run


# ---- the reference's functions -----------------------------------------------------------------------------------------------
def convert_to_bn(factors, Vd, Vc, return_logZ=False, lanes=None):
    """``hybrid_gaussian_mrf.convert_to_bn`` (:13-73): (disc_marginal_table [v1..vNd], gaussian_means [v1..vNd, Nc],
    gaussian_covs [v1..vNd, Nc, Nc] (, logZ)) as NumPy arrays.  lanes: lanes per configuration of the kernel (default: packed)."""
    dstates = [rv.dstates for rv in Vd]
    model = flatten_factors(factors, dstates, len(Vc))
    run = _DeviceRun(model, keep_cov=True, lanes=lanes)
    Nc = len(Vc)
    table = run.table.cpu().numpy().reshape(dstates)
    means = run.means.cpu().numpy().reshape(dstates + [Nc])
    covs = run.covs.cpu().numpy().reshape(dstates + [Nc, Nc])
    if not return_logZ:
        return table, means, covs
    return table, means, covs, float(run.logZ.item())


def get_crv_marg(disc_marginal_table, gaussian_means, gaussian_covs, crv_idx, flatten_params=True):
    """(:76-95) the univariate mixture of a continuous variable: (weights, means, variances)"""
    out = (disc_marginal_table, gaussian_means[..., crv_idx], gaussian_covs[..., crv_idx, crv_idx])
    return tuple(map(np.ravel, out)) if flatten_params else out


def get_drv_marg(disc_marginal_table, drv_idx):
    """(:98-109)"""
    axes = tuple(a for a in range(np.ndim(disc_marginal_table)) if a != drv_idx)
    return np.sum(disc_marginal_table, axis=axes)


def get_drv_marg_map(disc_marginal_table, drv_idx, best_prob=False):
    """(:112-125)"""
    marg = get_drv_marg(disc_marginal_table, drv_idx)
    state = np.argmax(marg)
    return (state, marg[state]) if best_prob else state


def get_rv_marg_map_from_bn_params(disc_marginal_table, gaussian_means, gaussian_covs, Vd_idx, Vc_idx, rv):
    """(:128-142); the continuous case on the device (``_DeviceRun.cont_map`` on this one variable's mixture)"""
    if rv in Vd_idx:
        return get_drv_marg_map(disc_marginal_table, Vd_idx[rv], best_prob=False)
    w, mu, var = get_crv_marg(disc_marginal_table, gaussian_means, gaussian_covs, Vc_idx[rv], flatten_params=True)
    return float(_mixture_run(w, mu, var).cont_map([rv.values[0]], [rv.values[1]])[0][0].item())


def _mixture_run(w, mu, var):
    """a one-variable _DeviceRun around given mixture parameters"""
    _abi.require_gpu()
    run = _DeviceRun.__new__(_DeviceRun)
    run.model = ExactModel([len(w)], 1)
    run.table = _abi.to_dev(np.ascontiguousarray(w, dtype=np.float64))
    run.logp = run.table
    run.means = _abi.to_dev(np.ascontiguousarray(mu, dtype=np.float64).reshape(-1, 1))
    run.vars = _abi.to_dev(np.ascontiguousarray(var, dtype=np.float64).reshape(-1, 1))
    run._mix = None
    return run


def get_scalar_gm_log_prob(x, w, mu, var):
    """``utils.get_scalar_gm_log_prob`` on the device: the log density of the mixture at the points x (any shape)"""
    x = np.asarray(x, dtype=np.float64)
    out = _mixture_run(w, mu, var).mixture(_abi.to_dev(x.reshape(1, -1)))[0, :, 0]
    return out.cpu().numpy().reshape(x.shape)


def joint_map_from_bn(factors, Vd, Vc):
    """the exact joint MAP as the experiment drivers find it (``osi/hybrid_mln_experiment.py:267-279``): the largest
    ``eval_joint_assignment_energy`` over the discrete configurations at their conditional means ``bn[1][disc_config]``, all on
    the device.  Returns (map_energy, config: tuple of state indices over Vd, xc: ndarray [Nc]); on ties the first
    configuration in C order wins.  The continuous part is not clipped to its domain, as the reference's is not."""
    dstates = [rv.dstates for rv in Vd]
    run = _DeviceRun(flatten_factors(factors, dstates, len(Vc)), keep_cov=False)
    index, energy, xc = run.joint_map()
    return energy, tuple(int(k) for k in np.unravel_index(index, dstates)) if dstates else (), xc


def joint_map_dict(solver, config, index, xc, energy, **extra):
    """the result of ``joint_map()`` of the exact and Gibbs solvers: config (state indices over ``solver.Vd``), index (the flat
    configuration index, None when the configurations cannot be numbered), xd (domain values), xc [Nc], inside (xc within every
    ``rv.values``), energy, assignment ({rv: value} over ``solver.rvs``, evidence included), and what the caller adds"""
    config = tuple(int(k) for k in config)
    xc = np.asarray(xc, dtype=np.float64).reshape(len(solver.Vc))
    xd = tuple(rv.domain.values[k] for rv, k in zip(solver.Vd, config))
    inside = all(rv.domain.values[0] <= x <= rv.domain.values[1] for rv, x in zip(solver.Vc, xc))
    assignment = {}
    for rv in solver.rvs:
        if rv.value is not None:
            assignment[rv] = rv.value
        elif rv in solver.Vd_idx:
            assignment[rv] = xd[solver.Vd_idx[rv]]
        else:
            assignment[rv] = float(xc[solver.Vc_idx[rv]])
    out = dict(config=config, index=index, xd=xd, xc=xc, inside=bool(inside), energy=float(energy), assignment=assignment)
    out.update(extra)
    return out


def states_of(solver, X):
    """(x_d [S, Nd] int32 state indices, x_c [S, Nc]) of the assignments X [S, V] over ``solver.rvs``: discrete columns hold domain
    values, observed columns are ignored; a discrete value that is no state raises ``ValueError``"""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[1] != len(solver.rvs):
        raise ValueError('X must be [S, %d] over the solver\'s rvs' % len(solver.rvs))
    x_d = np.zeros((X.shape[0], len(solver.Vd)), dtype=np.int32)
    x_c = np.zeros((X.shape[0], len(solver.Vc)))
    for v, rv in enumerate(solver.rvs):
        if rv.value is not None:
            continue
        if rv in solver.Vc_idx:
            x_c[:, solver.Vc_idx[rv]] = X[:, v]
            continue
        hit = X[:, v][:, None] == np.asarray(rv.domain.values, dtype=np.float64)[None, :]
        if not hit.any(axis=1).all():
            row = int(np.flatnonzero(~hit.any(axis=1))[0])
            raise ValueError('%s: %r in row %d is none of its states' % (rv, X[row, v], row))
        x_d[:, solver.Vd_idx[rv]] = hit.argmax(axis=1)
    return x_d, x_c


# ---- the solver-shaped class ---------------------------------------------------------------------------------------------------
class ExactHybridGaussian:
    """Exact marginals of a hybrid Gaussian MRF.  ``ExactHybridGaussian(g)`` or ``ExactHybridGaussian(factors=, Vd=, Vc=)``;
    variables with ``rv.value`` set are evidence.  After ``run()``: ``logZ`` (of the conditioned model, constants of fully
    observed factors included), ``disc_table``, ``means``, ``variances`` (NumPy, shaped [v1..vNd(, Nc)]), ``covs`` with
    ``keep_cov``; ``map`` / ``belief`` / ``map_all`` / ``belief_all``; ``config_energies`` / ``joint_map`` (the exact joint MAP, which is
    not ``argmax(disc_table)``: the table carries the mass term -1/2 log det J) and ``energy`` (docs/kernels_hg_energy.md)."""

    def __init__(self, g=None, factors=None, Vd=None, Vc=None):
        if g is not None:
            factors = g.factors_list
            rvs = g.rvs_list
        else:
            if factors is None or Vd is None or Vc is None:
                raise ValueError('ExactHybridGaussian needs a graph, or factors=, Vd= and Vc=')
            rvs = list(Vd) + list(Vc)
        self.rvs = list(rvs)
        self.Vd = [rv for rv in rvs if not rv.domain.continuous and rv.value is None]
        self.Vc = [rv for rv in rvs if rv.domain.continuous and rv.value is None]
        self.Vd_idx = {rv: i for i, rv in enumerate(self.Vd)}
        self.Vc_idx = {rv: i for i, rv in enumerate(self.Vc)}
        self.dstates = [rv.dstates for rv in self.Vd]
        self.log_const = 0.0
        cache, self.factors = {}, []
        for f in factors:
            lp = log_potential_of(f, cache)
            if isinstance(lp, float):
                self.log_const += lp
                continue
            hidden = [rv for rv in f.nb if rv.value is None]
            self.factors.append(_Factor(f, lp, tuple(self.Vd_idx[rv] for rv in hidden if not rv.domain.continuous),
                                        tuple(self.Vc_idx[rv] for rv in hidden if rv.domain.continuous)))
        self.model = flatten_factors(self.factors, self.dstates, len(self.Vc))
        self._run = None
        self._dev_model = None

    def run(self, keep_cov=False, lanes=None):
        self._run = r = _DeviceRun(self.model, keep_cov=keep_cov, lanes=lanes)
        Nc = len(self.Vc)
        self.logZ = float(r.logZ.item()) + self.log_const
        self.disc_table = r.table.cpu().numpy().reshape(self.dstates)
        self.means = r.means.cpu().numpy().reshape(self.dstates + [Nc])
        self.variances = r.vars.cpu().numpy().reshape(self.dstates + [Nc])
        self.covs = r.covs.cpu().numpy().reshape(self.dstates + [Nc, Nc]) if keep_cov else None
        marg = r.marg.cpu().numpy()
        off = np.concatenate([[0], np.cumsum(self.dstates)]).astype(int)
        self.disc_marginals = [marg[off[i]:off[i + 1]] for i in range(len(self.Vd))]
        self._maps = None
        self._config_energies = None
        return self

    def config_energies(self):
        """the joint log potential of every configuration at its conditional mean, ``(x_d, mu(x_d))`` with the evidence in place
        (``log_const`` included, like ``logZ``): an ndarray shaped like ``disc_table``, computed on the device from the run's
        means once per ``run()``"""
        r = self._need_run()
        if self._config_energies is None:
            self._config_energies = (r.config_energies().cpu().numpy() + self.log_const).reshape(self.dstates)
        return self._config_energies

    def joint_map(self):
        """the exact joint MAP: the configuration of largest ``config_energies()`` (the first in C order on ties) with its
        conditional mean, which is not clipped to the domain (``inside`` tells).  A dict: config, index, xd, xc, inside,
        energy, assignment (``joint_map_dict``)."""
        index, energy, xc = self._need_run().joint_map()
        config = np.unravel_index(index, self.dstates) if self.dstates else ()
        return joint_map_dict(self, config, index, xc, energy + self.log_const)

    def energy(self, X, host=False):
        """the joint log potential (``log_const`` included) of the assignments X [S, V] over ``self.rvs`` as an ndarray [S]:
        the driver's ``map_energy`` of any solver's joint MAP on this model.  Discrete columns hold domain values, observed
        columns are ignored.  ``host=True`` runs the kernel's host twin."""
        x_d, x_c = states_of(self, X)
        if host:
            return hg_energy.energies(self.model.host_struct(), x_d=x_d, x_c=x_c, host=True) + self.log_const
        if self._dev_model is None:
            t = _abi.upload({n: (a if a.size else np.zeros(1, dtype=a.dtype))
                             for n, a in ((n, getattr(self.model, n)) for n in ExactModel.FIELDS)})
            self._dev_model = (t, self.model.struct(lambda n: _abi.ptr(t[n])))
        out = hg_energy.energies(self._dev_model[1], x_d=_abi.to_dev(x_d), x_c=_abi.to_dev(x_c))
        return out.cpu().numpy() + self.log_const

    def _need_run(self):
        if self._run is None:
            raise RuntimeError('call run() first')
        return self._run

    def _cont_maps(self, max_starts=4096):
        r = self._need_run()
        if self._maps is None or self._maps[0] != max_starts:
            if self.Vc:
                x, lf = r.cont_map([rv.values[0] for rv in self.Vc], [rv.values[1] for rv in self.Vc], max_starts=max_starts)
                self._maps = (max_starts, x.cpu().numpy(), lf.cpu().numpy())
            else:
                self._maps = (max_starts, np.zeros(0), np.zeros(0))
        return self._maps[1], self._maps[2]

    def map(self, rv, max_starts=4096):
        if rv.value is not None:
            return rv.value
        self._need_run()
        if rv in self.Vd_idx:
            return rv.domain.values[int(np.argmax(self.disc_marginals[self.Vd_idx[rv]]))]
        return float(self._cont_maps(max_starts)[0][self.Vc_idx[rv]])

    def map_all(self, max_starts=4096):
        """(map [V], log belief at the map [V]) over ``self.rvs``; an observed variable returns its value and 0"""
        x, lf = self._cont_maps(max_starts)
        out, val = np.zeros(len(self.rvs)), np.zeros(len(self.rvs))
        for v, rv in enumerate(self.rvs):
            if rv.value is not None:
                out[v] = rv.value
            elif rv in self.Vd_idx:
                marg = self.disc_marginals[self.Vd_idx[rv]]
                k = int(np.argmax(marg))
                out[v], val[v] = rv.domain.values[k], np.log(marg[k])
            else:
                out[v], val[v] = x[self.Vc_idx[rv]], lf[self.Vc_idx[rv]]
        return out, val

    def belief(self, x, rv, log_belief=False):
        """exact marginal at x: the probability of a discrete state, the mixture density of a continuous variable"""
        if rv.value is not None:
            hit = x == rv.value
            return (0 if hit else -np.inf) if log_belief else (1 if hit else 0)
        r = self._need_run()
        if rv in self.Vd_idx:
            vals = list(rv.domain.values)
            p = float(self.disc_marginals[self.Vd_idx[rv]][vals.index(x)]) if x in vals else 0.0
            return np.log(p) if log_belief else p
        torch = _abi._torch()
        pts = torch.zeros(len(self.Vc), 1, dtype=torch.float64, device=r.logp.device)
        pts[self.Vc_idx[rv], 0] = float(x)
        lb = float(r.mixture(pts)[self.Vc_idx[rv], 0, 0].item())
        return lb if log_belief else float(np.exp(lb))

    def marginals(self):
        """the exact marginals of the continuous hidden variables ``self.Vc`` as ``ScalarMixtures`` [Nc, M] on the device: one
        component per discrete configuration, weights the configuration table (shared by the rows), means and variances the
        transposes of the run's arrays -- views, nothing is copied or downloaded.  Evidence has no row, as in ``belief_all``
        (an observed variable is a point mass there); ``marginals().kl(other)`` is the reference's ``kl_err`` per variable."""
        r = self._need_run()
        from .gmfit import ScalarMixtures
        Nc, M = len(self.Vc), self.model.M
        return ScalarMixtures(r.table[None, :].expand(Nc, M), r.means.t(), r.vars.t())

    def belief_all(self, x):
        """exact marginals of every variable of ``self.rvs``: x (V, m).  Continuous hidden rows: the mixture density at x[v, :];
        discrete hidden rows: the marginal of the states in columns [0, #states) (x ignored, 0 beyond); observed rows: 1 where
        x equals the value.  Returns a (V, m) device tensor (what ``lhvi.utils.kl_tables`` takes)."""
        r = self._need_run()
        torch = _abi._torch()
        xq = x if torch.is_tensor(x) else _abi.to_dev(np.ascontiguousarray(x, dtype=np.float64))
        xq = xq.reshape(len(self.rvs), -1)
        m = xq.shape[1]
        out = torch.zeros(len(self.rvs), m, dtype=torch.float64, device=xq.device)
        crows = [v for v, rv in enumerate(self.rvs) if rv in self.Vc_idx]
        if crows:
            idx = torch.tensor(crows, device=xq.device)
            out[idx] = torch.exp(r.mixture(xq[idx])[:, :, 0])
        for v, rv in enumerate(self.rvs):
            if rv.value is not None:
                out[v] = (xq[v] == float(rv.value)).to(torch.float64)
            elif rv in self.Vd_idx:
                k = min(m, rv.dstates)
                out[v, :k] = torch.from_numpy(self.disc_marginals[self.Vd_idx[rv]][:k].copy()).to(xq.device)
        return out
