"""Exact marginals of a Gaussian MRF on the device: the ground truth the Gaussian solvers are compared against
(``Demo/RGM/RGMKLDivergence.py``: ``get_conditional_mrf``, ``get_quadratic_params_from_factor_graph``,
``get_gaussian_mean_params_from_quadratic_params`` of ``osi/utils.py``).

The host conditions every factor on the evidence and sorts the entries of the joint quadratic (``sorted_contributions``); the
device sums them into the precision matrix ``J = -(A + A^T)``, factorises it by a blocked dense fp64 Cholesky and forms
``X = L^-1``, from which come the means, the variances, ``log det J`` and any covariance block (``csrc/gauss_exact.hip``).
There is no CPU path: without a GPU the calls raise ``LhviError`` (``host_solve`` runs the same tile routines on the CPU for the
tests).

Deliberate differences (docs/kernels_gauss_exact.md): Cholesky instead of ``np.linalg.inv``; a ``J`` that is not positive
definite raises ``ValueError`` naming the variable of the first bad pivot; sizes beyond the free device memory raise
``MemoryError`` before a launch.
"""
from __future__ import annotations

import numpy as np

from . import _abi
from .flat import flatten
from .potentials import (POT_GAUSSIAN, POT_LINEAR_GAUSSIAN, POT_QUADRATIC, POT_X2, POT_XY, LinearGaussianPotential, LogQuadratic,
                         X2Potential, XYPotential, mu_prec_to_quad_params)
from .utils import get_conditional_quadratic

NB = _abi.GAUSS_EXACT_NB
LOG_2PI = 1.8378770664093453
_INT32_MAX = 2 ** 31 - 1


def _row_quadratic(kind, row):
    """(A, b, c) of a row of the flat potential table (``device_spec`` of the five quadratic classes), or None"""
    if kind == POT_GAUSSIAN:
        n = int(row[0])
        return mu_prec_to_quad_params(row[1:1 + n], row[1 + n:1 + n + n * n].reshape(n, n))
    if kind == POT_QUADRATIC:
        n = int(row[0])
        return row[1:1 + n * n].reshape(n, n), row[1 + n * n:1 + n * n + n], float(row[1 + n * n + n])
    if kind == POT_LINEAR_GAUSSIAN:
        return LinearGaussianPotential(row[0], row[1]).get_quadratic_params()
    if kind == POT_X2:
        return X2Potential(row[0], row[1]).get_quadratic_params()
    if kind == POT_XY:
        return XYPotential(row[0], row[1]).get_quadratic_params()
    return None


def conditioned_quadratics(flat):
    """the factors of a flat graph conditioned on its evidence (``var_value``), in factor order: (params [(A, b, c)], scopes
    [tuple of hidden-variable positions], log constant of the fully observed factors, hidden [N] variable indices).  Raises
    ``ValueError`` on a hidden discrete variable and ``TypeError`` on a factor that is not exp-quadratic."""
    hidden_mask = flat.var_hidden
    bad = np.flatnonzero(hidden_mask & ~flat.var_cont)
    if bad.size:
        raise ValueError('variable %d is discrete and hidden: ExactGaussian takes Gaussian MRFs only (lhvi.exact enumerates '
                         'discrete states)' % int(bad[0]))
    if flat.lifted:
        raise ValueError('ExactGaussian takes a ground graph: a lifted graph\'s cluster multiplicities are not expanded here')
    hidden = np.flatnonzero(hidden_mask)
    pos = np.full(flat.V, -1, dtype=np.int64)
    pos[hidden] = np.arange(hidden.size)
    params, scopes, const, cache = [], [], 0.0, {}
    base = {}
    for f in range(flat.F):
        args = flat.edge_var[flat.fac_ptr[f]:flat.fac_ptr[f + 1]]
        obj = flat.factors[f] if flat.factors else None
        lp = getattr(obj, 'log_potential_fun', None)
        if isinstance(lp, LogQuadratic):
            src = ('lp', id(lp))
            if src not in base:
                n = len(args)
                base[src] = (np.asarray(lp.A, dtype=np.float64).reshape(n, n), np.asarray(lp.b, dtype=np.float64).reshape(n),
                             float(lp.c), lp)
        else:
            p = int(flat.fac_pot[f])
            src = ('pot', p)
            if src not in base:
                q = _row_quadratic(int(flat.pot_kind[p]), flat.pot_param[flat.pot_off[p]:flat.pot_off[p + 1]])
                if q is None:
                    name = type(obj.potential).__name__ if obj is not None else 'potential kind %d' % int(flat.pot_kind[p])
                    raise TypeError('factor %d (%s): %s is not exp-quadratic; ExactGaussian takes GaussianPotential, '
                                    'QuadraticPotential, LinearGaussianPotential, X2Potential, XYPotential or a LogQuadratic '
                                    'log_potential_fun' % (f, obj if obj is not None else 'flat', name))
                base[src] = (np.asarray(q[0], dtype=np.float64), np.asarray(q[1], dtype=np.float64), float(q[2]))
        vals = flat.var_value[args]
        obs = {i: float(v) for i, v in enumerate(vals) if not np.isnan(v)}
        key = (src, tuple(sorted(obs.items())))
        if key not in cache:
            A, b, c = base[src][:3]
            cache[key] = get_conditional_quadratic(A, b, c, obs) if obs else (A, b, c)
        A, b, c = cache[key]
        if len(b) == 0:
            const += float(c)
            continue
        params.append((A, b, c))
        scopes.append(tuple(int(pos[v]) for v, x in zip(args, vals) if np.isnan(x)))
    return params, scopes, const, hidden


def sorted_contributions(params, scopes, N):
    """the terms of the joint quadratic (``utils.get_joint_quadratic_params``) as the device sums them
    (``lhvi_gauss_exact_assemble``): one entry per pair row >= col that some factor touches, holding the terms of A[row][col] and
    then those of A[col][row], each in the reference's (factor, i, j) order; the terms of b by row; c, summed here"""
    rows, cols, vals, brow, bval, c = [], [], [], [], [], 0
    for (A, b, c_), scope in zip(params, scopes):
        s = np.asarray(scope, dtype=np.int64)
        n = s.size
        rows.append(np.repeat(s, n))
        cols.append(np.tile(s, n))
        vals.append(np.asarray(A, dtype=np.float64).reshape(n * n))
        brow.append(s)
        bval.append(np.asarray(b, dtype=np.float64).reshape(n))
        c += c_
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dtype=dt)
    rows, cols, vals = cat(rows, np.int64), cat(cols, np.int64), cat(vals, np.float64)
    brow, bval = cat(brow, np.int64), cat(bval, np.float64)
    R, Cc, upper = np.maximum(rows, cols), np.minimum(rows, cols), (rows < cols).astype(np.int64)
    order = np.lexsort((np.arange(rows.size), upper, Cc, R))          # by (row, col, which triangle, sequence)
    R, Cc, upper, vals = R[order], Cc[order], upper[order], vals[order]
    first = np.ones(R.size, dtype=bool)
    first[1:] = (R[1:] != R[:-1]) | (Cc[1:] != Cc[:-1])
    start = np.flatnonzero(first)
    ent_ptr = np.concatenate([start, [R.size]]).astype(np.int64)
    n_upper = np.add.reduceat(upper, start) if start.size else np.zeros(0, dtype=np.int64)
    ent_mid = (ent_ptr[1:] - n_upper).astype(np.int64)
    border = np.argsort(brow, kind='stable')
    b_ptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(np.bincount(brow, minlength=N), out=b_ptr[1:])
    return dict(ent_row=R[start].astype(np.int32), ent_col=Cc[start].astype(np.int32), ent_ptr=ent_ptr, ent_mid=ent_mid,
                vals=vals, b_ptr=b_ptr, b_vals=bval[border]), c


def output_bytes(N, keep_inverse=False):
    """device bytes of a run on N hidden variables: the packed triangles of L and X = L^-1 (X is needed for the moments whether
    or not it is kept afterwards, so ``keep_inverse`` changes what stays allocated, not this peak), the moments' workspace and
    the vectors"""
    T = (int(N) + NB - 1) // NB
    tri = T * (T + 1) // 2 * NB * NB
    ws = 3 * (T * (T + 1) // 2) * NB + T * NB
    return 8 * (2 * tri + ws + 4 * T * NB + T + 2)


def dense_bytes(N, mu_only=True, a_resident=False):
    """device bytes of ``mean_params_from_quadratic``: ``output_bytes`` plus the dense A (unless it already is a contiguous fp64
    device tensor) and, unless ``mu_only``, the N x N covariance"""
    N = int(N)
    return output_bytes(N, not mu_only) + (0 if a_resident else 8 * N * N) + (0 if mu_only else 8 * N * N)


def _check_memory(N, keep_inverse):
    torch = _abi.require_gpu()
    need, free = output_bytes(N, keep_inverse), int(torch.cuda.mem_get_info()[0])
    if need > free:
        raise MemoryError('the dense factorisation of N = %d variables needs %d bytes of device memory, %d are free'
                          % (N, need, free))


class _NotPD(ValueError):
    def __init__(self, column):
        ValueError.__init__(self, column)
        self.column = column


class _DeviceSolve:
    """one factorisation on the device.  ``fill(Jt, b)`` writes J (a packed triangle, zero on entry) and b [T NB].  Afterwards:
    mu, var (device tensors [N]), logdet (float), Xt (the packed triangle of L^-1)."""

    def __init__(self, N, fill, keep_inverse=False, times=None):
        torch = _abi.require_gpu()
        _check_memory(N, keep_inverse)
        l, st = _abi.lib(), _abi.stream_ptr()
        f64 = torch.float64
        self.N = N = int(N)
        T = (N + NB - 1) // NB
        tri = int(l.lhvi_gauss_exact_tri_doubles(N))
        Lt = torch.zeros(tri, dtype=f64, device='cuda')
        Xt = torch.zeros(tri, dtype=f64, device='cuda')
        b = torch.zeros(T * NB, dtype=f64, device='cuda')
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if times is not None else None
        if ev:
            ev[0].record()
        fill(Lt, b)
        if ev:
            ev[1].record()
        tlog = torch.empty(T, dtype=f64, device='cuda')
        logdet = torch.empty(1, dtype=f64, device='cuda')
        bad = torch.full((1,), _INT32_MAX, dtype=torch.int32, device='cuda')
        _abi.check(l.lhvi_gauss_exact_factor(N, _abi.ptr(Lt), _abi.ptr(Xt), _abi.ptr(tlog), _abi.ptr(bad), _abi.ptr(logdet), st))
        if ev:
            ev[2].record()
        _abi.check(l.lhvi_gauss_exact_inverse(N, _abi.ptr(Lt), _abi.ptr(Xt), st))
        ws = torch.empty(int(l.lhvi_gauss_exact_ws_doubles(N)), dtype=f64, device='cuda')
        mu = torch.empty(T * NB, dtype=f64, device='cuda')
        var = torch.empty(T * NB, dtype=f64, device='cuda')
        _abi.check(l.lhvi_gauss_exact_moments(N, _abi.ptr(Xt), _abi.ptr(b), _abi.ptr(ws), _abi.ptr(mu), _abi.ptr(var), st))
        if ev:
            ev[3].record()
        first = int(bad.item())
        if ev:
            times.update(assemble_ms=ev[0].elapsed_time(ev[1]), factor_ms=ev[1].elapsed_time(ev[2]),
                         inverse_moments_ms=ev[2].elapsed_time(ev[3]))
        if first != _INT32_MAX:
            raise _NotPD(first)
        self.mu, self.var, self.b = mu[:N], var[:N], b[:N]
        self.logdet = float(logdet.item())
        self.Xt = Xt if keep_inverse else None

    def cov(self, cols):
        """Sig[cols][:, cols] as a device tensor"""
        torch = _abi._torch()
        if self.Xt is None:
            raise RuntimeError('cov needs run(keep_inverse=True)')
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        S = int(cols.size)
        if S > 65535:
            raise ValueError('cov takes at most 65535 columns at a time')
        out = torch.empty(S, S, dtype=torch.float64, device='cuda')
        if S:
            cd = _abi.to_dev(cols)
            _abi.check(_abi.lib().lhvi_gauss_exact_cov(self.N, _abi.ptr(self.Xt), S, _abi.ptr(cd), _abi.ptr(out), _abi.stream_ptr()))
        return out


def _assemble_fill(N, contrib):
    def fill(Jt, b):
        t = _abi.upload({k: (a if a.size else np.zeros(1, dtype=a.dtype)) for k, a in contrib.items()})
        fill.keep = t
        _abi.check(_abi.lib().lhvi_gauss_exact_assemble(N, int(contrib['ent_row'].size), _abi.ptr(t['ent_row']), _abi.ptr(t['ent_col']),
                                                        _abi.ptr(t['ent_ptr']), _abi.ptr(t['ent_mid']), _abi.ptr(t['vals']),
                                                        _abi.ptr(t['b_ptr']), _abi.ptr(t['b_vals']), _abi.ptr(Jt), _abi.ptr(b),
                                                        _abi.stream_ptr()))
    return fill


def mean_params_from_quadratic(A, b, mu_only=True, times=None):
    """``utils.get_gaussian_mean_params_from_quadratic_params``: dense A [N][N], b [N] as arrays or device tensors"""
    torch = _abi.require_gpu()
    tensors = torch.is_tensor(A)
    N = int(b.numel()) if torch.is_tensor(b) else int(np.size(b))
    if len(A.shape) != 2 or A.shape[0] != N or A.shape[1] != N:
        raise ValueError('A must be %d x %d to match b' % (N, N))
    resident = tensors and A.is_cuda and A.dtype == torch.float64 and A.is_contiguous()
    need, free = dense_bytes(N, mu_only, resident), int(torch.cuda.mem_get_info()[0])
    if need > free:
        raise MemoryError('the dense factorisation of N = %d variables%s needs %d bytes of device memory, %d are free'
                          % (N, '' if mu_only else ' with the full covariance', need, free))
    Ad = A.to(device='cuda', dtype=torch.float64).contiguous() if tensors else \
        _abi.to_dev(np.ascontiguousarray(A, dtype=np.float64))
    bd = b.to(device='cuda', dtype=torch.float64).reshape(-1) if torch.is_tensor(b) else \
        _abi.to_dev(np.ascontiguousarray(b, dtype=np.float64).reshape(-1))
    if N == 0:
        mu, Sig = torch.zeros(0, dtype=torch.float64, device='cuda'), torch.zeros(0, 0, dtype=torch.float64, device='cuda')
    else:
        if not mu_only and N > 65535:
            raise ValueError('the full covariance of N = %d variables is not formed; use ExactGaussian.cov on a subset' % N)

        def fill(Jt, bp):
            _abi.check(_abi.lib().lhvi_gauss_exact_pack(N, _abi.ptr(Ad), _abi.ptr(Jt), _abi.stream_ptr()))
            bp[:N] = bd
        try:
            s = _DeviceSolve(N, fill, keep_inverse=not mu_only, times=times)
        except _NotPD as e:
            raise ValueError('the precision matrix J = -(A + A^T) is not positive definite: the pivot of column %d is not '
                             'positive' % e.column) from None
        mu = s.mu
        Sig = None if mu_only else s.cov(np.arange(N))
    if not tensors:
        mu = mu.cpu().numpy()
        Sig = None if mu_only else Sig.cpu().numpy()
    return mu if mu_only else (mu, Sig)


def host_solve(J, b):
    """the blocked algorithm on the CPU through the device's tile routines (``lhvi_gauss_exact_host``): (rc, mu, var, log det J,
    first bad column or -1); rc = ``_abi.E_NOT_PD`` when J is not positive definite"""
    import ctypes as C
    J = np.ascontiguousarray(J, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64).reshape(-1)
    N = int(b.size)
    if J.shape != (N, N):
        raise ValueError('J must be %d x %d to match b' % (N, N))
    mu, var, logdet = np.zeros(max(N, 1)), np.zeros(max(N, 1)), np.zeros(1)
    bad = C.c_int64(-1)
    rc = _abi.lib().lhvi_gauss_exact_host(N, J.ctypes.data if N else None, b.ctypes.data if N else None, mu.ctypes.data,
                                          var.ctypes.data, logdet.ctypes.data, C.addressof(bad))
    if rc not in (0, _abi.E_NOT_PD):
        _abi.check(rc)
    return rc, mu[:N], var[:N], float(logdet[0]), int(bad.value)


class ExactGaussian:
    """Exact marginals of a Gaussian MRF.  ``ExactGaussian(g)`` with an object ``Graph`` or the flat arrays of
    ``RelationalGraph.ground_flat(evidence)``, as ``GaBP`` takes them; variables with a value are evidence.  After ``run()``:
    ``get_belief_params`` / ``mu_var`` / ``map`` / ``belief`` / ``map_all`` / ``belief_all`` / ``logZ``, and ``cov(rvs)`` after
    ``run(keep_inverse=True)``."""

    def __init__(self, g=None):
        self.g = g
        self.flat = flat = flatten(g)
        self.factor_params, self.factor_scopes, self.log_const, self.hidden = conditioned_quadratics(flat)
        self.N = int(self.hidden.size)
        self._contrib, self.c = sorted_contributions(self.factor_params, self.factor_scopes, self.N)
        self._run = None
        self._mean = self._var = None

    def joint_quadratic(self):
        """(A, b, c) of the conditioned model as dense NumPy arrays, in the reference's summation order"""
        from .utils import get_joint_quadratic_params
        return get_joint_quadratic_params(self.factor_params, self.factor_scopes, self.N)

    def run(self, keep_inverse=False, times=None):
        _abi.require_gpu()
        V, N = self.flat.V, self.N
        mean, var = np.array(self.flat.var_value, dtype=np.float64), np.zeros(V)
        if N == 0:
            self._run, logdet, mub = None, 0.0, 0.0
        else:
            try:
                self._run = r = _DeviceSolve(N, _assemble_fill(N, self._contrib), keep_inverse=keep_inverse, times=times)
            except _NotPD as e:
                v = int(self.hidden[e.column]) if e.column < N else -1
                name = ' (%s)' % self.flat.rvs[v] if self.flat.rvs and v >= 0 else ''
                raise ValueError('the precision matrix J = -2A is not positive definite: the pivot of variable %d%s is not '
                                 'positive' % (v, name)) from None
            mean[self.hidden], var[self.hidden] = r.mu.cpu().numpy(), r.var.cpu().numpy()
            logdet, mub = r.logdet, float(np.dot(mean[self.hidden], r.b.cpu().numpy()))
        self._mean, self._var = mean, var
        self.logdet = logdet
        self.logZ = N / 2 * LOG_2PI - 0.5 * logdet + 0.5 * mub + float(self.c) + self.log_const
        return self

    def _need_run(self):
        if self._mean is None:
            raise RuntimeError('call run() first')

    def _index(self, rv):
        return int(rv) if isinstance(rv, (int, np.integer)) else self.flat.var_index[rv]

    def _value(self, i):
        v = self.flat.var_value[i]
        return None if np.isnan(v) else float(v)

    @property
    def mu_var(self):
        """(mean [V], variance [V]) in variable-index order; an observed variable has its value and variance 0"""
        self._need_run()
        return self._mean, self._var

    def marginals(self):
        """the marginals of the hidden variables (``self.hidden``, in index order) as K = 1 ``ScalarMixtures``:
        ``ScalarMixtures.from_normals`` of their ``mu_var``.  Evidence has no row (its variance is 0)."""
        from .gmfit import ScalarMixtures
        mean, var = self.mu_var
        return ScalarMixtures.from_normals(mean[self.hidden], var[self.hidden])

    def get_belief_params(self, rv):
        self._need_run()
        i = self._index(rv)
        assert self._value(i) is None
        return float(self._mean[i]), float(self._var[i])

    def map(self, rv):
        self._need_run()
        return float(self._mean[self._index(rv)])

    def map_all(self):
        self._need_run()
        return self._mean.copy()

    def belief(self, x, rv, log_belief=False):
        """the normal density of (mean, variance) at x; an observed variable: the indicator of its value"""
        self._need_run()
        i = self._index(rv)
        val = self._value(i)
        if val is not None:
            hit = x == val
            return (0 if hit else -np.inf) if log_belief else (1 if hit else 0)
        d = x - self._mean[i]
        lb = -0.5 * (LOG_2PI + np.log(self._var[i])) - 0.5 * d * d / self._var[i]
        return lb if log_belief else np.exp(lb)

    def belief_all(self, x):
        """x (V, m) -> (V, m) device tensor: the normal density of every hidden variable at x[v, :], 1 where x equals the value
        of an observed one (what ``lhvi.utils.kl_tables`` takes)"""
        self._need_run()
        torch = _abi.require_gpu()
        xq = x if torch.is_tensor(x) else _abi.to_dev(np.ascontiguousarray(x, dtype=np.float64))
        xq = xq.reshape(self.flat.V, -1)
        mean = _abi.to_dev(self._mean)[:, None]
        hid = _abi.to_dev(self.flat.var_hidden.astype(np.float64))[:, None] > 0
        var = _abi.to_dev(np.where(self.flat.var_hidden, self._var, 1.0))[:, None]
        d = xq - mean
        dens = torch.exp(-0.5 * (LOG_2PI + torch.log(var)) - 0.5 * d * d / var)
        return torch.where(hid, dens, (xq == mean).to(torch.float64))

    def cov(self, rvs):
        """the |S| x |S| block of the covariance matrix of the hidden variables ``rvs`` (NumPy); needs run(keep_inverse=True)"""
        self._need_run()
        idx = [self._index(rv) for rv in rvs]
        pos = np.full(self.flat.V, -1, dtype=np.int64)
        pos[self.hidden] = np.arange(self.N)
        cols = pos[np.asarray(idx, dtype=np.int64)] if idx else np.zeros(0, dtype=np.int64)
        if (cols < 0).any():
            raise ValueError('cov: variable %d is observed' % idx[int(np.flatnonzero(cols < 0)[0])])
        if self._run is None or self._run.Xt is None:
            raise RuntimeError('cov needs run(keep_inverse=True)')
        return self._run.cov(cols).cpu().numpy()
