"""Scalar Gaussian mixtures fitted to samples by EM, every row of an ``[R, n]`` array in one launch (``csrc/gmfit.hip``,
docs/kernels_gmfit.md).

``fit_scalar_gms`` is the batched form of the reference's ``sampling_utils.fit_scalar_gm_from_samples`` (scikit-learn's
``GaussianMixture(n_components=K, covariance_type='diag')`` on one column): the same E- and M-step, ``reg_covar``, ``tol``
and ``max_iter``, on centred samples and from a deterministic start (quantile centres, Lloyd iterations) instead of a
randomly seeded k-means.  ``ScalarMixtures`` holds the fits and answers densities and modes through the mixture kernels
(``csrc/mixture.hip``) and the KL divergence to other mixtures through ``lhvi.gmkl``.

``host=True`` runs the host twin (``lhvi_gm_fit_host``: the device's code with one "lane") on NumPy arrays and needs no GPU;
it is what the CPU tests use.  Nothing switches to it by itself: without a GPU the default raises ``LhviError``."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi

MAX_K = _abi.GMFIT_MAX_K
_GROUP = 32         # rows of one call of the mixture kernels: a call evaluates every row of the group under every row's weights


def _is_tensor(a):
    return not isinstance(a, np.ndarray) and hasattr(a, 'data_ptr')


def _p(a):
    if a is None:
        return C.c_void_p(0)
    return C.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())


class ScalarMixtures:
    """R fitted mixtures: ``w``, ``mu``, ``var`` [R, K], ``lower_bound`` [R] (the mean log likelihood of the last E-step),
    ``n_iter`` [R], ``converged`` [R]; NumPy arrays when the samples were an array, device tensors when they were a tensor.
    ``host``: whether the queries below run the host twins."""

    def __init__(self, w, mu, var, lower_bound=None, n_iter=None, converged=None, host=False):
        self.w, self.mu, self.var = w, mu, var
        self.lower_bound, self.n_iter, self.converged = lower_bound, n_iter, converged
        self.host = bool(host)
        self.R, self.K = int(w.shape[0]), int(w.shape[1])
        self._np = None
        self._modes = {}

    @classmethod
    def from_normals(cls, mu, var, host=False):
        """one normal per row as K = 1 mixtures: ``mu``, ``var`` [R] (arrays or device tensors), weight 1"""
        if _is_tensor(mu):
            mu, var = mu.reshape(-1, 1), var.reshape(-1, 1)
            w = mu.new_ones(mu.shape)
        else:
            mu, var = np.asarray(mu, dtype=np.float64).reshape(-1, 1), np.asarray(var, dtype=np.float64).reshape(-1, 1)
            w = np.ones(mu.shape)
        if tuple(mu.shape) != tuple(var.shape):
            raise ValueError('mu and var must have the same length')
        return cls(w, mu, var, host=host)

    def kl(self, other, a=-np.inf, b=np.inf, rows=None, **kw):
        """``KL(self[r] || other[r])`` over ``[a, b]`` for every row (``lhvi.gmkl.kl_scalar_mixtures``; ``other``: a
        ``ScalarMixtures`` or a ``(w, mu, var)`` tuple).  ``host`` defaults to this object's.  ``other`` may also be a particle
        solver (``EPBP``, ``HybridLBP``): row r is then compared with the belief of the solver's variable ``rows[r]``
        (``kl_from`` of ``lhvi/pbp.py``; on the device only, ``rows`` defaults to every continuous hidden variable)."""
        if hasattr(other, 'kl_from'):
            return other.kl_from(self, rows=rows, a=a, b=b, **kw)
        if rows is not None:
            raise ValueError('rows= goes with a particle solver as the second operand')
        from .gmkl import kl_scalar_mixtures
        kw.setdefault('host', self.host)
        return kl_scalar_mixtures(self, other, a, b, **kw)

    def _params(self):
        if self._np is None:
            self._np = tuple(np.ascontiguousarray(a if isinstance(a, np.ndarray) else a.cpu().numpy(), dtype=np.float64)
                             for a in (self.w, self.mu, self.var))
        return self._np

    def params(self, r):
        """the reference's ``(weights, means, variances)`` of row r (``fit_scalar_gm_from_samples``)"""
        w, mu, var = self._params()
        return w[r].copy(), mu[r].copy(), var[r].copy()

    def _rows(self, rows):
        rows = np.arange(self.R) if rows is None else np.asarray(rows, dtype=np.int64).reshape(-1)
        if rows.size and (rows.min() < 0 or rows.max() >= self.R):
            raise ValueError('rows names a mixture outside [0, %d)' % self.R)
        return rows

    def _belief(self, rows, bds=None):
        """(belief over the mixtures `rows`, its side, their weights as an array of the side)"""
        from .mixture import MixtureBelief
        w, mu, var = self._params()
        belief = MixtureBelief(np.full(self.K, 1.0 / self.K), mu[rows], var[rows], bds=bds)
        side = belief._side(self.host)
        return belief, side, side.put(w[rows])

    def log_pdf(self, x, rows=None):
        """``out [R', P] = log sum_k w[r, k] N(x[r, p]; mu[r, k], var[r, k])`` for the mixtures ``rows`` (default: all R).  ``x``:
        [R', P], or [P] for the same points under every mixture; an array or a device tensor.  The result is of the kind of
        the mixtures.  ``lhvi_mix_log_belief`` over groups of rows, the diagonal kept."""
        rows = self._rows(rows)
        x = np.asarray(x.detach().cpu().numpy() if _is_tensor(x) else x, dtype=np.float64)
        if x.ndim == 1:
            x = np.broadcast_to(x, (rows.size, x.size))
        if x.ndim != 2 or x.shape[0] != rows.size:
            raise ValueError('x must be [%d, P] or [P]' % rows.size)
        P = int(x.shape[1])
        out = np.empty((rows.size, P))
        l = _abi.lib()
        for g0 in range(0, rows.size, _GROUP):
            g = rows[g0:g0 + _GROUP]
            G = int(g.size)
            if P == 0:
                break
            _, side, cw = self._belief(g)
            q_s, x_s, o = side.put(np.arange(G), np.int32), side.put(x[g0:g0 + G]), side.empty((G, G, P))
            args = (side.struct, G, _p(cw), G, _p(q_s), P, _p(x_s), _p(o))
            _abi.check(l.lhvi_mix_log_belief_host(*args) if side.host else l.lhvi_mix_log_belief(*args, _abi.stream_ptr()))
            out[g0:g0 + G] = side.numpy(o)[np.arange(G), np.arange(G)]
        return out if isinstance(self.w, np.ndarray) else _abi.to_dev(out)

    def pdf(self, x, rows=None):
        out = self.log_pdf(x, rows)
        return np.exp(out) if isinstance(out, np.ndarray) else out.exp()

    def modes(self, bds=None, max_iter=100):
        """``(x [R], log_pdf_at_x [R])`` as NumPy arrays: the mode of every mixture inside its bounds ``bds`` [2, R] (default:
        none), by ``lhvi_mix_marginal_map`` (a safeguarded Newton iteration from every component mean, the best kept)"""
        bds = np.array([[-np.inf] * self.R, [np.inf] * self.R]) if bds is None else np.asarray(bds, dtype=np.float64)
        if bds.shape != (2, self.R):
            raise ValueError('bds must be [2, R] = [2, %d]' % self.R)
        key = (bds.tobytes(), int(max_iter))
        if key not in self._modes:
            x, f = np.empty(self.R), np.empty(self.R)
            for g0 in range(0, self.R, _GROUP):
                g = np.arange(g0, min(g0 + _GROUP, self.R))
                belief, side, cw = self._belief(g, bds[:, g])
                xs, fs = belief._map(side, int(g.size), cw, np.arange(g.size, dtype=np.int32), max_iter=max_iter)
                x[g], f[g] = np.diagonal(xs), np.diagonal(fs)
            self._modes[key] = (x, f)
        x, f = self._modes[key]
        return x.copy(), f.copy()


def fit_scalar_gms(x, K, init=None, reg_covar=1e-6, tol=1e-3, max_iter=100, kmeans_its=10, host=False):
    """Fit a K-component Gaussian mixture to every row of ``x`` [R, n] (a 1-D input is one row; a NumPy array or a device
    tensor, fp64) and return ``ScalarMixtures``.  ``init``: ``(w0, mu0, var0)``, each [R, K], as scikit-learn's
    ``weights_init`` / ``means_init`` / ``precisions_init`` (as variances); default: the deterministic start of
    docs/kernels_gmfit.md with ``kmeans_its`` Lloyd iterations.  ``reg_covar``, ``tol``, ``max_iter``: scikit-learn's.
    ``ValueError`` for bad arguments (before any launch) and for a row with a non-finite sample (after it)."""
    tensor = _is_tensor(x)
    if tensor and host:
        raise ValueError('host=True takes a NumPy array')
    if not tensor:
        x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[None, :]
    if x.ndim != 2:
        raise ValueError('x must be [R, n] or [n]')
    R, n, K = int(x.shape[0]), int(x.shape[1]), int(K)
    if K < 1 or K > MAX_K:
        raise ValueError('K = %d components: the fit serves 1 <= K <= LHVI_GMFIT_MAX_K = %d' % (K, MAX_K))
    if R < 1:
        raise ValueError('x has no rows')
    if n < K:
        raise ValueError('n = %d samples per row are fewer than K = %d components' % (n, K))
    if int(max_iter) < 1:
        raise ValueError('max_iter must be positive')
    if int(kmeans_its) < 0:
        raise ValueError('kmeans_its must not be negative')
    if not float(reg_covar) >= 0:
        raise ValueError('reg_covar must not be negative')
    init_h = None
    if init is not None:
        try:
            parts = [np.asarray(a.detach().cpu().numpy() if _is_tensor(a) else a, dtype=np.float64) for a in init]
        except TypeError:
            parts = []
        if len(parts) != 3 or any(a.shape != (R, K) for a in parts):
            raise ValueError('init must be (w0, mu0, var0), each [R, K] = [%d, %d]' % (R, K))
        init_h = np.ascontiguousarray(np.stack(parts, axis=1))            # [R, 3, K]
    l = _abi.lib()
    if host:
        xs = np.ascontiguousarray(x)
        new = lambda shape, dt: np.empty(shape, dtype=dt)                                 # noqa: E731
        init_s = init_h
    else:
        torch = _abi.require_gpu()
        if tensor:
            if x.dtype != torch.float64 or not x.is_cuda:
                raise ValueError('a tensor x must be float64 on the device')
            xs = x.contiguous()
        else:
            xs = _abi.to_dev(x)
        new = lambda shape, dt: torch.empty(shape, dtype=torch.float64 if dt == np.float64 else torch.int32,  # noqa: E731
                                            device=xs.device)
        init_s = None if init_h is None else _abi.to_dev(init_h, xs.device)
    w, mu, var = (new((R, K), np.float64) for _ in range(3))
    lb, n_iter, flags = new((R,), np.float64), new((R,), np.int32), new((R,), np.int32)
    args = (R, n, K, _p(xs), _p(init_s), float(reg_covar), float(tol), int(max_iter), int(kmeans_its), _p(w), _p(mu), _p(var),
            _p(lb), _p(n_iter), _p(flags))
    _abi.check(l.lhvi_gm_fit_host(*args) if host else l.lhvi_gm_fit(*args, _abi.stream_ptr()))
    fl = flags if host else flags.cpu().numpy()
    bad = np.flatnonzero(fl & 2)
    if bad.size:
        raise ValueError('row %d of x holds a non-finite sample' % int(bad[0]))
    if host or tensor:
        conv = (fl & 1).astype(bool) if host else (flags & 1).bool()
        return ScalarMixtures(w, mu, var, lb, n_iter, conv, host=host)
    return ScalarMixtures(w.cpu().numpy(), mu.cpu().numpy(), var.cpu().numpy(), lb.cpu().numpy(), n_iter.cpu().numpy(),
                          (fl & 1).astype(bool), host=False)
