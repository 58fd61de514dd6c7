"""``KL(p || q)`` of scalar Gaussian mixtures, a batch of rows in one launch (``csrc/gmkl.hip``, docs/kernels_gmkl.md).

``kl_scalar_mixtures`` is the batched form of the reference's ``utils.kl_continuous_logpdf`` for the case its experiment
drivers have: both sides of ``kl_err`` are mixture marginals (the exact baseline's one component per discrete
configuration, the Gibbs fits, the K-component beliefs of the variational solvers, one normal for ``GaBP``).  Knowing that
``p`` is a mixture, the integration is seeded with panels no wider than 8 standard deviations of its narrowest component, so
no component can fall between the nodes of the first pass; each panel is then refined by bisection under QUADPACK's 21-point
Gauss-Kronrod rule.

``kl_mixture_logpdf`` is the same method with any Python log density as ``q`` (``lhvi_gm_kl_fn_host``, on the host only):
the reference's ``kl_continuous_logpdf(log_p = a mixture, log_q = any callable)``.  A particle solver's belief as ``q`` on the
device is ``EPBP.kl_from`` / ``HybridLBP.kl_from`` (``lhvi/pbp.py``, docs/kernels_pbkl.md).

``host=True`` runs the host twin (``lhvi_gm_kl_host``: the device's code, the nodes one after another) on NumPy arrays and
needs no GPU; it is what the CPU tests use.  Nothing switches to it by itself: without a GPU the default raises ``LhviError``."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi

MAX_PANELS = _abi.GMKL_MAX_PANELS
STATUS_TOLERANCE, STATUS_PANEL_CAP, STATUS_INVALID = 1, 2, 4      # the bits of ``status``


def _is_tensor(a):
    return not isinstance(a, np.ndarray) and hasattr(a, 'data_ptr')


def _p(a):
    if a is None:
        return C.c_void_p(0)
    return C.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())


def _parts(m, name):
    if hasattr(m, 'w') and hasattr(m, 'mu') and hasattr(m, 'var'):
        return m.w, m.mu, m.var
    try:
        w, mu, var = m
    except (TypeError, ValueError):
        raise ValueError('%s must be a ScalarMixtures or a (w, mu, var) tuple' % name) from None
    return w, mu, var


class _Numpy:
    tensor = False

    @staticmethod
    def array(a):
        return np.asarray(a, dtype=np.float64)

    @staticmethod
    def rows(a, shape):
        return np.ascontiguousarray(np.broadcast_to(a, shape))

    @staticmethod
    def empty(R, dtype):
        return np.empty(R, dtype=dtype)


class _Torch:
    tensor = True

    def __init__(self, torch, device):
        self.torch, self.device = torch, device

    def array(self, a):
        if _is_tensor(a):
            if a.dtype != self.torch.float64 or a.device != self.device:
                raise ValueError('a tensor operand must be float64 on the current device (%s): the launch goes to its stream'
                                 % self.device)
            return a
        return _abi.to_dev(np.asarray(a, dtype=np.float64), self.device)

    @staticmethod
    def rows(a, shape):
        return a.expand(shape).contiguous()

    def empty(self, R, dtype):
        return self.torch.empty(R, dtype=self.torch.float64 if dtype == np.float64 else self.torch.int32, device=self.device)


def _mixture(kind, m, name):
    """(w, mu, var) of `kind`, each [R' , K] with R' = 1 or the batch (a 1-D array is one row)"""
    parts = [kind.array(a) for a in _parts(m, name)]
    parts = [a[None, :] if a.ndim == 1 else a for a in parts]
    if any(a.ndim != 2 for a in parts) or len({int(a.shape[1]) for a in parts}) != 1:
        raise ValueError('%s: w, mu and var must be [K] or [R, K] with one K' % name)
    if int(parts[0].shape[1]) < 1:
        raise ValueError('%s has no components' % name)
    return parts


def kl_scalar_mixtures(p, q, a=-np.inf, b=np.inf, epsabs=1.49e-8, epsrel=1.49e-8, host=False, info=False):
    """``KL(p[r] || q[r])`` over ``[a[r], b[r]]`` for every row r.  ``p``, ``q``: a ``ScalarMixtures`` or a ``(w, mu, var)`` tuple
    with ``w``, ``mu``, ``var`` each [R, K], or [K] / [1, K] for one row taken for every row (the shared ``w`` of a belief); the
    two sides may differ in K, and a component of weight 0 is skipped (pad ragged rows with zeros).  ``a``, ``b``: scalars or [R].
    Arrays in give an array [R] out; when any operand is a device tensor the work stays on the device and the result is a
    device tensor.  ``info=True`` returns ``(kl, dict(abserr=, status=, neval=))``: the summed error estimates, the status bits
    (1: an interval was accepted above its share of the tolerance, 2: the panel cap ``LHVI_GMKL_MAX_PANELS`` was hit, 4: the
    row is invalid and its result NaN) and the integrand evaluations.  ``ValueError`` for bad shapes or tolerances."""
    parts = list(_parts(p, 'p')) + list(_parts(q, 'q')) + [a, b]
    tensors = [t for t in parts if _is_tensor(t)]
    if tensors and host:
        raise ValueError('host=True takes NumPy arrays')
    if not (float(epsabs) >= 0 and float(epsrel) >= 0):
        raise ValueError('epsabs and epsrel must not be negative')
    if host:
        kind = _Numpy
    else:
        torch = _abi.require_gpu()
        kind = _Torch(torch, torch.device('cuda', torch.cuda.current_device()))
    wp, mup, varp = _mixture(kind, p, 'p')
    wq, muq, varq = _mixture(kind, q, 'q')
    a, b = kind.array(a).reshape(-1), kind.array(b).reshape(-1)
    sizes = {int(t.shape[0]) for t in (wp, mup, varp, wq, muq, varq, a, b)} - {1}
    if len(sizes) > 1:
        raise ValueError('p, q, a and b disagree on the number of rows: %s' % sorted(sizes))
    R = sizes.pop() if sizes else 1
    Kp, Kq = int(mup.shape[1]), int(muq.shape[1])
    wp, mup, varp = (kind.rows(t, (R, Kp)) for t in (wp, mup, varp))
    wq, muq, varq = (kind.rows(t, (R, Kq)) for t in (wq, muq, varq))
    a, b = kind.rows(a, (R,)), kind.rows(b, (R,))
    kl, abserr = kind.empty(R, np.float64), kind.empty(R, np.float64)
    status, neval = kind.empty(R, np.int32), kind.empty(R, np.int32)
    l = _abi.lib()
    head = (R, Kp, _p(wp), _p(mup), _p(varp), Kq, _p(wq), _p(muq), _p(varq), _p(a), _p(b), float(epsabs), float(epsrel))
    tail = (_p(kl), _p(abserr), _p(status), _p(neval))
    if host:
        _abi.check(l.lhvi_gm_kl_host(*head, *tail))
    else:
        n_ws = int(l.lhvi_gm_kl_ws_doubles(R))
        ws = kind.empty(n_ws, np.float64) if n_ws else None
        _abi.check(l.lhvi_gm_kl(*head, _p(ws), *tail, _abi.stream_ptr()))
        if not tensors:
            kl, abserr, status, neval = (t.cpu().numpy() for t in (kl, abserr, status, neval))
    return (kl, dict(abserr=abserr, status=status, neval=neval)) if info else kl


def kl_mixture_logpdf(p, log_q, a=-np.inf, b=np.inf, epsabs=1.49e-8, epsrel=1.49e-8, info=False):
    """``KL(p[r] || q[r])`` over ``[a[r], b[r]]`` with ``q`` given by its log density: ``log_q(x, row) -> float``.  ``p``, ``a``,
    ``b``, the tolerances and ``info`` as for ``kl_scalar_mixtures``; the method is the same (the range and the panels come from
    ``p`` alone), run on the host through a ``ctypes`` callback (``lhvi_gm_kl_fn_host``), so NumPy arrays in and out.  Where
    ``log_q`` is ``-inf`` and ``p`` is not 0 the result is ``+inf`` with status bit 0.  An exception in ``log_q`` is raised
    again after the call."""
    if any(_is_tensor(t) for t in list(_parts(p, 'p')) + [a, b]):
        raise ValueError('kl_mixture_logpdf runs on the host and takes NumPy arrays')
    if not callable(log_q):
        raise ValueError('log_q must be a callable log_q(x, row)')
    if not (float(epsabs) >= 0 and float(epsrel) >= 0):
        raise ValueError('epsabs and epsrel must not be negative')
    kind = _Numpy
    wp, mup, varp = _mixture(kind, p, 'p')
    a, b = kind.array(a).reshape(-1), kind.array(b).reshape(-1)
    sizes = {int(t.shape[0]) for t in (wp, mup, varp, a, b)} - {1}
    if len(sizes) > 1:
        raise ValueError('p, a and b disagree on the number of rows: %s' % sorted(sizes))
    R = sizes.pop() if sizes else 1
    Kp = int(mup.shape[1])
    wp, mup, varp = (kind.rows(t, (R, Kp)) for t in (wp, mup, varp))
    a, b = kind.rows(a, (R,)), kind.rows(b, (R,))
    kl, abserr = kind.empty(R, np.float64), kind.empty(R, np.float64)
    status, neval = kind.empty(R, np.int32), kind.empty(R, np.int32)
    raised = []

    def call(x, row, _user):
        try:
            return float(log_q(x, row))
        except BaseException as exc:        # (an exception cannot cross the C frames: keep the first, finish the row on NaN)
            if not raised:
                raised.append(exc)
            return float('nan')
    cb = _abi.GMKL_LOGQ(call)
    _abi.check(_abi.lib().lhvi_gm_kl_fn_host(R, Kp, _p(wp), _p(mup), _p(varp), cb, None, _p(a), _p(b), float(epsabs), float(epsrel),
                                            _p(kl), _p(abserr), _p(status), _p(neval)))
    if raised:
        raise raised[0]
    return (kl, dict(abserr=abserr, status=status, neval=neval)) if info else kl
