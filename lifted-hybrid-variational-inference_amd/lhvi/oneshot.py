"""One-shot marginal inference on the GPU: ``OneShot`` and ``LiftedOneShot`` (the reference's ``osi/OneShot.py``).

The mixture belief of :mod:`lhvi.npvi` -- weights ``w = softmax(tau)``, a Gaussian ``(Mu, exp(lVar))`` per hidden continuous variable
and component, a categorical ``softmax(Rho)`` per hidden discrete one -- fitted to the Bethe free energy

    BFE = sum_f c_f E_b[-log phi_f + log b_f] + sum_v c_v (1 - deg_v) E_b[log b_v]

with TensorFlow's Adam on the reference's auxiliary objective.  The factor term is NPVI's factor kernel with ``log b`` inside the
expectant, the variable term a kernel of its own (``csrc/oneshot.hip``, docs/kernels_oneshot.md); parameters, their layout, the
parameter view, the optimiser and every query are inherited from ``NPVI``: a fit answers ``belief``, ``map_rows_device``,
``mixture_belief`` and ``MixtureBelief.from_solver`` with normal component densities.

``deg_v`` is ``len(rv.nb)``: the number of a variable's edges on a ground graph, and on a lifted graph the ground degree of a member
of the cluster -- the sum of the cluster's edge counts (``SuperRV.nb`` maps a member's ``nb`` and keeps duplicates).

Not reproduced, as for NPVI: ``init_grid`` / ``init_grid_noise``, ``LiftedOneShot2``'s regulariser, ``grad_check``, the per-array
mean-|gradient| records, TensorFlow's random start, ``ignore_const_when_group_eval_LogQuadratic`` (constants are kept).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from .npvi import NPVI, LiftedNPVI, _np_ptr


class OneShot(NPVI):
    """``OneShot(g, K, T, seed=None, Var_bds=None, var_count=None, fac_count=None)``: `g` an object graph or a ``FlatGraph``"""

    def __init__(self, g, K, T, seed=None, Var_bds=None, var_count=None, fac_count=None):
        NPVI.__init__(self, g, K, T, Var_bds=Var_bds, seed=seed, var_count=var_count, fac_count=fac_count)

    def _set_flat(self, flat, var_count=None, fac_count=None):
        NPVI._set_flat(self, flat, var_count, fac_count)
        # kappa_v = c_v (1 - deg_v) of the hidden rows, 0 for evidence
        deg = np.add.reduceat(np.concatenate([flat.edge_count[flat.var_edge], [0.0]]), flat.var_ptr[:-1])
        deg = np.where(np.diff(flat.var_ptr) > 0, deg, 0.0)
        cv = np.ones(flat.V) if self.var_count is None else self.var_count
        self.var_coef = np.ascontiguousarray(np.where(flat.var_hidden, cv * (1.0 - deg), 0.0), dtype=np.float64)

    def _ensure_dev(self):
        d = NPVI._ensure_dev(self)
        if 'var_coef' not in d:
            torch = _abi.require_gpu()
            d['var_coef'] = _abi.to_dev(self.var_coef)
            ws_bytes = int(_abi.lib().lhvi_oneshot_workspace_bytes(self.dg.g, self._struct()))
            d['ws'] = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=self.dg.device)
            d['ws_bytes'] = ws_bytes
        return d

    # ---- objective and gradient -------------------------------------------------------------------------------------------
    def grad(self, host=False):
        """``(obj, g_tau [K], g_c [V, K, 2] = (d / d Mu, d / d lVar), g_rho [V, K, Dmax])``: the Bethe free energy at the current
        parameters and the gradient of the reference's auxiliary objective"""
        l = _abi.lib()
        flat, K = self.flat, self.K
        if host:
            out = dict(obj=np.zeros(1), g_tau=np.zeros(K), g_c=np.zeros((flat.V, K, 2)), g_rho=np.zeros((flat.V, K, self.Dmax)))
            p = self._host_struct()
            _abi.check(l.lhvi_oneshot_grad_host(self._hg.g, self._hg.p, p, _np_ptr(self.var_count), _np_ptr(self.fac_count),
                                                _np_ptr(self.var_coef), _np_ptr(out['obj']), _np_ptr(out['g_tau']),
                                                _np_ptr(out['g_c']), _np_ptr(out['g_rho'])))
            return float(out['obj'][0]), out['g_tau'], out['g_c'], out['g_rho']
        d = self._ensure_dev()
        _abi.check(l.lhvi_oneshot_grad(self.dg.g, self.dg.p, self._struct(), _abi.ptr(d['var_count']), _abi.ptr(d['fac_count']),
                                       _abi.ptr(d['var_coef']), int(self.max_slots), int(self.max_arity), _abi.ptr(d['obj']),
                                       _abi.ptr(d['g_tau']), _abi.ptr(d['g_theta_c']), _abi.ptr(d['g_rho']), _abi.ptr(d['ws']),
                                       d['ws_bytes'], _abi.stream_ptr()))
        return (float(d['obj'].item()), d['g_tau'].cpu().numpy(), d['g_theta_c'].cpu().numpy(), d['g_rho'].cpu().numpy())

    # ---- optimisation -----------------------------------------------------------------------------------------------------
    def run(self, its=100, lr=5e-2, fix_mix_its=0, host=False):
        """OneShot.run (OneShot.py:175-310): `its` updates of TensorFlow's Adam from the current parameters; arguments, Adam state
        and the result dictionary are those of ``NPVI.run``, ``record['obj']`` is the Bethe free energy before each update"""
        its = int(its)
        if its < 0:
            raise ValueError('its must not be negative')
        if fix_mix_its == 'all':
            fix_mix_its = its
        fix_mix_its = int(fix_mix_its)
        l = _abi.lib()
        if host:
            log = np.zeros(max(its, 1))
            h = dict(self._h)
            h.update(obj=np.zeros(1), g_tau=np.zeros(self.K), g_theta_c=np.zeros_like(self._h['theta_c']),
                     g_rho=np.zeros_like(self._h['rho']), mu_lo=self._mu_lo, mu_hi=self._mu_hi, var_count=self.var_count,
                     fac_count=self.fac_count)
            p = self._host_struct()
            o = self._opt_struct(h, _np_ptr, lr)
            _abi.check(l.lhvi_oneshot_run_host(self._hg.g, self._hg.p, p, C.byref(o), _np_ptr(self.var_coef), its, fix_mix_its,
                                               _np_ptr(log)))
            self._dirty = True
            self._cache = {}
        else:
            torch = _abi.require_gpu()
            d = self._ensure_dev()
            log_dev = torch.zeros(max(its, 1), dtype=torch.float64, device=self.dg.device)
            o = self._opt_struct(d, _abi.ptr, lr)
            _abi.check(l.lhvi_oneshot_run(self.dg.g, self.dg.p, self._struct(), C.byref(o), _abi.ptr(d['var_coef']), its, fix_mix_its,
                                          _abi.ptr(log_dev), _abi.ptr(d['ws']), d['ws_bytes'], _abi.stream_ptr()))
            log = log_dev.cpu().numpy()
            self._download()
        self.t += its
        return self._result([float(x) for x in log[:its]])


class LiftedOneShot(LiftedNPVI, OneShot):
    """``LiftedOneShot(g, K, T, ...)``: colour passing once, then OneShot on the cluster graph with the cluster sizes as sharing
    counts (OneShot.py:329-353).  `g` as for ``LiftedNPVI``.  After ``run`` the members of a cluster carry its ``belief_params``."""

    def __init__(self, g, K, T, seed=None, Var_bds=None, var_count=None, fac_count=None):
        OneShot.__init__(self, g, K, T, seed=seed, Var_bds=Var_bds, var_count=var_count, fac_count=fac_count)
