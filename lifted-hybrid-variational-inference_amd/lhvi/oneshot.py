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

import numpy as np

from .npvi import NPVI, LiftedNPVI


class OneShot(NPVI):
    """``OneShot(g, K, T, seed=None, Var_bds=None, var_count=None, fac_count=None)``: `g` an object graph or a ``FlatGraph``.
    ``NPVI`` with the entry points of ``csrc/oneshot.hip`` and one more input, ``var_coef``."""

    _stem = 'oneshot'
    _extra = ('var_coef',)

    def __init__(self, g, K, T, seed=None, Var_bds=None, var_count=None, fac_count=None):
        NPVI.__init__(self, g, K, T, Var_bds=Var_bds, seed=seed, var_count=var_count, fac_count=fac_count)

    def _set_flat(self, flat, var_count=None, fac_count=None):
        NPVI._set_flat(self, flat, var_count, fac_count)
        # kappa_v = c_v (1 - deg_v) of the hidden rows, 0 for evidence
        deg = np.add.reduceat(np.concatenate([flat.edge_count[flat.var_edge], [0.0]]), flat.var_ptr[:-1])
        deg = np.where(np.diff(flat.var_ptr) > 0, deg, 0.0)
        cv = np.ones(flat.V) if self.var_count is None else self.var_count
        self.var_coef = np.ascontiguousarray(np.where(flat.var_hidden, cv * (1.0 - deg), 0.0), dtype=np.float64)

    def grad(self, host=False):
        """``(obj, g_tau [K], g_c [V, K, 2] = (d / d Mu, d / d lVar), g_rho [V, K, Dmax])``: the Bethe free energy at the current
        parameters and the gradient of the reference's auxiliary objective"""
        return NPVI.grad(self, host)

    def run(self, its=100, lr=5e-2, fix_mix_its=0, host=False):
        """OneShot.run (OneShot.py:175-310): `its` updates of TensorFlow's Adam from the current parameters; arguments, Adam state
        and the result dictionary are those of ``NPVI.run``, ``record['obj']`` is the Bethe free energy before each update"""
        return NPVI.run(self, its, lr, fix_mix_its, host)


class LiftedOneShot(LiftedNPVI, OneShot):
    """``LiftedOneShot(g, K, T, ...)``: colour passing once, then OneShot on the cluster graph with the cluster sizes as sharing
    counts (OneShot.py:329-353).  `g` as for ``LiftedNPVI``.  After ``run`` the members of a cluster carry its ``belief_params``."""

    def __init__(self, g, K, T, seed=None, Var_bds=None, var_count=None, fac_count=None):
        OneShot.__init__(self, g, K, T, seed=seed, Var_bds=Var_bds, var_count=var_count, fac_count=fac_count)
