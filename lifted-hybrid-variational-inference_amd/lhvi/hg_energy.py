"""Joint log potentials of assignments of a hybrid Gaussian MRF and the first-index arg-max over them, on the device
(``csrc/hg_energy.hip``, docs/kernels_hg_energy.md): what the joint MAP of the exact and Gibbs baselines is made of
(``lhvi/exact.py``, ``lhvi/gibbs.py``; the reference's ``osi/hybrid_mln_experiment.py:267-279``).

``energies`` is the batched ``eval_joint_assignment_energy`` (``osi/utils.py:164-169``) on the flat model of the exact baseline;
``argmax_first`` the arg-max with a documented tie rule (the smallest index).  Both return device tensors.  ``host=True`` runs
the host twins of the kernels on NumPy arrays, for the tests and for a machine without a GPU; nothing switches to them by
itself.
"""
from __future__ import annotations

import numpy as np

from . import _abi


def _host_ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def energies(model_struct, x_d=None, cfg_range=None, x_c=None, host=False, out=None):
    """the joint log potential of S assignments of the model ``model_struct`` (an ``_abi.ExactStruct``: ``ExactModel.struct`` over
    device tensors, or ``ExactModel.host_struct()`` with ``host=True``).  The discrete states are either ``x_d`` [S, Nd] int32
    state indices or ``cfg_range = (begin, count)``: the configurations begin .. begin + count of the enumeration; ``x_c`` is
    [S, Nc] float64 (None when Nc = 0).  Returns [S] float64: a device tensor (``out`` when given: a contiguous [S] float64
    device tensor, such as a slice of a longer one), or an ndarray with ``host=True``.  The states of ``x_d`` are not checked
    here: the callers validate host input."""
    Nd, Nc = int(model_struct.Nd), int(model_struct.Nc)
    if (x_d is None) == (cfg_range is None):
        raise ValueError('give either x_d or cfg_range')
    if cfg_range is not None:
        begin, S = int(cfg_range[0]), int(cfg_range[1])
        if begin < 0 or S < 0:
            raise ValueError('cfg_range = (begin, count) must not be negative')
    else:
        begin, S = 0, int(x_d.shape[0])
        if tuple(x_d.shape) != (S, Nd):
            raise ValueError('x_d must be [S, %d], not %s' % (Nd, tuple(x_d.shape)))
    if Nc and (x_c is None or tuple(x_c.shape) != (S, Nc)):
        raise ValueError('x_c must be [%d, %d]' % (S, Nc))
    l = _abi.lib()
    if host:
        xd = None if x_d is None else np.ascontiguousarray(x_d, dtype=np.int32)
        xc = np.ascontiguousarray(x_c, dtype=np.float64) if Nc else None
        out = np.zeros(S)           # (`out` is for the device path)
        # explicit digits of an Nd = 0 model: an empty array has no pointer to tell the mode by, and the two modes agree there
        _abi.check(l.lhvi_hg_energy_host(model_struct, S, begin, _host_ptr(xd) if Nd else None, _host_ptr(xc), _host_ptr(out)))
        return out
    torch = _abi.require_gpu()
    if x_d is not None:
        if x_d.dtype != torch.int32 or not x_d.is_contiguous():
            raise ValueError('x_d must be a contiguous int32 device tensor')
    if Nc and (x_c.dtype != torch.float64 or not x_c.is_contiguous()):
        raise ValueError('x_c must be a contiguous float64 device tensor')
    dev = x_c.device if Nc else (x_d.device if x_d is not None else 'cuda')
    if out is None:
        out = torch.empty(S, dtype=torch.float64, device=dev)
    elif out.dtype != torch.float64 or tuple(out.shape) != (S,) or not out.is_contiguous():
        raise ValueError('out must be a contiguous float64 device tensor [%d]' % S)
    _abi.check(l.lhvi_hg_energy(model_struct, S, begin, _abi.ptr(x_d) if x_d is not None and Nd else None,
                                _abi.ptr(x_c) if Nc else None, _abi.ptr(out) if S else None, _abi.stream_ptr()))
    return out


def argmax_first(v, host=False):
    """(index, value) of the largest entry of the flat float64 tensor ``v`` that is not NaN, the smallest index on ties (+0 and
    -0 tie); index -1 and value NaN when there is none.  Returns two one-element device tensors (int64, float64); with
    ``host=True`` ``v`` is an ndarray and the result a pair (int, float)."""
    l = _abi.lib()
    if host:
        a = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
        index, value = np.zeros(1, dtype=np.int64), np.zeros(1)
        _abi.check(l.lhvi_argmax_first_host(a.size, _host_ptr(a), index.ctypes.data, value.ctypes.data))
        return int(index[0]), float(value[0])
    torch = _abi.require_gpu()
    if v.dtype != torch.float64 or not v.is_contiguous():
        raise ValueError('argmax_first takes a contiguous float64 device tensor')
    n = v.numel()
    index = torch.empty(1, dtype=torch.int64, device=v.device)
    value = torch.empty(1, dtype=torch.float64, device=v.device)
    ws = torch.empty(int(l.lhvi_argmax_first_ws_bytes(n)), dtype=torch.uint8, device=v.device)
    _abi.check(l.lhvi_argmax_first(n, _abi.ptr(v) if n else None, _abi.ptr(index), _abi.ptr(value), _abi.ptr(ws), _abi.stream_ptr()))
    return index, value
