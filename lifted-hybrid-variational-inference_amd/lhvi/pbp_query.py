"""What the queries of ``lhvi/pbp.py`` compute around their launches: pure functions of their arguments -- no library, no GPU.
``expand_rows`` works on tensors, on the device they live on (the CPU in a test); the others on host values."""
from __future__ import annotations

from math import e

import numpy as np


def expand_rows(ptr, rows):
    """The entries of the CSR rows `rows` (int64 tensor: any order, repeats allowed) under the row pointer `ptr` (int64 tensor), row
    after row.  Returns ``(qptr, owner, idx)``: ``qptr [len(rows) + 1]`` is the selection's own row pointer, and entry k of the
    selection belongs to ``rows[owner[k]]`` and sits at position ``idx[k]`` of the arrays `ptr` indexes."""
    import torch
    dev = ptr.device
    deg = ptr[rows + 1] - ptr[rows]
    qptr = torch.zeros(rows.numel() + 1, dtype=torch.int64, device=dev)
    torch.cumsum(deg, 0, out=qptr[1:])
    total = int(qptr[-1].item())
    owner = torch.repeat_interleave(torch.arange(rows.numel(), device=dev), deg, output_size=total)
    idx = ptr[rows][owner] + (torch.arange(total, device=dev) - qptr[:-1][owner])
    return qptr, owner, idx


def domain_bounds(flat, rows=None):
    """``(lo, hi)`` of the domains of the variables `rows` of a ``FlatGraph`` (default: all of them) as host arrays; a discrete
    variable has 0 and 1"""
    cont, dom = (flat.var_cont, flat.var_dom) if rows is None else (flat.var_cont[rows], flat.var_dom[rows])
    return np.where(cont, flat.dom_lo[dom], 0.0), np.where(cont, flat.dom_hi[dom], 1.0)


def balance_shift(values, max_log_value):
    """what ``log_message_balance`` (EPBP:204-215) subtracts from a list of log values: their mean, or ``max - max_log_value`` once
    the maximum lies further than that above the mean"""
    mean_m = float(np.mean(values))
    max_m = max(values)
    return max_m - max_log_value if max_m - mean_m > max_log_value else mean_m


def balanced_trapezoid(y, d, shift, max_log_value):
    """The sum of ``log_area`` (EPBP:291-308, HLBP:324-341): the trapezoid of ``e ** (y - shift)`` for the log values `y` at
    abscissae `d` apart; `shift` None: ``balance_shift`` of them.  Returns (area, shift)."""
    y = list(y)
    if shift is None:
        shift = balance_shift(y, max_log_value)
    res, prev = 0, e ** (y[0] - shift)
    for val in y[1:]:
        cur = e ** (val - shift)
        res += (prev + cur) * d
        prev = cur
    return res * 0.5, shift


def typed_value(rv, m):
    """a batched answer `m` (a float64) as the type a per-variable call returns: float, or the type of a discrete domain's states"""
    return float(m) if rv.domain.continuous else type(rv.domain.values[0])(m)
