"""The pure helpers of the particle solvers' queries (lhvi/pbp_query.py) against plain restatements written out here."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import pbp_query_models as pq
from lhvi import pbp_query


# ---- expand_rows -----------------------------------------------------------------------------------------------------------------
def expand_loop(ptr, rows):
    qptr, owner, idx = [0], [], []
    for r, row in enumerate(rows):
        for k in range(ptr[row], ptr[row + 1]):
            owner.append(r)
            idx.append(k)
        qptr.append(len(idx))
    return qptr, owner, idx


def random_ptr(rng, nrows, max_deg, empty_share):
    deg = rng.integers(1, max_deg + 1, nrows) * (rng.random(nrows) >= empty_share)
    return np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)


ROW_CASES = {
    'every row in order': lambda rng, R: np.arange(R),
    'rows in no order': lambda rng, R: rng.permutation(R)[:max(R // 2, 1)],
    'repeated rows': lambda rng, R: rng.integers(0, R, 2 * R),
    'a single row': lambda rng, R: rng.integers(0, R, 1),
    'an empty selection': lambda rng, R: np.zeros(0, dtype=np.int64),
    'empty rows only': None,
}


@pytest.mark.parametrize('case', list(ROW_CASES))
@pytest.mark.parametrize('seed', range(4))
def test_expand_rows_is_the_plain_loop(case, seed):
    rng = np.random.default_rng(seed)
    R = int(rng.integers(1, 40))
    ptr = random_ptr(rng, R, 6, empty_share=(0.0, 0.3, 0.6, 0.9)[seed])
    if ROW_CASES[case] is None:
        rows = np.flatnonzero(np.diff(ptr) == 0)
        if rows.size == 0:                              # (no empty row drawn, as at share 0: make every row empty)
            ptr, rows = np.zeros(R + 1, dtype=np.int64), np.arange(R)
    else:
        rows = np.asarray(ROW_CASES[case](rng, R), dtype=np.int64)
    qptr, owner, idx = pbp_query.expand_rows(torch.from_numpy(ptr), torch.from_numpy(rows))
    assert qptr.dtype == owner.dtype == idx.dtype == torch.int64
    want = expand_loop(ptr.tolist(), rows.tolist())
    assert (qptr.tolist(), owner.tolist(), idx.tolist()) == want
    if case == 'empty rows only':
        assert rows.size and qptr.tolist() == [0] * (rows.size + 1)


def test_expand_rows_cases_hold_what_they_say():
    rng = np.random.default_rng(0)
    rows = ROW_CASES['repeated rows'](rng, 20)
    assert np.unique(rows).size < rows.size
    rows = ROW_CASES['rows in no order'](rng, 20)
    assert (np.diff(rows) < 0).any() and np.unique(rows).size == rows.size
    assert (np.diff(random_ptr(rng, 40, 6, 0.3)) == 0).any()


# ---- domain_bounds ---------------------------------------------------------------------------------------------------------------
def test_domain_bounds_are_the_per_variable_bounds():
    flat = pq.grid_state(8).flat
    assert flat.var_cont.any() and (~flat.var_cont).any() and (~flat.var_hidden).any()
    assert np.unique(flat.dom_lo[flat.var_dom[flat.var_cont]]).size > 1            # more than one continuous domain

    def loop(rows):
        out = []
        for v in rows:
            d = flat.var_dom[v]
            out.append((flat.dom_lo[d], flat.dom_hi[d]) if flat.var_cont[v] else (0.0, 1.0))
        return np.array(out, dtype=np.float64).reshape(-1, 2).T

    lo, hi = pbp_query.domain_bounds(flat)
    want = loop(range(flat.V))
    assert lo.dtype == hi.dtype == np.float64
    np.testing.assert_array_equal(lo, want[0])
    np.testing.assert_array_equal(hi, want[1])
    rng = np.random.default_rng(1)
    for rows in (rng.permutation(flat.V)[:7], rng.integers(0, flat.V, 30), np.flatnonzero(flat.var_hidden), np.zeros(0, dtype=np.int64)):
        lo, hi = pbp_query.domain_bounds(flat, rows)
        want = loop(rows)
        np.testing.assert_array_equal(lo, want[0])
        np.testing.assert_array_equal(hi, want[1])


# ---- balanced_trapezoid ----------------------------------------------------------------------------------------------------------
def trapezoid_restated(values, d, shift, max_log_value):
    """EPBP:291-308 from the tabulated log values on, with ``log_message_balance`` (EPBP:204-215) written in: a dict of the values
    by index, the shift taken off every entry, then the running sum over neighbours"""
    table = {i: v for i, v in enumerate(values)}
    if shift is None:
        mean = float(np.mean(list(table.values())))
        top = max(table.values())
        shift = mean
        if top - mean > max_log_value:
            shift = top - max_log_value
    for i in table:
        table[i] = table[i] - shift
    total = 0
    before = math.e ** table[0]
    for i in range(1, len(table)):
        here = math.e ** table[i]
        total += (before + here) * d
        before = here
    return total * 0.5, shift


def log_values(seed, npts, spread):
    return (np.random.default_rng(seed).normal(0.0, spread, npts) - 3.0).tolist()


@pytest.mark.parametrize('npts', (2, 5, 20))
@pytest.mark.parametrize('seed', range(3))
def test_balanced_trapezoid_shifts_by_the_mean(seed, npts):
    y = log_values(seed, npts, 30.0)
    assert max(y) - float(np.mean(y)) <= 700
    got = pbp_query.balanced_trapezoid(y, 0.37, None, 700)
    assert got == trapezoid_restated(y, 0.37, None, 700)
    assert got[1] == float(np.mean(y)) and got[0] > 0


@pytest.mark.parametrize('npts', (5, 20))
def test_balanced_trapezoid_shifts_by_the_maximum_less_700(npts):
    y = [-1400.0] * npts
    y[npts // 2], y[0] = 12.5, -3.0                 # one high point over a floor: max - mean > 700
    assert max(y) - float(np.mean(y)) > 700
    got = pbp_query.balanced_trapezoid(y, 1.5, None, 700)
    assert got == trapezoid_restated(y, 1.5, None, 700)
    assert got[1] == 12.5 - 700 and np.isfinite(got[0]) and got[0] > 0
    assert pbp_query.balance_shift(y, 700) == 12.5 - 700


@pytest.mark.parametrize('shift', (0.0, -4.25, 611.0))
def test_balanced_trapezoid_takes_a_given_shift(shift):
    y = log_values(7, 5, 3.0)
    got = pbp_query.balanced_trapezoid(y, 0.125, shift, 700)
    assert got == trapezoid_restated(y, 0.125, shift, 700) and got[1] == shift
    assert got != pbp_query.balanced_trapezoid(y, 0.125, None, 700)


@pytest.mark.parametrize('shift', (None, 1.5))
def test_log_area_of_a_callable(shift):
    """``log_area(f, a, b, n)`` with the reference's signature: the restatement on linspace's abscissae, value for value, and the
    NumPy twin of the trapezoid (``pbp_query_models.log_area_twin``: the same sum in another order of additions)"""
    from lhvi.pbp import EPBP, HybridLBP
    f = lambda x: -0.5 * (x - 1.0) ** 2 / 4.0 + math.sin(3.0 * x)
    for cls, a, b, n in ((EPBP, -10.0, 10.0, 20), (HybridLBP, -2.0, 3.5, 5), (EPBP, 0.0, 1e-3, 2)):
        solver = cls.__new__(cls)                       # log_area reads max_log_value only
        x = np.linspace(a, b, n)
        got = solver.log_area(f, a, b, n, shift)
        assert got == trapezoid_restated([f(v) for v in x], x[1] - x[0], shift, 700)
        twin = pq.log_area_twin(lambda xs: np.array([f(v) for v in xs]), a, b, n, shift)
        # the twin adds the n - 1 trapezoids pairwise and uses exp: a few roundings of a sum of positive terms
        assert got[0] == pytest.approx(twin[0], rel=4 * n * np.finfo(np.float64).eps) and got[1] == pytest.approx(twin[1], rel=1e-15, abs=1e-15)


def test_log_message_balance_subtracts_the_shift_in_place():
    from lhvi.pbp import EPBP
    y = log_values(2, 9, 5.0)
    message = dict(enumerate(y))
    shift = EPBP.__new__(EPBP).log_message_balance(message)
    assert shift == pbp_query.balance_shift(y, 700) == float(np.mean(y))
    assert list(message.values()) == [v - shift for v in y]


# ---- typed_value -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('values, continuous, m, want', [
    ((-15.0, 15.0), True, np.float64(2.5), 2.5),
    ((0.0, 1.0, 2.0), False, np.float64(2.0), 2.0),
    ((0, 1), False, np.float64(1.0), 1),
    ((False, True), False, np.float64(1.0), True),
    ((False, True), False, np.float64(0.0), False),
    ((0, 10), True, np.float64(3.0), 3.0),              # continuous: a float, whatever the type of the bounds
])
def test_typed_value(values, continuous, m, want):
    rv = SimpleNamespace(domain=SimpleNamespace(values=values, continuous=continuous))
    got = pbp_query.typed_value(rv, m)
    assert got == want and type(got) is type(want)
