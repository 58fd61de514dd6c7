"""The integral-point sums of the heavy f -> v kernel in quarter-wave lane groups (``grid_sums32_rows``, csrc/pbp.hip): the heavy
family alone (LHVI_PBP_F2V_HEAVY) on descriptor lists edited as in tests/test_gpu_pbp_heavy_paths.py, whose helpers this module
imports (that file is not changed).

Per list of 257 rows: every regular point within the recurrence bound of the longdouble twin and every dead point exactly -700.0
(``_hold_to_twin``), nothing non-finite, nothing written outside the edge's points, both statistics counters adding up to the
eligible edges, and the particle columns equal bit for bit to those of the LHVI_PBP_NO_GRID run (the grid block sits between
staging and the rounds, whose round-down windows must hold what they held).

Grid sizes: 1, 7, 8, 9 (one row of lanes, one row exactly, one point of the second row), 31, 32, 33 (a batch short of one
point, full, one point of a second batch), 64, 100, 128 (two full, four with the last partial, four full: GRID_MAX_T).  Partner
counts 24 (GRID_MIN_NJ), 25, 63, 64: padding lanes in the second row of lanes, an odd count, one padding lane, none.  Target
counts 1, 33, 64 (the rounds that follow the grid block: split, idle lanes, straight).

Two more states: the domain [-40, 40], where the range guard sends edges to the direct form -- the guard is restated on the host
from the descriptor's coefficients and the edges it surely refuses must come out bit for bit as in the LHVI_PBP_NO_GRID run --
and v -> f rows of +-550, so that start values and ratios sit next to the guard's limit of 600."""
import numpy as np
import pytest

import test_gpu_pbp_heavy_paths as hp
from test_gpu_pbp_heavy_paths import api  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

N, COUNTERS, ROWS = hp.N, hp.COUNTERS, 257
W_PV, W_PCE, W_COEF = 2, 3, 16          # partner variable, partner's canonical edge, the eight doubles ay by c axy bx kx gx0 gh
GUARD = 600.0


@pytest.fixture(scope='module')
def base128(api):  # noqa: F811
    """[-10, 10] with 128 points: every grid size up to GRID_MAX_T is an edit DOWN"""
    return hp._build(api, -10.0, 10.0, 128)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _runs(api, bp, rows):  # noqa: F811
    """the heavy kernel's messages with the recurrence and with LHVI_PBP_NO_GRID, and the recurrence run's counters, after the
    checks every list gets"""
    nj, npart, T, grid = (rows[:, w] for w in (hp.W_NJ, hp.W_NP, hp.W_T, hp.W_GRID))
    col = np.arange(bp.f2v.shape[1])[None, :]
    written = (col < npart[:, None]) | ((col >= N) & (col < N + T[:, None]))
    heavy, tick = hp._run(api, bp, rows, api.PBP_F2V_HEAVY)
    assert np.isfinite(heavy).all()
    assert (heavy[~written] == 0).all()
    eligible = (grid == 1) & (nj >= hp.GRID_MIN_NJ) & (T <= 128)
    n_grid, n_direct = int(tick[COUNTERS]), int(tick[COUNTERS + 1])
    assert n_grid + n_direct == int(eligible.sum())
    hp._hold_to_twin(bp, rows, heavy)
    direct, tick1 = hp._run(api, bp, rows, api.PBP_F2V_HEAVY, extra=api.PBP_NO_GRID)
    assert int(tick1[COUNTERS]) == 0 and np.isfinite(direct).all()
    assert (_bits(direct[:, :N]) == _bits(heavy[:, :N])).all()
    print('recurrence (%d edges) vs direct (%d): max |d| = %.3g' % (n_grid, n_direct, float(np.abs(heavy - direct).max())))
    return heavy, direct, n_grid, n_direct


CASES = ([(T, 64, 64) for T in (1, 7, 8, 9, 31, 32, 33, 64, 100, 128)] + [(100, nj, 64) for nj in (24, 25, 63)] +
         [(100, 64, npart) for npart in (1, 33)] + [(9, 25, 33), (33, 63, 1), (128, 24, 33), (7, 24, 1), (31, 63, 33)])


@pytest.mark.parametrize('T,nj,npart', CASES)
def test_rows_layout_on_edited_lists(api, base128, T, nj, npart):  # noqa: F811
    bp, rows = base128
    rows = hp._edit(rows[:ROWS], nj=nj, npart=npart, T=T)
    heavy, direct, n_grid, n_direct = _runs(api, bp, rows)
    assert n_grid > ROWS // 2                          # [-10, 10]: the guard refuses few edges, if any
    _hold_guard(bp, rows, heavy, direct, n_direct)
    np.testing.assert_allclose(heavy, direct, rtol=1e-12, atol=1e-12)


def _guard_bound(bp, rows):
    """the range guard of the heavy kernel restated in float64: max over the partner particles of |a_j| + (|b_j| + |kx| X) X"""
    if getattr(bp, '_host_state', None) is None:
        bp._host_state = hp._HostState(bp)
    st = bp._host_state
    ay, by, c, axy, bx, kx, gx0, gh = np.ascontiguousarray(rows[:, W_COEF:W_COEF + 16]).view(np.float64).T[:, :, None]
    y, m = st.old_particles[rows[:, W_PV]], st.v2f[rows[:, W_PCE]]
    a, b = (ay * y + by) * y + c + m, axy * y + bx
    X = np.maximum(np.abs(gx0), np.abs(gx0 + (rows[:, hp.W_T] - 1)[:, None] * gh))
    bound = (np.abs(b) + np.abs(kx) * X) * X + np.abs(a)
    live = np.arange(N)[None, :] < rows[:, hp.W_NJ][:, None]
    return np.where(live, bound, 0.0).max(axis=1)


def _hold_guard(bp, rows, heavy, direct, n_direct):
    """the edges the guard surely refuses (1e-9 off the limit: the device forms a_j with fused multiply-adds) took the direct form"""
    bound = _guard_bound(bp, rows)
    refused, unsure = bound > GUARD * (1 + 1e-9), np.abs(bound - GUARD) <= GUARD * 1e-9
    assert int(refused.sum()) <= n_direct <= int(refused.sum()) + int(unsure.sum())
    assert (_bits(heavy[refused]) == _bits(direct[refused])).all()
    taken = ~refused & ~unsure
    print('guard: %d refused, %d unsure; largest bound of an edge on the recurrence %.1f' % (refused.sum(), unsure.sum(), bound[taken].max() if taken.any() else 0.0))
    return refused, taken


def test_range_guard_sends_edges_to_the_direct_form(api):  # noqa: F811
    bp, rows = hp._build(api, -40.0, 40.0, 32)
    rows = rows[:ROWS]
    assert (rows[:, hp.W_GRID] == 1).all()
    heavy, direct, n_grid, n_direct = _runs(api, bp, rows)
    refused, taken = _hold_guard(bp, rows, heavy, direct, n_direct)
    assert refused.any() and n_direct > 0
    np.testing.assert_allclose(heavy, direct, rtol=1e-12, atol=1e-12)


def test_messages_next_to_the_guard_limit(api):  # noqa: F811
    """v -> f rows of +550 (two of three edges) and -550: |a_j| of the start values is 550 plus the potential's own terms"""
    import torch
    bp, rows = hp._build(api, -10.0, 10.0, 100)
    rows = rows[:ROWS]
    pce = torch.from_numpy(rows[:, W_PCE].astype(np.int64)).to(bp.v2f.device)
    sign = torch.from_numpy(np.where(np.arange(ROWS) % 3 == 2, -550.0, 550.0)).to(bp.v2f.device)
    bp.v2f[pce] = sign[:, None].expand(-1, bp.v2f.shape[1]).to(bp.v2f.dtype)
    bp._host_state = None
    heavy, direct, n_grid, n_direct = _runs(api, bp, rows)
    refused, taken = _hold_guard(bp, rows, heavy, direct, n_direct)
    assert n_grid > 0 and taken.any()
    assert _guard_bound(bp, rows)[taken].max() > 550.0
    np.testing.assert_allclose(heavy[taken], direct[taken], rtol=1e-12, atol=1e-12)
