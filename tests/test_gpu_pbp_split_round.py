"""The split round of the heavy f -> v kernel (``fast_accumulate_floor_split``, csrc/pbp.hip) against the loop it replaces for
the full particle round: the heavy family alone (LHVI_PBP_F2V_HEAVY) on descriptor lists edited as in
tests/test_gpu_pbp_heavy_paths.py, whose helpers this module imports (that file is not changed), into an output table filled
with NaN, once as built and once with LHVI_PBP_NO_SPLIT_ROUND.

Per list the WHOLE table must come out bit for bit the same either way -- the rows the launch does not own included, which are
still NaN -- with the grid recurrence and with LHVI_PBP_NO_GRID on both sides (then only the particle round differs); the run
without the flag is held to the longdouble twin of tests/pbp_f2v_models.py (``_hold_to_twin``: regular points within the derived
bound, dead points exactly -700.0).

The graph: V = 3000, n = 64, a uniform grid of T = 32 points and one of T = 100 (four batches of the recurrence behind the staging
that the split round reads).  The lists have 67 rows: more than one workgroup, an odd count.  Partner counts (word 7): 64 ... 60
(every remainder of four), 33, 32, 31 (the last iteration with one record, none, three), 24 and 23 (GRID_MIN_NJ: from 24 on the
grid points leave the rounds and the particle round is the full round of 64 points that splits; below, the rounds serve 64 + T
points with the other loop, T <= 64), 5, 2, 1.  Below GRID_MIN_NJ the split round is reached with a grid of no points (word 9 = 0):
there one half-wave's chains are all padding (1, 2), and the particle columns must be those of the same list with its grid points,
which the other loop computed.  An observed partner (one term, no particle row read), and a target count below 64 (word 8), which
must not take the split round.  A list long enough for the ticketed work cursor gives the same bits either way too."""
import numpy as np
import pytest

import pbp_f2v_models as fm  # noqa: F401  (the twin behind hp._hold_to_twin)
import test_gpu_pbp_heavy_paths as hp
from test_gpu_pbp_heavy_paths import api  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

N, ROWS = hp.N, 67
NJ = [64, 63, 62, 61, 60, 33, 32, 31, 24, 23, 5, 2, 1]


@pytest.fixture(scope='module')
def graphs(api):  # noqa: F811
    return {T: hp._build(api, -10.0, 10.0, T) for T in (32, 100)}


def _table(api, bp, rows, extra=0, ticket=True):  # noqa: F811
    """the whole f -> v table (NaN where the launch wrote nothing) after one lhvi_pbp_f2v of the heavy family on `rows`"""
    import torch
    dev = bp.f2v.device
    desc = torch.from_numpy(np.ascontiguousarray(rows)).to(dev)
    out = torch.full_like(bp.f2v, float('nan'))
    s = bp._struct()
    s.flags = (s.flags & ~api.PBP_NO_SPLIT_ROUND) | api.PBP_F2V_HEAVY | extra
    s.heavy_desc, s.n_heavy = api.ptr(desc), int(rows.shape[0])
    tick = torch.zeros(16, dtype=torch.int32, device=dev)
    s.f2v_ticket = api.ptr(tick) if ticket else None
    api.check(api.lib().lhvi_pbp_f2v(bp.dg.g, bp.dg.p, s, api.ptr(bp.v2f), api.ptr(out), api.stream_ptr()))
    torch.cuda.synchronize()
    return out, tick.cpu().numpy()


def _same_bits(a, b):
    import torch
    return torch.equal(a.view(torch.int64), b.view(torch.int64))


def _both_ways(api, bp, rows, twin=True):  # noqa: F811
    """the four runs of a list and the checks every list gets; returns the messages of the list's edges as built"""
    split, _ = _table(api, bp, rows)
    plain, _ = _table(api, bp, rows, extra=api.PBP_NO_SPLIT_ROUND)
    assert _same_bits(split, plain)
    split_direct, _ = _table(api, bp, rows, extra=api.PBP_NO_GRID)
    plain_direct, _ = _table(api, bp, rows, extra=api.PBP_NO_GRID | api.PBP_NO_SPLIT_ROUND)
    assert _same_bits(split_direct, plain_direct)
    table = split.cpu().numpy()
    npart, T = rows[:, hp.W_NP], rows[:, hp.W_T]
    col = np.arange(table.shape[1])[None, :]
    written = (col < npart[:, None]) | ((col >= N) & (col < N + T[:, None]))
    mine = table[rows[:, 0]]
    assert np.isfinite(mine[written]).all() and np.isnan(mine[~written]).all()
    others = np.ones(table.shape[0], dtype=bool)
    others[rows[:, 0]] = False
    assert np.isnan(table[others]).all()
    assert (table[rows[:, 0]][:, :N].view(np.int64) == split_direct.cpu().numpy()[rows[:, 0]][:, :N].view(np.int64)).all()
    if twin:
        hp._hold_to_twin(bp, rows, mine)
    return mine


def _edit_nj(rows, nj, T=None):
    """word 7 alone: the partner stays hidden, its first nj particles are the list"""
    rows = rows.copy()
    rows[:, hp.W_NJ] = nj
    if T is not None:
        rows[:, hp.W_T] = T
    return rows


@pytest.mark.parametrize('T', [32, 100])
@pytest.mark.parametrize('nj', NJ)
def test_partner_counts_both_ways(api, graphs, T, nj):  # noqa: F811
    bp, rows = graphs[T]
    rows = rows[:ROWS]
    assert (rows[:, hp.W_NP] == N).all() and (rows[:, hp.W_GRID] == 1).all()
    # below GRID_MIN_NJ the rounds serve the grid points too, at most 128 points in all
    listed = _edit_nj(rows, nj, T=64 if nj < hp.GRID_MIN_NJ and T > 64 else None)
    mine = _both_ways(api, bp, listed)
    if nj < hp.GRID_MIN_NJ:
        # no grid points: one full round of 64 particles, the split round; with them the other loop served the same particles
        bare = _both_ways(api, bp, _edit_nj(rows, nj, T=0), twin=False)
        assert (bare[:, :N].view(np.int64) == mine[:, :N].view(np.int64)).all()


@pytest.mark.parametrize('T', [32, 100])
def test_observed_partner_both_ways(api, graphs, T):  # noqa: F811
    """one term, its value in the descriptor: no particle row and no v -> f row is read for the partner"""
    bp, rows = graphs[T]
    listed = hp._edit(rows[:ROWS], nj=1, T=64 if T > 64 else None)
    assert not np.isnan(listed[:, hp.W_PVAL:hp.W_PVAL + 2].copy().view(np.float64)).any()
    mine = _both_ways(api, bp, listed)
    bare = _both_ways(api, bp, hp._edit(rows[:ROWS], nj=1, T=0), twin=False)
    assert (bare[:, :N].view(np.int64) == mine[:, :N].view(np.int64)).all()


@pytest.mark.parametrize('T', [32, 100])
@pytest.mark.parametrize('npart', [63, 33, 1])
def test_fewer_target_particles_keep_the_other_loop(api, graphs, T, npart):  # noqa: F811
    """word 8 below 64: a round with idle lanes or one split over lane groups, never the split round"""
    bp, rows = graphs[T]
    _both_ways(api, bp, hp._edit(rows[:ROWS], npart=npart))


def test_ticketed_list_both_ways(api, graphs):  # noqa: F811
    """a list long enough for the dispatcher to keep the work tickets (as test_ticketed_list_matches_static_striding builds it)"""
    import torch
    bp, rows = graphs[100]
    props = torch.cuda.get_device_properties(0)
    need = props.multi_processor_count * 8 * 4 * 32 + 1
    many = np.tile(rows, ((need + rows.shape[0] - 1) // rows.shape[0], 1))      # (edges repeat: every copy writes the same bits)
    many[:, hp.W_T] = 33
    split, tick = _table(api, bp, many)
    plain, tick0 = _table(api, bp, many, extra=api.PBP_NO_SPLIT_ROUND)
    assert (tick[:hp.COUNTERS] > 0).all() and (tick0[:hp.COUNTERS] > 0).all()
    assert _same_bits(split, plain)
    static, _ = _table(api, bp, many, ticket=False)
    assert _same_bits(split, static)
    assert torch.isfinite(split[torch.from_numpy(rows[:, 0].astype(np.int64)).to(split.device), :N]).all()
