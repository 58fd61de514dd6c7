"""The heavy f2v kernel alone (LHVI_PBP_F2V_HEAVY) on hand-built descriptor lists: every path of its per-edge code.

A list is cut from the descriptors of a small hybrid MRF and edited in place -- partner count (word 7), target particle
count (word 8), grid size (word 9), partner evidence (words 12-13), uniform-grid mark (word 15) -- always DOWN from what
the graph holds, so every access stays inside the graph's arrays.  The same list then goes through
``pbp_f2v_fast_kernel`` (which reads the same descriptor format), through the heavy kernel's direct form
(LHVI_PBP_NO_GRID) and through the heavy kernel without work tickets.

Every list's messages are also held to the longdouble twin of tests/pbp_f2v_models.py, called with the overrides that match the
edit, within that module's derived bound (``_hold_to_twin``).

Tolerances between the device variants (those of the heavy tests in test_gpu_pbp.py): 1e-11 against the fast kernel (another order of the sums when a
short round is split across lane groups, another unroll), 1e-12 for the grid recurrence against the direct form, and
bit for bit for ticket against static striding (the same code per edge either way).

A list shorter than 128 entries per resident wave is strided statically by the dispatcher whatever the caller asks for, so
the short lists below exercise the cursor's static form and its clamp; the ticket form (chunks of 8, one range per
counter, ``min(next, limit - 1)``) runs in ``test_ticketed_list_matches_static_striding`` on a list long enough."""
import numpy as np
import pytest

import pbp_f2v_models as fm

pytestmark = pytest.mark.gpu

W_NJ, W_NP, W_T, W_PVAL, W_GRID = 7, 8, 9, 12, 15
N = 64
COUNTERS = 8            # LHVI_PBP_TICKET_COUNTERS: work counters, then the grid / fallback edge counts
GRID_MIN_NJ = 24


@pytest.fixture(scope='module')
def api():
    from lhvi import _abi
    _abi.require_gpu()
    return _abi


def _build(api, lo, hi, T, V=3000, uneven=False):
    from lhvi import synth
    from lhvi.flat import build_flat
    from lhvi.graph import Domain
    from lhvi.pbp import EPBP
    import torch
    pts = np.linspace(lo, hi, T)
    if uneven:
        pts = np.sign(pts) * np.abs(pts) ** 1.3 / 10 ** 0.3
    flat = synth.hybrid_mrf_flat(V=V, deg=4, seed=11, frac_discrete=0.1)
    specs = [(int(k), flat.pot_param[int(o):int(o2)].tolist()) for k, o, o2 in zip(flat.pot_kind, flat.pot_off[:-1], flat.pot_off[1:])]
    dom = Domain((lo, hi), continuous=True, integral_points=pts)
    flat = build_flat(flat.fac_ptr, flat.edge_var, flat.fac_pot, specs, np.clip(flat.var_value, lo, hi), flat.var_dom, [dom, flat.domains[1]])
    bp = EPBP(None, n=N, proposal_approximation='simple', sampler='device', seed=2)
    bp.long_grid_min_edges = 0
    bp._setup(None, flat=flat)
    api.check(api.lib().lhvi_pbp_init(bp.dg.g, bp._struct(), api.ptr(bp.eta), api.ptr(bp.q_dev), api.ptr(bp.f2v), api.ptr(bp.v2f), api.stream_ptr()))
    bp._generate_sample()
    for _ in range(2):
        bp.sweep(last=False)
    rows = bp.heavy_desc.view(torch.int32).view(-1, 32).cpu().numpy().copy()
    hidden = np.isnan(rows[:, W_PVAL:W_PVAL + 2].copy().view(np.float64)[:, 0])
    full = hidden & (rows[:, W_NJ] == N) & (rows[:, W_NP] == N) & (rows[:, W_T] == T)
    assert full.sum() > 500
    return bp, rows[full]


@pytest.fixture(scope='module')
def base(api):
    """[-10, 10] with the 100 points of the reference's RGM grid"""
    return _build(api, -10.0, 10.0, 100)


def _run(api, bp, rows, family, extra=0, ticket=True, take=None):
    """the messages of the list's edges ([len, N + T]) and the ticket words after one lhvi_pbp_f2v of one family"""
    import torch
    dev = bp.f2v.device
    desc = torch.from_numpy(np.ascontiguousarray(rows)).to(dev)
    edges = torch.from_numpy(np.ascontiguousarray(rows[:, 0])).to(dev)
    out = torch.zeros_like(bp.f2v)
    s = bp._struct()
    s.flags |= family | extra
    if family == api.PBP_F2V_HEAVY:
        s.heavy_desc, s.n_heavy = api.ptr(desc), int(rows.shape[0])
    else:
        s.fast_desc, s.fast_edges, s.n_fast = api.ptr(desc), api.ptr(edges), int(rows.shape[0])
    tick = torch.zeros(16, dtype=torch.int32, device=dev)
    s.f2v_ticket = api.ptr(tick) if ticket else None
    api.check(api.lib().lhvi_pbp_f2v(bp.dg.g, bp.dg.p, s, api.ptr(bp.v2f), api.ptr(out), api.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy()[rows[:take, 0]], tick.cpu().numpy()


class _HostState:
    """the solver's particles, old particles, v -> f messages and counts on the host: what ``pbp_f2v_models.f2v_twin`` reads"""

    def __init__(self, bp):
        self.particles, self.old_particles = bp.particles.cpu().numpy(), bp.old_particles.cpu().numpy()
        self.v2f, self.counts = bp.v2f.cpu().numpy(), bp.np_host


def _hold_to_twin(bp, rows, heavy):
    """the heavy kernel's messages of the edited rows against the longdouble twin called with the overrides that match the edit
    (partner count, target count, grid size, partner observed at the descriptor's value): regular points within
    ``pbp_f2v_models.f2v_bound`` -- the recurrence's for the grid points of an edge that may take it, the direct one elsewhere --
    and dead points at the floor.  (On the domain [-40, 40] some points lie between the two classes: those are counted, not held.)"""
    if getattr(bp, '_host_state', None) is None:
        bp._host_state = _HostState(bp)
    st, fl = bp._host_state, bp.flat
    pval = rows[:, W_PVAL:W_PVAL + 2].copy().view(np.float64)[:, 0]
    worst, between, held = 0.0, 0, 0
    for row, value, out in zip(rows, pval, heavy):
        e, nj, npart, T, grid = (int(row[w]) for w in (0, W_NJ, W_NP, W_T, W_GRID))
        tw = fm.f2v_twin(fl, st, e, nj=nj, np_=npart, T=T, partner_value=None if np.isnan(value) else value)
        L = tw.L.astype(np.float64)
        regular = (L >= fm.REGULAR_MIN_L) & (tw.top <= fm.REGULAR_MAX_EXPONENT)
        dead = tw.top <= fm.DEAD_MAX_EXPONENT
        bound = fm.f2v_bound(tw.M, tw.n_terms, tw.L, 'direct')
        if grid == 1 and nj >= GRID_MIN_NJ and 1 <= T <= 128:
            g = fm.grid_deviation(fl, fl.var_dom[fl.edge_var[e]])
            bound[npart:] = fm.f2v_bound(tw.M[npart:].max(), tw.n_terms, tw.L[npart:], 'recurrence', t=np.arange(T), grid_dev=g)
        got = np.concatenate([out[:npart], out[N:N + T]])
        ratio = np.abs(got - L)[regular] / bound[regular]
        worst = max(worst, float(ratio.max()) if ratio.size else 0.0)
        assert (ratio <= 1.0).all(), (e, float(ratio.max()))
        assert (got[dead] == fm.FLOOR).all(), (e, got[dead])
        between, held = between + int((~regular & ~dead).sum()), held + int(regular.sum() + dead.sum())
    print('heavy vs longdouble twin: worst |d| / bound = %.3f on %d points (%d between the classes)' % (worst, held, between))
    assert held > between


def _check(api, bp, rows, expect_fallback=None):
    nj, npart, T, grid = (rows[:, w] for w in (W_NJ, W_NP, W_T, W_GRID))
    S = bp.f2v.shape[1]
    col = np.arange(S)[None, :]
    written = (col < npart[:, None]) | ((col >= N) & (col < N + T[:, None]))
    heavy, tick = _run(api, bp, rows, api.PBP_F2V_HEAVY)
    assert np.isfinite(heavy).all() and (heavy[~written] == 0).all()          # nothing outside the edge's own points
    _hold_to_twin(bp, rows, heavy)                                            # ... and a host value for every one of them
    # ticket words 8 / 9: edges through the recurrence / edges the range guard sent to the direct form
    eligible = (grid == 1) & (nj >= GRID_MIN_NJ) & (T <= 128)
    assert int(tick[COUNTERS]) + int(tick[COUNTERS + 1]) == int(eligible.sum())
    if expect_fallback is not None:
        assert (int(tick[COUNTERS + 1]) > 0) == expect_fallback
    # the same list without work tickets: bit for bit
    static, tick0 = _run(api, bp, rows, api.PBP_F2V_HEAVY, ticket=False)
    assert (static == heavy).all() and (tick0 == 0).all()
    # the fast kernel on the same descriptors
    fast, _ = _run(api, bp, rows, api.PBP_F2V_FAST)
    print('heavy vs fast: max |d| = %.3g' % float(np.abs(heavy - fast)[written].max()))
    np.testing.assert_allclose(heavy[written], fast[written], rtol=1e-11, atol=1e-11)
    # the direct form of the heavy kernel itself: particle part identical, grid part to 1e-12
    direct, tick1 = _run(api, bp, rows, api.PBP_F2V_HEAVY, extra=api.PBP_NO_GRID)
    assert int(tick1[COUNTERS]) == 0
    assert (direct[:, :N] == heavy[:, :N]).all()
    print('recurrence vs direct: max |d| = %.3g' % float(np.abs(heavy - direct)[written].max()))
    np.testing.assert_allclose(heavy[written], direct[written], rtol=1e-12, atol=1e-12)
    same = (direct == heavy).all(axis=1)
    assert same[~eligible].all()
    assert int((~same).sum()) <= int(tick[COUNTERS])
    return heavy


def _edit(rows, nj=None, npart=None, T=None, grid=None):
    rows = rows.copy()
    if nj is not None:
        rows[:, W_NJ] = nj
        if nj == 1:             # an observed partner: its value in the descriptor, no particle row read
            rows[:, W_PVAL:W_PVAL + 2] = np.array([0.3]).view(np.int32)[None, :]
    if npart is not None:
        rows[:, W_NP] = npart
    if T is not None:
        rows[:, W_T] = T
    if grid is not None:
        rows[:, W_GRID] = grid
    return rows


@pytest.mark.parametrize('nj', [1, 23, 24, 63, 64])
def test_partner_counts(api, base, nj):
    """1 = observed partner; 23 / 24: both sides of GRID_MIN_NJ; 63: one padded record; 64: the full wave.  Below GRID_MIN_NJ
    the grid points go through the rounds, which serve at most 128 points: such an edge is on the list with np + T <= 128"""
    bp, rows = base
    _check(api, bp, _edit(rows[:257], nj=nj, T=64 if nj < GRID_MIN_NJ else None), expect_fallback=False if nj < GRID_MIN_NJ else None)


@pytest.mark.parametrize('npart', [1, 33, 64])
def test_target_particle_counts(api, base, npart):
    """64: the fetch's straight path (lane = particle); 33: a full-width round with idle lanes; 1: a round split over 64 lane groups"""
    bp, rows = base
    _check(api, bp, _edit(rows[:257], npart=npart))


@pytest.mark.parametrize('T', [1, 31, 32, 33, 100])
def test_grid_sizes(api, base, T):
    """batches of 32 grid points: one partial, one full, one more than full, four (the last partial)"""
    bp, rows = base
    _check(api, bp, _edit(rows[:257], T=T))


@pytest.mark.parametrize('npart,T', [(64, 33), (31, 33), (64, 64), (1, 1)])
def test_non_uniform_grid(api, base, npart, T):
    """no uniform-grid mark: the integral points are fetched with the particles and served by the rounds (np + T <= 128),
    two rounds, one round of exactly 64 points with particles and grid points mixed, and a single split round"""
    bp, rows = base
    rows = _edit(rows[:257], npart=npart, T=T, grid=0)
    heavy = _check(api, bp, rows, expect_fallback=False)
    assert heavy.shape[0] == 257


def test_graph_with_non_uniform_points(api):
    """a domain whose points are not evenly spaced, as the describe kernel marks it"""
    bp, rows = _build(api, -10.0, 10.0, 32, uneven=True)
    assert (rows[:, W_GRID] == 0).all()
    _check(api, bp, rows[:300], expect_fallback=False)


def test_range_guard_fallback(api):
    """domain [-40, 40]: exponents near +-800 on the grid, the guard sends those edges through the direct form"""
    bp, rows = _build(api, -40.0, 40.0, 32)
    assert (rows[:, W_GRID] == 1).all()
    _check(api, bp, rows[:600], expect_fallback=True)


@pytest.mark.parametrize('length', [1, 7, 8, 9, 8 * COUNTERS + 1])
def test_list_lengths(api, base, length):
    """chunk and range boundaries of the work cursor, and the clamp of the descriptor prefetch at the end of the list"""
    bp, rows = base
    _check(api, bp, rows[:length])


def test_ticketed_list_matches_static_striding(api, base):
    """a list long enough for the dispatcher to keep the tickets (128 entries per resident wave): the counters were used,
    every range was walked to its end, and the messages are those of static striding bit for bit"""
    import torch
    bp, rows = base
    props = torch.cuda.get_device_properties(0)
    need = props.multi_processor_count * 8 * 4 * 32 + 1           # above the threshold at any residency up to 8 workgroups per CU
    reps = (need + rows.shape[0] - 1) // rows.shape[0]
    many = np.tile(rows, (reps, 1))                               # (edges repeat: every copy writes the same bits)
    many[:, W_T] = 33
    a, tick = _run(api, bp, many, api.PBP_F2V_HEAVY, take=rows.shape[0])
    b, _ = _run(api, bp, many, api.PBP_F2V_HEAVY, ticket=False, take=rows.shape[0])
    assert (tick[:COUNTERS] > 0).all()
    assert int(tick[COUNTERS]) + int(tick[COUNTERS + 1]) == many.shape[0]
    assert (a == b).all() and np.isfinite(a).all()
