"""The owner-computes sharded sweep (``lhvi/dist.py::OwnerRunner``) against the single-GPU sweep, bit for bit, beyond the synthetic
pairwise MRF at 64 particles: the routing-table zoo under a round-robin ownership (rows for several peers, discrete ghosts of 3, 4
and 5 states, every f -> v family on a cut edge, the sampler without lists), the paper-popularity MLN (cut conditional-quadratic
factors with continuous ghosts, a rank that owns nothing), its hub variant (rows above LHVI_HUB_DEGREE that go out), few and odd
particle counts, the EP proposal and both f -> v schedules.  The ranks are simulated in one process (``dist.LoopbackGroup``);
``dist_models.assert_owner_equals_single`` compares and reports what each rank exercised, and every case asserts that it reached
the path it is there for.

The matrix is cut where two cells run the same kernels on the same lists: the proposal ('simple' / 'EP') changes the proposal
kernel only, so 'EP' runs at one world size per graph and particle count."""
import numpy as np
import pytest

import dist_models as dm
import pbp_f2v_models as fm

pytestmark = pytest.mark.gpu

# the families that must serve a cut edge of the zoo, by particle count (docs/kernels_particle.md 4.3: at 16 particles the
# heavy-class edges are on the small lists); 'light' when the light edges are served per edge (``paired_light`` off)
ZOO_FAMILIES = {64: {'heavy', 'pair', 'fast', 'cq', 'generic'}, 16: {'small', 'pair', 'fast', 'cq', 'generic'}}
ZOO_FAMILIES_UNPAIRED = {'heavy', 'light', 'fast', 'cq', 'generic'}
assert set().union(ZOO_FAMILIES_UNPAIRED, *ZOO_FAMILIES.values()) == set(fm.FAMILIES)


@pytest.fixture(scope='module', autouse=True)
def gpu():
    from lhvi import _abi
    _abi.require_gpu()


def run(name, n, world, kind, proposal, **kw):
    return dm.assert_owner_equals_single(dm.graph(name), n, world, dm.ownership(name, world, kind), proposal, **kw)


def check_zoo(stats, world, families):
    with_state = [st for st in stats if st.n_owned]
    assert len(with_state) == world
    if world >= 3:
        assert any(st.n_send_more > 0 for st in stats)
    else:
        assert all(st.n_send_more == 0 for st in stats)
    assert {3, 4, 5} <= set().union(*(st.ghost_row_widths for st in stats))
    assert all(st.n_cont_ghost_edges > 0 and st.n_cut_factors > 0 for st in stats)
    cut = set().union(*(st.cut_families for st in stats))
    assert cut >= families, 'no cut edge is served by %s' % sorted(families - cut)


@pytest.mark.parametrize('n,proposal,world', [(n, p, w) for n in (16, 64) for p, w in (('simple', 2), ('simple', 3), ('simple', 8), ('EP', 3))])
def test_zoo_round_robin(n, proposal, world):
    stats = run('zoo', n, world, 'round_robin', proposal)
    check_zoo(stats, world, ZOO_FAMILIES[n])
    assert all(st.res_lists is not None for st in stats)


def test_zoo_light_edges_served_one_by_one(monkeypatch):
    """``paired_light`` off: the light kernel reads a ghost partner's row on its own"""
    from lhvi.pbp import EPBP
    monkeypatch.setattr(EPBP, 'paired_light', False)
    check_zoo(run('zoo', 64, 3, 'round_robin', 'simple'), 3, ZOO_FAMILIES_UNPAIRED)


def test_zoo_sampler_without_lists():
    """more than 64 particles: the draws go by variable range, owned and ghost; the chunked v -> f path copies the cut rows"""
    stats = run('zoo', 100, 3, 'round_robin', 'simple')
    assert all(st.res_lists is None for st in stats)
    assert all(st.n_cont_ghost_edges > 0 for st in stats) and any(st.n_send_more > 0 for st in stats)


HMLN = [(n, 'simple', w, k) for n in (10, 64) for w in (2, 3) for k in ('refined', 'round_robin')] + \
       [(n, 'EP', 3, 'refined') for n in (10, 64)]


@pytest.mark.parametrize('n,proposal,world,kind', HMLN)
def test_hmln(n, proposal, world, kind):
    stats = run('hmln', n, world, kind, proposal)
    if world == 3:
        assert any(st.n_send_more > 0 for st in stats)
    assert sum(st.n_cut_cq_cont_ghost for st in stats) > 0
    # ... and they are served by the quadratic-family kernels, which read the ghost's row where it arrived
    assert set().union(*(st.cq_ghost_families for st in stats)) - {'generic'}
    assert all(st.n_owned > 0 for st in stats)


def test_hmln_eight_ranks_one_of_which_owns_nothing():
    stats = run('hmln', 64, 8, 'refined', 'simple')
    assert [st.n_owned == 0 for st in stats] == [r == 1 for r in range(8)]
    assert any(st.n_send_more > 0 for st in stats) and sum(st.n_cut_cq_cont_ghost for st in stats) > 0


def test_hmln_hub_rows_that_go_out():
    """a variable of more than LHVI_HUB_DEGREE factors, owned by a rank where some of them are cut: the hub kernel's halo copy and
    the sliced proposal"""
    flat = dm.graph('hmln_hub')
    assert dm.hidden_hubs(flat).size == 2 and int(np.diff(flat.var_ptr).max()) == 68
    stats = run('hmln_hub', 20, 3, 'round_robin', 'simple')
    assert sum(st.n_hub_rows for st in stats) == 2 and sum(st.n_prop_hubs for st in stats) == 2
    assert any(st.owned_hubs_cut > 0 and st.n_hub_rows > 0 and st.n_prop_hubs > 0 for st in stats)


@pytest.mark.parametrize('n', [16, 20, 33])
def test_mrf_small_ep(n):
    """the few-particle lists (small16, small32 in lane groups of ten, the first count past 32) at an odd grid size"""
    stats = run('mrf_small', n, 3, 'refined', 'EP')
    assert all(st.n_cut_factors > 0 and st.n_cont_ghost_edges > 0 for st in stats)
    want = 'small' if n <= 32 else 'heavy'
    assert all(want in st.cut_families for st in stats)


@pytest.mark.parametrize('split', [True, False])
@pytest.mark.parametrize('name,kind', [('zoo', 'round_robin'), ('hmln', 'refined')])
def test_both_f2v_schedules(name, kind, split):
    """two launches (factors without a ghost, then the cut ones) and one launch after the exchange: the same bits"""
    stats = run(name, 64, 3, kind, 'simple', split_f2v=split)
    assert all(st.split_f2v == split for st in stats)
    # both parts of the lists have work, so the forced schedule differs from the other one
    assert all(st.n_cut_factors > 0 and st.n_interior_edges > 0 for st in stats)
