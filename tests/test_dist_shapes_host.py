"""The owner-computes plan (``lhvi/dist.py::OwnerPlan``) beyond the synthetic pairwise MRF, on the host: the invariants of
tests/test_dist.py::test_owner_plan_invariants on the routing-table zoo (every variable kind, factors of three variables) under a
round-robin ownership and on the paper-popularity MLN under the refined and the round-robin one, at 2, 3 and 8 ranks; the rank
that owns nothing; and one gloo exchange of rows of width 3 to 5 and of rows that go to several peers."""
import os
import socket
import sys

import numpy as np
import pytest

import dist_models as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [('zoo', 'round_robin'), ('hmln', 'refined'), ('hmln', 'round_robin')]


@pytest.mark.parametrize('world', [2, 3, 8])
@pytest.mark.parametrize('name,kind', CASES)
def test_owner_plan_invariants_on_the_zoo_and_the_mln(name, kind, world):
    flat, owner = dm.graph(name), dm.ownership(name, world, kind)
    plans = dm.assert_plan_invariants(flat, owner, world)
    n_more = {n: sum(dm.send_more_rows(p, n)[0].size for p in plans) for n in (10, 16, 64, 100)}
    assert len(set(n_more.values())) == 1                   # which rows go out twice does not depend on the particle count
    n_more = n_more[16]
    print(name, kind, world, 'send_more rows:', n_more, 'owned / ghosts / edges per rank:', [(p.n_owned, p.n_ghost, p.flat.E) for p in plans])
    if world == 2:
        assert n_more == 0                                  # one peer: no row has a second place
    elif name == 'zoo':
        assert n_more == 24
    elif kind == 'refined':
        assert n_more == {3: 54, 8: 60}[world]
    else:
        assert n_more > 0
    if name == 'zoo':
        # the refined partition cuts nothing of a graph whose factors share no variable: the round-robin ownership is what cuts it
        from lhvi.dist import OwnerPlan, partition_variables
        refined = partition_variables(flat, 3)
        assert sum(int(OwnerPlan(flat, r, 3, var_owner=refined).edge_key.sum()) for r in range(3)) == 0
        widths = set()
        for p in plans:
            widths |= set(p.layout(16)['recv']['row_width'].tolist())
        assert widths == {2, 3, 4, 5}
        assert all(p.layout(16)['recv']['cont_edge'].size > 0 for p in plans)
    if world >= 3 and n_more:
        # a row's further places lie in other peers' blocks than its first one, and no two of them in the same block
        for p in plans:
            for n in (10, 16, 64, 100):
                edge, off, peer, first_peer = dm.send_more_rows(p, n)
                assert (peer != first_peer).all() and (peer != p.rank).all()
                pairs = set(zip(edge.tolist(), peer.tolist()))
                assert len(pairs) == edge.size
                for e, s in pairs:
                    assert e in p.send_rows[s]


def test_the_refined_partition_of_the_mln_at_eight_ranks_leaves_a_rank_that_owns_nothing():
    """rank 1 of 8: no owned variable, no factor, nothing to send or to receive at any particle count -- and the other ranks list
    nothing for it"""
    from lhvi.dist import OwnerPlan
    flat, owner = dm.graph('hmln'), dm.ownership('hmln', 8, 'refined')
    assert not (np.isnan(flat.var_value) & (owner == 1)).any()
    plans = [OwnerPlan(flat, r, 8, var_owner=owner) for r in range(8)]
    p = plans[1]
    assert p.n_owned == 0 and p.n_ghost == 0 and p.flat.V == 0 and p.flat.F == 0 and p.flat.E == 0 and p.fac_ids.size == 0
    assert p.edge_skip.size == 0 and p.edge_key.size == 0
    for n in (10, 16, 64, 100):
        lay = p.layout(n)
        for side in ('send', 'recv'):
            assert lay[side]['size'] == 0 and not any(lay[side]['counts'])
            assert all(lay[side][k].size == 0 for k in ('cont_edge', 'row_edge', 'q_var'))
        canon, extra = p.ghost_rows(n)
        assert canon.size == 0 and extra == 0
        for q in plans:
            if q.rank != 1:
                assert q.layout(n)['send']['counts'][1] == 0 and q.layout(n)['recv']['counts'][1] == 0


def _zoo_gloo_worker(rank, world, port, out):
    """the scheme of tests/test_dist.py::_owner_compute_gloo_worker on the zoo: a row / a proposal is a function of its global id,
    so every rank checks what it received on its own"""
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'lifted-hybrid-variational-inference_amd'), os.path.join(ROOT, 'tests')]
    import torch
    import torch.distributed as td
    import dist_models
    from lhvi.dist import OwnerPlan
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    td.init_process_group('gloo', rank=rank, world_size=world)
    flat = dist_models.graph('zoo')
    plan = OwnerPlan(flat, rank, world, var_owner=dist_models.round_robin(flat, world))
    n = 6
    lf = plan.flat
    lay = plan.layout(n)
    row = lambda ge: np.sin(0.1 * ge + np.arange(n))
    prop = lambda gv: np.array([np.cos(0.3 * gv), 1.0 + gv % 7])
    S, R = lay['send'], lay['recv']
    send = torch.zeros(max(S['size'], 1), dtype=torch.float64)
    # as OwnerRunner fills the buffer: every listed place of a row, the further places of a row for several peers included
    for e, o, w in zip(*plan.rows_of(S, n)):
        send[o:o + w] = torch.from_numpy(row(plan.edge_ids[e])[:w])
    for v, o in zip(S['q_var'], S['q_off']):
        send[o:o + 2] = torch.from_numpy(prop(plan.var_gid[v]))
    recv = torch.empty(R['size'], dtype=torch.float64)
    td.all_to_all_single(recv, send[:S['size']], output_split_sizes=R['counts'], input_split_sizes=S['counts'])
    ok = True
    for e, o, w in zip(*plan.rows_of(R, n)):
        ok = ok and bool((recv[o:o + w].numpy() == row(plan.edge_ids[e])[:w]).all())
    for v, o in zip(R['q_var'], R['q_off']):
        ok = ok and bool((recv[o:o + 2].numpy() == prop(plan.var_gid[v])).all())
    canon, extra = plan.ghost_rows(n)
    ok = ok and bool((R['cont_off'] % n == 0).all()) and bool((canon[R['cont_edge']] == lf.E + R['cont_off'] // n).all()) \
        and extra * n >= R['size'] and all(c % n == 0 for c in R['counts'] + S['counts'])
    out.put((rank, ok, sorted(set(R['row_width'].tolist())), int(dist_models.send_more_rows(plan, n)[0].size), int(R['cont_edge'].size)))
    td.barrier()
    td.destroy_process_group()


def test_zoo_exchange_gloo_world3():
    """three real processes over gloo: rows of 3, 4 and 5 doubles and rows listed for two peers arrive intact"""
    import torch.multiprocessing as mp
    world = 3
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    ctx = mp.get_context('spawn')
    out = ctx.Queue()
    procs = [ctx.Process(target=_zoo_gloo_worker, args=(r, world, port, out)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(out.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert all(ok for _, ok, _, _, _ in res), res
    widths = set().union(*(w for _, _, w, _, _ in res))
    assert {2, 3, 4, 5} <= widths, res
    assert sum(m for _, _, _, m, _ in res) == 24 and all(c > 0 for _, _, _, _, c in res), res
