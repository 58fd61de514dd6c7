"""Edge sharding: plan invariants and the boundary exchange with world_size 2 over gloo (CPU), plus -- on a GPU --
the sharded sweep simulated for 2 and 3 ranks in one process against the single-GPU sweep."""
import os
import socket
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plans(flat, world):
    from lhvi.dist import ShardPlan
    return [ShardPlan(flat, r, world) for r in range(world)]


@pytest.mark.parametrize('world', [2, 3, 8])
def test_shard_plan_invariants(world):
    from lhvi import synth
    flat = synth.hybrid_mrf_flat(V=1500, deg=4, seed=2)
    plans = _plans(flat, world)
    assert sum(p.flat.E for p in plans) == flat.E and sum(p.flat.F for p in plans) == flat.F
    assert sorted(np.concatenate([p.fac_ids for p in plans]).tolist()) == list(range(flat.F))     # a partition of the factors
    assert max(p.flat.F for p in plans) <= 1.15 * min(p.flat.F for p in plans)                    # balanced (the refined cut: by variable degree, to a few per cent)
    # locality: the refined cut has fewer exchange rows than the breadth-first blocks, and those fewer than cutting the construction order
    from lhvi.dist import ShardPlan
    bfs_rows = sum(ShardPlan(flat, r, world, partition='bfs').n_rows for r in range(world))
    assert sum(p.n_rows for p in plans) < bfs_rows < sum(ShardPlan(flat, r, world, partition='block').n_rows for r in range(world))
    bfs_plans = [ShardPlan(flat, r, world, partition='bfs') for r in range(world)]
    assert max(p.flat.F for p in bfs_plans) - min(p.flat.F for p in bfs_plans) <= 1
    deg = np.bincount(flat.edge_var, minlength=flat.V)
    owners = np.zeros(flat.V, dtype=int)
    for p in plans:
        # local graph is the induced sub-incidence with consistent renumbering
        np.testing.assert_array_equal(p.var_gid[p.flat.edge_var], flat.edge_var[p.edge_ids])
        np.testing.assert_array_equal(p.var_degree, deg[p.var_gid])
        np.testing.assert_array_equal(np.isnan(p.flat.var_value), np.isnan(flat.var_value[p.var_gid]))
        owners[p.var_gid] += 1
        local_deg = np.diff(p.flat.var_ptr)
        # boundary = hidden variables with edges on another rank (observed variables never need sums)
        np.testing.assert_array_equal((local_deg < p.var_degree) & np.isnan(p.flat.var_value), p.bslot >= 0)
        # every exchange row is listed exactly once, grouped per boundary variable in ascending peer order
        assert sorted(p.brow_idx.tolist()) == list(range(p.n_rows)) and p.brow_ptr[-1] == p.n_rows
        for b in range(0, p.bvars.size, max(1, p.bvars.size // 50)):
            peers = p.brow_peer[p.brow_ptr[b]:p.brow_ptr[b + 1]]
            assert (np.diff(peers) > 0).all() and p.rank not in peers.tolist()
    # both ends of every pair list the shared variables in the same (gid) order
    for r, p in enumerate(plans):
        for s, rows in p.peer_rows.items():
            mine = p.var_gid[p.bvars[rows]]
            theirs = plans[s].var_gid[plans[s].bvars[plans[s].peer_rows[r]]]
            np.testing.assert_array_equal(mine, theirs)
    assert (owners >= 1).all()


@pytest.mark.parametrize('world', [2, 4, 8])
def test_refined_partition_cuts_fewer_factors_at_the_same_balance(world):
    """``refine_partition`` (balanced label propagation on top of the breadth-first blocks): deterministic, every part's load
    (degree + 1 per variable) stays within its 3 % capacity of the mean, and fewer hidden-hidden factors are cut than by the
    breadth-first blocks, which in turn cut fewer than the construction order; a graph of one part comes back unchanged"""
    from lhvi import synth
    from lhvi.dist import hidden_adjacency, partition_variables, refine_partition
    flat = synth.hybrid_mrf_flat(V=4000, deg=4, seed=5)
    A = hidden_adjacency(flat).tocoo()

    def cut(owner):
        return int((owner[A.row] != owner[A.col]).sum()) // 2
    w = np.diff(flat.var_ptr) + 1.0
    owners = {p: partition_variables(flat, world, p) for p in ('block', 'bfs', 'refined')}
    assert cut(owners['refined']) < cut(owners['bfs']) < cut(owners['block'])
    load = np.bincount(owners['refined'], weights=w, minlength=world)
    assert load.max() <= 1.03 * w.sum() / world + w.max()
    assert set(np.unique(owners['refined']).tolist()) == set(range(world))
    np.testing.assert_array_equal(owners['refined'], partition_variables(flat, world, 'refined'))      # seeded: every rank could rebuild it
    np.testing.assert_array_equal(refine_partition(flat, owners['bfs'], 1), owners['bfs'])
    # an isolated or observed variable has no neighbour to follow: it stays where the blocks put it
    lonely = np.flatnonzero(np.diff(hidden_adjacency(flat).indptr) == 0)
    np.testing.assert_array_equal(owners['refined'][lonely], owners['bfs'][lonely])


@pytest.mark.parametrize('world', [3, 8])
def test_owner_exchange_layout_adds_up(world):
    """reduce-to-owner exchange, both collectives played in NumPy over all ranks' layouts: every replica ends up with the sum
    of the ranks' rows taken in ascending rank order (bit for bit), the two ends of every block agree on its size, and the
    payload is smaller than the all-to-all form's whenever a variable lives on three or more ranks"""
    from lhvi import synth
    from lhvi.dist import owner_exchange_layout
    flat = synth.hybrid_mrf_flat(V=1500, deg=4, seed=2)
    plans = _plans(flat, world)
    rng = np.random.default_rng(0)
    W = 6
    lays, A, B, local = [], [], [], []
    for p in plans:
        width = np.where(np.arange(p.bvars.size) % 3 == 0, 2, W)          # two row widths, like discrete / continuous variables
        # (the width of a variable must be the same on every rank: make it a function of the global id)
        width = np.where(p.var_gid[p.bvars] % 3 == 0, 2, W)
        lay = owner_exchange_layout(p, width)
        lays.append(lay)
        rows = rng.normal(size=(p.bvars.size, W))
        local.append(rows)
        a = np.full(lay['a_size'], np.nan)
        for b in range(p.bvars.size):
            a[lay['pack_off'][b]:lay['pack_off'][b] + width[b]] = rows[b, :width[b]]
        A.append(a)
        B.append(np.full(lay['b_size'], np.nan))
    for r in range(world):
        for s in range(world):
            assert lays[r]['a_send'][s] == lays[s]['a_recv'][r] and lays[r]['b_send'][s] == lays[s]['b_recv'][r]
        assert lays[r]['a_send'][r] == 0 and lays[r]['b_send'][r] == 0

    def all_to_all(bufs, send_key, recv_key, recv_base_key):
        for dst in range(world):
            pos = lays[dst][recv_base_key]
            for src in range(world):
                cnt = lays[src][send_key][dst]
                off = int(sum(lays[src][send_key][:dst]))
                bufs[dst][pos:pos + cnt] = bufs[src][off:off + cnt]
                pos += cnt
    all_to_all(A, 'a_send', 'a_recv', 'a_recv_base')
    for r, lay in enumerate(lays):
        for i in range(lay['items'].size):
            w = lay['width'][i]
            tot = np.zeros(w)
            for k in range(lay['src_ptr'][i], lay['src_ptr'][i + 1]):
                tot = tot + A[r][lay['src_off'][k]:lay['src_off'][k] + w]
            for k in range(lay['dst_ptr'][i], lay['dst_ptr'][i + 1]):
                B[r][lay['dst_off'][k]:lay['dst_off'][k] + w] = tot
    all_to_all(B, 'b_send', 'b_recv', 'b_recv_base')
    # expected: the ranks' rows added in ascending rank order
    by_gid = {}
    for r, p in enumerate(plans):
        for b, lv in enumerate(p.bvars):
            by_gid.setdefault(int(p.var_gid[lv]), []).append((r, local[r][b]))
    many = 0
    for r, p in enumerate(plans):
        lay = lays[r]
        for b, lv in enumerate(p.bvars):
            gid = int(p.var_gid[lv])
            w = 2 if gid % 3 == 0 else W
            want = np.zeros(w)
            for _, row in sorted(by_gid[gid], key=lambda t: t[0]):
                want = want + row[:w]
            got = B[r][lay['total_off'][b]:lay['total_off'][b] + w]
            assert (got == want).all()
            assert len(by_gid[gid]) == p.brow_ptr[b + 1] - p.brow_ptr[b] + 1
            many += len(by_gid[gid]) >= 3
            # one owner per variable, the same on every rank that holds it
            assert len({int(lays[q]['owner'][list(plans[q].var_gid[plans[q].bvars]).index(gid)]) for q, _ in by_gid[gid]}) == 1 \
                if b % 40 == 0 else True
    pairs = sum(int(np.where(p.var_gid[p.bvars][np.repeat(np.arange(p.bvars.size), np.diff(p.brow_ptr))] % 3 == 0, 2, W).sum())
                for p in plans)
    owner = sum(sum(l['a_send']) + sum(l['b_send']) for l in lays)
    assert many > 0 and owner < pairs
    # owners are spread over the ranks
    owned = np.array([l['items'].size for l in lays])
    assert owned.min() > 0 and owned.max() < 3 * max(owned.mean(), 1)


def _gloo_worker(rank, world, port, out):
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'lifted-hybrid-variational-inference_amd')]
    import torch
    import torch.distributed as td
    from lhvi import synth
    from lhvi.dist import ShardPlan, broadcast_partition, partition_factors
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    td.init_process_group('gloo', rank=rank, world_size=world)
    flat = synth.hybrid_mrf_flat(V=800, deg=4, seed=4)
    # the factor partition is computed on rank 0 only and broadcast; the plan is then built from this rank's slice
    fac_owner = broadcast_partition(flat, rank, world)
    assert (fac_owner == partition_factors(flat, world)).all()
    plan = ShardPlan(flat, rank, world, fac_owner=fac_owner)
    W = 5
    rng = np.random.default_rng(0)
    edge_val = rng.normal(size=(flat.E, W))                     # same on every rank
    local = edge_val[plan.edge_ids]
    part = np.zeros((plan.flat.V, W))
    np.add.at(part, plan.flat.edge_var, local)                  # per-variable partial sum over LOCAL edges
    rows = torch.from_numpy(part[plan.bvars])
    counts = plan.send_counts()
    index = torch.cat([torch.from_numpy(plan.peer_rows[s]) for s in range(world) if s != rank])
    send = rows.index_select(0, index)
    recv = torch.empty_like(send)
    td.all_to_all_single(recv, send, output_split_sizes=counts, input_split_sizes=counts)
    remote = torch.zeros_like(rows)
    off = 0
    for s in range(world):
        if s == rank:
            continue
        remote.index_add_(0, torch.from_numpy(plan.peer_rows[s]), recv[off:off + counts[s]])
        off += counts[s]
    total = part.copy()
    total[plan.bvars] += remote.numpy()
    want = np.zeros((flat.V, W))
    np.add.at(want, flat.edge_var, edge_val)
    hid = np.isnan(plan.flat.var_value)
    ok = np.allclose(total[hid], want[plan.var_gid][hid], rtol=1e-12, atol=1e-12)
    out.put((rank, bool(ok), int(plan.bvars.size)))
    td.destroy_process_group()


def test_boundary_exchange_gloo_world2():
    """two real processes over gloo: local partials + one all_to_all == the global per-variable sums"""
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    ctx = mp.get_context('spawn')
    out = ctx.Queue()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    res = [out.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert all(ok for _, ok, _ in res), res
    assert all(nb > 0 for _, _, nb in res)


def _owner_gloo_worker(rank, world, port, out):
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'lifted-hybrid-variational-inference_amd')]
    import torch
    import torch.distributed as td
    from lhvi import synth
    from lhvi.dist import ShardPlan, owner_exchange_layout
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    td.init_process_group('gloo', rank=rank, world_size=world)
    flat = synth.hybrid_mrf_flat(V=1200, deg=4, seed=7)
    plan = ShardPlan(flat, rank, world)
    W = 5
    gid = plan.var_gid[plan.bvars]
    width = np.where(gid % 3 == 0, 2, W)                       # (a function of the global id: the same on every rank)
    lay = owner_exchange_layout(plan, width)
    # every rank's row of a variable is a function of (rank, gid), so each rank can form the expected totals on its own
    row = lambda r, g_: np.sin(np.arange(W) + 0.37 * g_ + 1.7 * r)
    A = torch.zeros(max(lay['a_size'], 1), dtype=torch.float64)
    for b in range(plan.bvars.size):
        A[lay['pack_off'][b]:lay['pack_off'][b] + width[b]] = torch.from_numpy(row(rank, int(gid[b]))[:width[b]])
    sa, ra = int(sum(lay['a_send'])), int(sum(lay['a_recv']))
    recv = torch.empty(ra, dtype=torch.float64)
    td.all_to_all_single(recv, A[:sa].clone(), output_split_sizes=lay['a_recv'], input_split_sizes=lay['a_send'])
    A[lay['a_recv_base']:lay['a_recv_base'] + ra] = recv
    B = torch.zeros(max(lay['b_size'], 1), dtype=torch.float64)
    for i in range(lay['items'].size):
        w = int(lay['width'][i])
        tot = torch.zeros(w, dtype=torch.float64)
        for k in range(lay['src_ptr'][i], lay['src_ptr'][i + 1]):
            tot = tot + A[lay['src_off'][k]:lay['src_off'][k] + w]
        for k in range(lay['dst_ptr'][i], lay['dst_ptr'][i + 1]):
            B[lay['dst_off'][k]:lay['dst_off'][k] + w] = tot
    sb, rb = int(sum(lay['b_send'])), int(sum(lay['b_recv']))
    recv = torch.empty(rb, dtype=torch.float64)
    td.all_to_all_single(recv, B[:sb].clone(), output_split_sizes=lay['b_recv'], input_split_sizes=lay['b_send'])
    B[lay['b_recv_base']:lay['b_recv_base'] + rb] = recv
    ok = True
    for b in range(plan.bvars.size):
        peers = plan.brow_peer[plan.brow_ptr[b]:plan.brow_ptr[b + 1]].tolist()
        want = np.zeros(width[b])
        for r in sorted(peers + [rank]):
            want = want + row(r, int(gid[b]))[:width[b]]
        got = B[lay['total_off'][b]:lay['total_off'][b] + width[b]].numpy()
        ok = ok and bool((got == want).all())
    out.put((rank, ok, int(plan.bvars.size), int((np.diff(plan.brow_ptr) >= 2).sum())))
    td.barrier()
    td.destroy_process_group()


def test_owner_exchange_gloo_world3():
    """three real processes over gloo: rows to the owners, the owners' sums, totals back -- two all_to_all_single calls with
    unequal split lists; every replica ends with the sum of the ranks' rows in ascending rank order, bit for bit"""
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    ctx = mp.get_context('spawn')
    out = ctx.Queue()
    procs = [ctx.Process(target=_owner_gloo_worker, args=(r, 3, port, out)) for r in range(3)]
    for p in procs:
        p.start()
    res = [out.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert all(ok for _, ok, _, _ in res), res
    assert all(nb > 0 for _, _, nb, _ in res) and any(three > 0 for _, _, _, three in res)      # some variable lives on all three ranks


def _run_bench(args, env=None, timeout=600):
    import subprocess
    e = dict(os.environ)
    e.pop('WORLD_SIZE', None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args, env=e, capture_output=True, text=True,
                          timeout=timeout)


def test_bench_rejects_a_launcher_of_another_size():
    """--gpus must equal the launcher's WORLD_SIZE, whatever the two are (checked before anything touches a GPU)"""
    for world, gpus in ((4, 2), (1, 2), (2, 1)):
        r = _run_bench(['--gpus', str(gpus)], env={'WORLD_SIZE': str(world)})
        assert r.returncode != 0 and 'does not match WORLD_SIZE' in r.stderr
    assert _run_bench(['--gpus', '0']).returncode != 0


@pytest.mark.gpu
def test_bench_times_both_splits_in_one_launch():
    """`python bench.py --gpus 2 --full` without a launcher (gloo rehearsal backend, both ranks on the box's one GPU): the parent
    (no GPU call) starts two ranks under torch.distributed.run; rank 0 prints ONE JSON line whose `value` is the default split's
    (owner computes) and whose `exchanges` holds every split timed in this launch -- the other one (factor-partitioned rows
    between pairs) built, timed and freed after it -- each with its phase times, so that one node run compares them"""
    import json
    r = _run_bench(['--gpus', '2', '--edges', '200000', '--steps', '3', '--warmup', '1', '--no-cpu-baseline', '--full'],
                   env={'LHVI_DIST_BACKEND': 'gloo'})
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out['n_gpus'] == 2 and out['steps'] == 3 and out['value'] > 0 and out['config']['edges'] == 200000
    assert out['scaling'] == 'strong' and out['roofline']['bound'] == 'fp64_valu'
    assert out['config']['exchange'] == 'ownercompute' and 'owner computes' in out['config']['sharding']
    ex = out['exchanges']
    assert list(ex) == ['ownercompute', 'pairs'] and ex['ownercompute']['value'] == out['value']
    ph = ex['ownercompute']['phases_ms']
    assert ph['owned_variables'] > 0 and ph['ghost_variables'] > 0 and ph['cut_edge_rows_sent'] > 0 and ph['exchanged_MB_per_sweep'] > 0
    assert ex['pairs']['value'] > 0 and ex['pairs']['phases_ms']['boundary_variables'] > 0
    # every rank named its phases on stderr (what a stuck run would end with)
    assert 'rank 1: ownercompute: 3 timed sweeps' in r.stderr and 'rank 0: pairs: 3 timed sweeps' in r.stderr


@pytest.mark.gpu
def test_bench_flag_picks_the_split_and_a_stuck_phase_exits_non_zero():
    """`--exchange pairs --also none`: one split only, the factor-partitioned one; and the phase watchdog: with a phase limit no
    run can meet, every rank says where it stood and exits 124 instead of hanging"""
    import json
    r = _run_bench(['--gpus', '2', '--edges', '200000', '--steps', '2', '--warmup', '1', '--no-cpu-baseline', '--exchange', 'pairs',
                    '--also', 'none'], env={'LHVI_DIST_BACKEND': 'gloo'})
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][0])
    assert list(out['exchanges']) == ['pairs'] and 'factor-partitioned' in out['config']['sharding']
    r = _run_bench(['--gpus', '2', '--edges', '200000', '--steps', '2', '--warmup', '1', '--no-cpu-baseline'],
                   env={'LHVI_DIST_BACKEND': 'gloo', 'LHVI_BENCH_PHASE_TIMEOUT': '0.001'})
    assert r.returncode != 0 and 'STUCK in phase' in r.stderr


@pytest.mark.gpu
def test_bench_plain_run_and_its_dumped_outputs(tmp_path):
    """`bench.py --gpus 1` without --full: the headline line alone (no CPU baselines, no kernel timed on its own), `steps`
    timed sweeps; `--dump-outputs DIR`: float64 .npy files under 64 MB in all, the same bits in two runs of the same command"""
    import json
    dirs = [os.path.join(str(tmp_path), 'run%d' % k) for k in range(2)]
    for d in dirs:
        r = _run_bench(['--gpus', '1', '--edges', '200000', '--steps', '3', '--warmup', '1', '--dump-outputs', d])
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
        assert len(lines) == 1
        out = json.loads(lines[0])
        assert out['steps'] == 3 and out['unit'] == 'sweeps/s' and out['higher_is_better'] and out['dtype'] == 'f64'
        assert out['ms_per_step'] > 0 and abs(out['value'] * out['ms_per_step'] - 1e3) < 1e-6 * 1e3
        assert 'cpu_baseline' not in out and out['roofline']['alone'] is None
        assert 'CPU baseline' not in r.stderr and '3 timed sweeps' in r.stderr
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1]))
    assert {'f2v.npy', 'v2f.npy', 'eta.npy', 'proposal.npy', 'particles.npy', 'edge_index.npy', 'variable_index.npy'} <= set(names)
    total = 0
    for name in names:
        a, b = (np.load(os.path.join(d, name)) for d in dirs)
        assert a.dtype == np.float64 and a.shape[0] > 0 and np.array_equal(a, b, equal_nan=True), name
        total += os.path.getsize(os.path.join(dirs[0], name))
    assert total <= 64 << 20


@pytest.mark.gpu
@pytest.mark.parametrize('two_part', [False, True])
def test_owner_reduce_exchange_equals_the_all_to_all_form(two_part):
    """three simulated ranks, the same sweeps with the boundary rows exchanged between all pairs and reduced to an owner rank:
    proposals, particles and messages are the same bits (both forms add the ranks' sums in ascending rank order)"""
    import torch
    from lhvi import synth, dist, _abi
    _abi.require_gpu()
    world = 3
    flat = synth.hybrid_mrf_flat(V=2000, deg=4, seed=6)
    n = 64
    sets = []
    for owner in (False, True):
        group = dist.LoopbackGroup(world)
        runners = [dist.ShardedRunner(flat, n=n, seed=3, rank=r, world=world, group=group, owner_reduce=owner) for r in range(world)]
        for r in runners:
            r.init()
        for it in range(3):
            sends = [r.pre(part=1) if two_part else r.pre() for r in runners]
            for r, s in zip(runners, sends):
                group.post(r.rank, s, r.counts)
            if two_part:
                for r in runners:
                    r.interior()
            if owner:
                back = [r.owner_sums(group.collect(r.rank, r.W)) for r in runners]
                for r, s in zip(runners, back):
                    group.post(r.rank, s, r.lay['b_send'])
            for r in runners:
                (r.boundary if two_part else r.post)(group.collect(r.rank, r.W))
        sets.append(runners)
    pairs, owners = sets
    assert all(r.owner_reduce for r in owners) and not any(r.owner_reduce for r in pairs)
    assert any((np.diff(r.plan.brow_ptr) >= 2).any() for r in pairs)           # some variable lives on all three ranks
    sent_pairs = sum(r.n_elems for r in pairs)
    sent_owner = sum(r.a_send_elems + r.b_send_elems for r in owners)
    assert sent_owner < sent_pairs
    for a, b in zip(pairs, owners):
        hid = torch.from_numpy(a.plan.flat.var_hidden).to(a.bp.q_dev.device)
        assert torch.equal(a.bp.q_dev[hid], b.bp.q_dev[hid]) and torch.equal(a.bp.particles[hid], b.bp.particles[hid])
        he = hid[torch.from_numpy(a.plan.flat.edge_var.astype(np.int64)).to(hid.device)]
        assert torch.equal(a.bp.v2f[he], b.bp.v2f[he]) and torch.equal(a.bp.f2v[he], b.bp.f2v[he])
        assert torch.isfinite(b.bp.q_dev[hid]).all()


@pytest.mark.gpu
@pytest.mark.parametrize('world,two_part', [(2, False), (3, False), (2, True), (3, True)])
def test_sharded_sweep_matches_single_gpu(world, two_part):
    """simulate `world` ranks in one process (loopback exchange): messages and proposals equal the unsharded sweep, with
    the plain schedule (everything after the exchange) and the two-part one (interior part while the rows are in flight)"""
    import torch
    from lhvi import synth, dist, _abi
    from lhvi.pbp import EPBP
    _abi.require_gpu()
    flat = synth.hybrid_mrf_flat(V=2000, deg=4, seed=6)
    n = 64
    bp = EPBP(None, n=n, proposal_approximation='simple', sampler='device', seed=3)
    bp._setup(None, flat=flat)
    single = dist.SingleRunner(bp)
    single.init()
    group = dist.LoopbackGroup(world)
    runners = [dist.ShardedRunner(flat, n=n, seed=3, rank=r, world=world, group=group) for r in range(world)]
    for r in runners:
        r.init()
    for it in range(3):
        single.sweep()
        sends = [r.pre(part=1) if two_part else r.pre() for r in runners]
        for r, s in zip(runners, sends):
            group.post(r.rank, s, r.counts)
        if two_part:
            assert all(r.overlap for r in runners)
            for r in runners:
                r.interior()
            for r in runners:
                r.boundary(group.collect(r.rank, r.W))
        else:
            for r in runners:
                r.post(group.collect(r.rank, r.W))
        q = bp.q_dev.cpu().numpy()
        f2v = bp.f2v.cpu().numpy()
        v2f = bp.v2f.cpu().numpy()
        P = bp.particles.cpu().numpy()
        for r in runners:
            plan = r.plan
            hid = plan.flat.var_hidden
            # same draws as the unsharded run (Philox keyed by global id); q differs by summation-order rounding only
            np.testing.assert_allclose(r.bp.particles.cpu().numpy()[hid], P[plan.var_gid][hid], rtol=1e-11, atol=1e-12)
            np.testing.assert_allclose(r.bp.q_dev.cpu().numpy()[hid], q[plan.var_gid][hid], rtol=1e-11, atol=1e-13)
            he = hid[plan.flat.edge_var]
            # remote partial sums are added as a block: same values up to fp64 rounding of the summation order
            np.testing.assert_allclose(r.bp.v2f.cpu().numpy()[he], v2f[plan.edge_ids][he], rtol=1e-9, atol=1e-9)
            np.testing.assert_allclose(r.bp.f2v.cpu().numpy()[he], f2v[plan.edge_ids][he], rtol=1e-9, atol=1e-9)
        # replicas of a boundary variable hold bit-identical proposals and particles on every rank that owns it
        seen = {}
        for r in runners:
            Pr, Qr = r.bp.particles.cpu().numpy(), r.bp.q_dev.cpu().numpy()
            for lv in r.plan.bvars[:200]:
                if not r.plan.flat.var_hidden[lv] or not r.plan.flat.var_cont[lv]:
                    continue
                gid = int(r.plan.var_gid[lv])
                if gid in seen:
                    assert (seen[gid][0] == Pr[lv]).all() and (seen[gid][1] == Qr[lv]).all()
                else:
                    seen[gid] = (Pr[lv].copy(), Qr[lv].copy())


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['owner', 'sharded'])
def test_a_runner_sweep_drops_the_query_caches_of_the_previous_sample(kind):
    """a query between two sweeps of a runner caches the normalisers of that sample (``_batched``: quad, area, map, kl_logz); the
    next sweep starts a new sample and must drop them, as the solver's own sweep does.  Two identical sets of two loopback ranks,
    three sweeps each: set A answers ``kl_from`` after sweep 2 and after sweep 3, set B after sweep 3 only -- the two answers after
    sweep 3 are the same bits (a stale normaliser of sweep 2 would shift A's by a difference of logarithms), and A's two differ"""
    from lhvi import synth, dist, _abi
    _abi.require_gpu()
    flat = synth.hybrid_mrf_flat(V=300, deg=4, seed=37, frac_discrete=0.3, T=32)
    n, world = 16, 2
    owner = dist.partition_variables(flat, world)

    def runners():
        group = dist.LoopbackGroup(world)
        if kind == 'owner':
            rs = [dist.OwnerRunner(flat, n=n, seed=3, rank=r, world=world, group=group, var_owner=owner) for r in range(world)]
        else:
            rs = [dist.ShardedRunner(flat, n=n, seed=3, rank=r, world=world, group=group) for r in range(world)]
            assert all(r.overlap for r in rs)                                       # the two-part schedule
        for r in rs:
            r.init()
        return group, rs

    def sweep(group, rs):
        sends = [r.owned_half() if kind == 'owner' else r.pre(part=1) for r in rs]
        for r, s in zip(rs, sends):
            group.post(r.rank, s, r.counts)
        for r in rs:
            r.interior()
        for r in rs:
            r.boundary(group.collect(r.rank, None))

    def query(r):
        """KL of a unit Gaussian at the middle of the domain from the beliefs of a handful of owned (interior) continuous variables"""
        lf = r.plan.flat
        mine = r.plan.n_owned if kind == 'owner' else r.plan.n_interior
        rows = np.flatnonzero(lf.var_hidden & lf.var_cont & (np.arange(lf.V) < mine))[:5]
        assert rows.size == 5
        lo, hi = lf.dom_lo[lf.var_dom[rows]], lf.dom_hi[lf.var_dom[rows]]
        p = (np.ones((5, 1)), (0.5 * (lo + hi))[:, None], np.ones((5, 1)))
        kl, info = r.bp.kl_from(p, rows=rows, a=lo, b=hi, info=True)
        return kl, info['status']

    ga, A = runners()
    gb, B = runners()
    for _ in range(2):
        sweep(ga, A)
    first = [query(r) for r in A]
    sweep(ga, A)
    second = [query(r) for r in A]
    for _ in range(3):
        sweep(gb, B)
    fresh = [query(r) for r in B]
    for (kl1, st1), (kl2, st2), (klb, stb) in zip(first, second, fresh):
        print(kind, 'after sweep 2:', kl1.tolist(), st1.tolist(), ' after sweep 3:', kl2.tolist(), st2.tolist(), ' fresh:', klb.tolist(), stb.tolist())
        assert np.isfinite(kl1).all() and np.isfinite(kl2).all() and np.isfinite(klb).all()
        assert kl2.tobytes() == klb.tobytes() and st2.tolist() == stb.tolist()
        assert kl2.tobytes() != kl1.tobytes()


def _gpu_rank_worker(rank, world, port, out_dir, owner_reduce=False):
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'lifted-hybrid-variational-inference_amd')]
    import torch
    import torch.distributed as td
    from lhvi import synth, dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    td.init_process_group('gloo', rank=rank, world_size=world)
    flat = synth.hybrid_mrf_flat(V=1500, deg=4, seed=6)
    r = dist.ShardedRunner(flat, n=64, seed=3, rank=rank, world=world, owner_reduce=owner_reduce)
    assert r.owner_reduce == owner_reduce
    r.init()
    for _ in range(3):
        r.sweep()                      # pre -> all_to_all_single (gloo: staged through the host) -> post
    torch.cuda.synchronize()
    np.savez(os.path.join(out_dir, 'rank%d.npz' % rank), gid=r.plan.var_gid, q=r.bp.q_dev.cpu().numpy(),
             f2v=r.bp.f2v.cpu().numpy(), edge_ids=r.plan.edge_ids)
    td.barrier()
    td.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize('owner_reduce', [False, True])
def test_two_process_sharded_sweep_matches_single_gpu(tmp_path, owner_reduce):
    """two real processes (torch.distributed, gloo rehearsal backend, both on cuda:0) run the sharded sweep with the real
    collective call path (one all-to-all, or the two of the reduce-to-owner form); proposals and messages equal the unsharded run"""
    import torch.multiprocessing as mp
    from lhvi import synth, dist, _abi
    from lhvi.pbp import EPBP
    _abi.require_gpu()
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    ctx = mp.get_context('spawn')
    procs = [ctx.Process(target=_gpu_rank_worker, args=(r, 2, port, str(tmp_path), owner_reduce)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    flat = synth.hybrid_mrf_flat(V=1500, deg=4, seed=6)
    bp = EPBP(None, n=64, proposal_approximation='simple', sampler='device', seed=3)
    bp._setup(None, flat=flat)
    single = dist.SingleRunner(bp)
    single.init()
    for _ in range(3):
        single.sweep()
    q, f2v = bp.q_dev.cpu().numpy(), bp.f2v.cpu().numpy()
    hid = flat.var_hidden
    for r in range(2):
        z = np.load(os.path.join(str(tmp_path), 'rank%d.npz' % r))
        h = hid[z['gid']]
        np.testing.assert_allclose(z['q'][h], q[z['gid']][h], rtol=1e-10, atol=1e-12)
        he = hid[flat.edge_var[z['edge_ids']]]
        np.testing.assert_allclose(z['f2v'][he], f2v[z['edge_ids']][he], rtol=1e-9, atol=1e-8)


def _rccl_self_worker(port, out):
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'lifted-hybrid-variational-inference_amd')]
    import torch
    import torch.distributed as td
    from lhvi import synth, dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK='0', WORLD_SIZE='1')
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    torch.cuda.set_device(0)
    td.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))
    flat = synth.hybrid_mrf_flat(V=600, deg=4, seed=8)
    runner = dist.ShardedRunner(flat, n=64, seed=3, rank=0, world=1)
    runner.init()
    # the exchange call of a real run, on a fabricated row block addressed to this rank itself
    k = 5 * (64 + 2)
    runner.n_elems, runner.counts = k, [k]
    runner.send = torch.arange(k, dtype=torch.float64, device='cuda')
    runner.recv = torch.zeros(k, dtype=torch.float64, device='cuda')
    got = runner.exchange(runner.send[:k])
    td.barrier()
    t = torch.tensor([1.5], dtype=torch.float64, device='cuda')
    td.all_reduce(t, op=td.ReduceOp.MAX)
    torch.cuda.synchronize()
    ok = bool(torch.equal(got, runner.send)) and float(t.item()) == 1.5
    # the overlapped schedule's stream pattern: the collective started asynchronously (RCCL's copy kernel on RCCL's stream),
    # the slot-filling persistent f2v kernels launched right behind it on the compute stream (LEAVE_ROOM, as sharded runs
    # set it), then work.wait().  Both must finish, the received rows must be the sent ones, and the messages must equal
    # those of the same launch with nothing beside it.
    from lhvi import _abi
    from lhvi.pbp import EPBP
    big = synth.hybrid_mrf_flat(V=60000, deg=4, seed=9)            # heavy list long enough to fill every CU
    bp = EPBP(None, n=64, proposal_approximation='simple', sampler='device', seed=4)
    bp._setup(None, flat=big)
    single = dist.SingleRunner(bp)
    single.init()
    single.sweep()
    alone = bp.f2v.clone()
    sref = bp._struct()
    _abi.check(_abi.lib().lhvi_pbp_f2v(bp.dg.g, bp.dg.p, sref, _abi.ptr(bp.v2f), _abi.ptr(alone), _abi.stream_ptr()))
    k2 = 4_000_000                                                  # 32 MB: a copy that takes as long as the f2v launch's start-up
    send2 = torch.arange(k2, dtype=torch.float64, device='cuda')
    for it in range(3):
        recv2 = torch.zeros(k2, dtype=torch.float64, device='cuda')
        beside = torch.zeros_like(alone)
        work = td.all_to_all_single(recv2, send2, output_split_sizes=[k2], input_split_sizes=[k2], async_op=True)
        s2 = bp._struct()
        s2.flags |= _abi.PBP_LEAVE_ROOM
        _abi.check(_abi.lib().lhvi_pbp_f2v(bp.dg.g, bp.dg.p, s2, _abi.ptr(bp.v2f), _abi.ptr(beside), _abi.stream_ptr()))
        work.wait()
        torch.cuda.synchronize()
        ok = ok and bool(torch.equal(recv2, send2)) and bool(torch.equal(beside, alone))
    td.destroy_process_group()
    with open(out, 'w') as f:
        f.write('ok' if ok else 'mismatch')


@pytest.mark.gpu
def test_rccl_exchange_call_path(tmp_path):
    """the RCCL (backend 'nccl') calls of the multi-GPU run -- init with a device id, all_to_all_single with split lists on
    fp64 device buffers, barrier, max all-reduce -- on the one GPU a test box has (world size 1, rank 0 <-> rank 0); then
    the overlapped schedule's pattern, an asynchronous collective with the persistent f2v kernels launched beside it"""
    import torch.multiprocessing as mp
    from lhvi import _abi
    _abi.require_gpu()
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    out = os.path.join(str(tmp_path), 'rccl.txt')
    p = mp.get_context('spawn').Process(target=_rccl_self_worker, args=(port, out))
    p.start()
    p.join(timeout=300)
    assert p.exitcode == 0
    assert open(out).read() == 'ok'


# ---- owner-computes split (variables partitioned; a rank computes every message whose target it owns) ---------------------------
@pytest.mark.parametrize('world', [2, 3, 8])
def test_owner_plan_invariants(world):
    from lhvi import synth
    from lhvi.dist import OwnerPlan, partition_variables
    flat = synth.hybrid_mrf_flat(V=1500, deg=4, seed=2)
    owner = partition_variables(flat, world)
    assert sorted(np.unique(owner).tolist()) == list(range(world))
    plans = [OwnerPlan(flat, r, world, var_owner=owner) for r in range(world)]
    hid = np.isnan(flat.var_value)
    computed = np.zeros(flat.E, dtype=int)
    for p in plans:
        lf = p.flat
        np.testing.assert_array_equal(p.var_gid[lf.edge_var], flat.edge_var[p.edge_ids])
        own = np.arange(lf.V) < p.n_owned
        assert (owner[p.var_gid[own]] == p.rank).all() and (owner[p.var_gid[~own]] != p.rank).all()
        # an owned hidden variable has ALL its edges here, in the order of its row in the whole graph
        for v in np.flatnonzero(own & np.isnan(lf.var_value))[:200]:
            g = p.var_gid[v]
            want = flat.var_edge[flat.var_ptr[g]:flat.var_ptr[g + 1]]
            got = p.edge_ids[lf.var_edge[lf.var_ptr[v]:lf.var_ptr[v + 1]]]
            np.testing.assert_array_equal(got, want)
        computed[p.edge_ids[~p.edge_skip]] += 1
        # cut factors: exactly those with a ghost
        ghost = (np.arange(lf.V) >= p.n_owned) & (np.arange(lf.V) < p.n_owned + p.n_ghost)
        assert (np.isnan(lf.var_value[ghost])).all()
        np.testing.assert_array_equal(p.edge_key.astype(bool), np.repeat(np.maximum.reduceat(ghost[lf.edge_var].astype(np.int8), lf.fac_ptr[:-1]), np.diff(lf.fac_ptr)).astype(bool))
    # every message towards a hidden variable is computed exactly once
    np.testing.assert_array_equal(computed, hid[flat.edge_var].astype(int))
    # both ends of every pair list the same rows / proposals in the same order; every ghost edge receives exactly one row
    for p in plans:
        got_rows = np.concatenate([p.recv_rows[s] for s in range(world) if s != p.rank])
        ghost = (np.arange(p.flat.V) >= p.n_owned) & (np.arange(p.flat.V) < p.n_owned + p.n_ghost)
        np.testing.assert_array_equal(np.sort(got_rows), np.flatnonzero(ghost[p.flat.edge_var]))
        for s in range(world):
            if s == p.rank:
                continue
            q = plans[s]
            np.testing.assert_array_equal(p.edge_ids[p.send_rows[s]], q.edge_ids[q.recv_rows[p.rank]])
            np.testing.assert_array_equal(p.var_gid[p.send_q[s]], q.var_gid[q.recv_q[p.rank]])
        n = 16
        lay = p.layout(n)
        for side in ('send', 'recv'):
            L = lay[side]
            e, o, w = p.rows_of(L, n)
            used = int(w.sum()) + 2 * L['q_var'].size
            # per peer: continuous rows, discrete rows, proposals, then padding to whole rows of n doubles (fewer than n per peer)
            assert sum(L['counts']) == L['size'] and all(c % n == 0 for c in L['counts']) and 0 <= L['size'] - used < n * world
            offs = np.concatenate([np.repeat(o, w) + np.concatenate([np.arange(k) for k in w] or [np.zeros(0, int)]),
                                   np.repeat(L['q_off'], 2) + np.tile([0, 1], L['q_var'].size)])
            assert np.unique(offs).size == offs.size == used and offs.min(initial=0) >= 0 and offs.max(initial=-1) < L['size']    # nothing overlaps
            assert (L['cont_off'] % n == 0).all() and (p.flat.var_cont[p.flat.edge_var[L['cont_edge']]]).all()
        canon, extra = p.ghost_rows(n)
        R = lay['recv']
        assert (canon[R['cont_edge']] == p.flat.E + R['cont_off'] // n).all() and extra * n >= R['size']
        rest = np.setdiff1d(np.arange(p.flat.E), R['cont_edge'])
        assert (canon[rest] == rest).all()
        # the two ends of a pair cut a block at the same places
        for s in range(world):
            if s != p.rank:
                assert lay['send']['counts'][s] == plans[s].layout(n)['recv']['counts'][p.rank]


def _owner_compute_gloo_worker(rank, world, port, out):
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'lifted-hybrid-variational-inference_amd')]
    import torch
    import torch.distributed as td
    from lhvi import synth
    from lhvi.dist import OwnerPlan, partition_variables
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    td.init_process_group('gloo', rank=rank, world_size=world)
    flat = synth.hybrid_mrf_flat(V=900, deg=4, seed=5)
    plan = OwnerPlan(flat, rank, world, var_owner=partition_variables(flat, world))
    n = 6
    lf = plan.flat
    np_host = np.where(np.isnan(lf.var_value), np.where(lf.var_cont, n, 2), 0)
    lay = plan.layout(n, np_host)
    # a row / a proposal is a function of its global id, so every rank can check what it received on its own
    row = lambda ge: np.sin(0.1 * ge + np.arange(n))
    prop = lambda gv: np.array([np.cos(0.3 * gv), 1.0 + gv % 7])
    S = lay['send']
    send = torch.zeros(max(S['size'], 1), dtype=torch.float64)
    for e, o, w in zip(*plan.rows_of(S, n)):
        send[o:o + w] = torch.from_numpy(row(plan.edge_ids[e])[:w])
    for v, o in zip(S['q_var'], S['q_off']):
        send[o:o + 2] = torch.from_numpy(prop(plan.var_gid[v]))
    R = lay['recv']
    recv = torch.empty(R['size'], dtype=torch.float64)
    td.all_to_all_single(recv, send[:S['size']], output_split_sizes=R['counts'], input_split_sizes=S['counts'])
    ok = True
    for e, o, w in zip(*plan.rows_of(R, n)):
        ok = ok and bool((recv[o:o + w].numpy() == row(plan.edge_ids[e])[:w]).all())
    # every continuous row starts a whole number of rows from the buffer's base (it is read in place behind the E message rows)
    canon, extra = plan.ghost_rows(n)
    ok = ok and bool((R['cont_off'] % n == 0).all()) and bool((canon[R['cont_edge']] == lf.E + R['cont_off'] // n).all()) \
        and extra * n >= R['size'] and all(c % n == 0 for c in R['counts'] + S['counts'])
    for v, o in zip(R['q_var'], R['q_off']):
        ok = ok and bool((recv[o:o + 2].numpy() == prop(plan.var_gid[v])).all())
    out.put((rank, ok, int(R['row_edge'].size + R['cont_edge'].size), int(R['q_var'].size)))
    td.barrier()
    td.destroy_process_group()


def _subgroup_worker(rank, world, port, out):
    """ranks 1 and 2 of three form a sub-group and run the owner-computes exchange inside it; rank 0 stays outside"""
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'lifted-hybrid-variational-inference_amd')]
    import torch
    import torch.distributed as td
    from lhvi import synth
    from lhvi.dist import OwnerPlan, broadcast_partition, broadcast_variable_partition, partition_factors, partition_variables
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    td.init_process_group('gloo', rank=rank, world_size=world)
    members = [1, 2]
    grp = td.new_group(members)                    # (every rank of the default group calls new_group)
    ok, nrows = True, 0
    if rank in members:
        r, w = members.index(rank), len(members)
        flat = synth.hybrid_mrf_flat(V=700, deg=4, seed=9)
        # the partitions come from the GROUP's first rank (global rank 1), not from global rank 0
        owner = broadcast_variable_partition(flat, r, w, group=grp)
        fac_owner = broadcast_partition(flat, r, w, group=grp)
        ok = ok and bool((owner == partition_variables(flat, w)).all()) and bool((fac_owner == partition_factors(flat, w)).all())
        plan = OwnerPlan(flat, r, w, var_owner=owner)
        n = 4
        lf = plan.flat
        lay = plan.layout(n, np.where(np.isnan(lf.var_value), np.where(lf.var_cont, n, 2), 0))
        row = lambda ge: np.sin(0.1 * ge + np.arange(n))
        S, R = lay['send'], lay['recv']
        send = torch.zeros(max(S['size'], 1), dtype=torch.float64)
        for e, o, wd in zip(*plan.rows_of(S, n)):
            send[o:o + wd] = torch.from_numpy(row(plan.edge_ids[e])[:wd])
        recv = torch.empty(R['size'], dtype=torch.float64)
        td.all_to_all_single(recv, send[:S['size']], output_split_sizes=R['counts'], input_split_sizes=S['counts'], group=grp)
        for e, o, wd in zip(*plan.rows_of(R, n)):
            ok = ok and bool((recv[o:o + wd].numpy() == row(plan.edge_ids[e])[:wd]).all())
        nrows = int(R['row_edge'].size + R['cont_edge'].size)
    out.put((rank, ok, nrows))
    td.barrier()
    td.destroy_process_group()


def test_partition_broadcast_and_exchange_on_a_sub_group():
    """the runners take a process group: partitions are broadcast from the GROUP's first rank and the exchange runs inside the group
    (three gloo processes, the group is ranks 1 and 2; ADVICE round 4: the collectives used to ignore the group they were given)"""
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    ctx = mp.get_context('spawn')
    out = ctx.Queue()
    procs = [ctx.Process(target=_subgroup_worker, args=(r, 3, port, out)) for r in range(3)]
    for p in procs:
        p.start()
    res = sorted(out.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert all(ok for _, ok, _ in res), res
    assert res[0][2] == 0 and res[1][2] > 0 and res[2][2] > 0


@pytest.mark.parametrize('world', [2, 3])
def test_owner_compute_exchange_gloo(world):
    """real processes over gloo: the one all_to_all of the owner-computes sweep with its unequal split lists delivers every cut
    edge's row and every ghost's proposal to the right place (both ends derive the order on their own)"""
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    ctx = mp.get_context('spawn')
    out = ctx.Queue()
    procs = [ctx.Process(target=_owner_compute_gloo_worker, args=(r, world, port, out)) for r in range(world)]
    for p in procs:
        p.start()
    res = [out.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert all(ok for _, ok, _, _ in res), res
    assert all(nr > 0 and nq > 0 for _, _, nr, nq in res)


@pytest.mark.gpu
@pytest.mark.parametrize('world', [2, 3, 8])
def test_owner_compute_sweep_equals_single_gpu_bit_for_bit(world):
    """`world` simulated ranks of the owner-computes split (loopback exchange) against the single-GPU sweep: proposals, particles
    and both message arrays are the same BITS -- every variable is swept once, over all its factors, in the single-GPU order, and
    ghosts are re-drawn from their owner's proposal with the sampler keyed by the global id"""
    import dist_models
    from lhvi import synth, dist, _abi
    _abi.require_gpu()
    flat = synth.hybrid_mrf_flat(V=2000, deg=4, seed=6)
    # (the loop and its comparisons live in tests/dist_models.py, shared with tests/test_gpu_dist_shapes.py)
    stats = dist_models.assert_owner_equals_single(flat, 64, world, dist.partition_variables(flat, world), 'simple', sweeps=3)
    assert all(st.n_owned > 0 and st.n_cut_factors > 0 and st.n_cont_ghost_edges > 0 for st in stats)


def _owner_compute_gpu_worker(rank, world, port, out_dir):
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'lifted-hybrid-variational-inference_amd')]
    import torch
    import torch.distributed as td
    from lhvi import synth, dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    td.init_process_group('gloo', rank=rank, world_size=world)
    flat = synth.hybrid_mrf_flat(V=1500, deg=4, seed=6)
    r = dist.OwnerRunner(flat, n=64, seed=3, rank=rank, world=world, var_owner=dist.broadcast_variable_partition(flat, rank, world))
    r.init()
    for _ in range(3):
        r.sweep()                      # owned half -> all_to_all_single (gloo: staged through the host) -> interior, boundary
    torch.cuda.synchronize()
    np.savez(os.path.join(out_dir, 'rank%d.npz' % rank), gid=r.plan.var_gid, q=r.bp.q_dev.cpu().numpy(), f2v=r.bp.f2v.cpu().numpy(),
             v2f=r.message_rows().cpu().numpy(), edge_ids=r.plan.edge_ids, mine=~r.plan.edge_skip, n_owned=r.plan.n_owned)
    td.barrier()
    td.destroy_process_group()


@pytest.mark.gpu
def test_two_process_owner_compute_sweep_equals_single_gpu(tmp_path):
    """two real processes (torch.distributed, gloo rehearsal backend, both on cuda:0) run the owner-computes sweep with the real
    collective call path; proposals and messages of the owned variables equal the unsharded run bit for bit"""
    import torch.multiprocessing as mp
    from lhvi import synth, dist, _abi
    from lhvi.pbp import EPBP
    _abi.require_gpu()
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    ctx = mp.get_context('spawn')
    procs = [ctx.Process(target=_owner_compute_gpu_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    flat = synth.hybrid_mrf_flat(V=1500, deg=4, seed=6)
    bp = EPBP(None, n=64, proposal_approximation='simple', sampler='device', seed=3)
    bp._setup(None, flat=flat)
    single = dist.SingleRunner(bp)
    single.init()
    for _ in range(3):
        single.sweep()
    q, f2v = bp.q_dev.cpu().numpy(), bp.f2v.cpu().numpy()
    hid = flat.var_hidden
    for r in range(2):
        z = np.load(os.path.join(str(tmp_path), 'rank%d.npz' % r))
        own = (np.arange(z['gid'].size) < int(z['n_owned'])) & hid[z['gid']]
        assert own.any() and (z['q'][own] == q[z['gid']][own]).all()
        m = z['mine']
        assert m.any() and (z['f2v'][m] == f2v[z['edge_ids']][m]).all()
