"""The free-running device search (csrc/mws.hip, its own random draws) against the host twin (tests/mws_twin.py), flip by flip.

The C ABI is driven as ``run()`` drives it, but one flip per launch, and the whole device state is copied back after each
launch.  Every flip's input is the device's own pre-state, so nothing accumulates.  The rules are mws_twin.check_trajectory /
check_best / likelihood_log, which tests/test_mws_twin_host.py exercises on the CPU (mutated twins included)."""
import numpy as np
import pytest

import mws_twin as tw
from lhvi import _abi
from lhvi.mws import HybridMaxWalkSAT

pytestmark = pytest.mark.gpu


def stepped(h, seed, try_ids, flips, epsilon, noise_std):
    """lhvi_mws_init, then lhvi_mws_flips(j, j + 1) for every flip; dict of host arrays: x [flips + 1, T, V], init_score [T],
    rec_score / rec_zero [T, flips], best_score [T], best_x [T, V], cur_score [flips + 1, T]"""
    torch = _abi.require_gpu()
    fl = h._flat
    dg, p, t = h._device()
    dev = dg.device
    T = len(try_ids)
    f64, i32 = torch.float64, torch.int32
    x = torch.empty(T, fl.V, dtype=f64, device=dev)
    bx = torch.full((T, fl.V), float('nan'), dtype=f64, device=dev)
    cur, best = torch.empty(T, dtype=f64, device=dev), torch.empty(T, dtype=f64, device=dev)
    status, err = torch.zeros(T, dtype=i32, device=dev), torch.zeros(T, dtype=i32, device=dev)
    rec_score = torch.zeros(T, max(flips, 1), dtype=f64, device=dev)
    rec_zero = torch.zeros(T, max(flips, 1), dtype=i32, device=dev)
    rec_ticks = torch.zeros(T, max(flips, 1), dtype=torch.int64, device=dev)
    tid = torch.from_numpy(np.asarray(try_ids, dtype=np.int32)).to(dev)
    s = _abi.MwsStruct()
    s.T, s.max_flips, s.epsilon, s.noise_std, s.seed = T, flips, float(epsilon), float(noise_std), int(seed)
    s.try_id = _abi.ptr(tid)
    s.disc, s.n_disc = _abi.ptr(t['disc']), int(h.discrete_factors.size)
    s.num, s.n_num = _abi.ptr(t['num']), int(h.numeric_factors.size)
    s.fac_class = _abi.ptr(t['cls'])
    s.x, s.best_x, s.cur_score, s.best_score = _abi.ptr(x), _abi.ptr(bx), _abi.ptr(cur), _abi.ptr(best)
    s.status, s.err_flip = _abi.ptr(status), _abi.ptr(err)
    s.rec_score, s.rec_zero, s.rec_ticks = _abi.ptr(rec_score), _abi.ptr(rec_zero), _abi.ptr(rec_ticks)
    l = _abi.lib()
    _abi.check(l.lhvi_mws_init(dg.g, p, s, _abi.stream_ptr()))
    xs, curs = [x.cpu().numpy().copy()], [cur.cpu().numpy().copy()]
    for j in range(flips):
        _abi.check(l.lhvi_mws_flips(dg.g, p, s, j, j + 1, _abi.stream_ptr()))
        xs.append(x.cpu().numpy().copy())
        curs.append(cur.cpu().numpy().copy())
        assert (status.cpu().numpy() == 0).all(), (j, status.cpu().numpy(), err.cpu().numpy())
    return dict(x=np.array(xs), init_score=curs[0], cur_score=np.array(curs), rec_score=rec_score.cpu().numpy()[:, :flips],
                rec_zero=rec_zero.cpu().numpy()[:, :flips], best_score=best.cpu().numpy(), best_x=bx.cpu().numpy())


def try_traj(d, i):
    return dict(x=d['x'][:, i], init_score=d['init_score'][i], rec_score=d['rec_score'][i], rec_zero=d['rec_zero'][i])


def check_case(name, g, flips, epsilon, noise_std):
    """Observed on an MI355X (ambiguous share / worst continuous error per model): see docs/kernels_mws.md."""
    h = HybridMaxWalkSAT(g)
    twin = tw.Twin(g)
    np.testing.assert_array_equal(h.numeric_factors, twin.numeric)
    np.testing.assert_array_equal(h.discrete_factors, twin.discrete)
    d = stepped(h, tw.SEED, tw.TRY_IDS, flips, epsilon, noise_std)
    # the score the kernel carries from flip to flip is the one it records
    np.testing.assert_array_equal(d['cur_score'][1:].T, d['rec_score'])
    stats = []
    for i, tid in enumerate(tw.TRY_IDS):
        tr = try_traj(d, i)
        stats.append(tw.check_trajectory(twin, tr, tw.SEED, tid, epsilon, noise_std))
        tw.check_best(tr, d['best_score'][i], d['best_x'][i])
    share, worst = tw.check_model_totals(stats)
    print('%s: ambiguous share %.4f, tight-margin flips %d, worst continuous error %.3g over %d moves' % (
        name, share, sum(s['tight'] for s in stats), worst, sum(len(s['errs']) for s in stats)))
    return h, d


@pytest.mark.parametrize('name', sorted(tw.CASES))
def test_free_run_matches_twin_flip_by_flip(name):
    g, flips = tw.build_case(name)
    h, d = check_case(name, g, flips, tw.EPSILON, tw.NOISE_STD)
    # run() against the stepped drive: the same seed, try ids and flips in launches of run()'s own choosing
    r = HybridMaxWalkSAT(g).run(max_tries=len(tw.TRY_IDS), max_flips=flips, epsilon=tw.EPSILON, noise_std=tw.NOISE_STD,
                                seed=tw.SEED, try_ids=list(tw.TRY_IDS))
    np.testing.assert_array_equal(r.try_best_scores, d['best_score'])
    np.testing.assert_array_equal(r.try_best_x.cpu().numpy(), d['best_x'])
    k = int(np.argmax(d['best_score']))
    assert r.best_score == d['best_score'][k]
    np.testing.assert_array_equal(r.best_x, d['best_x'][k])
    want = tw.likelihood_log(d['init_score'], d['rec_score'], d['rec_zero'])
    assert [row[1] for row in r.time_log] == want
    assert any(v == -np.inf for v in want) == bool(((d['rec_zero'] > 0) & _logged(d)).any())
    secs = [row[0] for row in r.time_log]
    assert all(b >= a for a, b in zip(secs, secs[1:]))


def _logged(d):
    """[T, flips] bool: the flips whose new state the sequential log rule records"""
    out, best = np.zeros(d['rec_score'].shape, dtype=bool), -np.inf
    for i in range(out.shape[0]):
        for j in range(out.shape[1]):
            best = max(best, d['init_score'][i] if j == 0 else d['rec_score'][i, j - 1])
            out[i, j] = d['rec_score'][i, j] > best
    return out


@pytest.mark.parametrize('epsilon', [0.0, 1.0])
def test_small_hybrid_all_greedy_and_all_walk(epsilon):
    g, flips = tw.build_case('small_hybrid')
    check_case('small_hybrid eps=%g' % epsilon, g, flips, epsilon, tw.NOISE_STD)


@pytest.mark.parametrize('name', ['many_130', 'every_kind', 'small_hybrid'])
def test_results_do_not_depend_on_launch_chunks(name):
    g, flips = tw.build_case(name)

    class OneFlip(HybridMaxWalkSAT):
        MAX_FLIPS_PER_LAUNCH = 1

    class SevenFlips(HybridMaxWalkSAT):
        MAX_FLIPS_PER_LAUNCH = 7

    kw = dict(max_tries=len(tw.TRY_IDS), max_flips=flips, epsilon=tw.EPSILON, noise_std=tw.NOISE_STD, seed=tw.SEED,
              try_ids=list(tw.TRY_IDS))
    runs = [cls(g).run(**kw) for cls in (OneFlip, SevenFlips, HybridMaxWalkSAT)]
    assert len(runs[0].launch_ms) == flips and len(runs[1].launch_ms) < flips
    for r in runs[1:]:
        np.testing.assert_array_equal(r.try_best_scores, runs[0].try_best_scores)
        np.testing.assert_array_equal(r.try_best_x.cpu().numpy(), runs[0].try_best_x.cpu().numpy())
        assert [row[1] for row in r.time_log] == [row[1] for row in runs[0].time_log]


@pytest.mark.parametrize('name', ['multi_state', 'every_kind'])
def test_one_flip_keeps_the_initial_state_as_best(name):
    g, _ = tw.build_case(name)
    twin = tw.Twin(g)
    r = HybridMaxWalkSAT(g).run(max_tries=len(tw.TRY_IDS), max_flips=1, epsilon=tw.EPSILON, noise_std=tw.NOISE_STD, seed=tw.SEED,
                                try_ids=list(tw.TRY_IDS))
    bx = r.try_best_x.cpu().numpy()
    for i, tid in enumerate(tw.TRY_IDS):
        init = twin.init(tw.SEED, tid)
        np.testing.assert_array_equal(bx[i], init)
        sc, _ = twin.score(init, 'fsum')
        assert abs(r.try_best_scores[i] - sc) <= 1e-9 * max(1.0, abs(sc))
