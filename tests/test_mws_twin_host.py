"""CPU suite of the host twin of the free-running HybridMaxWalkSAT search (tests/mws_twin.py): the twin against the reference's
recorded trajectories, its draws, the ambiguity cap and the coverage of the runs that tests/test_gpu_mws_twin.py repeats on the
device, and the comparison rules themselves against mutated twins."""
import glob
import os
import warnings

import numpy as np
import pytest

import mws_models
import mws_twin as tw

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FIXTURES = sorted(os.path.basename(p)[5:-4] for p in glob.glob(os.path.join(GOLDEN, 'hmws_*.npz')))
ALL_CASES = sorted({**tw.CASES, **tw.CPU_ONLY_CASES})


# ---- the twin against the reference's recorded trajectories (the rules of test_gpu_mws_replay.py) ------------------------------
@pytest.mark.parametrize('name', FIXTURES)
def test_replay_step_matches_reference_fixture(name):
    d = np.load(os.path.join(GOLDEN, 'hmws_%s.npz' % name))
    twin = tw.Twin(getattr(mws_models, str(d['builder']))())
    np.testing.assert_array_equal(twin.numeric, d['numeric'])
    np.testing.assert_array_equal(twin.discrete, d['discrete'])
    n = len(d['clause'])
    assert n == int(d['params'][1]) and len(FIXTURES) >= 6
    x = d['init'].copy()
    diff, errs = [], []
    for j in range(n):
        sc, _ = twin.score(x)
        assert abs(sc - d['score'][j]) <= 1e-9 * max(1.0, abs(d['score'][j])), (j, sc, d['score'][j])
        s = twin.replay_step(x, d['clause'][j], d['walk'][j], d['walk_k'][j], d['noise'][j])
        assert (len(s.hard), len(s.soft)) == (d['n_hard'][j], d['n_soft'][j]), j
        assert s.winner == d['winner'][j], (j, s.cands)
        has = ~np.isnan(d['post'][j])
        cont = d['post_cont'][j].astype(bool)
        assert len(s.hv) == has.sum()
        val = np.array([s.post[v] for v in s.hv])
        ref = d['post'][j][:len(s.hv)]
        if s.accept != d['accept'][j]:
            # only where the clause's move is a continuous variable already at its optimum, and the value stays
            k = s.winner
            assert d['walk'][j] == 0 and (cont & has).any() and k >= 0, j
            assert abs(val[k] - ref[k]) <= 1e-7 * max(1.0, abs(ref[k])), j
            diff.append(j)
        else:
            for k, v in enumerate(s.hv):
                if not cont[k]:
                    assert val[k] == ref[k], (j, k)
                else:
                    errs.append(abs(val[k] - ref[k]) / max(1.0, abs(ref[k])))
        x[s.hv] = ref
    assert len(diff) <= 0.01 * n, diff
    if errs:
        errs = np.array(errs)
        assert errs.max() <= 1e-4, (float(errs.max()), int(np.argmax(errs)))
        assert (errs <= 1e-7).mean() >= 0.95, float((errs <= 1e-7).mean())


# ---- draws ------------------------------------------------------------------------------------------------------------------------
def test_uniforms_lie_in_the_unit_interval_and_depend_on_every_counter_word():
    base = tw.uniform2(5, 3, 4, 1, tw.TAG_FLIP)
    for other in (tw.uniform2(5, 2, 4, 1, tw.TAG_FLIP), tw.uniform2(5, 3, 5, 1, tw.TAG_FLIP), tw.uniform2(5, 3, 4, 2, tw.TAG_FLIP),
                  tw.uniform2(5, 3, 4, 1, tw.TAG_INIT), tw.uniform2(6, 3, 4, 1, tw.TAG_FLIP)):
        assert other[0] != base[0] and other[1] != base[1]
    us = [u for flip in range(200) for u in tw.flip_draws(11, flip, 1000)]
    assert all(0.0 <= u < 1.0 for u in us)
    assert 0.45 < np.mean(us) < 0.55
    assert tw.TAG_FLIP == 0x4d575346 and tw.TAG_INIT == 0x4d575349


def test_pick_reaches_both_ends_and_never_n():
    for n in (1, 2, 3, 7, 64, 130):
        ks = [tw.pick(u, n) for u in (0.0, 0.5, 1.0 - 2.0 ** -53)] + [tw.pick(i / 1000.0, n) for i in range(1000)]
        assert min(ks) == 0 and max(ks) == n - 1
    assert tw.pick(np.nextafter(1.0, 0.0), 3) == 2


def test_box_muller_is_the_cosine_branch():
    assert tw.box_muller(0.7, 0.0, 0.3) == 0.0
    r = np.sqrt(-2.0 * np.log(1.0 - 0.25))
    assert abs(tw.box_muller(2.0, 0.25, 0.5) + 2.0 * r) <= 1e-15 * r
    z = np.array([tw.box_muller(1.0, *tw.uniform2(3, i, 0, 2, tw.TAG_FLIP)) for i in range(4000)])
    assert abs(z.mean()) < 0.06 and abs(z.std() - 1.0) < 0.05


@pytest.mark.parametrize('name', ['multi_state', 'every_kind', 'small_hybrid'])
def test_init_values_lie_in_their_domains(name):
    g, _ = tw.build_case(name)
    twin = tw.Twin(g)
    seen = {v: set() for v in range(twin.V)}
    for tid in range(40):
        x = twin.init(tw.SEED, tid)
        for v, rv in enumerate(twin.rvs):
            if not twin.hidden[v]:
                assert x[v] == float(rv.value)
            elif twin.cont[v]:
                assert twin.bounds[v][0] <= x[v] < twin.bounds[v][1]
            else:
                assert x[v] in twin.states[v]
                seen[v].add(x[v])
    for v in range(twin.V):
        if twin.hidden[v] and not twin.cont[v]:
            assert seen[v] == set(twin.states[v])              # every state is reached, the last one too


# ---- the free runs the GPU tests repeat: ambiguity cap, agreement of the summation orders, coverage ---------------------------
@pytest.fixture(scope='module')
def free_runs():
    """name -> (twin, [run per try]) in forward order"""
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)          # XYPotential.get overflows to inf far from the mode
        for name in ALL_CASES:
            g, flips = tw.build_case(name)
            twin = tw.Twin(g)
            out[name] = (g, twin, [twin.run(tw.SEED, tid, flips, tw.EPSILON, tw.NOISE_STD) for tid in tw.TRY_IDS])
    return out


@pytest.mark.parametrize('name', ALL_CASES)
def test_ambiguous_flips_stay_under_the_cap_in_every_summation_order(name, free_runs):
    g, fwd, runs = free_runs[name]
    others = [tw.Twin(g, order) for order in tw.ORDERS if order != 'forward']
    flips = sum(len(r['steps']) for r in runs)
    amb = {order: 0 for order in tw.ORDERS}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        for tid, r in zip(tw.TRY_IDS, runs):
            for j, s in enumerate(r['steps']):
                amb['forward'] += s.ambiguous
                for o in others:
                    so = o.step(s.pre, j, tid, tw.SEED, tw.EPSILON, tw.NOISE_STD)
                    amb[o.order] += so.ambiguous
                    if not s.tight and not so.tight:
                        assert (so.clause, so.branch, so.winner, so.accept, so.numeric, so.changed) == \
                            (s.clause, s.branch, s.winner, s.accept, s.numeric, s.changed), (tid, j, o.order)
                        disc = ~fwd.cont_mask
                        assert np.array_equal(so.post[disc], s.post[disc]), (tid, j, o.order)
                        # continuous values: the optimiser amplifies the rounding of its objective (docs/kernels_mws.md)
                        assert np.all(np.abs(so.post - s.post) <= tw.VAL_LOOSE * np.maximum(1.0, np.abs(s.post))), (tid, j, o.order)
    for order, n in amb.items():
        assert n <= tw.AMBIGUOUS_CAP * flips, (order, n, flips)


def _events(free_runs):
    ev = set()
    for name, (g, t, runs) in free_runs.items():
        for r in runs:
            if (r['zeros'] > 0).any():
                ev.add('rec_zero')
            for s in r['steps']:
                at = t.discrete.index(s.clause) if s.c_disc else -1
                if s.hard:
                    if s.hard.index(s.clause) > 0:
                        ev.add('hard pick > 0')
                    if at >= 64 and name == 'many_130':
                        ev.add('hard pick in the second chunk')
                elif s.took_soft:
                    ev.add('u0 < p')
                    if at >= 128:
                        ev.add('soft pick in the third chunk')
                elif s.took_soft is False:
                    ev.add('u0 >= p')
                if s.branch == 'walk':
                    ev.add('walk continuous' if t.cont[s.walk_var] else 'walk discrete')
                    if not t.cont[s.walk_var] and s.walk_val not in t.states[s.walk_var]:
                        ev.add('off-domain walk value')
                else:
                    for v, _, _ in s.cands:
                        ev.add('greedy continuous' if t.cont[v] else 'greedy discrete %d' % len(t.states[v]))
                    if s.winner > 0:
                        ev.add('non-first winner')
                    if s.numeric == 'noop':
                        ev.add('rejected with a hidden discrete variable')
                    if s.numeric == 'joint':
                        ev.add('rejected without a hidden discrete variable')
                        if len(s.changed) >= 2:
                            ev.add('joint move over >= 2 continuous variables')
    return ev


def test_free_runs_cover_the_branches_the_fixtures_miss(free_runs):
    want = {'hard pick > 0', 'hard pick in the second chunk', 'soft pick in the third chunk', 'u0 < p', 'u0 >= p',
            'walk continuous', 'walk discrete', 'greedy continuous', 'greedy discrete 2', 'greedy discrete 3', 'greedy discrete 4',
            'non-first winner', 'rejected with a hidden discrete variable', 'rejected without a hidden discrete variable',
            'joint move over >= 2 continuous variables', 'off-domain walk value', 'rec_zero'}
    assert not want - _events(free_runs), want - _events(free_runs)


def test_models_have_the_shapes_they_are_for():
    for n in (63, 64, 65, 130):
        t = tw.Twin(mws_models.many_clauses(n))
        assert len(t.discrete) == n and len(t.numeric) == 3
        assert 0.15 * n <= sum(t.cls[f] == 1 for f in t.discrete) <= 0.4 * n
    t = tw.Twin(mws_models.wide_hub())
    deg = sorted(len(r) for r in t.rows)
    assert deg[-4:] == [65, 70, 70, 130] and t.V < 300
    c3 = [f for f in range(t.F) if len(t.scope[f]) == 3][0]
    assert 0 < t.rows[t.scope[c3][0]].index(c3) < 64 and len(t.union(t.scope[c3])) == 65 + 70 - 1
    t = tw.Twin(mws_models.multi_state())
    assert {len(s) for s in t.states if s} == {3, 4} and sum(c == 1 for c in t.cls) == 4
    t = tw.Twin(mws_models.shared_scope())
    pairs = [tuple(sorted(sc)) for sc in t.scope if len(sc) == 2]
    assert sorted(pairs.count(p) for p in set(pairs))[-2:] == [2, 3] and all(any(len(t.scope[f]) == 1 for f in r) for v, r in enumerate(t.rows) if t.hidden[v])
    t = tw.Twin(mws_models.every_kind())
    assert {type(f.potential).__name__ for f in t.factors} >= {'TablePotential', 'GaussianPotential', 'LinearGaussianPotential',
                                                               'XYPotential', 'X2Potential', 'MLNHardPotential', 'MLNPotential'}


# ---- the comparison rules must notice a subtly wrong search: mutated twins against an unmutated trajectory -----------------------
class NextClause(tw.Twin):                # the (k + 1)-th unsatisfied clause instead of the k-th
    @staticmethod
    def _kth(lst, k):
        return lst[(k + 1) % len(lst)]


class SwappedDraws(tw.Twin):              # u0 and u1 change roles
    @staticmethod
    def _roles(u):
        return (u[1], u[0]) + tuple(u[2:])


def _stand_in(name):
    """the device's stand-in: the reversed-order twin's own free runs"""
    g, flips = tw.build_case(name)
    dev = tw.Twin(g, 'reversed')
    return g, flips, [dev.run(tw.SEED, tid, flips, tw.EPSILON, tw.NOISE_STD) for tid in tw.TRY_IDS]


@pytest.mark.parametrize('name', ['many_130', 'small_hybrid'])
def test_comparison_rules_pass_the_unmutated_twin_and_trip_on_mutations(name):
    g, flips, runs = _stand_in(name)
    good = tw.Twin(g)
    stats = [tw.check_trajectory(good, tw.trajectory_of(r), tw.SEED, tid, tw.EPSILON, tw.NOISE_STD) for tid, r in zip(tw.TRY_IDS, runs)]
    tw.check_model_totals(stats)
    for cls in (NextClause, SwappedDraws):
        bad = cls(g)
        with pytest.raises(AssertionError, match=r"'flip'"):
            for tid, r in zip(tw.TRY_IDS, runs):
                tw.check_trajectory(bad, tw.trajectory_of(r), tw.SEED, tid, tw.EPSILON, tw.NOISE_STD)


def test_best_state_rule_trips_on_its_mutations():
    g, flips, runs = _stand_in('small_hybrid')
    tripped = {'late': 0, 'last': 0, 'ge': 0}
    for r in runs:
        tr = tw.trajectory_of(r)
        sc, st = r['scores'], r['states']
        tw.check_best(tr, *tw.best_of(sc[:flips], st[:flips]))
        k = int(np.argmax(sc[:flips]))
        wrong = {'late': (sc[k], st[k + 1]),                             # best_x copied one flip late
                 'last': tw.best_of(sc, st),                             # the state after the last flip considered
                 'ge': (sc[k], st[max(i for i in range(flips) if sc[i] == sc[k])])}      # the last maximum instead of the first
        for key, (bs, bx) in wrong.items():
            if bs != sc[k] or not np.array_equal(bx, st[k]):
                with pytest.raises(AssertionError, match='best_'):
                    tw.check_best(tr, bs, bx)
                tripped[key] += 1
    assert tripped['late'] > 0, tripped


def test_likelihood_log_rule():
    init = np.array([-5.0, -1.0])
    post = np.array([[-4.0, -6.0, -3.0], [-2.0, -0.5, -0.5]])
    zero = np.array([[0, 0, 1], [0, 0, 0]])
    assert tw.likelihood_log(init, post, zero) == [4.0, -np.inf, 0.5]
