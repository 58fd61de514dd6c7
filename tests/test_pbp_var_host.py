"""CPU tests of the twin and the bounds of tests/pbp_var_models.py: the twin against the C oracle (``PbpOracle.step_v2f``,
``step_proposal``) on every live value of every state family, the longdouble values against mpmath at 50 digits, the two classes of
values (live / must not be written) with the branches each family reaches, and that each defect the GPU tests are there to catch
moves some value by more than 100 bounds."""
import functools

import numpy as np
import pytest

import pbp_var_models as vm

STATES = {
    'zoo epbp simple n64': dict(n=64),
    'zoo hlbp EP lifted n20': dict(n=20, epbp=False, ep=True, lifted=True, var_threshold=0.02),
    'zoo epbp EP n33': dict(n=33, ep=True, var_threshold=0.02),
    'zoo hlbp simple lifted n5': dict(n=5, epbp=False, lifted=True),
    'ranges epbp simple n64': dict(n=64, family='ranges'),
    'ranges hlbp EP lifted n100': dict(n=100, family='ranges', epbp=False, ep=True, lifted=True, var_threshold=0.02),
    'ranges epbp simple lifted n17': dict(n=17, family='ranges', lifted=True),
    'init epbp EP n16': dict(n=16, family='init', ep=True),
    'init hlbp simple lifted n48': dict(n=48, family='init', epbp=False, lifted=True),
}


@functools.lru_cache(maxsize=None)
def state(name):
    return vm.build(**STATES[name])


@pytest.mark.parametrize('name', list(STATES))
def test_twin_agrees_with_the_c_oracle(name):
    """the oracle is fp64 in another order of summation (O(deg^2) re-summation, sequential moments): every live value of v2f, eta
    and q within the bound, every other value untouched"""
    st = state(name)
    o = st.oracle()
    before = o.v2f.copy()
    o.step_v2f()
    tw = st.v2f()
    r = vm.ratio(o.v2f, tw.out, tw.bound)
    assert (o.v2f[~tw.live] == before[~tw.live]).all()
    worst = {'v2f': float(r[tw.live].max())}
    o.step_proposal()
    pr = st.proposal()
    for k, what in ((0, 'eta mu'), (1, 'eta sig')):
        worst[what] = float(vm.ratio(o.eta[pr.owned, k], pr.eta[pr.owned, k], pr.eta_bound[pr.owned, k]).max())
    for k, what in ((0, 'q mu'), (1, 'q sig')):
        worst[what] = float(vm.ratio(o.q[pr.q_live, k], pr.q[pr.q_live, k], pr.q_bound[pr.q_live, k]).max())
    print('%s: worst |oracle - twin| / bound: %s' % (name, ', '.join('%s %.3f' % kv for kv in worst.items())))
    assert all(v <= 1.0 for v in worst.values()), worst
    # kept sites and the sites of other variables: the old bits
    same = ~pr.owned | pr.kept
    assert (o.eta[same] == st.eta[same]).all()
    live_q = pr.q_live
    assert np.array_equal(o.q[~live_q], st.q[~live_q], equal_nan=True)


@pytest.mark.parametrize('name', list(STATES))
def test_every_value_is_live_or_untouched_and_every_branch_is_reached(name):
    st = state(name)
    fl = st.flat
    tw, pr = st.v2f(), st.proposal()
    cov = vm.coverage(st)
    print(name, cov)
    # v2f: live = the first np particles of the edges of hidden variables; nothing else
    want = np.zeros_like(tw.live)
    for v in st.hidden():
        want[st.rows(v), :st.counts[v]] = True
    assert (want == tw.live).all() and cov['live v2f'] + cov['untouched v2f'] == fl.E * st.n
    assert cov['untouched v2f'] > 0 and cov['untouched sites'] > 0                       # observed variables of every class
    assert {k for k in st.kinds} >= {'cont', 'cont observed', 'disc', 'disc observed'}
    assert np.isfinite(tw.bound[tw.live]).all() and (tw.bound[tw.live] > 0).all()
    assert cov['sites'] + cov['untouched sites'] == fl.E and pr.owned.sum() == sum(st.rows(v).size for v in st.cont())
    assert cov['duplicates'] >= 50 and cov['penalised'] >= 100 and cov['degree 4'] >= 10 and cov['degree 5'] >= 10 and cov['hub'] >= 20
    assert cov['T'] == sorted(vm.T_LIST)
    # rows across the register cache (4 / 5), the fused records (6 / 7) and chunks (8 / 9), the hub kernel's unroll (79, 80, 81:
    # four waves, k + 12 < deg), the slices (63, 64, 65) and a row of 200
    assert set(cov['degrees']) >= {1, 2, 4, 5, 6, 7, 8, 9, 16, 17, 63, 64, 65, 79, 80, 81, 200}
    assert (st.n > 64) == ('n100' in name) and cov['max rule'] + cov['mean rule'] == int(tw.live.any(axis=1).sum())
    if 'lifted' in name:
        assert cov['counts'] == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
    if name.startswith('ranges'):
        assert cov['max rule'] >= 500 and cov['mean rule'] >= 500
        kinds = [t for v in st.hidden() for t in st.tags.get(int(v), ())]
        assert all(kinds.count(k) >= 10 for k in ('under', 'over', 'floor entries', 'dup max')), {k: kinds.count(k) for k in set(kinds)}
    if not name.startswith('init'):
        assert cov['clamped'] >= 40 and cov['kept z=0'] >= 100 and cov['kept zero'] >= 100 and cov['floored'] >= 100
    if 'EP' in name:
        assert cov['cavity'] >= 500 and cov['no cavity'] >= 10 and cov['eta eq'] >= 10 and cov['kept negative'] >= 100
        assert cov['unfloored'] >= 100 and cov['floored'] >= 100
    if name.startswith('init'):
        total = np.array([fl.edge_count[st.rows(v)].sum() for v in range(fl.V)])
        for v in st.cont():
            assert (st.q[v] == (0.0, 5.0)).all() and (st.eta[st.rows(v)] == (0.0, 5.0 * total[v])).all()


def test_count_totals_handed_over_are_used():
    """``var_degree``: the twin takes the floor from the totals it is given"""
    a = vm.build(n=10, lifted=True, ep=True, var_threshold=0.02)
    b = vm.build(n=10, lifted=True, ep=True, var_threshold=0.02, var_degree=True)
    pa, pb = a.proposal(), b.proposal()
    moved = pa.floored & pb.floored
    assert moved.sum() > 100 and (pb.eta[moved, 1] > pa.eta[moved, 1]).all()
    c = vm.build(n=10, lifted=True, ep=True, var_threshold=0.02)
    c.var_degree = np.array([a.flat.edge_count[a.rows(v)].sum() for v in range(a.flat.V)])
    pc = vm.proposal_twin(c)
    assert (pc.eta == pa.eta).all() and np.array_equal(pc.q, pa.q, equal_nan=True)


def test_twin_against_mpmath_at_50_digits():
    """the longdouble values of a sample across the families -- rows under either shift rule, clamped and penalised particles,
    sites with and without the cavity, floored and kept ones -- are good to a small fraction of their bounds"""
    import mpmath as mp
    rng = np.random.default_rng(5)
    worst, count = {'v2f': 0.0, 'eta': 0.0}, {'v2f mean': 0, 'v2f max': 0, 'clamped': 0, 'cavity': 0, 'plain': 0, 'kept': 0}
    with mp.workdps(50):
        def as_mp(x):
            hi = float(x)
            return mp.mpf(hi) + mp.mpf(float(x - vm.LD(hi)))

        for name in ('zoo hlbp EP lifted n20', 'ranges epbp simple lifted n17', 'ranges hlbp EP lifted n100', 'init epbp EP n16'):
            st = state(name)
            fl = st.flat
            tw, pr = st.v2f(), st.proposal()
            deg = np.diff(fl.var_ptr)
            for rule in (False, True):
                pool = np.flatnonzero((tw.max_rule == rule) & tw.live.any(axis=1) & (deg[fl.edge_var] <= 17))
                for e in rng.choice(pool, size=min(6, pool.size), replace=False):
                    ref = vm.v2f_value_mp(st, int(e), mp)
                    v = fl.edge_var[e]
                    for j, r in enumerate(ref):
                        err = abs(float(as_mp(tw.out[e, j]) - r))
                        worst['v2f'] = max(worst['v2f'], err / tw.bound[e, j])
                        count['clamped'] += int(tw.clamped[v, j])
                    count['v2f max' if rule else 'v2f mean'] += len(ref)
            sites = np.flatnonzero(pr.owned)
            for e in rng.choice(sites, size=60, replace=False):
                mu, sig, ok = vm.site_mp(st, int(e), mp)
                assert bool(ok) == (not pr.kept[e]), (name, e)
                if not ok:
                    count['kept'] += 1
                    continue
                count['cavity' if pr.cavity[e] else 'plain'] += 1
                pairs = [(pr.eta[e, 0], mu, pr.eta_bound[e, 0])] + ([] if pr.floored[e] else [(pr.eta[e, 1], sig, pr.eta_bound[e, 1])])
                for got, want, bound in pairs:
                    worst['eta'] = max(worst['eta'], abs(float(as_mp(got) - want)) / bound)
    print('worst |longdouble twin - mpmath| / bound: %s; values: %s' % (worst, count))
    assert count['v2f mean'] >= 100 and count['v2f max'] >= 100 and count['clamped'] >= 10
    assert count['cavity'] >= 20 and count['plain'] >= 20 and count['kept'] >= 20
    assert worst['v2f'] <= 0.02 and worst['eta'] <= 0.02


MUTANT_STATES = {'own_kept': 'ranges epbp simple n64', 'own_count': 'ranges hlbp EP lifted n100', 'mean_all': 'ranges epbp simple n64',
                 'max_all': 'ranges epbp simple n64', 'rule_max': 'ranges epbp simple n64', 'no_bound_penalty': 'zoo epbp simple n64',
                 'no_clamp': 'zoo epbp simple n64', 'no_counts': 'zoo hlbp EP lifted n20', 'floor_degree': 'zoo hlbp EP lifted n20',
                 'cavity_inverted': 'zoo epbp EP n33', 'overwrite_failed': 'zoo epbp EP n33', 'last_point': 'zoo epbp EP n33'}


@pytest.mark.parametrize('mutant', vm.V2F_MUTANTS + vm.PROPOSAL_MUTANTS)
def test_the_bounds_reject_a_wrong_twin(mutant):
    """own message not subtracted, own count not reduced by one (all copies dropped), mean over all particles, max over all
    particles, the shift rule's comparison against max instead of max - mean, bound particles not penalised, clamp missing; counts
    dropped in the proposal sums, floor from the degree, cavity switch inverted, failed site overwritten, last integral point dropped:
    each moves some live value by more than 100 bounds"""
    st = state(MUTANT_STATES[mutant])
    if mutant in vm.V2F_MUTANTS:
        tw, bad = st.v2f(), vm.v2f_twin(st, mutant=mutant)
        r = vm.ratio(bad.out, tw.out, tw.bound)[tw.live]
        hit, moved = float(r.max()), int((r > 100).sum())
    else:
        pr, bad = st.proposal(), vm.proposal_twin(st, mutant=mutant)
        r = np.concatenate([vm.ratio(bad.eta[pr.owned, k], pr.eta[pr.owned, k], pr.eta_bound[pr.owned, k]) for k in (0, 1)] +
                           [vm.ratio(bad.q[pr.q_live, k], pr.q[pr.q_live, k], pr.q_bound[pr.q_live, k]) for k in (0, 1)])
        hit, moved = float(r.max()), int((r > 100).sum())
    print('%s on %s: largest difference = %.3g bounds, %d values beyond 100' % (mutant, MUTANT_STATES[mutant], hit, moved))
    assert hit > 100.0 and moved >= 10, (mutant, hit, moved)


def test_bounds_at_typical_magnitudes():
    """the sizes the docstring's formulas give on the states: v -> f a few 1e-12 (up to a few 1e-10 on a hub row of lifted
    counts); sites 1e-14 to 1e-12 without the cavity; with it the median stays there and the largest follow the condition of the
    division sig c1 / (c1 - sig) -- a variance of thousands where the moments' variance comes close to the cavity's --, below
    1e-6 of the value"""
    for name in STATES:
        st = state(name)
        tw, pr = st.v2f(), st.proposal()
        acc = pr.owned & ~pr.kept & ~pr.floored
        assert tw.bound[tw.live].max() < 1e-9 and np.median(tw.bound[tw.live]) < 1e-10
        sig_bound = pr.eta_bound[acc, 1]
        print('%s: site variance bound median %.2e, max %.2e; q bound max %.2e' % (name, np.median(sig_bound), sig_bound.max(), pr.q_bound[pr.q_live].max()))
        # (the init state under EP takes nearly every site through the cavity: its median is the cavity's, 3e-11)
        assert np.median(sig_bound) < (1e-10 if 'EP' in name else 1e-11) and (sig_bound / pr.eta[acc, 1].astype(np.float64)).max() < 1e-6
        if 'EP' not in name:
            assert pr.eta_bound[acc].max() < 1e-11 and pr.q_bound[pr.q_live].max() < 1e-11
