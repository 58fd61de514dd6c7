"""CPU tests of the f -> v twin and bound of tests/pbp_f2v_models.py: the twin against the C oracle on every point of every state
family, the twin's longdouble value against mpmath at 50 digits, the two point classes, the override arguments, and that each
defect the GPU tests are there to catch moves a message by more than 100 bounds."""
import functools

import numpy as np
import pytest

import pbp_f2v_models as fm

STATES = {'zoo n12': lambda: fm.zoo(12, 20), 'zoo n64': lambda: fm.zoo(64, 32), 'zoo uneven': lambda: fm.zoo(20, 33, uneven=True),
          'lifted': lambda: fm.lifted(), 'ranges n16': lambda: fm.ranges(16, 32), 'ranges n64': lambda: fm.ranges(64, 32)}


@functools.lru_cache(maxsize=None)
def state(name):
    return STATES[name]()


def points_of(st, e, table):
    """the columns of an [E, n + T] message table that hold the points of edge e's twin, in the twin's order"""
    tw = st.twin(e)
    return np.concatenate([table[e, :tw.np_], table[e, st.n:st.n + tw.x.size - tw.np_]])


@pytest.mark.parametrize('name', list(STATES))
def test_twin_agrees_with_the_c_oracle(name):
    """every regular point within the oracle's own fp64 bound (``oracle_bound``), every dead point at the floor"""
    st = state(name)
    o = st.oracle()
    o.step_f2v()
    worst, n_regular, n_dead = 0.0, 0, 0
    for e in st.edges():
        tw = st.twin(e)
        regular, dead = fm.classify(tw)
        got = points_of(st, e, o.f2v)
        ratio = np.abs(got[regular] - tw.L[regular].astype(np.float64)) / fm.oracle_bound(tw.M, tw.n_terms, tw.L)[regular]
        worst = max(worst, float(ratio.max()) if ratio.size else 0.0)
        assert (ratio <= 1.0).all(), (e, st.labels[st.flat.edge_fac[e]], float(ratio.max()))
        assert (got[dead] == fm.FLOOR).all(), (e, got[dead])
        n_regular, n_dead = n_regular + int(regular.sum()), n_dead + int(dead.sum())
    print('%s: %d regular points, worst |oracle - twin| / bound = %.3f; %d dead points' % (name, n_regular, worst, n_dead))
    assert n_regular > 0 and (n_dead > 0 or not name.startswith('ranges'))


@pytest.mark.parametrize('name', list(STATES))
def test_every_point_is_regular_or_dead(name):
    """no point between the classes and none left out; the ranges family holds every kind of row, and its dead rows make dead
    points, its other rows regular ones"""
    st = state(name)
    fl = st.flat
    seen = {k: [0, 0] for k in fm.RANGE_KINDS}
    for e in st.edges():
        regular, dead = fm.classify(st.twin(e))
        assert (regular ^ dead).all() and regular.size == st.twin(e).x.size
        f = fl.edge_fac[e]
        rows = [r for r in range(fl.fac_ptr[f], fl.fac_ptr[f + 1]) if r != e]
        kinds = {st.kinds[fl.edge_canon[r]] for r in rows if fl.var_hidden[fl.edge_var[r]]} - {'ordinary'}
        for k in kinds or {'ordinary'}:
            seen[k][0] += int(regular.sum())
            seen[k][1] += int(dead.sum())
        if 'dead' in kinds:
            assert dead.all(), e
    if name.startswith('ranges'):
        print({k: tuple(v) for k, v in seen.items()})
        assert all(seen[k][0] > 100 for k in ('ordinary', 'dominated', 'up', 'down')) and seen['dead'][1] > 100
        # the particles hold the domain's bounds, a duplicate and both zeros
        cont = np.flatnonzero(fl.var_hidden & fl.var_cont)
        for p in (st.particles[cont], st.old_particles[cont]):
            assert ((p == fm.LO).any(axis=1) & (p == fm.HI).any(axis=1)).all()
            assert (np.signbit(p) & (p == 0)).any(axis=1).all() and (~np.signbit(p) & (p == 0)).any(axis=1).all()
            assert all(np.unique(row).size < row.size for row in p)


def test_twin_against_mpmath_at_50_digits():
    """the longdouble value of at least 200 points drawn across the families, the dominated and shifted rows included, is good to
    a small fraction of the smallest GPU bound"""
    import mpmath as mp

    class Num:
        """mpf at 50 digits as the twin's number type"""
        log, exp = staticmethod(mp.log), staticmethod(mp.exp)

        def __new__(cls, v):
            return mp.mpf(v)

    rng = np.random.default_rng(7)
    worst, count, by_kind = 0.0, 0, {k: 0 for k in fm.RANGE_KINDS}
    with mp.workdps(50):
        for name in ('zoo n12', 'lifted', 'ranges n16', 'ranges n64'):
            st = state(name)
            fl = st.flat
            edges = st.edges()
            labels = np.array([st.labels[fl.edge_fac[e]] + ('/%d' % fl.edge_pos[e]) for e in edges])
            for lab in np.unique(labels):
                pool = edges[labels == lab]
                if name.startswith('ranges'):           # one edge per kind of partner row
                    kind_of = {e: next((st.kinds[r] for r in range(fl.fac_ptr[fl.edge_fac[e]], fl.fac_ptr[fl.edge_fac[e] + 1])
                                        if r != e and st.kinds[r] != 'ordinary'), 'ordinary') for e in pool}
                    chosen = [next(e for e in pool if kind_of[e] == k) for k in fm.RANGE_KINDS if k in kind_of.values()]
                else:
                    chosen, kind_of = [int(rng.choice(pool))], {}
                for e in chosen:
                    tw = st.twin(e)
                    if tw.n_terms > 300:
                        continue                        # (the joint sums: thousands of 50-digit exponentials per point)
                    regular, _ = fm.classify(tw)
                    pts = np.flatnonzero(regular)
                    if pts.size == 0:
                        continue
                    pts = rng.choice(pts, size=min(2, pts.size), replace=False)
                    ref = fm.f2v_twin(fl, st, e, num=Num, points=pts)
                    path = fm.PATH_OF_FAMILY[fm.expected_family(st, e)]
                    bound = np.minimum(fm.f2v_bound(tw.M[pts], tw.n_terms, tw.L[pts], path), fm.f2v_bound(tw.M[pts], tw.n_terms, tw.L[pts], 'ocml'))
                    err = np.array([abs(float(mp.mpf(float(tw.L[p])) + mp.mpf(float(tw.L[p] - fm.LD(float(tw.L[p])))) - r)) for p, r in zip(pts, ref.L)])
                    worst = max(worst, float((err / bound).max()))
                    count += pts.size
                    by_kind[kind_of.get(e, 'ordinary')] += pts.size
    print('%d points (%s): worst |longdouble twin - mpmath| / GPU bound = %.2e' % (count, by_kind, worst))
    assert count >= 200 and all(by_kind[k] >= 10 for k in ('dominated', 'up', 'down'))
    assert worst <= 0.02


def test_overrides_at_their_full_values_change_nothing():
    st = state('zoo n12')
    fl = st.flat
    for e in st.edges()[::7]:
        tw = st.twin(e)
        f = fl.edge_fac[e]
        partners = [fl.edge_var[r] for r in range(fl.fac_ptr[f], fl.fac_ptr[f + 1]) if r != e]
        nj = max([int(st.counts[v]) for v in partners if fl.var_hidden[v]], default=1)
        other = fm.f2v_twin(fl, st, e, nj=nj, np_=int(st.counts[fl.edge_var[e]]), T=tw.x.size - tw.np_)
        assert (other.L == tw.L).all() and (other.M == tw.M).all() and other.n_terms == tw.n_terms


def test_overrides_cut_from_the_front():
    """nj / np / T keep the FIRST particles and points; an observed partner enters at the given value without a message"""
    st = state('zoo n64')
    fl = st.flat
    e = next(e for e in st.edges() if st.labels[fl.edge_fac[e]] == 'linear_gaussian' and fl.edge_pos[e] == 0
             and fl.var_hidden[fl.edge_var[e + 1]])
    full = st.twin(e)
    cut = fm.f2v_twin(fl, st, e, nj=23, np_=33, T=7)
    assert cut.n_terms == 23 and cut.np_ == 33 and cut.x.size == 40
    assert (cut.x[:33] == full.x[:33]).all() and (cut.x[33:] == full.x[64:71]).all() and (cut.L < full.L[np.r_[0:33, 64:71]]).all()
    obs = fm.f2v_twin(fl, st, e, partner_value=0.3)
    a, var = fl.pot_param[fl.pot_off[fl.fac_pot[fl.edge_fac[e]]]:][:2]
    want = -(fm.LD(0.3) - fm.LD(a) * full.x.astype(fm.LD)) ** 2 / (2 * fm.LD(var))
    assert obs.n_terms == 1 and np.abs(obs.L - want).max() < 1e-17 * 300


MUTANTS = {'swap': ('gaussian', 'quadratic', 'linear_gaussian', 'formula', 'image_node'), 'drop': ('gaussian', 'hybrid3', 'table34', 'cq3', 'image_edge'),
           'nomsg': ('xy', 'hybrid2', 'table232', 'cq3', 'formula'), 'shift': ('quadratic', 'hybrid4', 'cq1', 'cq3', 'image_node')}


@pytest.mark.parametrize('mutant', list(MUTANTS))
def test_the_bound_rejects_a_wrong_twin(mutant):
    """argument-0 and argument-1 coefficients swapped, the last partner particle dropped, one partner's message omitted, grid
    point t + 1 in place of t: each differs from the twin by more than 100 bounds on a regular point of every edge class it touches"""
    st = state('ranges n16')
    fl = st.flat
    for label in MUTANTS[mutant]:
        hit = 0.0
        for e in st.edges():
            f = fl.edge_fac[e]
            if st.labels[f] != label or (mutant == 'shift' and not fl.var_cont[fl.edge_var[e]]):
                continue
            if mutant in ('drop', 'nomsg') and not any(fl.var_hidden[fl.edge_var[r]] for r in range(fl.fac_ptr[f], fl.fac_ptr[f + 1]) if r != e):
                continue
            tw, bad = st.twin(e), fm.f2v_twin(fl, st, e, mutant=mutant)
            regular, _ = fm.classify(tw)
            path = fm.PATH_OF_FAMILY[fm.expected_family(st, e)]
            bound = np.maximum(fm.f2v_bound(tw.M, tw.n_terms, tw.L, path), fm.f2v_bound(tw.M, tw.n_terms, tw.L, 'direct'))
            with np.errstate(invalid='ignore'):
                diff = np.abs((bad.L - tw.L).astype(np.float64))[regular] / bound[regular]
            if diff.size:
                hit = max(hit, float(np.nanmax(diff)))
        print('%s on %s: largest difference = %.3g bounds' % (mutant, label, hit))
        assert hit > 100.0, (mutant, label, hit)


def test_bound_at_the_edge_of_the_regular_class():
    """the figures of the module docstring: M = 600, n = 64, |L| = 600"""
    direct = float(fm.f2v_bound(600.0, 64, 600.0, 'direct'))
    ocml = float(fm.f2v_bound(600.0, 64, 600.0, 'ocml'))
    rec = float(fm.f2v_bound(600.0, 64, 600.0, 'recurrence', t=127, grid_dev=2.0))
    print('direct %.3g, ocml %.3g, recurrence %.3g' % (direct, ocml, rec))
    assert 1e-13 < ocml < direct < rec < 1e-11
    assert abs(direct - 2.0e-12) < 1e-13 and abs(ocml - 1.6e-12) < 1e-13 and abs(rec - 3.0e-12) < 2e-13


def test_routing_table_names_every_family():
    """the states of the GPU tests put edges on every family's list, with the target at argument 0 and at argument 1 of at least
    eight edges of every pair class, and with hidden and observed partners"""
    got = {}
    for n, T, kw in ((64, 32, {}), (16, 32, {}), (64, 100, {'long_grid': True}), (64, 32, {'paired_light': False})):
        st = fm.zoo(n, T)
        for e in st.edges():
            got.setdefault(fm.expected_family(st, e, **kw), set()).add(st.labels[st.flat.edge_fac[e]])
    print(got)
    assert set(got) == set(fm.FAMILIES)
    st = state('zoo n64')
    fl = st.flat
    for label in set(st.labels):
        es = [e for e in st.edges() if st.labels[fl.edge_fac[e]] == label]
        arity = int(np.diff(fl.fac_ptr)[fl.edge_fac[es[0]]])
        if arity == 1:
            assert len(es) >= 8
            continue
        for pos in range(arity):
            assert sum(fl.edge_pos[e] == pos for e in es) >= 8, (label, pos)
        hid = [all(fl.var_hidden[fl.edge_var[r]] for r in range(fl.fac_ptr[fl.edge_fac[e]], fl.fac_ptr[fl.edge_fac[e] + 1])) for e in es]
        assert any(hid) and not all(hid), label
