"""GPU suite of the mixture-belief queries (csrc/mixture.hip through lhvi/mixture.py): the kernels against the restatements of
tests/mixture_models.py under the criteria of tests/test_mixture_host.py (its docstring states them), bit equality where
docs/kernels_mixture.md claims it, and the solver-facing API."""
import os
import types

import numpy as np
import pytest

import mixture_models as mm
from lhvi import mixture
from lhvi.mixture import MixtureBelief

pytestmark = pytest.mark.gpu
LD = np.longdouble
WORST = mm.new_worst()


def device_run(belief):
    def run(X, obs):
        comp = belief.comp_log_prob(X, obs)
        condw, logp = belief.condition(X, obs)
        return comp, logp, condw
    return run


# ---- parts 1 and 3 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N_o', mm.NOS + mm.NOS_TWO_TILES)
@pytest.mark.parametrize('K', mm.KS)
def test_condition_within_the_derived_bounds(K, N_o):
    for M in mm.MS:
        case = mm.condition_case(K, N_o, M)
        belief = mm.belief_of(case)
        run = device_run(belief)
        r = mm.check_condition(belief, case, run, WORST)
        comp, logp, condw = run(case['X'], case['obs'])
        if K > 1 and N_o >= 63:
            assert (np.asarray(r['logcw'][:, K - 1], dtype=np.float64) < -760).all()
        if N_o == 0:
            np.testing.assert_allclose(condw, np.broadcast_to(case['w'], condw.shape), rtol=4 * mm.U * (K + 8), atol=0)
        # bit equality: a row alone against the row inside the batch; two runs
        for m in range(M):
            c1, l1, w1 = run(case['X'][m], case['obs'])
            assert np.array_equal(c1, comp[m], equal_nan=True) and l1 == logp[m] and np.array_equal(w1, condw[m])
        # the component sums are additions and multiplications in a fixed order, contraction off: given the device's records
        # the host twin forms the same bits (the records, logp and condw take logs and exps, which the two libraries round
        # differently in the last place)
        dev, host = belief._side(False), belief._side(True)
        host.rec[...] = dev.rec.cpu().numpy()
        host.lpi[...] = dev.lpi.cpu().numpy()
        np.testing.assert_array_equal(belief.comp_log_prob(case['X'], case['obs'], host=True), comp)
    print('largest error in units of its bound: comp %.3f, logp %.3f, log condw %.3f' % (WORST['comp'], WORST['logp'],
                                                                                     WORST['logcw']))


def test_row_bits_do_not_depend_on_the_batch():
    """a row at position 0 of a batch of 1, at position 6 of 9 (third row group) and at position 130 of 300"""
    case = mm.condition_case(8, 65, 1)
    belief = mm.belief_of(case)
    rng = np.random.RandomState(3)
    alone = device_run(belief)(case['X'], case['obs'])
    for M, pos in ((9, 6), (300, 130)):
        X = np.where(rng.rand(M, 65) < 0.3, np.nan, np.repeat(case['X'], M, axis=0) + rng.randn(M, 65).round())
        for j, v in enumerate(case['obs']):
            if v >= mm.NC:
                X[:, j] = np.where(np.isnan(X[:, j]), np.nan, 0.0)
        X[pos] = case['X'][0]
        comp, logp, condw = device_run(belief)(X, case['obs'])
        assert np.array_equal(comp[pos], alone[0][0]) and logp[pos] == alone[1][0] and np.array_equal(condw[pos], alone[2][0])


@pytest.mark.parametrize('K,N_o', [(1, 0), (3, 1), (5, 65), (8, 64), (33, 63), (33, 0)])
def test_log_belief_within_the_derived_bounds(K, N_o):
    case = mm.condition_case(K, N_o, 5)
    belief = mm.belief_of(case)
    query, x = mm.belief_points(case)
    r = mm.restate_condition(case, dtype=LD)
    r['e_logcw'] = mm.condition_bounds(r)[2]
    got = belief.log_belief_all(case['X'], case['obs'], query, x)
    mm.check_log_belief(case, r, got, query, x, WORST)
    np.testing.assert_array_equal(got[:, -1], got[:, 2])
    np.testing.assert_array_equal(belief.log_belief_all(case['X'][3], case['obs'], query, x), got[3])
    np.testing.assert_array_equal(belief.log_belief_all(case['X'], case['obs'], query, x), got)
    print('largest error of a log belief in units of its bound: %.3f' % WORST['belief'])


# ---- part 2 --------------------------------------------------------------------------------------------------------------------
def test_marginal_map_against_scipy_and_for_every_lane_count():
    stats = dict(cases=0, ambiguous=0, lower=-np.inf, far=0.0)
    for grp in mm.mode_groups(256):
        belief = mm.belief_of(grp)
        condw, _ = belief.condition(grp['X'], grp['obs'])
        x, f = belief.marginal_map_all(grp['X'], grp['obs'], grp['query'], info=True)
        mm.check_modes(grp, x, f, condw, stats)
        for lanes in (1, 2, 4, 8, 16, 32, 64):
            xl, fl = belief.marginal_map_all(grp['X'], grp['obs'], grp['query'], lanes=lanes, info=True)
            assert np.array_equal(xl, x, equal_nan=True) and np.array_equal(fl, f, equal_nan=True), lanes
    assert stats['cases'] == 256 and stats['ambiguous'] <= 0.05 * stats['cases']
    print('%(cases)d cases: %(ambiguous)d ambiguous, reference above the answer by at most %(lower).3g, farthest %(far).3g' % stats)


def test_marginal_map_with_65_components():
    """K = 65: at 64 lanes lane 0 takes the starts 0 and 64 (the second trip of the lane loop)"""
    stats = dict(cases=0, ambiguous=0, lower=-np.inf, far=0.0)
    for grp in mm.mode_groups(4, seed0=500, K_of=65):
        belief = mm.belief_of(grp)
        condw, _ = belief.condition(grp['X'], grp['obs'])
        x, f = belief.marginal_map_all(grp['X'], grp['obs'], grp['query'], lanes=64, info=True)
        mm.check_modes(grp, x, f, condw, stats)
        for lanes in (1, 16):
            xl, fl = belief.marginal_map_all(grp['X'], grp['obs'], grp['query'], lanes=lanes, info=True)
            assert np.array_equal(xl, x, equal_nan=True) and np.array_equal(fl, f, equal_nan=True), lanes
    assert stats['cases'] == 4


def test_observed_query_and_repeats():
    case = mm.condition_case(5, 65, 5)
    belief = mm.belief_of(case)
    query = np.concatenate([np.arange(mm.NC + mm.ND2 + mm.ND5), [3, 3]])
    x, f = belief.marginal_map_all(case['X'], case['obs'], query, info=True)
    xh, fh = belief.marginal_map_all(case['X'], case['obs'], query, info=True, host=True)
    np.testing.assert_array_equal(x[:, -1], x[:, 3])
    for m in range(5):
        for v in query[:-2]:
            seen = [case['X'][m, j] for j in np.flatnonzero(case['obs'] == v) if not np.isnan(case['X'][m, j])]
            if seen:
                assert x[m, v] == seen[0] and np.isnan(f[m, v])
            elif v >= mm.NC:
                assert x[m, v] == xh[m, v]
            else:
                assert abs(x[m, v] - xh[m, v]) <= 1e-6 and abs(f[m, v] - fh[m, v]) <= 1e-9


# ---- part 4 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', mm.JOINT_SHAPES + ('mixed',))
def test_joint_map_against_the_restatement(shape):
    case, _ = mm.joint_reference(shape)
    belief = mm.belief_of(case)
    got = belief.joint_map()
    mm.check_joint(shape, got)
    again = belief.joint_map()
    for key in ('xds', 'xcs', 'objs'):
        np.testing.assert_array_equal(got[key], again[key])


def test_reference_joint_functions_over_the_kernel(golden_dir):
    from lhvi import utils
    rec = np.load(os.path.join(golden_dir, 'mixture_joint.npz'))
    shape = (6, 5, 3, 2)
    case, pre = mm.joint_case(shape), 'j%d_%d_%d_%d_' % shape
    val = mixture.joint_map_from_belief_params(case['w'], case['Pi'], case['Mu'], case['Var'], case['bds'])
    np.testing.assert_array_equal(val['xd'], rec[pre + 'xd'])
    np.testing.assert_allclose(val['xc'], rec[pre + 'xc'], rtol=0, atol=1e-9)
    from lhvi.graph import RV, Domain
    Vc = [RV(Domain((-3, 3), continuous=True)) for _ in range(5)]
    Vd = [RV(Domain((0, 1))) for _ in range(6)]
    order = [Vd[2], Vc[0], Vc[4], Vd[0]]
    out = mixture.joint_map(order, Vd, Vc, {rv: i for i, rv in enumerate(Vd)}, {rv: i for i, rv in enumerate(Vc)},
                            dict(w=case['w'], Mu=case['Mu'], Var=case['Var'], Pi=case['Pi']))
    np.testing.assert_array_equal(out, [val['xd'][2], val['xc'][0], val['xc'][4], val['xd'][0]])
    x, f = utils.get_multivar_gm_mode(np.log(case['w']), case['Mu'], case['Var'], case['bds'], best_log_pdf=True)
    np.testing.assert_allclose(x, rec[pre + 'gm_x'], rtol=0, atol=1e-9)
    assert abs(f - float(rec[pre + 'gm_f'])) <= 1e-9


# ---- the reference's functions over the kernels -----------------------------------------------------------------------------
def rvs_of(case):
    rvs = [types.SimpleNamespace(domain_type='c-g', belief_params={'mu': case['Mu'][v], 'var': case['Var'][v]},
                                 values=np.array(case['bds'][:, v])) for v in range(len(case['Mu']))]
    return rvs + [types.SimpleNamespace(domain_type='d-%d' % pi.shape[1], belief_params={'pi': pi},
                                        values=np.arange(pi.shape[1], dtype=float)) for pi in case['Pi']]


@pytest.mark.parametrize('K,N_o', [(3, 1), (8, 65)])
def test_reference_functions_over_the_kernels(K, N_o, golden_dir):
    rec = np.load(os.path.join(golden_dir, 'mixture_cond_k%d.npz' % K))
    case = mm.condition_case(K, N_o, 5, holes=False)
    rvs = rvs_of(case)
    obs_rvs = [rvs[v] for v in case['obs']]
    w = case['w']

    def run(X, obs):
        return (mixture.calc_marg_comp_log_prob(X, obs_rvs), mixture.calc_marg_log_prob(X, obs_rvs, w),
                mixture.calc_cond_mixture_weights(X, obs_rvs, w))
    mm.check_condition(None, case, run, mm.new_worst())
    comp, logp, condw = run(case['X'], case['obs'])
    assert comp.shape == (5, K) and logp.shape == (5,) and condw.shape == (5, K)
    c1, l1, w1 = run(case['X'][0], case['obs'])
    assert c1.shape == (K,) and np.ndim(l1) == 0 and w1.shape == (K,)
    assert np.array_equal(c1, comp[0]) and l1 == logp[0] and np.array_equal(w1, condw[0])
    pre = 'no%d_' % N_o
    for n, pi in enumerate(case['Pi']):
        s, p = mixture.drv_belief_map(rec[pre + 'condw'], pi)
        want, best, gap = mm.drv_belief_map(rec[pre + 'condw'], pi)
        assert (gap >= 1e-9).all()
        np.testing.assert_array_equal(s, rec[pre + 'dmap'][n])
        np.testing.assert_allclose(p, best, rtol=4 * mm.U * K)
        s1, p1 = mixture.drv_belief_map(rec[pre + 'condw1'], pi)
        assert s1 == rec[pre + 'dmap1'][n] and isinstance(s1, int)
    if N_o == 1:
        for v, want in zip(rec[pre + 'query'], rec[pre + 'mmap']):
            got = mixture.marginal_map(case['X'][0], obs_rvs, rvs[v], w)
            if v >= mm.NC:
                assert got == want
            else:
                cw = rec[pre + 'condw1']
                _, fr, runs = mm.scalar_gm_mode(cw, case['Mu'][v], case['Var'][v], case['bds'][:, v])
                assert mm.gm_log_pdf(got, cw, case['Mu'][v], case['Var'][v]) >= fr - 1e-9
                assert mm.ambiguous(runs) or abs(got - want) <= 1e-4
                assert mixture.crv_belief_map(cw, case['Mu'][v], case['Var'][v], case['bds'][:, v]) == pytest.approx(got, abs=1e-9)


# ---- beliefs of fitted solvers -------------------------------------------------------------------------------------------------
def fitted(golden_dir, name, lifted):
    import modelio
    from test_oracle_golden import API
    from test_oracle_vi import load_vi
    from lhvi.vi import LiftedVarInference, VarInference
    z, meta = load_vi(golden_dir, name)
    g, rvs, factors = modelio.load_model(meta['model'], API)
    vi = (LiftedVarInference if lifted else VarInference)(g, 3, 3)
    np.random.seed(4)
    vi.run(4, lr=0.1, is_log=False)
    return vi, list(g.rvs)


def solver_checks(vi, rvs):
    K = vi.K
    belief = vi.mixture_belief()
    assert belief.normaliser == 'vi'
    hidden = [rv for rv in rvs if rv.value is None]
    evid = [rv for rv in rvs if rv.value is not None]
    rows = [belief.row(rv) for rv in hidden]
    # without evidence the log belief is log vi.belief; ground queries of a lifted solver go through rv.cluster (repeated rows)
    P = 3
    x = np.empty((len(hidden), P))
    pts = []
    for j, rv in enumerate(hidden):
        if rv.domain.continuous:
            pts.append(list(np.linspace(rv.domain.values[0] * 0.3, rv.domain.values[1] * 0.3, P)))
            x[j] = pts[-1]
        else:
            idx = [i % len(rv.domain.values) for i in range(P)]
            pts.append([rv.domain.values[i] for i in idx])
            x[j] = idx
    got = belief.log_belief_all(np.zeros((1, 0)), [], rows, x)[0]
    eta_c = vi._host('eta_c')
    for j, rv in enumerate(hidden):
        for p in range(P):
            want = np.log(vi.belief(pts[j][p], rv))
            if rv.domain.continuous:
                mu, var = eta_c[rows[j], :, 0], eta_c[rows[j], :, 1]
                size = np.max(np.abs(np.log(2.506628274631 * var)) + (pts[j][p] - mu) ** 2 * 0.5 / var)
            else:
                size = 0.0
            assert abs(got[j, p] - want) <= 16 * mm.U * (size + K + 8 + abs(want)), (j, p, got[j, p], want)
    same = {}
    for j, r in enumerate(rows):                                  # members of one cluster: one row, the same answers
        if r in same and np.array_equal(x[j], x[same[r]]):
            np.testing.assert_array_equal(got[j], got[same[r]])
        same.setdefault(r, j)
    # evidence rows of the solver: no observation of them, their value as a query
    if evid:
        with pytest.raises(ValueError, match='no parameters'):
            belief.condition(np.zeros((1, 1)), [belief.row(evid[0])])
        got = belief.marginal_map_all(np.zeros((2, 0)), [], [belief.row(evid[0]), rows[0]])
        assert (got[:, 0] == evid[0].value).all()
    # marginal_map_all with evidence against the per-call marginal_map (Gaussian normaliser: what the per-call functions use)
    gb = vi.mixture_belief(normaliser='gaussian')
    gb.set_belief_params(hidden)
    rng = np.random.RandomState(0)
    obs, cols = [next(rv for rv in hidden if rv.domain.continuous)], [rng.uniform(-1, 1, 3)]
    disc = [rv for rv in hidden if not rv.domain.continuous]
    if disc:
        obs.append(disc[0])
        cols.append(rng.randint(0, len(disc[0].domain.values), 3))
    query = [rv for rv in hidden if rv not in obs][:6]
    X = np.column_stack(cols).astype(float)
    allq = gb.marginal_map_all(X, [gb.row(rv) for rv in obs], [gb.row(rv) for rv in query])
    w = vi.w
    for m in range(3):
        for j, rv in enumerate(query):
            one = mixture.marginal_map(X[m], obs, rv, w)
            assert allq[m, j] == one, (m, j, allq[m, j], one)
    # the joint MAP of every hidden row: states of their rows, finite points and objectives, the winner the largest objective
    jm = belief.joint_map(coord_its=5)
    assert np.isfinite(jm['objs']).all() and jm['objs'].shape == (K,)
    for n, v in enumerate(jm['drows']):
        assert ((0 <= jm['xds'][:, n]) & (jm['xds'][:, n] < belief.nstates[v])).all()
    if jm['xc'] is not None:
        assert np.isfinite(jm['xcs']).all()
        np.testing.assert_array_equal(jm['xc'], jm['xcs'][int(np.argmax(jm['objs']))])
    return belief


def test_belief_of_a_fitted_ground_solver(golden_dir):
    vi, rvs = fitted(golden_dir, 'hybrid_k2', lifted=False)
    solver_checks(vi, rvs)


@pytest.mark.parametrize('name', ['lifted_hybrid_k2', 'lifted_rgm_small_k2'])
def test_belief_of_a_fitted_lifted_solver(golden_dir, name):
    """lifted_hybrid_k2: discrete and continuous clusters; lifted_rgm_small_k2: 20 ground variables in 9 clusters"""
    vi, rvs = fitted(golden_dir, name, lifted=True)
    belief = solver_checks(vi, rvs)
    assert belief.V == vi.flat.V                                  # rows are clusters: nothing was expanded
    if name == 'lifted_rgm_small_k2':
        hidden = [rv for rv in rvs if rv.value is None]
        assert belief.V < len(rvs) and len({belief.row(rv) for rv in hidden}) < len(hidden)
