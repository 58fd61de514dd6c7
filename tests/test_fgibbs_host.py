"""CPU suite of the flat-graph Gibbs sampler (lhvi/fgibbs.py): the colouring, and the host twin ``lhvi_fgibbs_chain_host`` --
the device's code (csrc/fgibbs.hpp) with one "lane" in the sequential order -- against the NumPy restatement of
tests/fgibbs_models.py with injected draws: discrete states and every counter equal, continuous values to rtol 1e-12 (the
restatement adds ``L + u (R - L)`` as NumPy rounds it, the twin rounds the product first too; the bound allows one contracted
multiply-add)."""
import dataclasses
import os
import re

import numpy as np
import pytest

import fgibbs_models as fm
from lhvi import _abi, fgibbs, generators
from lhvi.graph import F, RV, Domain, Graph
from lhvi.potentials import TablePotential, X2Potential

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def built():
    if not os.path.exists(_abi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _abi.lib()


MODELS = {}


def model_of(name):
    if name not in MODELS:
        m = fm.build(name)
        MODELS[name] = (m, fgibbs.FlatGibbs(m.g))
    return MODELS[name]


# ---- colouring ---------------------------------------------------------------------------------------------------------------------
def check_colouring(flat):
    colour, n = fgibbs.colour_variables(flat)
    hidden = np.isnan(flat.var_value)
    assert colour.shape == (flat.V,) and (colour[~hidden] == -1).all() and (colour[hidden] >= 0).all()
    assert n == (colour.max() + 1 if hidden.any() else 0)
    assert set(colour[hidden]) == set(range(n))                     # no empty colour
    nbrs = [set() for _ in range(flat.V)]
    for f in range(flat.F):
        scope = [v for v in flat.edge_var[flat.fac_ptr[f]:flat.fac_ptr[f + 1]] if hidden[v]]
        assert len({colour[v] for v in scope}) == len(set(scope)), 'factor %d has two hidden variables of one colour' % f
        for v in scope:
            nbrs[v].update(w for w in scope if w != v)
    assert n <= 1 + max((len(s) for s in nbrs), default=0)
    # greedy in variable order: the smallest colour no earlier neighbour holds
    for v in np.flatnonzero(hidden):
        used = {colour[w] for w in nbrs[v] if w < v}
        assert colour[v] == min(c for c in range(len(used) + 1) if c not in used)
    return colour, n


@pytest.mark.parametrize('name', fm.DET_MODELS)
def test_colouring_of_the_models(name):
    m, s = model_of(name)
    colour, n = check_colouring(m.flat)
    want, order = fm.schedule(m)
    assert list(colour) == want and n == s.n_colours
    col_ptr, col_var, hub_ptr, hub_var = fgibbs.work_lists(m.flat, colour, n, 64)
    assert list(col_var) == order and col_ptr[0] == 0 and col_ptr[-1] == len(order)
    for c in range(n):
        seg = col_var[col_ptr[c]:col_ptr[c + 1]]
        assert (colour[seg] == c).all() and (np.diff(seg) > 0).all()
        hubs = hub_var[hub_ptr[c]:hub_ptr[c + 1]]
        deg = np.diff(m.flat.var_ptr)
        assert list(hubs) == [v for v in seg if deg[v] > 64]
    if name == 'hub':
        assert list(hub_var) == [0, 1]


def test_colouring_of_paper_popularity_and_rgm():
    rg = generators.paper_popularity(30, 4)
    flat, _ = rg.ground_flat()
    _, n = check_colouring(flat)
    assert n >= 2
    flat, _ = generators.rgm(12, 3).ground_flat()
    check_colouring(flat)


# ---- the twin against the restatement -----------------------------------------------------------------------------------------------
def host_run(name, **kw):
    m, s = model_of(name)
    x0, u = fm.draws(name, m)
    hid = np.flatnonzero(s.hidden)
    args = dict(chains=fm.CHAINS, num_burnin=0, num_samples=fm.ITERS, keep_vars=list(hid), init_x=x0, max_shrink=fm.MAX_SHRINK[name],
                u=u)
    args.update(kw)
    return m, s, x0, u, hid, fgibbs.HostChains(s, **args)


@pytest.mark.parametrize('name', fm.DET_MODELS)
def test_twin_equals_numpy_restatement(built, name):
    m, s, x0, u, hid, r = host_run(name)
    r.run()
    got = r.samples.reshape(hid.size, fm.CHAINS, fm.ITERS)
    cont = m.flat.dom_cont[m.flat.var_dom[hid]].astype(bool)
    for c in range(fm.CHAINS):
        ref = fm.restate(m, x0[c], u[:, c], fm.MAX_SHRINK[name])
        assert ref.closest >= fm.MARGIN
        np.testing.assert_array_equal(got[~cont, c].T, ref.x[:, hid[~cont]])
        np.testing.assert_allclose(got[cont, c].T, ref.x[:, hid[cont]], rtol=1e-12, atol=0)
        assert (r.stuck[c], r.capped[c], r.evals[c]) == (ref.stuck, ref.capped, ref.evals)
        # the final state and its indices
        np.testing.assert_allclose(r.x[:, c], ref.x[-1], rtol=1e-12, atol=0)
        np.testing.assert_array_equal(r.idx[:, c], fm.state_index(m, ref.x[-1]))
    if name == 'cap':
        assert r.capped.sum() > 0
    if name == 'hard_stuck':
        assert r.stuck.sum() > 0
        # the continuous variable starts at zero mass (y = -inf): its first proposal is accepted whatever its g
        np.testing.assert_array_equal(got[2, :, 0], u[0, :, 2, 1])
        assert (r.evals >= 2).all()


@pytest.mark.parametrize('name', ['kinds', 'hub'])
def test_split_calls_equal_one_call(built, name):
    kw = dict(num_burnin=1, num_samples=3, thin=2)            # iterations 1, 3, 5 are kept
    *_, one = host_run(name, **kw)
    *_, two = host_run(name, **kw)
    one.run()
    assert one.iters == 6
    two.advance(1).advance(4).advance(6)
    for a in ('x', 'idx', 'counts', 'sum1', 'sum2', 'samples', 'stuck', 'capped', 'evals'):
        np.testing.assert_array_equal(getattr(one, a), getattr(two, a), err_msg=a)


def test_accumulators_are_the_sums_of_the_kept_samples(built):
    m, s, x0, u, hid, full = host_run('kinds')
    *_, r = host_run('kinds', num_burnin=1, num_samples=3, thin=2)
    full.run()
    r.run()
    every = full.samples.reshape(hid.size, fm.CHAINS, fm.ITERS)
    kept = r.samples.reshape(hid.size, fm.CHAINS, 3)
    np.testing.assert_array_equal(kept, every[:, :, [1, 3, 5]])
    s.adopt(r)
    cont = m.flat.dom_cont[m.flat.var_dom[hid]].astype(bool)
    xs = kept[cont]                                            # [Nc, chains, 3]
    want1, want2 = np.zeros(xs.shape[:2]), np.zeros(xs.shape[:2])
    for k in range(3):
        want1 += xs[:, :, k]
        want2 += xs[:, :, k] * xs[:, :, k]
    np.testing.assert_array_equal(s.sum1, want1.T)
    np.testing.assert_array_equal(s.sum2, want2.T)
    for i, row in enumerate(np.flatnonzero(~cont)):
        d = int(s.dstates[i])
        states = np.asarray(m.rvs[hid[row]].domain.values, dtype=np.float64)
        want = (kept[row][:, :, None] == states[None, None, :]).sum(axis=1)
        np.testing.assert_array_equal(s.counts[:, s.dstate_off[i]:s.dstate_off[i] + d], want)
    assert s.stats()['evals'] == int(r.evals.sum()) and s.stats()['evals_per_slice_update'] >= 2
    dm = s.disc_marginals()
    assert len(dm) == 2 and abs(dm[1][0].sum() - 1) < 1e-12
    np.testing.assert_allclose(s.moments().mean, want1.mean(axis=1) / 3, rtol=1e-12)
    assert s.map(m.rvs[8]) == 0.35 and -4 <= s.map(m.rvs[2]) <= 4
    assert s.map_all()[0] == s.map(m.rvs[0])


def test_restated_philox_layout_equals_the_twins_own_draws(built):
    m, s = model_of('kinds')
    seed, ms = 20261021, 5
    own = fgibbs.HostChains(s, chains=3, num_samples=4, seed=seed, keep_vars='cont', max_shrink=ms).run()
    u = fm.philox_uniforms(seed, 4, 3, m.flat.V, ms)
    x0 = fm.philox_init(seed, 3, m.flat)
    assert ((u >= 0) & (u < 1)).all()
    inj = fgibbs.HostChains(s, chains=3, num_samples=4, seed=0, keep_vars='cont', max_shrink=ms, init_x=x0, u=u).run()
    for a in ('x', 'idx', 'samples', 'counts', 'capped', 'evals'):
        np.testing.assert_array_equal(getattr(own, a), getattr(inj, a), err_msg=a)
    # a chain's draws do not depend on the number of chains
    two = fgibbs.HostChains(s, chains=2, num_samples=4, seed=seed, keep_vars='cont', max_shrink=ms).run()
    np.testing.assert_array_equal(two.x, own.x[:, :2])
    other = fgibbs.HostChains(s, chains=3, num_samples=4, seed=seed + 1, keep_vars='cont', max_shrink=ms).run()
    assert not np.array_equal(other.x, own.x)


def test_isolated_variables_draw_uniformly(built):
    m, s, x0, u, hid, r = host_run('isolated')
    r.run()
    got = r.samples.reshape(hid.size, fm.CHAINS, fm.ITERS)
    # the continuous one: the first proposal is accepted (g = 0 >= log(1 - u_0)): exactly lo + u_1 (hi - lo)
    np.testing.assert_array_equal(got[1].T, -2.0 + u[:, :, 1, 1] * (5.0 - -2.0))
    # the discrete one: three equal masses
    np.testing.assert_array_equal(got[0].T, np.minimum(np.searchsorted(np.cumsum(np.full(3, np.exp(-np.log(3.0)))), u[:, :, 0, 0]), 2))
    assert r.capped.sum() == 0 and r.stuck.sum() == 0


# ---- the binding and the error cases ------------------------------------------------------------------------------------------------
def test_struct_matches_header_layout():
    text = open(os.path.join(ROOT, 'include', 'lhvi.h')).read()
    body = re.search(r'typedef struct lhvi_fgibbs \{(.*?)\} lhvi_fgibbs_t;', text, flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = [re.findall(r'([A-Za-z_][A-Za-z0-9_]*)\s*$', part.strip())[0] for decl in body.split(';') if decl.strip()
             for part in decl.split(',')]
    assert names == [f[0] for f in _abi.FgibbsStruct._fields_]
    assert int(re.search(r'#define\s+LHVI_FGIBBS_MAX_STATES\s+(\d+)', text).group(1)) == _abi.FGIBBS_MAX_STATES == fgibbs.MAX_STATES


def test_error_cases(built):
    m, s = model_of('kinds')
    with pytest.raises(NotImplementedError):
        fgibbs.FlatGibbs(None, flat=dataclasses.replace(m.flat, lifted=True))
    big = RV(Domain(tuple(range(fgibbs.MAX_STATES + 1))))
    with pytest.raises(NotImplementedError):
        fgibbs.FlatGibbs(fm._graph([big], [F(TablePotential(np.ones(fgibbs.MAX_STATES + 1)), nb=[big])]))
    at_limit = RV(Domain(tuple(range(fgibbs.MAX_STATES))))
    fgibbs.FlatGibbs(fm._graph([at_limit], [F(TablePotential(np.ones(fgibbs.MAX_STATES)), nb=[at_limit])]))
    inf = RV(Domain((-np.inf, 3.0), continuous=True, integral_points=np.linspace(-1, 1, 3)))
    with pytest.raises(ValueError):
        fgibbs.FlatGibbs(fm._graph([inf], [F(X2Potential(1.0, 1.0), nb=[inf])]))

    class NoSpec:
        symmetric = False

        def get(self, parameters):
            return 1.0
    v = RV(Domain((0, 1)))
    with pytest.raises(NotImplementedError):
        fgibbs.FlatGibbs(fm._graph([v], [F(NoSpec(), nb=[v])]))
    off = RV(Domain((0, 1)), value=0.5)
    w = RV(Domain((0, 1)))
    with pytest.raises(ValueError):
        fgibbs.FlatGibbs(fm._graph([off, w], [F(TablePotential(np.ones((2, 2))), nb=[off, w])]))
    with pytest.raises(ValueError):
        fgibbs.FlatGibbs(None)
    for bad in (dict(chains=0), dict(thin=0), dict(max_shrink=fgibbs.MAX_SHRINK + 1), dict(num_burnin=-1), dict(keep_vars=[8]),
                dict(keep_vars=[2, 2]), dict(init_x=np.zeros(3)), dict(u=np.zeros((1, 1, 9, 65)), num_samples=2),
                dict(init_x=np.full(9, 7.0))):
        with pytest.raises(ValueError):
            fgibbs.HostChains(s, **bad)
    with pytest.raises(RuntimeError):
        fgibbs.FlatGibbs(m.g).disc_marginals()
    # the C entry points refuse what the host wrapper would not build
    st = _abi.FgibbsStruct()
    st.thin = 0
    hg = s.host_graph()
    x, idx = np.zeros((9, 1)), np.zeros((9, 1), dtype=np.int32)
    assert built.lhvi_fgibbs_chain_host(hg.g, hg.p, st, 1, 0, 1, 0, 0, x.ctypes.data, idx.ctypes.data) == -1
    st.thin, st.max_shrink = 1, fgibbs.MAX_SHRINK + 1
    assert built.lhvi_fgibbs_chain_host(hg.g, hg.p, st, 1, 0, 1, 0, 0, x.ctypes.data, idx.ctypes.data) == -3
    st.max_shrink = 4
    assert built.lhvi_fgibbs_chain_host(hg.g, hg.p, st, 1, 1, 1, 0, 0, x.ctypes.data, idx.ctypes.data) == -1     # chain >= chains
    assert built.lhvi_fgibbs_chain_host(hg.g, hg.p, st, 1, 0, 1, 0, 0, x.ctypes.data, idx.ctypes.data) == 0      # no colours: init only
    np.testing.assert_array_equal(x[8], [0.35])
