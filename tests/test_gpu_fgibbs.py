"""GPU suite of the flat-graph Gibbs sampler (lhvi/fgibbs.py, csrc/fgibbs.hip).

Deterministic: the kernels with injected draws against the NumPy restatement of tests/fgibbs_models.py (potentials through the
Python classes' ``get``) on every model at 1, 3, 64 and 130 chains: discrete states and every counter equal, continuous values
rtol 1e-12.  The restatement asserts that every decision has a margin of 1e-9, far above the difference between the lane
kernel's sum (row order), the hub kernel's (64 strided partial sums, then the wave reduction) and the restatement's.
Bit equality over hub_degree, number of chains, launch splits and runs; the device generator against its restated layout.
Statistical, 4096 chains, burn-in 100, 200 kept at thin 2 (chosen on the host twin: R-hat 1.02 on ref_hybrid2, 1.00 on the
others): every discrete marginal, E[x] and E[x^2] within 4.5 standard errors over chains of ExactHybridGaussian (ref_hybrid2,
rand_3_2) or of the grid quadratures written out in tests/fgibbs_models.py (image, abs_mln), and R-hat <= 1.1."""
import functools

import numpy as np
import pytest

import exact_models as em
import fgibbs_models as fm
from lhvi import _abi, fgibbs
from lhvi.exact import ExactHybridGaussian
from lhvi.gmfit import fit_scalar_gms

pytestmark = pytest.mark.gpu
SEED = 20261021
MAXC = 130
BURN, KEEP, THIN = 100, 200, 2


@functools.lru_cache(maxsize=None)
def reference(name):
    """(model, sampler, x0 [130, V], u [6, 130, V, 1 + max_shrink], the restatement of every chain): computed once"""
    m = fm.build(name)
    s = fgibbs.FlatGibbs(m.g)
    x0, u = fm.draws(name, m, chains=MAXC)
    refs = [fm.restate(m, x0[c], u[:, c], fm.MAX_SHRINK[name]) for c in range(MAXC)]
    assert min(r.closest for r in refs) >= fm.MARGIN
    return m, s, x0, u, refs


def injected(name, C, **kw):
    m, s, x0, u, _ = reference(name)
    hid = np.flatnonzero(s.hidden)
    args = dict(chains=C, num_burnin=0, num_samples=fm.ITERS, keep_vars=list(hid), init_x=x0[:C], max_shrink=fm.MAX_SHRINK[name],
                u=np.ascontiguousarray(u[:, :C]))
    args.update(kw)
    s.run(**args)
    r = s._run
    return {a: r.numpy(a) for a in ('x', 'idx', 'counts', 'sum1', 'sum2', 'samples', 'stuck', 'capped', 'evals')}


@pytest.mark.parametrize('C', [1, 3, 64, 130])
@pytest.mark.parametrize('name', fm.DET_MODELS)
def test_kernel_equals_numpy_restatement(name, C):
    """1 and 3 chains: a wavefront spans several variables; 64: one variable a wavefront; 130: a partial last wavefront"""
    m, s, x0, u, refs = reference(name)
    got = injected(name, C)
    hid = np.flatnonzero(s.hidden)
    cont = m.flat.dom_cont[m.flat.var_dom[hid]].astype(bool)
    samples = got['samples'].reshape(hid.size, C, fm.ITERS)
    for c in range(C):
        ref = refs[c]
        np.testing.assert_array_equal(samples[~cont, c].T, ref.x[:, hid[~cont]])
        np.testing.assert_allclose(samples[cont, c].T, ref.x[:, hid[cont]], rtol=1e-12, atol=0)
        assert (got['stuck'][c], got['capped'][c], got['evals'][c]) == (ref.stuck, ref.capped, ref.evals)
        np.testing.assert_allclose(got['x'][:, c], ref.x[-1], rtol=1e-12, atol=0)
        np.testing.assert_array_equal(got['idx'][:, c], fm.state_index(m, ref.x[-1]))
    if name == 'cap':
        assert got['capped'].sum() > 0
    if name == 'hard_stuck':
        assert got['stuck'].sum() == C


@pytest.mark.parametrize('name', fm.DET_MODELS)
def test_hub_degree_changes_nothing(name):
    """everything through the hub kernel (0; isolated variables stay with the lane kernel), the default, and everything through
    the lane kernel: identical samples, accumulators and counters"""
    base = injected(name, 67, hub_degree=_abi.HUB_DEGREE)
    for hd in (0, 1 << 20):
        got = injected(name, 67, hub_degree=hd)
        for a, v in base.items():
            np.testing.assert_array_equal(got[a], v, err_msg='%s, hub_degree %d' % (a, hd))


@pytest.mark.parametrize('name', ['kinds', 'hub'])
def test_device_generator_equals_its_specification(name):
    m, s, *_ = reference(name)
    C, its, ms = 67, 4, 5
    s.run(chains=C, num_burnin=0, num_samples=its, seed=SEED, keep_vars='cont', max_shrink=ms)
    own = {a: s._run.numpy(a) for a in ('x', 'idx', 'samples', 'counts', 'capped', 'evals')}
    u = fm.philox_uniforms(SEED, its, C, m.flat.V, ms)
    s.run(chains=C, num_burnin=0, num_samples=its, seed=0, keep_vars='cont', max_shrink=ms, init_x=fm.philox_init(SEED, C, m.flat), u=u)
    for a, v in own.items():
        np.testing.assert_array_equal(s._run.numpy(a), v, err_msg=a)
    # and the host twin draws the same numbers
    host = fgibbs.HostChains(s, chains=C, num_samples=its, seed=SEED, keep_vars='cont', max_shrink=ms).run()
    np.testing.assert_array_equal(host.idx, own['idx'])
    np.testing.assert_allclose(host.x, own['x'], rtol=1e-12, atol=0)


# ---- invariance with the device generator --------------------------------------------------------------------------------------------
NAMES = ('x', 'idx', 'counts', 'sum1', 'sum2', 'samples', 'stuck', 'capped', 'evals')


def generated(chains=130, seed=SEED, **kw):
    _, s, *_ = reference('kinds')
    args = dict(chains=chains, num_burnin=3, num_samples=4, thin=2, seed=seed, keep_vars=list(np.flatnonzero(s.hidden)))
    args.update(kw)
    s.run(**args)
    return s, {a: s._run.numpy(a) for a in NAMES}


@pytest.fixture(scope='module')
def kinds_run():
    return generated()[1]


def test_fewer_chains_are_a_prefix(kinds_run):
    _, got = generated(chains=37)
    for a in ('x', 'idx', 'counts', 'sum1', 'sum2'):
        np.testing.assert_array_equal(got[a], kinds_run[a][:, :37], err_msg=a)
    for a in ('stuck', 'capped', 'evals'):
        np.testing.assert_array_equal(got[a], kinds_run[a][:37], err_msg=a)
    np.testing.assert_array_equal(got['samples'].reshape(-1, 37, 4), kinds_run['samples'].reshape(-1, 130, 4)[:, :37])


def test_split_launches_equal_one(kinds_run):
    for step in (1, 4):
        _, got = generated(its_per_launch=step)
        for a in NAMES:
            np.testing.assert_array_equal(got[a], kinds_run[a], err_msg='%s, %d iterations a launch' % (a, step))


def test_accumulators_are_the_sums_of_the_kept_samples(kinds_run):
    s, got = generated()
    fl = s.flat
    hid = np.flatnonzero(s.hidden)
    kept = got['samples'].reshape(hid.size, 130, 4)
    cont = fl.dom_cont[fl.var_dom[hid]].astype(bool)
    want1, want2 = np.zeros((hid.size, 130)), np.zeros((hid.size, 130))
    for k in range(4):
        want1 += kept[:, :, k]
        want2 += kept[:, :, k] * kept[:, :, k]
    np.testing.assert_array_equal(got['sum1'][hid[cont]], want1[cont])
    np.testing.assert_array_equal(got['sum2'][hid[cont]], want2[cont])
    assert (got['sum1'][hid[~cont]] == 0).all()
    for i, v in enumerate(s.Vd_ids):
        row = int(np.flatnonzero(hid == v)[0])
        d = fl.var_dom[v]
        states = fl.dom_val[fl.dom_ptr[d]:fl.dom_ptr[d + 1]]
        want = (kept[row][:, :, None] == states[None, None, :]).sum(axis=1)
        np.testing.assert_array_equal(s.counts[:, s.dstate_off[i]:s.dstate_off[i + 1]], want)
    assert (got['counts'].sum(axis=0) == 4 * s.Vd_ids.size).all()


def test_two_runs_are_identical_and_seeds_differ(kinds_run):
    _, again = generated()
    for a in NAMES:
        np.testing.assert_array_equal(again[a], kinds_run[a], err_msg=a)
    _, other = generated(seed=SEED + 1)
    assert not np.array_equal(other['x'], kinds_run['x'])
    assert not np.array_equal(other['idx'], kinds_run['idx'])


# ---- statistical -------------------------------------------------------------------------------------------------------------------
def z_scores(got, want):
    return np.abs(got.mean(axis=0) - want) / (got.std(axis=0, ddof=1) / np.sqrt(got.shape[0]))


def sampled(s):
    s.run(chains=4096, num_burnin=BURN, num_samples=KEEP, thin=THIN, seed=SEED)
    st = s.stats()
    assert st['stuck'] == 0 and st['capped'] == 0
    rh = s.rhat().max
    assert rh <= 1.1, rh
    return np.concatenate([s.counts, s.sum1, s.sum2], axis=1) / float(KEEP), rh, st


@pytest.mark.parametrize('name', ['ref_hybrid2', 'rand_3_2'])
def test_sampled_moments_match_the_exact_baseline(name):
    model = em.build(name)
    g = fm.with_potentials(model)
    ex = ExactHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc']).run()
    Nd = len(model['Vd'])
    t = ex.disc_table.reshape(-1)
    mu, var = ex.means.reshape(t.size, -1), ex.variances.reshape(t.size, -1)
    want = np.concatenate(list(ex.disc_marginals) + [t @ mu, t @ (var + mu * mu)])
    s = fgibbs.FlatGibbs(g)
    assert list(s.Vd_ids) == list(range(Nd))                    # the models list their discrete variables first
    got, rh, st = sampled(s)
    assert got.shape == (4096, want.size)
    z = z_scores(got, want)
    print('%s: %d quantities, max z = %.2f, R-hat %.3f, %.2f evaluations a slice update' % (name, want.size, z.max(), rh,
                                                                                          st['evals_per_slice_update']))
    assert z.max() <= 4.5
    # the class's own summaries are these numbers
    dm, mo = s.disc_marginals(), s.moments()
    np.testing.assert_allclose(np.concatenate([m for m, _ in dm]), got.mean(axis=0)[:s.n_states], rtol=1e-12)
    np.testing.assert_allclose(mo.mean, got.mean(axis=0)[s.n_states:s.n_states + s.Vc_ids.size], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(mo.var, mo.second - mo.mean ** 2)
    for n, rv in enumerate(model['Vd']):
        assert s.map(rv) == rv.domain.values[int(np.argmax(dm[n][0]))]
        assert s.belief(rv.domain.values[0], rv) == dm[n][0][0]


def test_sampled_moments_of_the_image_chain_match_the_quadrature():
    e1, e2 = fm.image_quadrature(2048)
    h1, h2 = fm.image_quadrature(1024)
    want, half = np.concatenate([e1, e2]), np.concatenate([h1, h2])
    got, rh, st = sampled(fgibbs.FlatGibbs(fm.image().g))
    se = got.std(axis=0, ddof=1) / np.sqrt(4096)
    assert np.abs(want - half).max() < 0.1 * se.min()
    z = z_scores(got, want)
    print('image: max z = %.2f, R-hat %.3f, %.2f evaluations a slice update' % (z.max(), rh, st['evals_per_slice_update']))
    assert z.max() <= 4.5


def test_sampled_moments_of_the_abs_formulas_match_the_quadrature():
    p, e1, e2 = fm.abs_quadrature(2048)
    hp, h1, h2 = fm.abs_quadrature(1024)
    want, half = np.concatenate([p, e1, e2]), np.concatenate([hp, h1, h2])
    s = fgibbs.FlatGibbs(fm.abs_mln().g)
    assert s.device_graph().p.interpreted == 2                  # both formulas go through the interpreter
    got, rh, st = sampled(s)
    se = got.std(axis=0, ddof=1) / np.sqrt(4096)
    assert np.abs(want - half).max() < 0.1 * se.min()
    z = z_scores(got, want)
    print('abs_mln: max z = %.2f, R-hat %.3f, %.2f evaluations a slice update' % (z.max(), rh, st['evals_per_slice_update']))
    assert z.max() <= 4.5


def test_fit_marginals_is_fit_scalar_gms_on_the_kept_samples():
    m = fm.image()
    s = fgibbs.FlatGibbs(m.g)
    s.run(chains=256, num_burnin=20, num_samples=16, seed=SEED, keep_vars='cont')
    assert tuple(s.samples.shape) == (3, 256 * 16)
    fit = s.fit_marginals(2)
    direct = fit_scalar_gms(s.samples, 2)
    for a in ('w', 'mu', 'var', 'lower_bound'):
        np.testing.assert_array_equal(getattr(fit, a).cpu().numpy(), getattr(direct, a).cpu().numpy(), err_msg=a)
    assert fit.R == 3 and fit.K == 2
    rv = m.rvs[1]
    b = s.belief(0.5, rv)
    assert b > 0 and b == float(fit.pdf(np.array([[0.5]]), rows=[1]).cpu().numpy()[0, 0])
    with pytest.raises(RuntimeError):
        fgibbs.FlatGibbs(m.g).run(chains=8, num_burnin=0, num_samples=2).fit_marginals(2)
