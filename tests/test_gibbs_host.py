"""CPU suite of the block Gibbs sampler (lhvi/gibbs.py): the sampler model derived from the flat model, the device's per-chain
code run on the host with injected draws (lhvi_gibbs_chain_host) against the NumPy restatement of the reference's loop
(tests/gibbs_models.py), splitting a run over calls, the accumulators, the errors and the compat alias.

Tolerances: discrete samples equal; continuous samples rtol 1e-9, atol 1e-12 (both sides are backward-stable solves with the
same Cholesky factor; cond(J) <= 500 is asserted by the restatement, the bound of docs/kernels_exact.md)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gibbs_models as gmod
from lhvi import _abi, exact, gibbs
from lhvi.graph import F, RV, Domain
from lhvi.potentials import LogQuadratic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'lifted-hybrid-variational-inference_amd')


@pytest.fixture(scope='module', params=gmod.DET_MODELS + ('scratch_tables',))
def case(request):
    model = gmod.build(request.param)
    x0, z, u = gmod.draws(model)
    want = [gmod.restate(model, x0[c], z[:, c], u[:, c], gmod.BURNIN) for c in range(gmod.CHAINS)]
    return model, x0, z, u, want


def test_sampler_model_of_ref_hybrid2():
    gm = gmod.build('ref_hybrid2')['gm']
    # factors: hybrid (d0; x, y), table (d0), table (d0, d1), quadratic (x)
    assert (gm.n_hyb, gm.table_doubles, gm.max_states, gm.n_states) == (1, 3, 3, 5)
    assert list(gm.hyb_quad) == [0] and list(gm.hyb_off) == [0, 3] and list(gm.dstate_off) == [0, 3, 5]
    assert list(gm.vt_ptr) == [0, 2, 3] and list(gm.vt_fac) == [0, 1, 1]
    assert list(gm.vh_ptr) == [0, 1, 1] and list(gm.vh_fac) == [0]


def test_quadratic_without_discrete_axis_counts_as_continuous():
    gm = gmod.build('no_disc')['gm']
    assert gm.n_hyb == 0 and gm.table_doubles == 0 and gm.ex.n_quad == 11


def test_model_with_more_states_than_an_integer_holds():
    """Nd = 100: prod(dstates) fits no integer type; the sampler's model never forms it, the enumeration refuses"""
    model = gmod.em.rand_model(gmod.em.local_ns(), 100, 4, 3)
    gmod.em.set_indices(model)
    dstates = [rv.dstates for rv in model['Vd']]
    ex = exact.flatten_factors(model['factors'], dstates, 4)
    assert ex.M == 0 and not ex.dstride.any()
    gm = gibbs.GibbsModel(ex)
    assert gm.n_states == sum(dstates) and gm.vt_ptr[-1] == gm.vt_fac.size
    rng = np.random.RandomState(0)
    r = gibbs.chain_host(gm, [0] * 100, rng.randn(3, 4), rng.rand(3, 2, 100), 2, 1, 2)
    assert r.disc.shape == (2, 100) and r.counts.sum() == 200 and (r.disc < np.array(dstates)).all()


def test_host_chain_equals_numpy_restatement(case):
    model, x0, z, u, want = case
    Nd = len(model['Vd'])
    for c in range(gmod.CHAINS):
        r = gibbs.chain_host(model['gm'], x0[c], z[:, c], u[:, c], gmod.ITS, gmod.BURNIN, gmod.ITERS - gmod.BURNIN)
        disc, cont, closest = want[c]
        assert closest >= gmod.MARGIN
        np.testing.assert_array_equal(r.disc, disc)
        np.testing.assert_allclose(r.cont, cont, rtol=1e-9, atol=1e-12)
        if Nd:
            np.testing.assert_array_equal(r.x_d, disc[-1])
    print('smallest distance of a uniform from a cumulative probability: %.3g' % min(w[2] for w in want))


def test_host_split_run_and_accumulators(case):
    """iterations 0 .. 5 in one call equal 0 .. 1 + 2 .. 5 in two, bit for bit; the accumulators are the sums of the kept
    samples"""
    model, x0, z, u, _ = case
    gm, kept = model['gm'], gmod.ITERS - gmod.BURNIN
    one = gibbs.chain_host(gm, x0[1], z[:, 1], u[:, 1], gmod.ITS, gmod.BURNIN, kept)
    a = gibbs.chain_host(gm, x0[1], z[:, 1], u[:, 1], gmod.ITS, gmod.BURNIN, kept, 0, 3)
    b = gibbs.chain_host(gm, a.x_d, z[:, 1], u[:, 1], gmod.ITS, gmod.BURNIN, kept, 3, gmod.ITERS)
    np.testing.assert_array_equal(one.disc[0], a.disc[0])
    np.testing.assert_array_equal(one.disc[1:], b.disc[1:])
    np.testing.assert_array_equal(one.cont[1:], b.cont[1:])
    np.testing.assert_array_equal(one.x_d, b.x_d)
    Nd, Nc = gm.ex.Nd, gm.ex.Nc
    counts = np.zeros(gm.n_states, dtype=int)
    for n in range(Nd):
        counts[gm.dstate_off[n]:gm.dstate_off[n + 1]] = np.bincount(one.disc[:, n], minlength=model['dstates'][n])
    np.testing.assert_array_equal(one.counts, counts)
    i, j = np.tril_indices(Nc)
    np.testing.assert_allclose(one.sum1, one.cont.sum(axis=0), rtol=1e-13)
    np.testing.assert_allclose(one.sum2, (one.cont[:, i] * one.cont[:, j]).sum(axis=0), rtol=1e-13)


def test_one_discrete_variable_runs_one_sweep():
    """Nd = 1 (:167-168): u has one sweep per iteration whatever disc_block_its asks for"""
    model = gmod.em.rand_model(gmod.em.local_ns(), 1, 3, 7)
    gmod.em.set_indices(model)
    model['dstates'] = [rv.dstates for rv in model['Vd']]
    gm = gibbs.GibbsModel(exact.flatten_factors(model['factors'], model['dstates'], 3))
    x0, z, u = gmod.draws(model, chains=2, iters=5, its=100)
    assert u.shape == (5, 2, 1, 1)
    r = gibbs.chain_host(gm, x0[0], z[:, 0], u[:, 0], 100, 0, 5)
    disc, cont, _ = gmod.restate(model, x0[0], z[:, 0], u[:, 0])
    np.testing.assert_array_equal(r.disc, disc)
    np.testing.assert_allclose(r.cont, cont, rtol=1e-9, atol=1e-12)


def test_not_positive_definite_names_the_discrete_state():
    model = gmod.build('not_pd')
    rng = np.random.RandomState(4)
    z, u = rng.randn(4, 2), rng.rand(4, 2, 2)
    with pytest.raises(ValueError, match=r'not positive definite.*\(0, 1\)'):
        gibbs.chain_host(model['gm'], [0, 1], z, u, 2, 0, 4)
    # from (1, 0) with every uniform at 0.9999 the first sweep takes both variables to their last state; the next iteration
    # fails at (1, 1)
    with pytest.raises(ValueError, match=r'not positive definite.*\(1, 1\)'):
        gibbs.chain_host(model['gm'], [1, 0], z, np.full((4, 2, 2), 0.9999), 2, 0, 4)


def test_limits_and_arguments():
    l = _abi.lib()
    assert l.lhvi_gibbs_lds_bytes(8, 8, 3, 8) == 8 * (8 * 9 + 40 + 3 + 4 + 1) * 8
    assert l.lhvi_gibbs_lds_bytes(8, 8, 3, 3) == 0 and l.lhvi_gibbs_lds_bytes(8, 8, 3, 128) == 0
    assert l.lhvi_gibbs_lds_bytes(0, 0, 1, 64) == 16
    assert gibbs.default_lanes(0) >= 1 and gibbs.default_lanes(64) <= 64
    dc = Domain((-10, 10), continuous=True)
    Vc = [RV(dc) for _ in range(exact.MAX_NC + 1)]
    factors = [F(nb=(rv,), log_potential_fun=LogQuadratic(-np.ones((1, 1)), np.zeros(1), 0.)) for rv in Vc]
    s = gibbs.GibbsHybridGaussian(factors=factors, Vd=[], Vc=Vc)
    with pytest.raises(ValueError, match='LHVI_EXACT_MAX_NC'):      # Nc = 65: before any launch, before the GPU is asked for
        s.run(chains=4, num_burnin=1, num_samples=1)
    arrs = s.model.arrays()
    st = s.model.struct(lambda n: arrs[n].ctypes.data if arrs[n].size else None, 1, 0, 1, 0)
    assert l.lhvi_gibbs_chain_host(st, 0, 1, None, np.zeros(65).ctypes.data, None, None, None, None, None, None) == -3
    with pytest.raises(RuntimeError):
        s.disc_marginals()


def test_no_cpu_fallback_without_gpu():
    from conftest import has_gpu
    if has_gpu():
        return
    model = gmod.build('ref_hybrid2')
    with pytest.raises(_abi.LhviError):
        gibbs.block_gibbs_sample(model['factors'], model['Vd'], model['Vc'], 2, 2, seed=1)
    with pytest.raises(_abi.LhviError):
        gibbs.GibbsHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc']).run(chains=2, num_burnin=1, num_samples=1)


def test_compat_alias_exports_the_sampler():
    code = ('import sys; sys.path[:] = [%r, %r] + [p for p in sys.path if "site-packages" in p or "dist-packages" in p or '
            '"python3" in p and "repo" not in p]\n'
            'import hybrid_gaussian_mrf as h, lhvi.gibbs as g\n'
            'for n in ("block_gibbs_sample", "HybridGaussianSampler"):\n'
            '    assert getattr(h, n) is getattr(g, n), n\n'
            'assert g.gibbs_sample and g.GibbsHybridGaussian\n'
            'print("ok")') % (os.path.join(PKG, 'compat'), PKG)
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, cwd='/')
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == 'ok'


def test_sampled_table_and_map_of_the_sampler_class():
    """HybridGaussianSampler on given samples: the joint table of sampling_utils, the discrete map the reference cannot run,
    the K = 1 continuous map clipped to the domain"""
    model = gmod.build('ref_hybrid2')
    Vd_idx = {rv: i for i, rv in enumerate(model['Vd'])}
    Vc_idx = {rv: i for i, rv in enumerate(model['Vc'])}
    s = gibbs.HybridGaussianSampler(model['factors'], model['Vd'], model['Vc'], Vd_idx, Vc_idx)
    s.disc_samples = np.array([[2, 0], [2, 1], [0, 1], [2, 1]])
    s.cont_samples = np.array([[1., 9.], [2., 9.], [3., 9.], [4., 9.]])
    s.sampled_disc_marginal_table = gibbs.get_disc_marg_table_from_samples(s.disc_samples, s.dstates)
    want = np.zeros((3, 2))
    want[2, 0], want[2, 1], want[0, 1] = 0.25, 0.5, 0.25
    np.testing.assert_array_equal(s.sampled_disc_marginal_table, want)
    assert s.map(model['Vd'][0]) == 2 and s.map(model['Vd'][1]) == 1
    assert s.map(model['Vc'][0]) == 2.5 and s.map(model['Vc'][1]) == 5.0


def test_restated_conditional_tables_equal_the_formula_written_out():
    """the yardstick's reduced tables at arity 3, independently of the potentials' helper: x^T A_k x + b_k . x + c_k for every
    local state k of both hybrid factors of deep_scope, indexed in the factor's own argument order"""
    model = gmod.build('deep_scope')
    _, _, hyb_f = gmod.split_factors(model['factors'])
    assert [f.disc_nb_idx for f in hyb_f] == [(2, 0, 1), (3, 1, 0)] and [f.cont_nb_idx for f in hyb_f] == [(3, 0, 2), (1,)]
    x_c = np.array([0.7, -1.3, 2.1, -0.4])
    got = gmod.reduced_tables(hyb_f, x_c)
    for f, t in zip(hyb_f, got):
        lp = f.log_potential_fun
        dims = tuple(model['dstates'][i] for i in f.disc_nb_idx)
        assert t.shape == dims
        x = np.array([x_c[i] for i in f.cont_nb_idx])
        for k in np.ndindex(*dims):
            want = sum(lp.A[k][a, b] * x[a] * x[b] for a in range(len(x)) for b in range(len(x)))
            want += sum(lp.b[k][a] * x[a] for a in range(len(x))) + lp.c[k]
            assert abs(t[k] - want) <= 1e-13 * max(1.0, abs(want))


def test_philox_restatement_is_a_generator():
    """the NumPy restatement of the device generator (gibbs_models.philox_*), before the GPU suite compares the kernel with it:
    the Philox4x32-10 known-answer vectors of Random123 (kat_vectors: zero and all-ones counter and key), uniforms in [0, 1),
    normals and initial states with the moments of their distributions"""
    m = 0xffffffff
    assert [int(w) for w in gmod.philox4(0, 0, 0, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert [int(w) for w in gmod.philox4(m, m, m, m, (m << 32) | m)] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    z = gmod.philox_normals(7, 64, 20, 5)
    u = gmod.philox_uniforms(7, 64, 20, 3, 5)
    assert z.shape == (20, 64, 5) and u.shape == (20, 64, 3, 5) and u.min() >= 0 and u.max() < 1
    n = z.size
    assert abs(z.mean()) <= 4.5 / np.sqrt(n) and abs(z.var() - 1) <= 4.5 * np.sqrt(2. / n)
    assert abs(u.mean() - 0.5) <= 4.5 / np.sqrt(12. * u.size)
    assert len(np.unique(z)) == z.size and len(np.unique(u)) == u.size
    x = gmod.philox_init(7, 4096, [9, 5, 2])
    for k, d in enumerate((9, 5, 2)):
        freq = np.bincount(x[:, k], minlength=d) / 4096.
        assert np.abs(freq - 1. / d).max() <= 4.5 * np.sqrt((1. / d) * (1 - 1. / d) / 4096)
