"""CPU suite of the joint energies and the joint MAP (lhvi/hg_energy.py, csrc/hg_energy.hpp) through the host twins
lhvi_hg_energy_host / lhvi_argmax_first_host and lhvi_exact_config_host: no GPU.

Energies are held to ``|e - e_ref| <= 2 n_terms * 1.1e-16 * sum |term|`` against the np.longdouble restatement on the factor
objects (hg_energy_models.numpy_energy); the arg-max is compared with its plain Python definition; the exact joint MAP with the
reference's recorded results through ``energy(cfg) = log table + logZ - Nc/2 log 2 pi - 1/2 log det Sig`` at the fixtures' own
tolerance 1e-10 (cond(J) <= 500 asserted at capture).  Each model of the GPU suite is proven here first."""
import os
import subprocess
import sys

import numpy as np
import pytest

import exact_models as em
import hg_energy_models as hm
from lhvi import _abi, exact, hg_energy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'lifted-hybrid-variational-inference_amd')
RTOL = 1e-10


def host_energies(flat, x_d=None, cfg_range=None, x_c=None):
    return hg_energy.energies(flat.host_struct(), x_d=x_d, cfg_range=cfg_range, x_c=x_c, host=True)


def host_config_energies(flat):
    """(energies [M], means [M, Nc]) of every configuration at its conditional mean, through the host twins"""
    means = np.array([exact.config_host(flat, cfg)[1] for cfg in range(flat.M)]).reshape(flat.M, flat.Nc)
    return host_energies(flat, cfg_range=(0, flat.M), x_c=means), means


@pytest.mark.parametrize('name', hm.ENERGY_MODELS)
def test_host_energies_within_the_derived_bound(name):
    model, flat = hm.build(name)
    for S in hm.S_LIST:
        cfgs, x_d, x_c = hm.rows(model, flat, S, seed=S)
        got = host_energies(flat, x_d=x_d, x_c=x_c)
        assert got.shape == (S,)
        hm.assert_within_bound(got, model['factors'], x_d, x_c, '%s, S = %d' % (name, S))


def test_host_implicit_addressing_equals_explicit_digits():
    model, flat = hm.build('wide_states')
    cfgs, x_d, x_c = hm.rows(model, flat, 83, seed=7, cfg_begin=7)
    assert list(cfgs[[0, -1]]) == [7, 89] and flat.M == 90
    a = host_energies(flat, cfg_range=(7, 83), x_c=x_c)
    b = host_energies(flat, x_d=x_d, x_c=x_c)
    np.testing.assert_array_equal(a, b)
    hm.assert_within_bound(a, model['factors'], x_d, x_c, 'wide_states, configurations 7 .. 89')
    # unravel_index is what the digits mean
    np.testing.assert_array_equal(x_d, np.array(np.unravel_index(cfgs, tuple(flat.dstates))).T)


def test_energy_return_codes():
    l = _abi.lib()
    model, flat = hm.build('nc1')
    s = flat.host_struct()
    x_c, out = np.zeros((4, 1)), np.zeros(4)
    assert l.lhvi_hg_energy_host(s, 0, 0, None, None, None) == 0
    assert l.lhvi_hg_energy(s, 0, 0, None, None, None, None) == 0            # S = 0: no launch, so no GPU is needed
    assert l.lhvi_hg_energy_host(s, -1, 0, None, x_c.ctypes.data, out.ctypes.data) == -1
    assert l.lhvi_hg_energy_host(None, 4, 0, None, x_c.ctypes.data, out.ctypes.data) == -1
    assert l.lhvi_hg_energy_host(s, 4, 0, None, None, out.ctypes.data) == -1
    assert l.lhvi_hg_energy_host(s, 4, 0, None, x_c.ctypes.data, None) == -1
    assert l.lhvi_hg_energy_host(s, 4, -1, None, x_c.ctypes.data, out.ctypes.data) == -1
    wide = exact.ExactModel([2], exact.MAX_NC + 1)
    for n in ('quad_ptr', 'tab_ptr'):
        setattr(wide, n, np.zeros(1, dtype=np.int32))
    for n in ('quad_desc', 'tab_desc'):
        setattr(wide, n, np.zeros(0, dtype=np.int32))
    wide.quad_par = wide.tab_par = np.zeros(0)
    for S in (0, 4):
        assert l.lhvi_hg_energy_host(wide.host_struct(), S, 0, None, np.zeros((4, 65)).ctypes.data, out.ctypes.data) == -3
        assert l.lhvi_hg_energy(wide.host_struct(), S, 0, None, np.zeros((4, 65)).ctypes.data, out.ctypes.data, None) == -3
    with pytest.raises(ValueError):
        hg_energy.energies(s, x_c=x_c, host=True)
    with pytest.raises(ValueError):
        hg_energy.energies(s, cfg_range=(0, 2), x_c=x_c, host=True)           # x_c is [4, 1], not [2, 1]


@pytest.mark.parametrize('n', hm.ARGMAX_N)
def test_host_argmax_first_is_the_definition(n):
    for pattern, v in hm.argmax_cases(n).items():
        want_i, want_v = hm.argmax_definition(v)
        got_i, got_v = hg_energy.argmax_first(v, host=True)
        assert got_i == want_i, (n, pattern, got_i, want_i)
        if want_i < 0:
            assert got_v != got_v
        else:       # that entry: its bits, the sign of a zero included
            assert np.float64(got_v).tobytes() == np.float64(v[want_i]).tobytes() == np.float64(want_v).tobytes(), (n, pattern)
    assert hg_energy.argmax_first(np.zeros(0), host=True)[0] == -1
    assert hm.argmax_definition(hm.argmax_cases(n)['signed_zeros'])[0] == n // 2
    assert hm.argmax_definition(hm.argmax_cases(n)['all_neg_inf']) == (0, -np.inf)


@pytest.mark.parametrize('name', sorted(hm.FIXTURES))
def test_host_joint_map_matches_the_recorded_results(name):
    gold = em.load_golden(name)
    _, s = em.solver(name)
    flat = s.model
    assert gold['max_cond'] <= 500 and len(gold['cfg']) == flat.M and list(gold['cfg']) == list(range(flat.M))
    want = hm.golden_energies(gold)
    order = np.argsort(-want)
    assert order[0] == hm.FIXTURES[name] and want[order[0]] - want[order[1]] >= hm.MIN_GAP[name] - 0.01
    e, means = host_config_energies(flat)
    e = e + s.log_const
    em.assert_log_close(e, want, RTOL, 'energy of every configuration')
    index, value = hg_energy.argmax_first(e, host=True)
    assert index == hm.FIXTURES[name]
    np.testing.assert_allclose(means[index], gold['means'][index], rtol=RTOL, atol=1e-12)
    assert abs(value - want[index]) <= RTOL * max(1.0, abs(want[index]))
    assert value == e[index]


def test_peak_vs_mass_separates_the_two_argmaxes():
    model, flat = hm.build('peak_vs_mass')
    e, means = host_config_energies(flat)
    logp = np.array([exact.config_host(flat, cfg)[0] for cfg in range(2)])
    np.testing.assert_array_equal(e, [0.0, -1.0])
    np.testing.assert_array_equal(means, [[0.0], [0.0]])
    np.testing.assert_allclose(logp, [0.5 * np.log(2 * np.pi / 100), 0.5 * np.log(2 * np.pi / 0.01) - 1], rtol=1e-14)
    np.testing.assert_allclose(logp, [-1.384, 2.222], atol=5e-4)
    assert hg_energy.argmax_first(e, host=True)[0] == 0 and hg_energy.argmax_first(logp, host=True)[0] == 1


def test_peak_vs_mass2_delivers_what_the_gpu_test_relies_on():
    """fails loudly if the seed does not give: different arg-maxes, an energy gap >= 0.1, cond(J) <= 500"""
    model, flat = hm.build('peak_vs_mass2')
    assert tuple(flat.dstates) == (2, 3) and flat.Nc == 3 and flat.M == 6
    e, means = host_config_energies(flat)
    logp = np.array([exact.config_host(flat, cfg)[0] for cfg in range(6)])
    conds = [np.linalg.cond(em.numpy_config(model['factors'], [2, 3], 3, np.unravel_index(cfg, (2, 3)))[2]) for cfg in range(6)]
    print('peak_vs_mass2: energies %s, log p~ %s, max cond(J) %.3g' % (np.round(e, 4), np.round(logp, 4), max(conds)))
    top = np.sort(e)[::-1]
    assert top[0] - top[1] >= 0.1
    assert int(np.argmax(e)) != int(np.argmax(logp))
    assert int(np.argmax(e)) < 3 <= int(np.argmax(logp))             # narrow state against wide state of the first variable
    assert max(conds) <= 500
    hm.assert_within_bound(e, model['factors'], hm.digits(flat, np.arange(6)), means, 'peak_vs_mass2')


def test_ties_go_to_the_first_configuration():
    model, flat = hm.build('tie_model')
    e, _ = host_config_energies(flat)
    assert e[0].tobytes() == e[1].tobytes() and e[2].tobytes() == e[3].tobytes() and e[2] > e[0]
    index, _ = hg_energy.argmax_first(e, host=True)
    assert index == 2 and np.unravel_index(index, (2, 2))[1] == 0


def test_solver_energy_validates_and_equals_the_compat_function():
    """eval_joint_assignment_energy (compat/osi/utils.py) on ref_mln0's factors against ExactHybridGaussian.energy"""
    from lhvi.utils import eval_joint_assignment_energy
    model, _ = hm.build('ref_mln0')                 # the hand conversion: log potentials of the three classes on every factor
    s = exact.ExactHybridGaussian(factors=model['factors'], Vd=model['Vd'], Vc=model['Vc'])
    rng = np.random.RandomState(11)
    X = np.column_stack([rng.randint(0, 2, size=(40, 2)), rng.uniform(-10, 10, size=(40, 2))]).astype(np.float64)
    got = s.energy(X, host=True)
    want = np.array([float(eval_joint_assignment_energy(model['factors'], {rv: (int(x) if rv in s.Vd_idx else x)
                                                                            for rv, x in zip(model['rvs'], row)})) for row in X])
    x_d, x_c = exact.states_of(s, X)
    _, T, n_terms = hm.numpy_energy(model['factors'], x_d, x_c)
    assert (np.abs(got - want) <= hm.bound(T, n_terms)).all()
    hm.assert_within_bound(got, model['factors'], x_d, x_c, 'ref_mln0 through ExactHybridGaussian.energy')
    bad = X.copy()
    bad[3, 1] = 2.0
    with pytest.raises(ValueError, match='none of its states'):
        s.energy(bad, host=True)
    with pytest.raises(ValueError):
        s.energy(X[:, :3], host=True)
    # evidence: observed columns are ignored, log_const is included
    _, ev = em.solver('rand_8_8_ev')
    Xe = np.zeros((2, len(ev.rvs)))
    for v, rv in enumerate(ev.rvs):
        Xe[:, v] = 123.0 if rv.value is not None else (rv.domain.values[0] if rv in ev.Vd_idx else 0.25)
    xd_e, xc_e = exact.states_of(ev, Xe)
    hm.assert_within_bound(ev.energy(Xe, host=True), ev.factors, xd_e, xc_e, 'rand_8_8_ev with evidence', offset=ev.log_const)


def test_compat_module_exports_the_energy_function():
    code = ('import sys; sys.path[:] = [%r, %r] + [p for p in sys.path if "site-packages" in p or "dist-packages" in p or '
            '"python3" in p and "repo" not in p]\n'
            'import osi.utils as u, utils, lhvi.utils as l\n'
            'assert u.eval_joint_assignment_energy is l.eval_joint_assignment_energy is utils.eval_joint_assignment_energy\n'
            'print("ok")') % (os.path.join(PKG, 'compat'), PKG)
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, cwd='/')
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == 'ok'


def test_joint_map_dict_fields():
    """the result shape of joint_map() on host values (the solvers' device paths fill it the same way)"""
    model, s = hm.solver('peak_vs_mass')
    d = exact.joint_map_dict(s, (0,), 0, np.array([0.0]), 0.0)
    assert d['config'] == (0,) and d['index'] == 0 and d['xd'] == (0,) and d['inside'] is True and d['energy'] == 0.0
    assert d['assignment'] == {model['rvs'][0]: 0, model['rvs'][1]: 0.0}
    assert exact.joint_map_dict(s, (1,), 1, np.array([10.5]), -1.0)['inside'] is False


def test_no_cpu_fallback_without_gpu():
    from conftest import has_gpu
    if has_gpu():
        return
    model, s = hm.solver('peak_vs_mass')
    with pytest.raises(_abi.LhviError):
        s.energy(np.array([[0.0, 0.0]]))
    with pytest.raises(_abi.LhviError):
        exact.joint_map_from_bn(model['factors'], model['Vd'], model['Vc'])
    with pytest.raises(_abi.LhviError):
        hg_energy.argmax_first(np.zeros(3))
