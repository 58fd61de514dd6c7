"""GPU suite of the block-tridiagonal Gaussian solver (lhvi.gauss_chain, lhvi.kalman, csrc/gauss_chain.hip) against dense NumPy on
the J that tests/gauss_chain_models.py assembles, at tol = 10 N cond(J) 1.1e-16 per model; device against host twin at 1e-13 of
each array's largest entry; bit-identical repeats, batch independence and keep_cov independence."""
import numpy as np
import pytest

import gauss_chain_models as cm
from test_gauss_chain_host import indefinite_batch

pytestmark = pytest.mark.gpu

TWIN = 1e-13
_runs = {}


def _solve(blocks, **kw):
    from lhvi.gauss_chain import solve_block_tridiagonal
    D, O, h = blocks
    return solve_block_tridiagonal(D, O if D.shape[-3] > 1 else None, h, **kw)


def _host(blocks, **kw):
    from lhvi.gauss_chain import host_solve_block_tridiagonal
    D, O, h = blocks
    return host_solve_block_tridiagonal(D, O if D.shape[-3] > 1 else None, h, **kw)


def _same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _check_device(what, blocks, ref, sizes):
    """device with the covariances against the yardstick and the host twin; a second run, and a run without the covariances,
    give the same bits"""
    out = _solve(blocks, keep_cov=True)
    cm.check_solution('device ' + what, ref, sizes, *out)
    gap = cm.twin_gap(out, _host(blocks, keep_cov=True)[:5])
    cm.report('twin vs device ' + what, gap, TWIN)
    assert gap <= TWIN
    assert _same_bits(out, _solve(blocks, keep_cov=True))
    assert _same_bits(out[:3], _solve(blocks))
    return out


@pytest.mark.parametrize('n,M', cm.SHAPES)
def test_shapes(n, M):
    ref = cm.shape_case(n, M)
    _check_device('(%d, %d)' % (n, M), ref['blocks'], ref, ref['sizes'])


def test_ragged_blocks():
    from lhvi.gauss_chain import ExactGaussianChain
    g, rvs, blocks, ref = cm.ragged_chain()
    ex = ExactGaussianChain(g, blocks)
    _check_device('ragged', (ex.D, ex.O, ex.h), ref, list(cm.RAGGED))
    ex.run(keep_cov=True)
    tol = cm.tolerance(ref['N'], ref['cond'])
    e, bnd = cm.report('device ragged logZ (rel)', abs(ex.logZ / ref['logZ'] - 1), tol)
    assert e <= bnd
    pick, at = [blocks[1][0], blocks[2][4], blocks[2][0]], [3, 8, 4]
    assert np.abs(ex.cov(pick) - ref['Sig'][np.ix_(at, at)]).max() <= tol * max(1.0, np.abs(ref['Sig']).max())
    with pytest.raises(RuntimeError):
        ExactGaussianChain(g, blocks).run().cov(pick)


def _fixture_batch(which):
    if which not in _runs:
        fx = cm.fixture(which)
        parts = [kf.block_tridiagonal(cm.T_FIXTURE, fx['data']) for kf in fx['filters']]
        blocks = tuple(np.stack([p[i] for p in parts]) for i in range(3))
        _runs[which] = (blocks, _solve(blocks, keep_cov=True))
    return _runs[which]


@pytest.mark.parametrize('which', ['tree', 'cycle'])
def test_fixtures_as_one_batch(which):
    """the five parameter sets of a demo as one launch against dense NumPy and the twin; system 3 alone gives the bits it has in
    the batch; ``exact_batch`` returns the same rows"""
    from lhvi import kalman
    fx = cm.fixture(which)
    n, M = fx['n'], cm.T_FIXTURE - 1
    blocks, out = _fixture_batch(which)
    for k in range(5):
        ref = cm.fixture_reference(which, k)
        cm.check_solution('device %s set %d' % (which, k), ref, [n] * M, *(o[k] for o in out))
    gap = cm.twin_gap(out, _host(blocks, keep_cov=True)[:5])
    cm.report('twin vs device %s batch' % which, gap, TWIN)
    assert gap <= TWIN
    assert _same_bits(out, _solve(blocks, keep_cov=True))
    alone = _solve(tuple(b[3] for b in blocks), keep_cov=True)
    assert _same_bits([o[3] for o in out], alone)
    mu, var, logZ = kalman.exact_batch(fx['filters'], cm.T_FIXTURE, fx['data'])
    assert np.array_equal(mu[:, 1:], out[0]) and np.array_equal(var[:, 1:], out[1]) and not var[:, 0].any()
    for k in range(5):
        ref = cm.fixture_reference(which, k)
        assert abs(logZ[k] / ref['logZ'] - 1) <= cm.tolerance(ref['N'], ref['cond'])


def test_device_tensors_in_and_out():
    import torch
    ref = cm.shape_case(5, 7)
    D, O, h = (torch.from_numpy(b).cuda() for b in ref['blocks'])
    from lhvi.gauss_chain import solve_block_tridiagonal
    mu, var, logdet = solve_block_tridiagonal(D, O, h)
    assert mu.is_cuda and tuple(mu.shape) == (7, 5) and tuple(logdet.shape) == ()
    want = _solve(ref['blocks'])
    assert _same_bits([mu.cpu().numpy(), var.cpu().numpy(), logdet.cpu().numpy()], want)


def _chain_cases(name):
    """(object graph, its blocks, flat arrays, their blocks, yardstick) of the cycle fixture (set 0) or the (5, 7) model"""
    if name == 'cycle':
        fx = cm.fixture('cycle')
        kf, T, data, ref = fx['filters'][0], cm.T_FIXTURE, fx['data'], cm.fixture_reference('cycle', 0)
    else:
        ref = cm.shape_case(5, 7)
        kf, T, data = ref['kf'], ref['T'], ref['data']
    g, table = kf.grounded_graph(T, data)
    return g, table[1:], ref['flat'], list(ref['state_id'][1:]), ref


@pytest.mark.parametrize('name', ['cycle', 'n5m7'])
def test_chain_class_against_exact_gaussian(name):
    """ExactGaussianChain on the object graph and on the arrays of grounded_flat against the dense ExactGaussian on the device, at
    tol: means, variances, logdet, logZ, a covariance block across two neighbouring steps; belief_all -> kl_tables"""
    from lhvi import utils
    from lhvi.gauss_chain import ExactGaussianChain
    from lhvi.gauss_exact import ExactGaussian
    g, gblocks, flat, fblocks, ref = _chain_cases(name)
    tol = cm.tolerance(ref['N'], ref['cond'])
    dense = ExactGaussian(flat).run(keep_inverse=True)
    dm, dv = dense.mu_var
    hid = flat.var_hidden
    a = ExactGaussianChain(g, gblocks).run(keep_cov=True)
    b = ExactGaussianChain(flat, fblocks).run(keep_cov=True)
    for what, ex in (('object graph', a), ('flat arrays', b)):
        m, v = ex.mu_var
        assert np.array_equal(m[~hid], dm[~hid]) and not v[~hid].any()
        e, bnd = cm.report('%s %s mu' % (name, what), float(np.abs(m - dm).max()), tol * max(1.0, float(np.abs(dm).max())))
        assert e <= bnd
        e, bnd = cm.report('%s %s var (rel)' % (name, what), float(np.abs(v[hid] / dv[hid] - 1).max()), tol)
        assert e <= bnd
        for q in ('logdet', 'logZ'):
            e, bnd = cm.report('%s %s %s (rel)' % (name, what, q), abs(getattr(ex, q) / getattr(dense, q) - 1), tol)
            assert e <= bnd
    assert np.array_equal(a.mu_var[0], b.mu_var[0]) and np.array_equal(a.mu_var[1], b.mu_var[1]) and a.logZ == b.logZ
    pick = [int(v) for v in np.concatenate([fblocks[2][:3], fblocks[3][1:4]])]
    want = dense.cov(pick)
    e, bnd = cm.report('%s cov of two steps' % name, float(np.abs(b.cov(pick) - want).max()), tol * max(1.0, float(np.abs(want).max())))
    assert e <= bnd
    v0 = int(fblocks[0][0])
    assert b.get_belief_params(v0) == (b.map(v0), float(b.mu_var[1][v0])) and np.array_equal(b.map_all(), b.mu_var[0])
    assert b.belief(0.25, v0) == pytest.approx(float(np.exp(b.belief(0.25, v0, log_belief=True))), rel=1e-14)
    # the two solvers' density tables on mean +- 4 sigma: log p - log q is at most tol (8.5 + 4 max(1, max |mu|) / sigma_min) on
    # that grid (mean error over sigma times |z| <= 4, relative variance error times (1 + z^2) / 2), and so is their KL sum
    V, m = flat.V, 41
    sig = np.sqrt(np.where(hid, dv, 1.0))
    lo, hi = dm - 4 * sig, dm + 4 * sig
    x = lo[:, None] + (hi - lo)[:, None] * np.linspace(0, 1, m)[None, :]
    x[~hid] = dm[~hid, None]
    kl = utils.kl_tables(b.belief_all(x), dense.belief_all(x), lo, hi).cpu().numpy()
    bound = tol * (8.5 + 4 * max(1.0, float(np.abs(dm).max())) / float(sig.min()))
    e, bnd = cm.report('%s kl_tables(chain, dense)' % name, float(np.abs(kl[hid]).max()), bound)
    assert e <= bnd


def test_kalman_exact_against_gabp_on_the_tree():
    """GaBP is exact on the tree model: KalmanFilter.exact against GaBP(flat).run(20) on the device at 1e-11"""
    from lhvi.gabp import GaBP
    fx = cm.fixture('tree')
    kf = fx['filters'][0]
    flat, state_id = kf.grounded_flat(cm.T_FIXTURE, fx['data'])
    bp = GaBP(flat)
    bp.run(20)
    mv = bp._state['mv'].cpu().numpy()[state_id]                   # [T][n][2]
    mu, var, logZ = kf.exact(cm.T_FIXTURE, fx['data'])
    e = max(float(np.abs(mu[1:] - mv[1:, :, 0]).max()), float(np.abs(var[1:] - mv[1:, :, 1]).max()))
    cm.report('KalmanFilter.exact vs GaBP(20), tree', e, 1e-11)
    assert e <= 1e-11
    assert np.array_equal(mu[0], fx['data'][:, 0]) and not var[0].any()


def test_indefinite_system_in_a_batch_and_the_run_after():
    D, O, h, refs, want = indefinite_batch()
    mu, var, logdet, bad = _solve((D, O, h), raise_on_bad=False)
    assert tuple(bad[1]) == want and tuple(bad[0]) == (-1, -1) and tuple(bad[2]) == (-1, -1)
    for b in (0, 2):
        cm.check_solution('device beside an indefinite system, %d' % b, refs[b], refs[b]['sizes'], mu[b], var[b], logdet[b])
    assert _same_bits([mu[0], var[0], logdet[0]], _solve(refs[0]['blocks']))
    with pytest.raises(ValueError, match='system 1 .*block %d, column %d' % want):
        _solve((D, O, h))
    ref = cm.shape_case(17, 5)
    cm.check_solution('device after the indefinite batch', ref, ref['sizes'], *_solve(ref['blocks'], keep_cov=True))


def test_memory_error_before_a_launch(monkeypatch):
    import torch
    from lhvi import _abi, gauss_chain
    free = int(torch.cuda.mem_get_info()[0])
    n, M = 32, free // (8 * 32 * 32)                               # W_t and C_t of the workspace alone are twice the free memory
    need = gauss_chain.output_bytes(1, M, n, False)
    assert need > free

    def no_launch(*a, **k):
        raise AssertionError('a kernel entry point was reached')
    monkeypatch.setattr(_abi, 'lib', no_launch)
    monkeypatch.setattr(_abi, 'to_dev', no_launch)
    zero = np.zeros(1)                                             # arrays of that shape without their memory
    D, O, h = np.broadcast_to(zero, (M, n, n)), np.broadcast_to(zero, (M - 1, n, n)), np.broadcast_to(zero, (M, n))
    with pytest.raises(MemoryError, match=str(need)):
        gauss_chain.solve_block_tridiagonal(D, O, h)
    assert int(torch.cuda.mem_get_info()[0]) >= free - (64 << 20)
