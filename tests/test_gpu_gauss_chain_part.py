"""GPU suite of the partitioned block-tridiagonal solve (``segments=``; csrc/gauss_chain_part.hip): every case of
tests/test_gauss_chain_part_host.py through the device against dense NumPy at tol = 10 N cond(J) 1.1e-16, against the host twin at
1e-13 of each array's largest entry and against the serial device solve at 2 tol; bit-identical repeats, batch independence and
keep_cov independence; the indefinite batch and the run after it; ``KalmanFilter.exact(segments='auto')``; ``MemoryError`` before
a launch."""
import numpy as np
import pytest

import gauss_chain_models as cm
from test_gauss_chain_host import indefinite_batch
from test_gauss_chain_part_host import CASES, check_against_serial, host, twin_case

pytestmark = pytest.mark.gpu

TWIN = 1e-13
_serial = {}


def _solve(blocks, segments, **kw):
    from lhvi.gauss_chain import solve_block_tridiagonal
    D, O, h = blocks
    return solve_block_tridiagonal(D, O if D.shape[-3] > 1 else None, h, segments=segments, **kw)


def _same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _check_device(what, blocks, ref, sizes, S, twin, serial):
    """device with the covariances against the yardstick, the host twin and the serial device solve; a second run, and a run
    without the covariances, give the same bits"""
    out = _solve(blocks, S, keep_cov=True)
    cm.check_solution('device ' + what, ref, sizes, *out)
    gap = cm.twin_gap(out, twin[:5])
    cm.report('twin vs device ' + what, gap, TWIN)
    assert gap <= TWIN
    check_against_serial('device ' + what, ref, out, serial)
    assert _same_bits(out, _solve(blocks, S, keep_cov=True))
    assert _same_bits(out[:3], _solve(blocks, S))
    return out


@pytest.mark.parametrize('n,M,S', CASES)
def test_cases(n, M, S):
    ref = cm.shape_case(n, M)
    if (n, M) not in _serial:
        _serial[n, M] = _solve(ref['blocks'], None, keep_cov=True)
    _check_device('(%d, %d) S = %d' % (n, M, S), ref['blocks'], ref, ref['sizes'], S, twin_case(n, M, S), _serial[n, M])


def test_ragged_blocks():
    from lhvi.gauss_chain import ExactGaussianChain
    g, rvs, blocks, ref = cm.ragged_chain()
    ex = ExactGaussianChain(g, blocks)
    b = (ex.D, ex.O, ex.h)
    out = _check_device('ragged S = 2', b, ref, list(cm.RAGGED), 2, host(b, 2), _solve(b, None, keep_cov=True))
    ex.run(keep_cov=True, segments=2)
    tol = cm.tolerance(ref['N'], ref['cond'])
    e, bnd = cm.report('device ragged S = 2 logZ (rel)', abs(ex.logZ / ref['logZ'] - 1), tol)
    assert e <= bnd
    assert ex.logdet == out[2]
    pick, at = [blocks[1][0], blocks[2][4], blocks[2][0]], [3, 8, 4]
    assert np.abs(ex.cov(pick) - ref['Sig'][np.ix_(at, at)]).max() <= tol * max(1.0, np.abs(ref['Sig']).max())


def test_tree_fixture():
    """parameter set 0 of the tree fixture (n = 76, M = 19) in four segments"""
    fx, ref = cm.fixture('tree'), cm.fixture_reference('tree', 0)
    D, O, h, const = fx['filters'][0].block_tridiagonal(cm.T_FIXTURE, fx['data'])
    _check_device('tree S = 4', (D, O, h), ref, [fx['n']] * (cm.T_FIXTURE - 1), 4, host((D, O, h), 4), _solve((D, O, h), None, keep_cov=True))


def test_system_of_a_batch_has_the_bits_of_its_solo_run():
    """system 3 of the five parameter sets of the cycle fixture through ``exact_batch(..., segments=3)`` against that filter alone"""
    from lhvi import kalman
    fx = cm.fixture('cycle')
    parts = [kf.block_tridiagonal(cm.T_FIXTURE, fx['data']) for kf in fx['filters']]
    blocks = tuple(np.stack([p[i] for p in parts]) for i in range(3))
    out = _solve(blocks, 3, keep_cov=True)
    assert _same_bits([o[3] for o in out], _solve(tuple(b[3] for b in blocks), 3, keep_cov=True))
    gap = cm.twin_gap(out, host(blocks, 3)[:5])
    cm.report('twin vs device cycle batch S = 3', gap, TWIN)
    assert gap <= TWIN
    mu, var, logZ, cov, cross = kalman.exact_batch(fx['filters'], cm.T_FIXTURE, fx['data'], keep_cov=True, segments=3)
    assert _same_bits([mu[:, 1:], var[:, 1:], cov, cross], [out[0], out[1], out[3], out[4]]) and not var[:, 0].any()
    alone = fx['filters'][3].exact(cm.T_FIXTURE, fx['data'], keep_cov=True, segments=3)
    assert _same_bits([mu[3], var[3], logZ[3], cov[3], cross[3]], alone)
    for k in range(5):
        ref = cm.fixture_reference('cycle', k)
        cm.check_solution('device cycle set %d S = 3' % k, ref, [fx['n']] * (cm.T_FIXTURE - 1), *(o[k] for o in out))
        assert abs(logZ[k] / ref['logZ'] - 1) <= cm.tolerance(ref['N'], ref['cond'])


def test_indefinite_system_in_a_batch_and_the_run_after():
    D, O, h, refs, want = indefinite_batch()
    mu, var, logdet, bad = _solve((D, O, h), 2, raise_on_bad=False)
    assert tuple(bad[0]) == (-1, -1) and tuple(bad[2]) == (-1, -1)
    assert bad[1][0] == 2 and 0 <= bad[1][1] < 3                   # the separator's pivot: both interiors are positive definite
    assert np.array_equal(bad, host((D, O, h), 2, keep_cov=False)[-1])
    for b in (0, 2):
        cm.check_solution('device S = 2 beside an indefinite system, %d' % b, refs[b], refs[b]['sizes'], mu[b], var[b], logdet[b])
    assert _same_bits([mu[0], var[0], logdet[0]], _solve(refs[0]['blocks'], 2))
    with pytest.raises(ValueError, match='system 1 .*block 2, column %d' % bad[1][1]):
        _solve((D, O, h), 2)
    ref = cm.shape_case(17, 9)
    cm.check_solution('device S = 3 after the indefinite batch', ref, ref['sizes'], *_solve(ref['blocks'], 3, keep_cov=True))


def test_kalman_exact_auto_against_gabp_on_the_tree():
    """GaBP is exact on the tree model: KalmanFilter.exact(segments='auto') against GaBP(flat).run(20) on the device at 1e-11;
    the same with four segments, which 'auto' does not pick for a chain this short"""
    from lhvi.gabp import GaBP
    fx = cm.fixture('tree')
    kf = fx['filters'][0]
    flat, state_id = kf.grounded_flat(cm.T_FIXTURE, fx['data'])
    bp = GaBP(flat)
    bp.run(20)
    mv = bp._state['mv'].cpu().numpy()[state_id]                   # [T][n][2]
    for segments in ('auto', 4):
        mu, var, logZ = kf.exact(cm.T_FIXTURE, fx['data'], segments=segments)
        e = max(float(np.abs(mu[1:] - mv[1:, :, 0]).max()), float(np.abs(var[1:] - mv[1:, :, 1]).max()))
        cm.report('KalmanFilter.exact(segments=%r) vs GaBP(20), tree' % (segments,), e, 1e-11)
        assert e <= 1e-11
        assert np.array_equal(mu[0], fx['data'][:, 0]) and not var[0].any()


def test_memory_error_before_a_launch(monkeypatch):
    import torch
    from lhvi import _abi, gauss_chain
    free = int(torch.cuda.mem_get_info()[0])
    n, M = 32, free // (4 * 8 * 32 * 32)                           # W_t, C_t and the two spikes alone take the free memory
    need = gauss_chain.output_bytes(1, M, n, False, segments=8)
    assert need > free and need - gauss_chain.output_bytes(1, M, n, False) >= 8 * 2 * M * n * n

    def no_launch(*a, **k):
        raise AssertionError('a kernel entry point was reached')
    monkeypatch.setattr(_abi, 'lib', no_launch)
    monkeypatch.setattr(_abi, 'to_dev', no_launch)
    zero = np.zeros(1)                                             # arrays of that shape without their memory
    D, O, h = np.broadcast_to(zero, (M, n, n)), np.broadcast_to(zero, (M - 1, n, n)), np.broadcast_to(zero, (M, n))
    with pytest.raises(MemoryError, match='in 8 segments needs %d' % need):
        gauss_chain.solve_block_tridiagonal(D, O, h, segments=8)
    assert int(torch.cuda.mem_get_info()[0]) >= free - (64 << 20)
