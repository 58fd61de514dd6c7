"""CPU suite of the partitioned block-tridiagonal solve (``segments=``; lhvi_gauss_chain_part_host: the device's code with one lane):
the partition rule, the twin on every case of CASES, on the ragged object chain and on the tree fixture, the clamp of S, the
serial path behind S_eff = 1, an indefinite system in a batch, the workspace size and ``auto_segments``.

Yardstick: NumPy on the dense J of tests/gauss_chain_models.py through ``check_solution``.  Tolerance: tol = 10 N cond(J) 1.1e-16
per model (block elimination in another order is still a Cholesky factorisation of the same SPD matrix); partitioned against
serial: 2 tol, by the triangle inequality.

CASES (n, M, S), the smallest that reach every branch: (1, 3, 2) both interiors one block; (3, 4, 2) interiors of 2 and 1 blocks;
(3, 11, 6) every interior one block; (5, 23, 7) interiors of 3 and 2 blocks; (17, 9), (33, 7), (65, 5) the padded edges 32, 64 and
128; (4, 300, 64) many segments."""
import numpy as np
import pytest

import gauss_chain_models as cm
from test_gauss_chain_host import indefinite_batch

CASES = [(n, M, S) for n, M, Ss in ((1, 3, (2,)), (1, 9, (2, 3, 5)), (3, 4, (2,)), (3, 11, (2, 3, 4, 6)), (5, 23, (7,)), (17, 9, (3,)),
                                    (33, 7, (3,)), (65, 5, (2, 3)), (4, 300, (64,))) for S in Ss]
_twin = {}


def host(blocks, segments, keep_cov=True):
    from lhvi.gauss_chain import host_solve_block_tridiagonal
    D, O, h = blocks
    return host_solve_block_tridiagonal(D, O if D.shape[-3] > 1 else None, h, keep_cov=keep_cov, segments=segments)


def twin_case(n, M, S):
    """the twin's (mu, var, logdet, cov, cross, bad) of a case, S = None for the serial twin; computed once"""
    if (n, M, S) not in _twin:
        _twin[n, M, S] = host(cm.shape_case(n, M)['blocks'], S)
    return _twin[n, M, S]


def check_against_serial(what, ref, part, serial):
    """partitioned against serial at 2 tol, in the measures of ``check_solution``"""
    tol = 2 * cm.tolerance(ref['N'], ref['cond'])
    scale_mu, scale_sig = max(1.0, float(np.abs(ref['mu']).max())), max(1.0, float(np.abs(ref['Sig']).max()))
    for name, e, bnd in (('mu', np.abs(part[0] - serial[0]).max(), tol * scale_mu),
                         ('var (rel)', np.abs(part[1] / serial[1] - 1).max(), tol),
                         ('log det J (rel)', abs(part[2] - serial[2]) / max(abs(serial[2]), 1e-300) if serial[2] else abs(part[2]), tol),
                         ('cov', np.abs(part[3] - serial[3]).max(), tol * scale_sig),
                         ('cross', np.abs(part[4] - serial[4]).max() if serial[4].size else 0.0, tol * scale_sig)):
        e, bnd = cm.report('%s vs serial %s' % (what, name), float(e), bnd)
        assert e <= bnd


def rule(M, S):
    """the partition rule, restated: S_eff, and the first and last block of every interior"""
    S = max(1, min(S, (M + 1) // 2))
    base, extra = divmod(M - (S - 1), S)
    first, last, t = [], [], 0
    for p in range(S):
        first.append(t)
        t += base + (1 if p < extra else 0)
        last.append(t - 1)
        t += 1                                                     # the separator after interior p
    assert t == M + 1
    return S, first, last


def test_segment_bounds_against_the_rule_and_the_library():
    import ctypes
    from lhvi import _abi, gauss_chain
    l = _abi.lib()
    for M in range(1, 13):
        for S in range(1, 9):
            Se, first, last = rule(M, S)
            got = gauss_chain.segment_bounds(M, S)
            assert got[0] == Se and list(got[1]) == first and list(got[2]) == last
            assert all(b >= a for a, b in zip(first, last)) and first[0] == 0 and last[-1] == M - 1
            assert all(first[p + 1] == last[p] + 2 for p in range(Se - 1))         # one separator between neighbours
            f, z = (ctypes.c_int64 * Se)(), (ctypes.c_int64 * Se)()
            assert l.lhvi_gauss_chain_segments(M, S, ctypes.addressof(f), ctypes.addressof(z)) == Se
            assert list(f) == first and list(z) == last
            assert l.lhvi_gauss_chain_segments(M, S, None, None) == Se
    assert l.lhvi_gauss_chain_segments(5, 0, None, None) == 0 and l.lhvi_gauss_chain_segments(0, 2, None, None) == 0
    with pytest.raises(ValueError, match='at least 1'):
        gauss_chain.segment_bounds(5, 0)


@pytest.mark.parametrize('n,M,S', CASES)
def test_host_twin_on_cases(n, M, S):
    from lhvi import _abi, gauss_chain
    ref = cm.shape_case(n, M)
    out = twin_case(n, M, S)
    assert tuple(out[5]) == (-1, -1)
    what = 'host (%d, %d) S = %d' % (n, M, S)
    cm.check_solution(what, ref, ref['sizes'], *out[:5])
    check_against_serial(what, ref, out, twin_case(n, M, None))
    assert all(np.array_equal(a, b) for a, b in zip(out[:3], host(ref['blocks'], S, keep_cov=False)[:3]))
    e, bnd = cm.report(what + ' logZ (rel)', abs(ref['kf'].exact(ref['T'], ref['data'], host=True, segments=S)[2] / ref['logZ'] - 1),
                       cm.tolerance(ref['N'], ref['cond']))
    assert e <= bnd
    for B in (1, 3):
        assert gauss_chain.ws_doubles(B, M, n, S) == _abi.lib().lhvi_gauss_chain_part_ws_doubles(B, M, n, S)
        assert gauss_chain.output_bytes(B, M, n, True, S) - gauss_chain.output_bytes(B, M, n, True) == \
            8 * (gauss_chain.ws_doubles(B, M, n, S) - gauss_chain.ws_doubles(B, M, n))
    assert gauss_chain.ws_doubles(1, M, n, S) >= gauss_chain.ws_doubles(1, M, n) + 2 * M * gauss_chain.padded_edge(n) ** 2    # the spikes


def test_host_twin_on_ragged_blocks():
    """the object chain of blocks 3, 1, 5, 2 in two segments: the identity padding enters neither logdet nor N"""
    from lhvi.gauss_chain import ExactGaussianChain
    g, rvs, blocks, ref = cm.ragged_chain()
    ex = ExactGaussianChain(g, blocks)
    out = host((ex.D, ex.O, ex.h), 2)
    assert tuple(out[5]) == (-1, -1)
    cm.check_solution('host ragged S = 2', ref, list(cm.RAGGED), *out[:5])
    check_against_serial('host ragged S = 2', ref, out, host((ex.D, ex.O, ex.h), None))
    ex.run(keep_cov=True, host=True, segments=2)
    tol = cm.tolerance(ref['N'], ref['cond'])
    e, bnd = cm.report('host ragged S = 2 logZ (rel)', abs(ex.logZ / ref['logZ'] - 1), tol)
    assert e <= bnd
    assert ex.logdet == out[2]
    mean, var = ex.mu_var
    assert mean[11] == 0.8 and var[11] == 0.0
    assert np.abs(mean[:11] - ref['mu']).max() <= tol * max(1.0, np.abs(ref['mu']).max())
    pick, at = [blocks[1][0], blocks[2][4], blocks[2][0]], [3, 8, 4]
    assert np.abs(ex.cov(pick) - ref['Sig'][np.ix_(at, at)]).max() <= tol * max(1.0, np.abs(ref['Sig']).max())


def test_host_twin_on_the_tree_fixture():
    """parameter set 0 of the tree fixture (n = 76, M = 19) in four segments"""
    fx, ref = cm.fixture('tree'), cm.fixture_reference('tree', 0)
    kf, n, M = fx['filters'][0], fx['n'], cm.T_FIXTURE - 1
    D, O, h, const = kf.block_tridiagonal(cm.T_FIXTURE, fx['data'])
    out = host((D, O, h), 4)
    assert tuple(out[5]) == (-1, -1)
    cm.check_solution('host tree S = 4', ref, [n] * M, *out[:5])
    check_against_serial('host tree S = 4', ref, out, host((D, O, h), None))
    mu, var, logZ = kf.exact(cm.T_FIXTURE, fx['data'], host=True, segments=4)
    assert np.array_equal(mu[1:], out[0]) and np.array_equal(var[1:], out[1])
    e, bnd = cm.report('host tree S = 4 logZ (rel)', abs(logZ / ref['logZ'] - 1), cm.tolerance(ref['N'], ref['cond']))
    assert e <= bnd


def test_segment_count_clamps():
    """S beyond (M + 1) // 2 is that count: (3, 11) has at most 6 segments"""
    want = twin_case(3, 11, 6)
    for S in (7, 100):
        assert all(np.array_equal(a, b) for a, b in zip(host(cm.shape_case(3, 11)['blocks'], S), want))


@pytest.mark.parametrize('n,M,S', [(3, 4, 1), (5, 7, 1), (1, 1, 3), (1, 2, 3), (1, 2, 'auto'), (3, 4, 'auto')])
def test_one_segment_is_the_serial_path(n, M, S):
    """S = 1, M < 3 and an 'auto' that picks 1 give the bits of segments=None, and take its workspace"""
    from lhvi import gauss_chain
    blocks = cm.shape_case(n, M)['blocks']
    assert all(np.array_equal(a, b) for a, b in zip(host(blocks, S), host(blocks, None)))
    assert gauss_chain.ws_doubles(2, M, n, S) == gauss_chain.ws_doubles(2, M, n)


def test_indefinite_system_in_a_batch():
    """three (3, 4) systems in two segments, the middle one indefinite: it is flagged at a block of the chain (its bad entry is in
    the separator, block 2); the outer two have the bits of their solo solves"""
    from lhvi import _abi
    D, O, h, refs, want = indefinite_batch()
    mu, var, logdet, bad = host((D, O, h), 2, keep_cov=False)
    assert tuple(bad[0]) == (-1, -1) and tuple(bad[2]) == (-1, -1)
    # both interiors (blocks 0-1 and block 3) are principal submatrices of a positive definite matrix: the bad pivot is the reduced chain's
    assert bad[1][0] == 2 and 0 <= bad[1][1] < 3
    for b in (0, 2):
        solo = host(tuple(x[b] for x in (D, O, h)), 2, keep_cov=False)
        assert np.array_equal(mu[b], solo[0]) and np.array_equal(var[b], solo[1]) and logdet[b] == solo[2]
        cm.check_solution('host S = 2 beside an indefinite system, %d' % b, refs[b], refs[b]['sizes'], mu[b], var[b], logdet[b])
    # a bad pivot inside an interior is reported at its chain block: block 3 is interior 1's only block
    D2 = D.copy()
    D2[1, 2, 1, 1] = D[0, 2, 1, 1]
    D2[1, 3, 0, 0] = -5.0
    bad = host((D2, O, h), 2, keep_cov=False)[-1]
    assert tuple(bad[1]) == (3, 0) and tuple(bad[0]) == (-1, -1) and tuple(bad[2]) == (-1, -1)
    p = lambda a: a.ctypes.data
    l, z = _abi.lib(), np.zeros(4)
    assert l.lhvi_gauss_chain_part_host(1, 4, 3, 0, p(D), p(O), p(h), p(z), p(z), p(z), None, None, p(z), p(z)) == -1
    assert l.lhvi_gauss_chain_part_host(1, 4, 129, 2, None, None, None, None, None, None, None, None, None, None) == -3
    assert l.lhvi_gauss_chain_part_ws_doubles(1, 4, 3, 0) == 0
    with pytest.raises(ValueError, match='at least 1'):
        host((D, O, h), 0)
    with pytest.raises(ValueError, match="'auto'"):
        host((D, O, h), 'many')


def test_auto_segments_properties():
    from lhvi.gauss_chain import auto_segments
    for n in (1, 8, 30, 76, 128):
        assert auto_segments(256, 20000, n) == 1 and auto_segments(5000, 199, n) == 1          # the batch fills the device
        assert auto_segments(64, 199, n) == 1                                                  # the benchmark's batch of short chains
        assert all(auto_segments(1, M, n) == 1 for M in (0, 1, 2))
        for B in (1, 2, 7):
            picks = [auto_segments(B, M, n) for M in range(1, 600)] + [auto_segments(B, M, n) for M in (1000, 5000, 19999, 10 ** 6)]
            Ms = list(range(1, 600)) + [1000, 5000, 19999, 10 ** 6]
            assert all(1 <= s <= max(1, (M + 1) // 2) for s, M in zip(picks, Ms))
            assert all(a <= b for a, b in zip(picks, picks[1:]))                               # monotone in M
            assert all(B * s <= 256 for s in picks)
    assert auto_segments(1, 19999, 30) > 1
    assert auto_segments(1, 19999, 30) == auto_segments(1, 19999, 30)
