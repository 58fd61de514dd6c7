"""Exact marginals of Gaussian chains on the device: a batched block-tridiagonal fp64 Cholesky with the covariance recursion
(``csrc/gauss_chain.hip``), the ground truth of the relational Kalman filters (``Demo/RKF``) at sizes the dense ``ExactGaussian``
cannot hold: O(M n^3) work and O(M n^2) memory for M blocks of edge n instead of O((M n)^3) and O((M n)^2).

``solve_block_tridiagonal(D, O, h)`` takes the blocks of ``J`` and ``h`` of one system or a batch; ``ExactGaussianChain(g, blocks)``
is the solver-shaped class on a graph whose hidden variables are given in ordered blocks (``ExactGaussian``'s surface);
``lhvi.kalman.KalmanFilter.exact`` builds the blocks of a conditioned filter in closed form.  There is no CPU path: without a GPU
the calls raise ``LhviError`` (``host_solve_block_tridiagonal`` runs the same code on the CPU for the tests).  A system takes one
workgroup; ``segments=`` on these calls cuts a long chain into segments solved in parallel (``csrc/gauss_chain_part.hip``,
``segment_bounds``, ``auto_segments``).

docs/kernels_gauss_chain.md: a system that is not positive definite raises ``ValueError`` naming the system, block and column;
sizes beyond the free device memory raise ``MemoryError`` before a launch; blocks wider than 128 raise ``ValueError``.
"""
from __future__ import annotations

import numpy as np

from . import _abi
from .flat import flatten
from .gauss_exact import LOG_2PI, ExactGaussian, conditioned_quadratics

MAX_BLOCK = _abi.GAUSS_CHAIN_MAX_BLOCK


def padded_edge(n):
    """the block edge the kernel is instantiated for (csrc/gauss_chain.hpp)"""
    return 8 if n <= 8 else 16 if n <= 16 else 32 if n <= 32 else 64 if n <= 64 else 128


def ws_doubles(B, M, n, segments=None):
    """``lhvi_gauss_chain_ws_doubles`` and, with ``segments``, ``lhvi_gauss_chain_part_ws_doubles`` restated (checked against the
    library by the tests)"""
    P = padded_edge(n)
    ld, nbuf = (P + 1 if P <= 64 else P), (0 if P < 64 else 5 if P == 64 else 6)
    serial = lambda m: m * P * P + max(m - 1, 0) * P * P + m * P + nbuf * P * ld
    S = 1 if segments is None or M < 1 else segment_bounds(M, _segments(segments, B, M, n))[0]
    if S == 1:
        return B * serial(M)
    R, R1 = S - 1, max(S - 2, 0)
    per_system = 4 * M * P * P + M * P + S * (nbuf * P * ld + 3 * n * n + 2 * n + 2)      # W, C, VL, VR, y; tiles and record per interior
    reduced = 2 * (R + R1) * n * n + 3 * R * n + 2 + serial(R)                              # D~, O~, cov, cross; h~, mu, var; logdet, bad
    return B * (per_system + reduced)


def output_bytes(B, M, n, keep_cov=False, segments=None):
    """device bytes of a run: the inputs, the workspace (W_t, C_t, y_t of every block; with ``segments`` the spikes and the reduced
    chain too) and the results"""
    mo = max(M - 1, 0)
    doubles = B * (M * n * n + mo * n * n + M * n) + ws_doubles(B, M, n, segments) + B * (2 * M * n + 1)
    if keep_cov:
        doubles += B * (M + mo) * n * n
    return 8 * doubles + 8 * B


def segment_bounds(M, S):
    """The partition of ``M`` blocks into ``S`` segments (``lhvi_gauss_chain_segments`` restated, checked against the library by the
    tests): ``(S_eff, first [S_eff], last [S_eff])`` with ``S_eff = max(1, min(S, (M + 1) // 2))``.  ``S_eff - 1`` single-block
    separators lie between ``S_eff`` interiors; the interiors share the other ``M - (S_eff - 1)`` blocks, the first
    ``(M - S_eff + 1) % S_eff`` of them one block longer; interior p covers ``first[p] .. last[p]``, separator p is block
    ``last[p] + 1``."""
    M, S = int(M), int(S)
    if S < 1:
        raise ValueError('segments = %d: at least 1' % S)
    S = max(1, min(S, (M + 1) // 2))
    base, extra = divmod(M - (S - 1), S)
    size = np.full(S, base, dtype=np.int64)
    size[:extra] += 1
    first = np.cumsum(size + 1) - (size + 1)
    return S, first, first + size - 1


# r: the cost of a block in stages 1 and 3 of the partitioned solve over a block of the serial solve.  Measured on the MI355X by
# scripts/bench_gauss_chain.py --segments sweep (profiles/gauss_chain_part_bench.json): 2.16 on the long chain (n = 30, M = 19 999) at
# S = 64, 128 and 256 and 2.10 on the batch of 64 at S = 4, each with at most one workgroup on a compute unit; 2.69 (S = 512) and
# 2.87 (batch, S = 12) where two or three share one; 1.44 at the tree fixture's shape (n = 76, S = 4).  The operation count (a
# serial block ~4 P^3 multiply-adds, the spikes 6 P^3, the correction 4 P^3) had suggested 4.
SEGMENT_COST_RATIO = 2.2
COMPUTE_UNITS = 256         # MI355X
# workgroups of the segment kernel that r prices as running alone: one per compute unit, as the serial kernel's workgroup does
# (the LDS would hold three at P = 32; the measured r grows by a quarter as soon as two share a compute unit)
RESIDENT_PER_CU = 1
# the spikes double the workspace, so 'auto' partitions only for a predicted gain of at least this factor
AUTO_MIN_GAIN = 2.0


def auto_segments(B, M, n):
    """The segment count ``segments='auto'`` takes; a pure function of its arguments.  The time of a partitioned solve in serial
    blocks is ``r ceil(M / S) + S``: stages 1 and 3 on the longest interior, then the reduced chain (``r = SEGMENT_COST_RATIO``).
    Its relaxation ``r M / S + S`` is least at ``S = sqrt(r M)``; that value, rounded, is taken (it grows with M, which the
    minimiser of the stepped cost does not), capped by ``(M + 1) // 2`` and so that ``B S`` stays within the resident workgroups
    (``COMPUTE_UNITS * RESIDENT_PER_CU``).  1, the serial path, when ``M < 3``, when the batch alone fills the device, or when
    the relaxed cost at that S is not ``AUTO_MIN_GAIN`` times below the serial M."""
    B, M, n = int(B), int(M), int(n)
    resident = COMPUTE_UNITS * RESIDENT_PER_CU
    if B >= resident or M < 3:
        return 1
    S = min(int(round((SEGMENT_COST_RATIO * M) ** 0.5)), (M + 1) // 2, resident // max(B, 1))
    if S < 2 or AUTO_MIN_GAIN * (SEGMENT_COST_RATIO * M / S + S) > M:
        return 1
    return S


def _segments(segments, B, M, n):
    """the S of a ``segments=`` argument (an integer or 'auto')"""
    if isinstance(segments, str):
        if segments != 'auto':
            raise ValueError("segments must be None, an integer >= 1 or 'auto', got %r" % (segments,))
        return auto_segments(B, M, n)
    if int(segments) < 1:
        raise ValueError('segments = %d: at least 1' % int(segments))
    return int(segments)


def _shapes(D, O, h):
    """(B, M, n, single) of the arguments; raises ``ValueError`` on inconsistent shapes or n > MAX_BLOCK"""
    single = len(D.shape) == 3
    if len(D.shape) not in (3, 4) or D.shape[-1] != D.shape[-2]:
        raise ValueError('D must be [B][M][n][n] or [M][n][n], got %s' % (tuple(D.shape),))
    B, M, n = (1 if single else int(D.shape[0])), int(D.shape[-3]), int(D.shape[-1])
    if n > MAX_BLOCK:
        raise ValueError('blocks of edge n = %d: the block-tridiagonal solver takes n <= %d' % (n, MAX_BLOCK))
    lead = () if single else (B,)
    if tuple(h.shape) != lead + (M, n):
        raise ValueError('h must be %s, got %s' % (lead + (M, n), tuple(h.shape)))
    if M > 1 or O is not None:
        if O is None or tuple(O.shape) != lead + (max(M - 1, 0), n, n):
            raise ValueError('O must be %s, got %s' % (lead + (max(M - 1, 0), n, n), None if O is None else tuple(O.shape)))
    return B, M, n, single


def _bad_error(bad, what='system'):
    b = int(np.flatnonzero(bad[:, 0] >= 0)[0])
    return ValueError('%s %d is not positive definite: the pivot of block %d, column %d is not positive'
                      % (what, b, int(bad[b, 0]), int(bad[b, 1])))


def _pack(single, keep_cov, raise_on_bad, mu, var, logdet, cov, cross, bad):
    if single:
        mu, var, logdet = mu[0], var[0], logdet[0]
        cov, cross = (cov[0], cross[0]) if keep_cov else (None, None)
    out = (mu, var, logdet) + ((cov, cross) if keep_cov else ())
    return out if raise_on_bad else out + (bad[0] if single else bad,)


def solve_block_tridiagonal(D, O, h, keep_cov=False, raise_on_bad=True, segments=None):
    """Exact moments of ``B`` Gaussian systems ``J x = h`` with block-tridiagonal ``J``: ``D [B][M][n][n]`` the diagonal blocks,
    ``O [B][M-1][n][n] = J[block t, block t + 1]`` (None when M = 1), ``h [B][M][n]``; arrays or device tensors, with or without
    the leading batch axis.  Returns ``mu [B][M][n]``, ``var [B][M][n]``, ``logdet [B]`` and, with ``keep_cov``, ``cov [B][M][n][n]``
    (Sig[t, t]) and ``cross [B][M-1][n][n]`` (Sig[t, t + 1]), of the kind that came in.  A system that is not positive definite
    raises ``ValueError``; with ``raise_on_bad=False`` a last value ``bad [B][2]`` (NumPy: block and column of the first bad pivot,
    -1 where there is none) is returned instead and that system's results are meaningless.

    ``segments``: None solves every system block after block in one workgroup.  An integer S, or 'auto' (``auto_segments``), cuts
    each system into ``segment_bounds(M, S)`` segments solved in parallel and joined through a reduced chain of the separators
    (docs/kernels_gauss_chain.md): for the single long chain that cannot fill the device otherwise.  With (M, n, S) fixed the
    bits do not depend on B, on a system's position or on ``keep_cov``; they differ from the serial solve's and between different
    S within the tolerance.  A system is flagged in ``bad`` exactly when the serial solve flags it, but the (block, column) is
    that of the bad pivot with the lowest block among those the partitioned elimination meets, which may be another one."""
    torch = _abi._torch()
    tensors = torch.is_tensor(D)
    if not tensors:
        D, h = np.asarray(D, dtype=np.float64), np.asarray(h, dtype=np.float64)
        O = None if O is None else np.asarray(O, dtype=np.float64)
    B, M, n, single = _shapes(D, O, h)
    mo = max(M - 1, 0)
    if B == 0 or M == 0 or n == 0:
        z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=D.device) if tensors else np.zeros(s)
        return _pack(single and B > 0, keep_cov, raise_on_bad, z(B, M, n), z(B, M, n), z(B), z(B, M, n, n), z(B, mo, n, n),
                     np.full((B, 2), -1, dtype=np.int32))
    torch = _abi.require_gpu()
    S = None if segments is None else _segments(segments, B, M, n)
    need, free = output_bytes(B, M, n, keep_cov, S), int(torch.cuda.mem_get_info()[0])
    if need > free:
        raise MemoryError('the block-tridiagonal solve of %d systems of %d blocks of edge %d%s%s needs %d bytes of device memory, '
                          '%d are free' % (B, M, n, ' with the covariances' if keep_cov else '',
                                           '' if S is None else ' in %d segments' % S, need, free))
    f64 = torch.float64

    def dev(a):
        if a is None:
            return None
        return a.to(device='cuda', dtype=f64).contiguous() if tensors else _abi.to_dev(np.ascontiguousarray(a))
    Dd, Od, hd = dev(D), dev(O), dev(h)
    l, new = _abi.lib(), lambda *s: torch.empty(*s, dtype=f64, device='cuda')
    ws = new(int(l.lhvi_gauss_chain_ws_doubles(B, M, n) if S is None else l.lhvi_gauss_chain_part_ws_doubles(B, M, n, S)))
    mu, var, logdet = new(B, M, n), new(B, M, n), new(B)
    cov, cross = (new(B, M, n, n), new(B, mo, n, n)) if keep_cov else (None, None)
    bad = torch.empty(B, 2, dtype=torch.int32, device='cuda')
    args = (_abi.ptr(Dd), _abi.ptr(Od) if mo else None, _abi.ptr(hd), _abi.ptr(ws), _abi.ptr(mu), _abi.ptr(var), _abi.ptr(cov),
            _abi.ptr(cross) if mo else None, _abi.ptr(logdet), _abi.ptr(bad), _abi.stream_ptr())
    _abi.check(l.lhvi_gauss_chain_solve(B, M, n, *args) if S is None else l.lhvi_gauss_chain_part_solve(B, M, n, S, *args))
    bad = bad.cpu().numpy()
    if raise_on_bad and (bad[:, 0] >= 0).any():
        raise _bad_error(bad)
    if not tensors:
        mu, var, logdet = mu.cpu().numpy(), var.cpu().numpy(), logdet.cpu().numpy()
        cov, cross = (cov.cpu().numpy(), cross.cpu().numpy()) if keep_cov else (None, None)
    return _pack(single, keep_cov, raise_on_bad, mu, var, logdet, cov, cross, bad)


def host_solve_block_tridiagonal(D, O, h, keep_cov=False, segments=None):
    """the same on the CPU through the device's code (``lhvi_gauss_chain_host``, with ``segments`` ``lhvi_gauss_chain_part_host``),
    NumPy in and out; always returns ``bad`` last"""
    D, h = np.ascontiguousarray(D, dtype=np.float64), np.ascontiguousarray(h, dtype=np.float64)
    O = None if O is None else np.ascontiguousarray(O, dtype=np.float64)
    B, M, n, single = _shapes(D, O, h)
    mo = max(M - 1, 0)
    mu, var, logdet = np.zeros((B, M, n)), np.zeros((B, M, n)), np.zeros(B)
    cov, cross = (np.zeros((B, M, n, n)), np.zeros((B, mo, n, n))) if keep_cov else (None, None)
    bad = np.full((B, 2), -1, dtype=np.int32)
    if B and M and n:
        l = _abi.lib()
        S = None if segments is None else _segments(segments, B, M, n)
        ws = np.zeros(int(l.lhvi_gauss_chain_ws_doubles(B, M, n) if S is None else l.lhvi_gauss_chain_part_ws_doubles(B, M, n, S)))
        p = lambda a: None if a is None or a.size == 0 else a.ctypes.data
        args = (p(D), p(O), p(h), p(ws), p(mu), p(var), p(cov), p(cross), p(logdet), p(bad))
        rc = l.lhvi_gauss_chain_host(B, M, n, *args) if S is None else l.lhvi_gauss_chain_part_host(B, M, n, S, *args)
        if rc not in (0, _abi.E_NOT_PD):
            _abi.check(rc)
    return _pack(single and B > 0, keep_cov, False, mu, var, logdet, cov, cross, bad)


def scatter_blocks(params, scopes, N, blocks, names=None):
    """``D [M][n][n]``, ``O [M-1][n][n]``, ``h [M][n]`` of the conditioned factors ``(A, b, c)`` on ``scopes`` (positions among the N
    hidden variables) for ``blocks``: a list of position arrays; n = the widest block, the others padded with the identity on D
    and zeros on O and h.  ``J = -(A + A^T)`` summed over the factors in factor order.  Raises ``ValueError`` naming the factor
    (``names[f]``, or its index among the conditioned factors) when one links blocks more than one apart."""
    M = len(blocks)
    n = max([len(b) for b in blocks] + [1])
    blk, loc = np.full(N, -1, dtype=np.int64), np.zeros(N, dtype=np.int64)
    for t, b in enumerate(blocks):
        blk[b], loc[b] = t, np.arange(len(b))
    D, O, h = np.zeros((M, n, n)), np.zeros((max(M - 1, 0), n, n)), np.zeros((M, n))
    for t, b in enumerate(blocks):
        pad = np.arange(len(b), n)
        D[t, pad, pad] = 1.0
    for f, ((A, b, c), scope) in enumerate(zip(params, scopes)):
        s = np.asarray(scope, dtype=np.int64)
        bt, lc = blk[s], loc[s]
        if bt.max() - bt.min() > 1:
            raise ValueError('factor %d links blocks %d and %d: a block-tridiagonal model has no factor across blocks more than '
                             'one apart' % (names[f] if names is not None else f, int(bt.min()), int(bt.max())))
        A = np.asarray(A, dtype=np.float64).reshape(s.size, s.size)
        Jf = -(A + A.T)
        np.add.at(h, (bt, lc), np.asarray(b, dtype=np.float64).reshape(-1))
        I, K = np.meshgrid(np.arange(s.size), np.arange(s.size), indexing='ij')
        I, K = I.ravel(), K.ravel()
        same = bt[I] == bt[K]
        np.add.at(D, (bt[I[same]], lc[I[same]], lc[K[same]]), Jf[I[same], K[same]])
        up = bt[K] == bt[I] + 1
        np.add.at(O, (bt[I[up]], lc[I[up]], lc[K[up]]), Jf[I[up], K[up]])
    return D, O, h


class ExactGaussianChain(ExactGaussian):
    """Exact marginals of a Gaussian MRF whose hidden variables come in ordered blocks with factors inside a block or between
    neighbouring blocks only (a chain in time: the relational Kalman filters).  ``ExactGaussianChain(g, blocks)``: ``g`` an object
    ``Graph`` or flat arrays, as ``ExactGaussian`` takes them; ``blocks`` an ordered list of arrays of hidden variables (objects
    or variable indices), possibly of different lengths.  After ``run()``: ``ExactGaussian``'s surface; ``cov(rvs)`` takes
    variables of one block or of two neighbouring blocks and needs ``run(keep_cov=True)``."""

    def __init__(self, g, blocks):
        self.g = g
        self.flat = flat = flatten(g)
        self.factor_params, self.factor_scopes, self.log_const, self.hidden = conditioned_quadratics(flat)
        self.N = N = int(self.hidden.size)
        self.c = sum((c for _, _, c in self.factor_params), 0)
        pos = np.full(flat.V, -1, dtype=np.int64)
        pos[self.hidden] = np.arange(N)
        seen = np.full(flat.V, -1, dtype=np.int64)
        self.blocks = []
        for t, blk in enumerate(blocks):
            idx = np.array([self._index(rv) for rv in blk], dtype=np.int64)
            for v in idx:
                if pos[v] < 0:
                    raise ValueError('variable %d in block %d is observed: blocks hold hidden variables' % (int(v), t))
                if seen[v] >= 0:
                    raise ValueError('variable %d is in two blocks (%d and %d)' % (int(v), int(seen[v]), t))
                seen[v] = t
            self.blocks.append(pos[idx])
        missing = self.hidden[seen[self.hidden] < 0]
        if missing.size:
            raise ValueError('variable %d is hidden and in no block' % int(missing[0]))
        self.n = max([b.size for b in self.blocks] + [1])
        if self.n > MAX_BLOCK:
            raise ValueError('a block of %d variables: the block-tridiagonal solver takes n <= %d' % (self.n, MAX_BLOCK))
        # the conditioned factors are the graph's factors with a hidden argument, in factor order
        names = [f for f in range(flat.F) if np.isnan(flat.var_value[flat.edge_var[flat.fac_ptr[f]:flat.fac_ptr[f + 1]]]).any()]
        self.D, self.O, self.h = scatter_blocks(self.factor_params, self.factor_scopes, N, self.blocks, names)
        self._block_of = np.zeros(N, dtype=np.int64)
        self._local = np.zeros(N, dtype=np.int64)
        for t, b in enumerate(self.blocks):
            self._block_of[b], self._local[b] = t, np.arange(b.size)
        self._run = None
        self._mean = self._var = self._cov = self._cross = None

    def joint_quadratic(self):
        from .utils import get_joint_quadratic_params
        return get_joint_quadratic_params(self.factor_params, self.factor_scopes, self.N)

    def run(self, keep_cov=False, host=False, segments=None):
        """``host=True`` runs the CPU twin instead of the device (the CPU suite's route); ``segments``: as
        ``solve_block_tridiagonal`` takes it"""
        if not host:
            _abi.require_gpu()
        mean, var = np.array(self.flat.var_value, dtype=np.float64), np.zeros(self.flat.V)
        self._cov = self._cross = None
        if self.N == 0:
            logdet, mub = 0.0, 0.0
        else:
            O = self.O if len(self.blocks) > 1 else None
            out = host_solve_block_tridiagonal(self.D, O, self.h, keep_cov=keep_cov, segments=segments) if host else \
                solve_block_tridiagonal(self.D, O, self.h, keep_cov=keep_cov, raise_on_bad=False, segments=segments)
            bad, out = out[-1], out[:-1]
            if bad[0] >= 0:
                col = int(bad[1])
                blk = self.blocks[int(bad[0])]
                v = int(self.hidden[blk[col]]) if col < blk.size else -1
                name = ' (%s)' % self.flat.rvs[v] if self.flat.rvs and v >= 0 else ''
                raise ValueError('the precision matrix J = -2A is not positive definite: the pivot of block %d, column %d, '
                                 'variable %d%s is not positive' % (int(bad[0]), col, v, name))
            mu_b, var_b, logdet = out[0], out[1], float(out[2])
            if keep_cov:
                self._cov, self._cross = out[3], out[4]
            h_h = np.zeros(self.N)
            for t, b in enumerate(self.blocks):
                mean[self.hidden[b]], var[self.hidden[b]] = mu_b[t, :b.size], var_b[t, :b.size]
                h_h[b] = self.h[t, :b.size]
            mub = float(np.dot(mean[self.hidden], h_h))
        self._mean, self._var = mean, var
        self.logdet = logdet
        self.logZ = self.N / 2 * LOG_2PI - 0.5 * logdet + 0.5 * mub + float(self.c) + self.log_const
        return self

    def cov(self, rvs):
        """the |S| x |S| block of the covariance matrix of the hidden variables ``rvs`` of one block or of two neighbouring blocks
        (NumPy); needs run(keep_cov=True)"""
        self._need_run()
        idx = [self._index(rv) for rv in rvs]
        pos = np.full(self.flat.V, -1, dtype=np.int64)
        pos[self.hidden] = np.arange(self.N)
        cols = pos[np.asarray(idx, dtype=np.int64)] if idx else np.zeros(0, dtype=np.int64)
        if (cols < 0).any():
            raise ValueError('cov: variable %d is observed' % idx[int(np.flatnonzero(cols < 0)[0])])
        if self._cov is None:
            raise RuntimeError('cov needs run(keep_cov=True)')
        bt, lc = self._block_of[cols], self._local[cols]
        if cols.size and bt.max() - bt.min() > 1:
            raise ValueError('cov: variables of blocks %d and %d: only one block or two neighbouring blocks are kept'
                             % (int(bt.min()), int(bt.max())))
        out = np.zeros((cols.size, cols.size))
        for a in range(cols.size):
            for b in range(cols.size):
                if bt[a] == bt[b]:
                    out[a, b] = self._cov[bt[a], lc[a], lc[b]]
                elif bt[b] == bt[a] + 1:
                    out[a, b] = self._cross[bt[a], lc[a], lc[b]]
                else:
                    out[a, b] = self._cross[bt[b], lc[b], lc[a]]
        return out
