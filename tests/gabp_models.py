"""Models, input messages and the host twin for the tests of the Gaussian sweep kernels (csrc/gabp.hip).

The twin is a NumPy ``longdouble`` restatement of GaBP.message_rv_to_f / message_f_to_rv / get_belief_params and of their lifted
counterparts (GaBP.py:20-35, 37-138, 187-200; GaLBP.py:21-39, 201-217) on ``FlatGraph`` arrays, written from SURVEY.md A.1 / A.2
and oracle/c/gabp_oracle.c -- not from the kernels.  It keeps the conventions: a NaN variance is the reference's ``None`` (a linear
term only, subtracted), an observed variable sends (NaN, NaN), the own factor is skipped on a ground graph and taken count - 1
times on a lifted one, an alias edge belongs to its canonical edge.

Every row sum of the twin is a direct sum (no total-minus-own), and next to each output message the twin returns the condition
sums ``bound`` needs.  The bound is derived, not measured (u = 2^-53, gamma_k = k u / (1 - k u), a row of n entries):

    |P^ - P| <= gamma_{n+4} sum |p_i c_i| + dP      over ALL entries of the row, the own one included: the hub and the chunk paths
                                                    add it and take it out again; + 4: the reciprocal, the count product, the
                                                    subtraction and the final reciprocal
    |H^ - H| <= gamma_{n+5} sum |h_i c_i| + dH
    rel(var) <= (gamma_{n+4} sum |p c| + dP) / |P| + u
    |mu^ - mu| <= |var| (gamma_{n+5} sum |h c| + dH) + |mu| (rel(var) + 2 u)

whatever the order of summation.  dP, dH are zero when the kernel's inputs are the twin's inputs bit for bit (v -> f, marginals); in
the pull form the entries are closed forms of the partners' messages which the device rounds and the twin does not, and dP, dH
carry the first-order effect of those roundings on the row sums (``closed_forms_of``: every operation of a closed form counted
with u, cancellations with the magnitude of the operands).
"""
import copy

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
HUB = 512                 # rows beyond: wave-parallel total-minus-own kernels
ROW_DIRECT = 32           # record pull kernel: rows up to this length are summed entry by entry
CHUNK = 8                 # ... longer ones through sums of eight-entry chunks
COND_CAP = 1e6

POT_GAUSSIAN, POT_LINEAR_GAUSSIAN, POT_X2, POT_XY = 2, 5, 6, 7

ROW_LENGTHS = [2, 3, 4, 5, 6, 8, 9,                        # GABP_BATCH and the four-at-a-time tails
               31, 32, 33, 34,                              # GABP_ROW_DIRECT
               39, 40, 41, 47, 48, 55, 56,                  # last-chunk remainders 0-15, 4-7 chunks (four-unrolled chunk-total loop)
               63, 64, 65, 66, 127, 128, 480, 511, 512,
               513, 514, 575, 576, 577, 700]                # hub rows: lanes with uneven stride counts
CLASSES = ('proper', 'none', 'inf', 'negative', 'zero_mean')


def gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1.0 - k * U)


class Msg:
    """messages (mu, var) in longdouble with the sums ``bound`` reads: n entries in the row, sp = sum |p c|, sh = sum |h c| over the
    whole row, the leave-one-out (or total) P and H, and dP, dH = first-order error of the row sums that the inputs bring along"""

    def __init__(self, size):
        self.mu = np.full(size, np.nan, dtype=LD)
        self.var = np.full(size, np.nan, dtype=LD)
        self.n = np.zeros(size, dtype=np.int64)
        for k in ('sp', 'sh', 'P', 'H', 'dP', 'dH'):
            setattr(self, k, np.zeros(size, dtype=LD))

    def array(self):
        """(size, 2) float64, the layout of the device buffers"""
        return np.stack([self.mu, self.var], axis=1).astype(np.float64)

    def cond(self):
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.where(self.n > 0, self.sp / np.abs(self.P), 0.0).astype(np.float64)


def bound(msg):
    """(bound of |mu^ - mu|, bound of |var^ - var|) per message, float64; see the module docstring"""
    with np.errstate(divide='ignore', invalid='ignore'):
        eP = gamma(msg.n + 4) * msg.sp + msg.dP
        rel = eP / np.abs(msg.P) + U
        bvar = np.abs(msg.var) * rel
        bmu = np.abs(msg.var) * (gamma(msg.n + 5) * msg.sh + msg.dH) + np.abs(msg.mu) * (rel + 2 * U)
    # nothing summed (an observed variable's marginal (value, 0)): the value itself, exactly
    exact = (msg.n == 0) & np.isfinite(msg.mu) & np.isfinite(msg.var)
    bmu, bvar = np.where(exact, 0.0, bmu), np.where(exact, 0.0, bvar)
    return np.asarray(bmu, dtype=np.float64), np.asarray(bvar, dtype=np.float64)


def report(what, err, bnd):
    """prints the worst error-to-bound ratio of `what` and returns it (an error of 0 under a bound of 0 counts as ratio 0)"""
    err, bnd = np.asarray(err, dtype=np.float64).ravel(), np.asarray(bnd, dtype=np.float64).ravel()
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(err == 0.0, 0.0, err / bnd)
    worst = float(ratio.max()) if ratio.size else 0.0
    i = int(np.argmax(ratio)) if ratio.size else 0
    print('%-58s %7d values  worst err/bound %.3e  (err %.3e, bound %.3e)' % (what, ratio.size, worst, err[i] if ratio.size else 0.0,
                                                                              bnd[i] if ratio.size else 0.0))
    return worst


def compare(what, got, msg, mask=None):
    """`got` (N, 2) float64 from the device or the oracle against the twin's messages: same NaN / infinity pattern, every finite
    value within ``bound``; returns the worst error / bound ratio (of mu and var together)"""
    got = np.asarray(got, dtype=np.float64)
    want = msg.array()
    bmu, bvar = bound(msg)
    if mask is None:
        mask = np.ones(got.shape[0], dtype=bool)
    g, w = got[mask], want[mask]
    assert (np.isnan(g) == np.isnan(w)).all(), '%s: NaN patterns differ at %s' % (what, np.argwhere(np.isnan(g) != np.isnan(w))[:5])
    inf = np.isinf(g) | np.isinf(w)
    assert (g[inf] == w[inf]).all(), '%s: infinities differ' % what
    fin = np.isfinite(g) & np.isfinite(w)
    ref = np.stack([msg.mu, msg.var], axis=1)[mask]
    with np.errstate(invalid='ignore'):
        err = np.abs(g.astype(LD) - ref)
    bnd = np.stack([bmu, bvar], axis=1)[mask]
    # a finite value whose bound is not finite (P = 0 or an infinity among the row's terms, e.g. the -0.0 variance that follows an
    # infinite one): there is no error to allow for, the value has to be the twin's exactly -- nothing leaves the comparison
    loose = fin & ~np.isfinite(bnd)
    assert (g[loose] == w[loose]).all(), '%s: %d values under a non-finite bound differ from the twin' % (what, int((g[loose] != w[loose]).sum()))
    fin &= ~loose
    worst = report(what, err[fin], bnd[fin])
    if np.any(msg.dP != 0) or np.any(msg.dH != 0):
        # how much of the margin the closed forms' share (dP, dH) supplies: the same errors against the row-sum bound alone
        bare = copy.copy(msg)
        bare.dP, bare.dH = np.zeros_like(msg.dP), np.zeros_like(msg.dH)
        b0 = np.stack(bound(bare), axis=1)[mask]
        report(what + ' (dP = dH = 0)', err[fin], b0[fin])
    assert worst <= 1.0, '%s: error %.3g times the bound' % (what, worst)
    return worst


# ---- the twin --------------------------------------------------------------------------------------------------------------------
def _terms(mu, var, bmu=None, bvar=None):
    """an incoming message's contribution (h, p) to the information-form sums, and the first-order error of it"""
    mu, var = np.asarray(mu, dtype=LD), np.asarray(var, dtype=LD)
    none = np.isnan(var)
    with np.errstate(divide='ignore', invalid='ignore'):
        p = np.where(none, LD(0), LD(1) / var)
        h = np.where(none, -mu, p * mu)
        if bmu is None:
            return h, p, np.zeros_like(h), np.zeros_like(h)
        dp = np.where(none | np.isinf(var) | (bvar == 0), LD(0), bvar / (var * var))
        dh = np.where(none, bmu, np.abs(p) * bmu + np.abs(mu) * dp)
    return h, p, dh, dp


def _row_sums(flat, h, p, dh, dp, leave_one_out):
    """information-form sums of every row of the variable CSR from the per-slot contributions (h, p) (not yet times the count):
    leave_one_out -> a ``Msg`` per slot, else per variable.  Direct sums in longdouble."""
    deg = np.diff(flat.var_ptr).astype(np.int64)
    nnz = int(flat.var_edge.size)
    cnt = flat.edge_count[flat.var_edge].astype(LD) if flat.lifted else np.ones(nnz, dtype=LD)
    out = Msg(nnz if leave_one_out else flat.V)
    hidden = np.isnan(flat.var_value)
    for n in np.unique(deg[hidden & (deg > 0)]):
        rows = np.flatnonzero(hidden & (deg == n))
        slots = flat.var_ptr[rows].astype(np.int64)[:, None] + np.arange(n)            # (R, n)
        c, hh, pp = cnt[slots], h[slots], p[slots]
        with np.errstate(invalid='ignore'):
            ah, ap = hh * c, pp * c
            sp, sh = np.abs(ap).sum(axis=1), np.abs(ah).sum(axis=1)
            dH, dP = (dh[slots] * c).sum(axis=1), (dp[slots] * c).sum(axis=1)
            if leave_one_out:
                own = (c - 1) if flat.lifted else np.zeros_like(c)
                H, P = np.empty(slots.shape, dtype=LD), np.empty(slots.shape, dtype=LD)
                step = max(1, (1 << 21) // int(n * n))
                for r0 in range(0, rows.size, step):
                    sl = slice(r0, r0 + step)
                    for src, a, dst in ((hh, ah, H), (pp, ap, P)):
                        m = np.repeat(a[sl][:, None, :], n, axis=1)                       # (r, slot, entry)
                        i = np.arange(n)
                        m[:, i, i] = src[sl] * own[sl]
                        dst[sl] = m.sum(axis=2)
                idx = slots
                rep = lambda a: np.repeat(a[:, None], n, axis=1)
                sp, sh, dH, dP = rep(sp), rep(sh), rep(dH), rep(dP)
            else:
                H, P = ah.sum(axis=1), ap.sum(axis=1)
                idx = rows
        with np.errstate(divide='ignore', invalid='ignore'):
            var = LD(1) / P
            mu = var * H
        out.mu[idx], out.var[idx], out.n[idx] = mu, var, n
        out.sp[idx], out.sh[idx], out.P[idx], out.H[idx], out.dP[idx], out.dH[idx] = sp, sh, P, H, dP, dH
    return out


def v2f(flat, f2v):
    """GaBP / GaLBP.message_rv_to_f for every edge: a ``Msg`` in edge order (alias edges and observed rows: (NaN, NaN) / untouched)"""
    f2v = np.asarray(f2v)
    ve = flat.var_edge
    h, p, dh, dp = _terms(f2v[ve, 0], f2v[ve, 1])
    slot = _row_sums(flat, h, p, dh, dp, True)
    out = Msg(flat.E)
    for k in ('mu', 'var', 'n', 'sp', 'sh', 'P', 'H', 'dP', 'dH'):
        getattr(out, k)[ve] = getattr(slot, k)
    return out


def marginals(flat, f2v):
    """get_belief_params per variable (observed: (value, 0))"""
    f2v = np.asarray(f2v)
    ve = flat.var_edge
    h, p, dh, dp = _terms(f2v[ve, 0], f2v[ve, 1])
    out = _row_sums(flat, h, p, dh, dp, False)
    obs = ~np.isnan(flat.var_value)
    out.mu[obs], out.var[obs] = flat.var_value[obs], 0.0
    return out


def closed_forms_of(kind, par, arity, pos, partner_hidden, u, s, y):
    """message_f_to_rv (GaBP.py:37-138) on arrays, in longdouble: (mu, var, bmu, bvar); the bounds count every operation of the
    fp64 evaluation with u and every cancellation with the magnitude of its operands (first order, times 1 + 2^-20 for the
    second-order terms: they are at most (condition u) of the first-order ones).  `par`: (N, 11) parameters"""
    N = kind.size
    par = np.asarray(par, dtype=LD)
    u, s, y = (np.asarray(a, dtype=LD) for a in (u, s, y))
    mu, var = np.zeros(N, dtype=LD), np.full(N, np.inf, dtype=LD)
    emu, evar = np.zeros(N, dtype=LD), np.zeros(N, dtype=LD)            # errors in units of u
    ph = partner_hidden
    ab = np.abs

    def put(mask, m, v, em, ev):
        mu[mask], var[mask], emu[mask], evar[mask] = m[mask], v[mask], em[mask], ev[mask]
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        h, s1 = par[:, 0], par[:, 1]
        zero = np.zeros(N, dtype=LD)
        put((kind == POT_X2) & (h != 0), zero, s1 / h, zero, ab(s1 / h))
        pair = arity == 2
        nz = pair & (h != 0)
        h2 = h * h
        lg = nz & (kind == POT_LINEAR_GAUSSIAN)
        v = (s1 + s) / h2
        put(lg & ph & (pos == 0), u / h, v, ab(u / h), 3 * ab(v))
        v = s1 + s * h2
        put(lg & ph & (pos == 1), u * h, v, ab(u * h), 2 * ab(s * h2) + ab(v))
        put(lg & ~ph & (pos == 0), y / h, s1 / h2, ab(y / h), 2 * ab(s1 / h2))
        put(lg & ~ph & (pos == 1), h * y, s1, ab(h * y), zero)
        xy = nz & (kind == POT_XY)
        m, v = 2 * s1 * u / (h * s), -4 * (s1 * s1) / (h * h * s)
        put(xy & ph, m, v, 3 * ab(m), 4 * ab(v))
        m = h * y / (2 * s1)
        put(xy & ~ph, m, np.full(N, np.nan, dtype=LD), 2 * ab(m), zero)
        ga = pair & (kind == POT_GAUSSIAN) & (par[:, 0] == 2)
        m0, m1, A = par[:, 1], par[:, 2], par[:, 7:11]
        one = pos == 1
        a1, a2, a3 = np.where(one, A[:, 0], A[:, 3]), A[:, 1], np.where(one, A[:, 3], A[:, 0])
        u1, u2 = np.where(one, m0, m1), np.where(one, m1, m0)
        a4 = 1 / s
        d = a4 + a1
        e_d = ab(a4) + ab(d)
        q2 = a2 * a2
        temp = a3 * d - q2
        e_t = ab(a3) * e_d + ab(a3 * d) + ab(q2) + ab(temp)
        Nn = a2 * a4 * (u1 - u)
        r = Nn / temp
        m = r + u2
        e_m = 4 * ab(r) + ab(r) * e_t / ab(temp) + ab(r) + ab(m)
        w = q2 / d
        e_w = ab(w) * (2 + e_d / ab(d))
        z = a3 - w
        e_z = e_w + ab(z)
        v = 1 / z
        e_v = ab(v) * (e_z / ab(z) + 1)
        put(ga & ph, m, v, e_m, e_v)
        t = a2 * (y - u1) / a3
        put(ga & ~ph, -u2 - t, 1 / a3, 3 * ab(t) + ab(-u2 - t), ab(1 / a3))
    scale = LD(U) * (1 + 2.0 ** -20)
    with np.errstate(invalid='ignore'):
        return mu, var, emu * scale, evar * scale


def _edge_inputs(flat, edges, partner_msg):
    """closed-form arguments of `edges`: partner_msg(pe) -> (u, s) of partner edges"""
    edges = np.asarray(edges, dtype=np.int64)
    f = flat.edge_fac[edges].astype(np.int64)
    base = flat.fac_ptr[f].astype(np.int64)
    arity = flat.fac_ptr[f + 1] - base
    pos = edges - base
    pot = flat.fac_pot[f]
    kind = flat.pot_kind[pot]
    npar = np.diff(flat.pot_off)
    par = np.zeros((edges.size, 11))
    for j in range(11):
        has = npar[pot] > j
        par[has, j] = flat.pot_param[flat.pot_off[pot[has]] + j]
    pe = np.where(arity == 2, base + 1 - np.minimum(pos, 1), edges)
    y = flat.var_value[flat.edge_var[pe]]
    ph = (arity == 2) & np.isnan(y)
    u, s = partner_msg(flat.edge_canon[pe].astype(np.int64))
    u, s = np.where(ph, u, 0.0), np.where(ph, s, 0.0)
    y = np.where((arity == 2) & ~ph, y, 0.0)
    return kind, par, arity, pos, ph, u, s, y


def f2v(flat, v2f_in, f2v_before):
    """message_f_to_rv for every canonical edge of a hidden variable; the others keep `f2v_before` (the kernel never writes them).
    Returns (mu, var, bmu, bvar, written) in edge order, longdouble"""
    v2f_in = np.asarray(v2f_in, dtype=np.float64)
    E = flat.E
    written = (flat.edge_canon == np.arange(E)) & np.isnan(flat.var_value[flat.edge_var])
    edges = np.flatnonzero(written)
    args = _edge_inputs(flat, edges, lambda pe: (v2f_in[pe, 0], v2f_in[pe, 1]))
    m, v, bm, bv = closed_forms_of(*args)
    mu, var = np.asarray(f2v_before[:, 0], dtype=LD).copy(), np.asarray(f2v_before[:, 1], dtype=LD).copy()
    bmu, bvar = np.zeros(E, dtype=LD), np.zeros(E, dtype=LD)
    mu[edges], var[edges], bmu[edges], bvar[edges] = m, v, bm, bv
    return mu, var, bmu, bvar, written


def compare_f2v(what, got, twin):
    mu, var, bmu, bvar, written = twin
    got = np.asarray(got, dtype=np.float64)
    want = np.stack([mu, var], axis=1)
    w64 = want.astype(np.float64)
    assert (got[~written] == w64[~written]).all() or np.array_equal(got[~written], w64[~written], equal_nan=True), \
        '%s: an edge of an observed variable or an alias edge was written' % what
    g, w = got[written], w64[written]
    assert (np.isnan(g) == np.isnan(w)).all(), '%s: NaN patterns differ' % what
    inf = np.isinf(g) | np.isinf(w)
    assert (g[inf] == w[inf]).all(), '%s: infinities differ' % what
    fin = np.isfinite(g) & np.isfinite(w)
    with np.errstate(invalid='ignore'):
        err = np.abs(g.astype(LD) - want[written])
    bnd = np.stack([bmu, bvar], axis=1)[written].astype(np.float64)
    loose = fin & ~np.isfinite(bnd)                  # (a pole of a closed form: the value has to be the twin's exactly)
    assert (g[loose] == w[loose]).all(), '%s: %d values under a non-finite bound differ from the twin' % (what, int((g[loose] != w[loose]).sum()))
    fin &= ~loose
    worst = report(what, err[fin], bnd[fin])
    assert worst <= 1.0, '%s: error %.3g times the bound' % (what, worst)
    return worst


def pull_contribution_classes(flat, vprev_slot):
    """class of every slot's incoming f -> v message in ``pull``: 0 proper, 1 `None`, 2 infinite, 3 negative variance, 4 mean 0"""
    vprev_slot = np.asarray(vprev_slot, dtype=np.float64)
    es = edge_slot(flat)
    args = _edge_inputs(flat, flat.var_edge.astype(np.int64), lambda pe: (vprev_slot[es[pe], 0], vprev_slot[es[pe], 1]))
    m, v, _, _ = closed_forms_of(*args)
    with np.errstate(invalid='ignore'):
        return np.where(np.isnan(v), 1, np.where(np.isinf(v), 2, np.where(v < 0, 3, np.where(m == 0, 4, 0))))


def edge_slot(flat):
    es = np.full(max(flat.E, 1), -1, dtype=np.int64)
    es[flat.var_edge] = np.arange(flat.var_edge.size)
    return es


def pull(flat, vprev_slot, first):
    """what ``lhvi_gabp_pull`` computes: the v -> f messages of the next sweep in slot order from the previous ones (`first`: every
    f -> v message still is (0, 1)), a ``Msg`` whose dP / dH carry the rounding of the closed forms"""
    nnz = int(flat.var_edge.size)
    ve = flat.var_edge.astype(np.int64)
    if first:
        h, p, dh, dp = _terms(np.zeros(nnz), np.ones(nnz))
    else:
        vprev_slot = np.asarray(vprev_slot, dtype=np.float64)
        es = edge_slot(flat)
        args = _edge_inputs(flat, ve, lambda pe: (vprev_slot[es[pe], 0], vprev_slot[es[pe], 1]))
        m, v, bm, bv = closed_forms_of(*args)
        h, p, dh, dp = _terms(m, v, bm, bv)
    return _row_sums(flat, h, p, dh, dp, True)


# ---- the C oracle on the same inputs (shared by test_gabp_host.py and test_gpu_gabp_kernels.py) ---------------------------------------
def covered(flat):
    """edges that own a message: the canonical edges listed in the variable CSR"""
    m = np.zeros(flat.E, dtype=bool)
    m[flat.var_edge] = True
    return m


def _cp(a):
    import ctypes as C
    return a.ctypes.data_as(C.c_void_p)


def oracle_f2v(flat, v2f_in, f2v_before):
    import ctypes as C
    from oracle import oracle
    hg = oracle.HostGraph(flat)
    out = np.array(f2v_before, dtype=np.float64)
    oracle.lib().oracle_gabp_f2v(C.byref(hg.g), _cp(np.ascontiguousarray(v2f_in, dtype=np.float64)), _cp(out))
    return out


def oracle_marginals(flat, f2v_in):
    import ctypes as C
    from oracle import oracle
    hg = oracle.HostGraph(flat)
    mv = np.zeros((flat.V, 2))
    oracle.lib().oracle_gabp_marginals(C.byref(hg.g), _cp(np.ascontiguousarray(f2v_in, dtype=np.float64)), _cp(mv))
    return mv


def oracle_pull(flat, vprev):
    """the composite of lhvi_gabp_pull through the oracle's two halves"""
    import ctypes as C
    from oracle import oracle
    v2f_in = np.zeros((flat.E, 2))
    v2f_in[flat.var_edge] = vprev
    init = np.zeros((flat.E, 2))
    init[:, 1] = 1.0
    f = oracle_f2v(flat, v2f_in, init)
    hg = oracle.HostGraph(flat)
    out = np.zeros((flat.E, 2))
    oracle.lib().oracle_gabp_v2f(C.byref(hg.g), _cp(f), _cp(out))
    return out[flat.var_edge]


def model(name):
    """the models by name, as the parametrised tests address them"""
    if name == 'rows':
        return rows()
    if name.startswith('layout'):
        return layout(int(name[6:]))
    if name == 'lifted_counts':
        return lifted_counts()
    if name == 'alias':
        return alias_chain()[1]
    if name == 'closed_forms':
        return closed_forms()[0]
    if name.startswith('pots'):
        return potentials_graph(int(name[4:]))
    return dominant()[0]


# ---- models ----------------------------------------------------------------------------------------------------------------------
def _domain():
    from lhvi.graph import Domain
    return Domain((-10, 10), continuous=True, integral_points=np.linspace(-10, 10, 8))


def _gauss_spec(mean, cov):
    """parameter row of a 2-d (or n-d) Gaussian potential: n, mean, precision, the matrix the closed forms read (sig ** -1)"""
    cov = np.asarray(cov, dtype=np.float64)
    inv = np.linalg.inv(cov)
    return [float(len(mean))] + [float(x) for x in mean] + inv.ravel().tolist() + inv.ravel().tolist()


# potential table of the star forests.  6 and 7 only ever sit where their (0, inf) / None message meets a second unary factor.
STAR_POTS = [(POT_LINEAR_GAUSSIAN, [0.7, 2.0]), (POT_XY, [0.3, 3.0]), (POT_GAUSSIAN, _gauss_spec([0.0, 0.0], [[2.0, 0.5], [0.5, 1.5]])),
             (POT_X2, [1.0, 4.0]), (POT_GAUSSIAN, _gauss_spec([0.4, -0.3], [[1.2, -0.4], [-0.4, 0.9]])), (POT_X2, [2.0, 3.0]),
             (POT_LINEAR_GAUSSIAN, [0.0, 1.5]), (POT_LINEAR_GAUSSIAN, [-1.3, 0.6])]
P_LG, P_XY, P_G, P_X2, P_G2, P_X2B, P_LG0, P_LG2 = range(8)


def special_positions(n):
    """positions of a row of n entries where the kernels change what they do: first, last, first and last entry of a middle chunk
    of eight, the remainder of the last chunk (which is also a hub lane's last stride)"""
    nc = n // CHUNK
    q = nc // 2
    rem = CHUNK * nc if n % CHUNK else n - 2
    out = []
    for x in (0, n - 1, CHUNK * q, CHUNK * q + CHUNK - 1, min(rem, n - 1)):
        x = int(min(max(x, 0), n - 1))
        if x not in out:
            out.append(x)
    return out


def _star_forest(centres, tail=()):
    """`centres`: list of (row length, observed) in slot order; `tail`: centres placed behind the leaves (so that a long row ends
    on the graph's last slot).  Every centre has a unary X2 (second or third in its row; in a row of up to four entries first, middle or last in turn) and
    row length - 1 leaves, tied by LG / XY / Gaussian factors with the centre in either argument position; at the special
    positions of the row the potentials rotate through the closed forms that give a `None` variance (XY, observed leaf), an
    infinite one (LG with h = 0), a negative one (XY, hidden leaf), a plain one from evidence (LG, observed leaf) and a Gaussian;
    about 10 % of the other leaves are observed.  Leaves whose pairwise message can be (0, inf) or `None` have two unary factors."""
    from lhvi.flat import build_flat
    rng = np.random.default_rng(11)
    dom = _domain()
    allc = list(centres) + list(tail)
    n_c = len(allc)
    # variable numbering: centres, leaves, tail centres
    lead = len(centres)
    n_leaves = sum(d - 1 for d, _ in allc)
    ids = list(range(lead)) + list(range(lead + n_leaves, lead + n_leaves + len(tail)))
    nv = lead + n_leaves + len(tail)
    value = np.full(nv, np.nan)
    scopes, pot = [], []
    leaf = lead
    extra_unary = []
    special_kind = [(P_XY, True), (P_LG0, False), (P_XY, False), (P_LG, True), (P_G2, False)]      # (potential, leaf observed)
    plain = [P_LG, P_G, P_LG2, P_G2, P_LG]
    for r, ((d, observed), c) in enumerate(zip(allc, ids)):
        if observed:
            value[c] = round(float(rng.uniform(-2, 2)), 3)
        sp = special_positions(d)
        # (rows of more than four entries keep the unary factor off the special positions, which belong to the pairwise closed forms)
        unary_at = (0, d // 2, d - 1)[r % 3] if d <= 4 else 1 + r % 2
        for i in range(d):
            if i == unary_at:
                scopes.append((c,))
                pot.append(P_X2)
                continue
            lf, leaf = leaf, leaf + 1
            if i in sp and not observed:
                # (a row of two or three entries keeps a precision in every leave-one-out sum: no `None`, no infinity there)
                kinds = special_kind if d > 3 else special_kind[2:]
                p, lobs = kinds[(sp.index(i) + r) % len(kinds)]
            else:
                p, lobs = plain[(i + r) % 5], bool(rng.random() < 0.1)
            if observed:
                p = plain[(i + r) % 5] if p in (P_XY, P_LG0) else p
            if lobs:
                value[lf] = round(float(rng.uniform(-2, 2)), 3)
            scopes.append((c, lf) if (i + r) % 2 == 0 else (lf, c))
            pot.append(p)
            if p in (P_LG0, P_XY):
                extra_unary.append(lf)
    assert leaf == lead + n_leaves
    for lf in range(lead, lead + n_leaves):
        scopes.append((lf,))
        pot.append(P_X2)
    for lf in extra_unary:
        scopes.append((lf,))
        pot.append(P_X2B)
    fac_ptr = np.zeros(len(scopes) + 1, dtype=np.int32)
    np.cumsum([len(s) for s in scopes], out=fac_ptr[1:])
    edge_var = np.array([v for s in scopes for v in s], dtype=np.int32)
    flat = build_flat(fac_ptr, edge_var, np.array(pot, dtype=np.int32), STAR_POTS, value, np.zeros(nv, dtype=np.int32), [dom])
    flat.centres = np.array(ids)
    return flat


_CACHE = {}


def _cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def rows():
    """the star forest with every row length of ROW_LENGTHS, each centre once hidden and once observed"""
    return _cached('rows', lambda: _star_forest([(d, False) for d in ROW_LENGTHS] + [(d, True) for d in ROW_LENGTHS]))


def layout(window):
    """the same rows in an order that puts rows where the pull kernels' bookkeeping can go wrong.  Array kernel (blocks of 256
    slots): the hidden 512-row starts inside one block and ends inside another, a hub row ends on a block's last slot and the next
    hub row starts on a block's first, and a chunked row ends on the last slot of the graph.  Record kernel: a row starts on the
    first slot of a window and the 512-row on the last, i.e. the longest segment the plan can make, window - 1 + 512 slots."""
    def make():
        todo = [(d, o) for o in (False, True) for d in ROW_LENGTHS]
        if window == 256:
            # 0: 127, 127: 128, 255: 512 (segment [0, 767)), 767: 128 observed ([127, 895) = 768 slots for a hand-built segment),
            # 895: 65 -> 960 = 3 * 256 + 192, 576-hub ends on 1536 = 6 * 256, where the 513-hub starts
            head = [(127, False), (128, False), (512, False), (128, True), (65, False), (576, False), (513, False)]
        else:
            # 0: 63, 63: 512 ([0, 575)), 575: 128 observed -> 703 = 2 * 256 + 191, 577-hub ends on 1280 = 5 * 256, 513-hub starts there
            head = [(63, False), (512, False), (128, True), (577, False), (513, False)]
        tail = [(66, False)]
        for c in head + tail:
            todo.remove(c)
        return _star_forest(head + todo, tail)
    return _cached(('layout', window), make)


def lifted_counts():
    """``rows()`` as a lifted graph: integer counts from {1, 2, 3, 7, 90}, rotating along every row so that each row has slots whose
    own count is 1 (weight exactly 0) and slots with every other count"""
    def make():
        g = rows()
        flat = copy.copy(g)
        flat.__dict__.pop('_view_cache', None)
        deg = np.diff(g.var_ptr).astype(np.int64)
        svar = np.repeat(np.arange(g.V), deg)
        within = np.arange(g.var_edge.size) - g.var_ptr[svar]
        cnt = np.array([1.0, 2.0, 3.0, 7.0, 90.0])[(within + svar) % 5]
        has = deg > 0
        cnt[g.var_ptr[:-1][has] + np.arange(g.V)[has] % deg[has]] = 1.0          # (rows of fewer than five entries too)
        ec = np.ones(g.E)
        ec[g.var_edge] = cnt
        flat.edge_count, flat.lifted = ec, True
        return flat
    return _cached('lifted_counts', make)


def alias_chain(refine=None):
    """(ground FlatGraph, lifted FlatGraph, rv colours, factor colours): a symmetric chain x0 - ... - x5 (equal symmetric Gaussian factors, equal
    unary factors, two symmetric observed leaves): colour refinement puts x2 and x3 into one cluster, so the middle factor's scope
    names that cluster twice -- an alias edge.  `refine(flat, sym, rv0, f0)` -> colours; default: the oracle's colour passing
    (pure Python; the GPU tests pass ``lifting.refine_flat``)."""
    from lhvi.flat import build_flat
    from lhvi import lifting
    dom = _domain()
    n = 6
    scopes = [(i, i + 1) for i in range(n - 1)] + [(0, n), (n - 1, n + 1)] + [(i,) for i in range(n)]
    pot = [0] * (n - 1) + [1, 1] + [2] * n
    pots = [(POT_GAUSSIAN, _gauss_spec([0.0, 0.0], [[1.5, 0.4], [0.4, 1.5]])), (POT_XY, [0.3, 3.0]), (POT_X2, [1.0, 4.0])]
    value = np.full(n + 2, np.nan)
    value[n] = value[n + 1] = 0.75
    fac_ptr = np.zeros(len(scopes) + 1, dtype=np.int32)
    np.cumsum([len(s) for s in scopes], out=fac_ptr[1:])
    edge_var = np.array([v for s in scopes for v in s], dtype=np.int32)
    g = build_flat(fac_ptr, edge_var, np.array(pot, dtype=np.int32), pots, value, np.zeros(n + 2, dtype=np.int32), [dom])
    hidden = np.isnan(value)
    rv0 = np.where(hidden, 0, 1).astype(np.int32)
    f0 = np.array(pot, dtype=np.int32)
    sym = np.array([1 if len(s) == 2 else 0 for s in scopes], dtype=np.uint8)
    if refine is None:
        from oracle import oracle
        refine = oracle.color_passing
    rvc, fc = refine(g, sym, rv0, f0)
    lifted = lifting.lift_flat(g, np.asarray(rvc), np.asarray(fc))
    assert (lifted.edge_canon != np.arange(lifted.E)).any(), 'the symmetric chain has no alias edge'
    return g, lifted, np.asarray(rvc), np.asarray(fc)


def closed_forms():
    """(FlatGraph, v2f): one factor per closed form -- 2-d Gaussian (symmetric, with a mean, with an asymmetric precision), linear
    Gaussian, XY, each with the partner hidden and observed in both positions, h = 0 for LG / XY / X2, a 3-d Gaussian and a linear
    Gaussian on factors of arity 3 (-> (0, inf)) -- repeated once per class of partner message: `v2f` holds hand-built v -> f
    messages whose class is that of the replica.  Every variable has two proper unary factors, so no row sum is empty."""
    def make():
        from lhvi.flat import build_flat
        dom = _domain()
        asym = _gauss_spec([0.2, -0.1], [[1.0, 0.3], [0.3, 2.0]])
        asym[3 + 1] *= 1.25                            # precision and sig ** -1 with a01 != a10: only a01 is read
        asym[7 + 1] *= 1.25
        pots = [(POT_GAUSSIAN, _gauss_spec([0.0, 0.0], [[2.0, 0.5], [0.5, 1.5]])), (POT_GAUSSIAN, _gauss_spec([0.4, -0.3], [[1.2, -0.4], [-0.4, 0.9]])),
                (POT_GAUSSIAN, asym), (POT_LINEAR_GAUSSIAN, [0.7, 2.0]), (POT_XY, [0.3, 3.0]),
                (POT_LINEAR_GAUSSIAN, [0.0, 2.0]), (POT_XY, [0.0, 3.0]), (POT_X2, [0.0, 4.0]),
                (POT_GAUSSIAN, _gauss_spec([0.0, 0.1, 0.2], np.diag([1.0, 2.0, 3.0]) + 0.2)), (POT_X2, [1.0, 4.0]), (POT_X2, [2.0, 3.0])]
        scopes, pot, value = [], [], []

        def var(observed):
            value.append(0.6 - 0.37 * len(value) % 1.7 if observed else np.nan)
            return len(value) - 1
        for rep in range(len(CLASSES)):
            for p in range(7):
                for oa, ob in ((False, False), (False, True), (True, False)):
                    a, b = var(oa), var(ob)
                    scopes.append((a, b))
                    pot.append(p)
            for p in (8, 3):                                   # arity 3: a 3-d Gaussian, a linear Gaussian
                scopes.append((var(False), var(False), var(rep % 2 == 1)))
                pot.append(p)
            scopes.append((var(False),))
            pot.append(7)                                      # X2 with h = 0
        nv = len(value)
        for v in range(nv):
            scopes += [(v,), (v,)]
            pot += [9, 10]
        fac_ptr = np.zeros(len(scopes) + 1, dtype=np.int32)
        np.cumsum([len(s) for s in scopes], out=fac_ptr[1:])
        edge_var = np.array([v for s in scopes for v in s], dtype=np.int32)
        flat = build_flat(fac_ptr, edge_var, np.array(pot, dtype=np.int32), pots, np.array(value), np.zeros(nv, dtype=np.int32), [dom])
        rng = np.random.default_rng(5)
        per_rep = nv // len(CLASSES)
        cls = np.minimum(flat.edge_var // per_rep, len(CLASSES) - 1)
        v2f_in = _draw(rng, flat.E, cls)
        v2f_in[~np.isnan(flat.var_value)[flat.edge_var]] = np.nan
        return flat, v2f_in
    return _cached('closed_forms', make)


def potentials_graph(n_pots):
    """a chain whose pairwise factors all have different linear-Gaussian potentials: exactly `n_pots` potentials, all referenced
    (the record kernels keep up to 32 in LDS and read the table from global memory beyond)"""
    from lhvi.flat import build_flat
    dom = _domain()
    m = n_pots - 2
    pots = [(POT_LINEAR_GAUSSIAN, [0.5 + 0.03 * i, 1.0 + 0.1 * i]) for i in range(m)] + [(POT_X2, [1.0, 4.0]), (POT_X2, [2.0, 3.0])]
    scopes = [(i, i + 1) for i in range(m)] + [(i,) for i in range(m + 1)] + [(i,) for i in range(m + 1)]
    pot = list(range(m)) + [m] * (m + 1) + [m + 1] * (m + 1)
    value = np.full(m + 1, np.nan)
    value[3::7] = 0.5
    fac_ptr = np.zeros(len(scopes) + 1, dtype=np.int32)
    np.cumsum([len(s) for s in scopes], out=fac_ptr[1:])
    edge_var = np.array([v for s in scopes for v in s], dtype=np.int32)
    flat = build_flat(fac_ptr, edge_var, np.array(pot, dtype=np.int32), pots, value, np.zeros(m + 1, dtype=np.int32), [dom])
    assert np.unique(flat.fac_pot).size == n_pots == flat.pot_kind.size
    return flat


# ---- hand-built messages ----------------------------------------------------------------------------------------------------------
def _draw(rng, size, cls):
    """(size, 2) messages of the classes `cls` (indices into CLASSES)"""
    cls = np.broadcast_to(np.asarray(cls), (size,))
    mu = rng.normal(0.0, 5.0, size)
    var = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), size))
    var = np.where(cls == 1, np.nan, np.where(cls == 2, np.inf, np.where(cls == 3, -var, var)))
    mu = np.where(cls == 4, 0.0, mu)
    return np.stack([mu, var], axis=1)


def messages(flat, rng):
    """hand-built f -> v messages in edge order: proper ones everywhere, and at the special positions of every row one message of
    each class, rotating with the row's number within its row class -- so every row class (direct, chunked, hub) has every class
    at every special position.  Negative variances only in rows of at least four entries.  A special message that would make a
    leave-one-out precision of its row vanish, or worse conditioned than COND_CAP, is drawn again as a proper one."""
    deg = np.diff(flat.var_ptr).astype(np.int64)
    nnz = int(flat.var_edge.size)
    cls = np.zeros(nnz, dtype=np.int64)
    seen = {}
    placed = {}
    for v in np.flatnonzero(deg >= 3):
        n = int(deg[v])
        rc = 0 if n <= ROW_DIRECT else (1 if n <= HUB else 2)
        r = seen[rc] = seen.get(rc, -1) + 1
        sp = special_positions(n)
        for i, x in enumerate(sp):
            c = (i + r) % 5
            if c == 3 and n < 4:
                c = 0
            cls[flat.var_ptr[v] + x] = c
        placed[v] = [int(flat.var_ptr[v]) + x for x in sp]
    slot_msg = _draw(rng, nnz, cls)
    # repair: rows whose leave-one-out precisions break the cap lose their special messages one by one, last position first
    cnt = flat.edge_count[flat.var_edge] if flat.lifted else np.ones(nnz)
    for v, slots in placed.items():
        lo, hi = int(flat.var_ptr[v]), int(flat.var_ptr[v + 1])
        for k in [None] + slots[::-1]:
            if k is not None:
                slot_msg[k] = _draw(rng, 1, 0)[0]
            with np.errstate(divide='ignore'):
                p = np.where(np.isnan(slot_msg[lo:hi, 1]), 0.0, 1.0 / slot_msg[lo:hi, 1]).astype(LD)
            c = cnt[lo:hi].astype(LD)
            tot = (p * c).sum()
            loo = tot - p * (LD(1) if flat.lifted else c)
            if (loo != 0).all() and (np.abs(p * c).sum() / np.abs(loo)).max() <= COND_CAP / 4:
                break
    out = np.zeros((flat.E, 2))
    out[:, 1] = 1.0                                              # (alias edges: never read)
    out[flat.var_edge] = slot_msg
    return out


def slot_messages(flat, rng):
    """hand-built v -> f messages in slot order for ``lhvi_gabp_pull(first=0)``: proper and zero-mean messages with a positive
    variance (a v -> f message is (H / P, 1 / P): it has no `None` and, with P != 0, no infinite variance).  The `None`, infinite
    and negative classes reach the pull kernels' row sums through the closed forms of the models' potentials
    (``pull_contribution_classes``; test_gabp_host.py asserts where they land); observed rows carry NaN"""
    nnz = int(flat.var_edge.size)
    svar = np.repeat(np.arange(flat.V), np.diff(flat.var_ptr))
    k = np.arange(nnz)
    cls = np.where(k % 11 == 3, 4, 0)
    out = _draw(rng, nnz, cls)
    # a variance in [0.05, 20]: keeps every closed form of the models away from its poles
    out[:, 1] = np.exp(rng.uniform(np.log(0.05), np.log(20.0), nnz))
    out[~np.isnan(flat.var_value)[svar]] = np.nan
    return out


def dominant():
    """(FlatGraph, f2v, vprev, slots): a hub row (577) and a chunked row (66) whose entry in the middle carries a precision 1e9
    times the sum of the others -- in `f2v` (edge order, for the pair kernels) and, through a linear-Gaussian factor with a tiny
    variance and a tiny partner variance, in the closed forms of `vprev` (slot order, for the pull kernels).  `slots`: the
    dominant entries' slots.  The leave-one-out sums of the OTHER slots of these rows are dominated, not cancelled; the
    dominant slot's own sum is the total minus 1e9 times itself: condition 1e9 by construction."""
    def make():
        from lhvi.flat import build_flat
        dom = _domain()
        rng = np.random.default_rng(9)
        lens = [577, 66]
        pots = [(POT_LINEAR_GAUSSIAN, [0.7, 2.0]), (POT_X2, [1.0, 4.0]), None, None]
        # all leaves sit at position 1 of LG(0.7, 2): the centre (position 0) receives var = (2 + s) / 0.49
        nv = len(lens) + sum(d - 1 for d in lens)
        scopes, pot = [], []
        leaf = len(lens)
        dom_leaf = []
        for c, d in enumerate(lens):
            for i in range(d - 1):
                scopes.append((c, leaf))
                pot.append(2 + c if i == d // 2 else 0)
                if i == d // 2:
                    dom_leaf.append(leaf)
                leaf += 1
            scopes.append((c,))
            pot.append(1)
        for lf in range(len(lens), nv):
            scopes.append((lf,))
            pot.append(1)
        s_leaf = 1.0                                              # every leaf's v -> f variance in vprev
        tiny = []
        for d in lens:
            others = (d - 2) * 0.49 / (2.0 + s_leaf) + 1.0 / 4.0
            tiny.append(0.5 / (1e9 * others))                     # s1 = s = tiny: precision 1 / (2 tiny) = 1e9 * others
        pots[2], pots[3] = (POT_LINEAR_GAUSSIAN, [1.0, tiny[0]]), (POT_LINEAR_GAUSSIAN, [1.0, tiny[1]])
        fac_ptr = np.zeros(len(scopes) + 1, dtype=np.int32)
        np.cumsum([len(s) for s in scopes], out=fac_ptr[1:])
        edge_var = np.array([v for s in scopes for v in s], dtype=np.int32)
        flat = build_flat(fac_ptr, edge_var, np.array(pot, dtype=np.int32), pots, np.full(nv, np.nan), np.zeros(nv, dtype=np.int32), [dom])
        nnz = int(flat.var_edge.size)
        svar = np.repeat(np.arange(flat.V), np.diff(flat.var_ptr))
        vprev = np.stack([rng.normal(0.0, 5.0, nnz), np.full(nnz, s_leaf)], axis=1)
        es = edge_slot(flat)
        slots = []
        for c, lf in enumerate(dom_leaf):
            f = scopes.index((c, lf))
            vprev[es[flat.fac_ptr[f] + 1], 1] = tiny[c]           # the leaf's message to the factor
            slots.append(int(es[flat.fac_ptr[f]]))
        f2v_in = _draw(rng, flat.E, 0)
        f2v_in[:, 1] = np.exp(rng.uniform(np.log(0.5), np.log(2.0), flat.E))
        for c, k in enumerate(slots):
            lo, hi = int(flat.var_ptr[c]), int(flat.var_ptr[c + 1])
            e_row = flat.var_edge[lo:hi]
            others = sum(1.0 / f2v_in[e, 1] for e in e_row if e != flat.var_edge[k])
            f2v_in[flat.var_edge[k], 1] = 1.0 / (1e9 * others)
        return flat, f2v_in, vprev, np.array(slots)
    return _cached('dominant', make)
