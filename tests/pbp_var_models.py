"""Hand-built states, a NumPy ``np.longdouble`` twin and derived error bounds for the per-variable kernels of csrc/pbp.hip: v -> f
with its balance step (``pbp_v2f_kernel``, ``pbp_v2f_hub_kernel``, ``pbp_v2f_narrow_kernel``, ``pbp_v2f_packed_kernel``), the
proposal update (``pbp_proposal_kernel`` with its slices and its partial / finish pair) and the fused one-pass kernels
(``pbp_var_fused_kernel``).

A state is a small ``FlatGraph`` of unary factors -- only the variables' rows matter to these kernels, so a variable of degree d
simply owns d factors -- with chosen ``particles [V, n]``, ``uniq [V, n]``, ``f2v [E, n + T]``, ``q [V, 2]`` and ``eta [E, 2]``.
No sweep is run.  The same arrays go into ``oracle.PbpOracle`` (tests/test_pbp_var_host.py) and over a solver's tensors on the
device (tests/test_gpu_pbp_var.py).  A lifted state is the same graph with multiplicities 1..6 written into ``edge_count``.

The twin restates the reference's definitions (EPBPLogVersion.py / HybridLBPLogVersion.py: ``message_rv_to_f``,
``important_weight``, ``log_message_balance``, ``update_proposal`` with ``eta_approximation(_simple)``, ``gaussian_division`` and
``gaussian_product``), not the kernels' order of operations:

  v -> f     res_e[j] = sum_{k != e} c_k m_k[j] + (c_e - 1) m_e[j] + log w_j, the sum formed directly (prefix + suffix, no
             "total minus own");  w_j = 1 / max(N(x_j; mu, sd), 1e-200), 1e-200 on a domain bound (and on the first two states of
             a discrete variable under the EPBP flag), 1 for a discrete variable without the flag;
  balance    shift = mean over the DISTINCT particles, or max - max_log_value when max - mean > max_log_value;
  proposal   per edge the T-point moments of exp(msg) (times the cavity density N(x; c) when ``!(q1 >= b1)`` under EP, followed
             by the division by the cavity), the accept test 0 < sig < inf, the floor total_count * var_threshold, the old site
             kept on failure; q from the information-form sums with counts.
             exp(msg) of a message <= -800 is exactly zero in fp64 (the last denormal is exp(-745.13)); the twin sets it to zero
             too, and the builders keep every message >= -700 or <= -800 and every nonzero z above 1e-280.

Bounds, in units of u = 2^-53 (one rounding to nearest; a routine good to k ulp costs 2 k u).  Any summation order of N terms
errs by at most (N - 1) u sum|terms| (first order), so the bounds hold for the kernels' row, half-wave and wave reductions, for the
hub kernel's and the slices' partial sums and for the C oracle's sequential sums alike; they name no order.
  Short routines: ``log_pos`` 2 ulp of |log| (tests/test_gpu_pbp.py::test_device_log_accuracy), ``sqrt_pos`` and ``rcp_newton``
  1 ulp (csrc/common.hpp; a rounded Newton correction of a 24 / 50-bit seed), ocml ``exp`` / ``sqrt`` / division 1 ulp.
  v -> f (``V2fTwin.bound``, formed in ``v2f_twin``), with A_j = sum_k |c_k m_k[j]|, U = (x - mu)^2 / (2 var), cnt = distinct particles, R = mean |res|:
     e_logw = u (15 U + 5 |log(2.5066 sd)| + 3 + |log w|)      rsd = rcp(sqrt(var)) 4 u, (x - mu) and the product 2 u: 6 u on the
                                                               normalised distance, 13 u on U with its square; the logarithm's
                                                               argument 3 u, log_pos 4 u |log|; the sum and the constant u |log w|.
                                                               Exact (u |log w| for the constant) where the particle is penalised
     e_res  = u ((deg + 1) A_j + 2 (A_j + |log w_j|)) + e_logw  the products c m and deg - 1 additions of partial sums <= A_j
                                                               ("total minus own": ulps of A, not of the result), then - m, + log w
     e_shift = max_j e_res + u (cnt + 2) R + u |shift|          cnt - 1 additions, the reciprocal of cnt and its product; the max rule
                                                               carries e_res of the largest particle and one subtraction
     |out - twin| <= e_res + e_shift + u |out|
  site (``ProposalTwin.eta_bound``, formed in ``proposal_twin``), with w_t the weights, z, a, b their sums against 1, x, x^2, E2 = b / z:
     rho_t = 2 u without cavity; with it u (6 v_t^2 + 8 K0 |v_t| / csd + 10), v_t = (x_t - c0) / csd, K0 = (|q0| (b1 + c1) +
             |b0| c1) / b1: the cavity variance c1 = q1 b1 / (b1 - q1) 3 u, its mean 8 u K0 (a difference of products), the density's
             exponent v^2 / 2 with v good to 4.5 u |v| + 8 u K0 / csd, its normalisation 5 u, exp and the product 3 u
     e_z = sum w rho + (T - 1) u z,  e_a = sum w |x| (rho + u) + (T - 1) u sum w |x|,  e_b likewise with x^2 and rho + 2 u
     e_mu  = (e_a + |mu| e_z) / z + 3 u |mu|
     e_sig = (e_b + E2 e_z) / z + 3 u E2 + 2 |mu| e_mu + u mu^2 + u max(E2, mu^2)
             -- the difference b / z - mu^2 is taken between two numbers of size E2: ulps of E[x^2], not of sigma^2
     division by the cavity: sig' = sig c1 / (c1 - sig), relative error e_sig / sig + (3 u c1 + e_sig) / |c1 - sig| + 6 u; mu' =
             (mu (c1 + sig') - c0 sig') / c1 with every addend's absolute error carried, + 5 u |mu'|
     a floored site is exactly total * var_threshold, a kept site exactly the old one: bound 0
  q (``ProposalTwin.q_bound``): ps = sum c / sig, pm = sum c mu / sig;
     e_ps = sum c (e_sig / sig + 4 u) / sig + deg u ps,  e_pm = sum c ((e_sig / sig + 5 u) |mu| + e_mu) / sig + deg u sum c |mu| / sig
     e_q1 = q1 (e_ps / ps + 2 u),  e_q0 = |q0| (e_ps / ps + 3 u) + q1 e_pm -- an error of a site's variance enters through 1 / sig^2

Decisions.  shift rule (margin |max - mean - max_log_value| over its error), accept test (|sig| over e_sig; exact where z = 0 or
where the mass sits on one grid point with weight 1 and an exactly representable square), floor (|sig - floor| over e_sig) and
cavity switch (a comparison of two inputs: exact).  ``build`` asserts that none lies within 4 bounds of its threshold, so no value is
ever undecided.  Under the switch (b1 > q1 > 0) a cavity variance is positive; the negative variance that keeps a site is the one the
division by the cavity returns when the moments' variance exceeds the cavity's ('negvar' rows).

Nothing here imports ``lhvi`` at module level or shares code with the kernels."""
from dataclasses import dataclass, field

import numpy as np

from pbp_f2v_models import EPS, FLOOR, HI, LD, LO, TABLE, X2, _Builder, grid_points
from pbp_sampler_models import first_occurrence

SQRT_2PI = 2.506628274631           # the reference's constant (EPBPLogVersion.py:49-53)
TINY = 1e-200
DEAD = -800.0
MARGIN = 4.0
T_LIST = (1, 7, 16, 17, 32, 33, 48, 64, 65, 100, 128)
SMALL_DEGREES = (1, 2, 4, 5, 6, 7, 8, 9, 16, 17)
HUB_DEGREES = (63, 64, 65, 79, 80, 81, 200)
HUB_T = (7, 32, 64, 100)
DISCRETE = (2, 3, 4, 5, 7, 20)
DISCRETE_DEGREES = (1, 2, 4, 5, 9, 17, 65, 80)
V2F_MUTANTS = ('own_kept', 'own_count', 'mean_all', 'max_all', 'rule_max', 'no_bound_penalty', 'no_clamp')
PROPOSAL_MUTANTS = ('no_counts', 'floor_degree', 'cavity_inverted', 'overwrite_failed', 'last_point')


@dataclass
class VarState:
    flat: object
    n: int
    epbp: bool                      # EPBP's flags (discrete variables weighted too), else HybridLBP's
    ep: bool                        # the 'EP' rule (cavity), else 'simple'
    var_threshold: float
    particles: np.ndarray
    uniq: np.ndarray
    f2v: np.ndarray
    q: np.ndarray
    eta: np.ndarray
    counts: np.ndarray
    var_degree: object = None       # [V] float64, or None: the kernels sum the row's counts
    max_log_value: float = 700.0
    tags: dict = field(default_factory=dict)       # variable -> what the builder put into its rows
    _cache: dict = field(default_factory=dict, repr=False)

    @property
    def T(self):
        sizes = np.diff(self.flat.dom_ptr)
        return int(sizes[self.flat.dom_cont.astype(bool)].max())

    def rows(self, v):
        return self.flat.var_edge[self.flat.var_ptr[v]:self.flat.var_ptr[v + 1]]

    def grid(self, v):
        d = self.flat.var_dom[v]
        return self.flat.dom_val[self.flat.dom_ptr[d]:self.flat.dom_ptr[d + 1]]

    def hidden(self):
        return np.flatnonzero(self.flat.var_hidden)

    def cont(self):
        return np.flatnonzero(self.flat.var_hidden & self.flat.var_cont)

    def oracle(self):
        from oracle import oracle
        o = oracle.PbpOracle(self.flat, self.n, ep=self.ep, epbp=self.epbp, var_threshold=self.var_threshold)
        o.set_particles(self.particles)
        assert (o.np == self.counts).all() and (o.particles == self.particles).all() and (o.uniq == self.uniq).all()
        o.f2v, o.q, o.eta = self.f2v.copy(), self.q.copy(), self.eta.copy()          # (the oracle updates eta and q in place)
        return o

    def v2f(self):
        if 'v2f' not in self._cache:
            self._cache['v2f'] = v2f_twin(self)
        return self._cache['v2f']

    def proposal(self):
        if 'prop' not in self._cache:
            self._cache['prop'] = proposal_twin(self)
        return self._cache['prop']


# ---- v -> f --------------------------------------------------------------------------------------------------------------------------
@dataclass
class V2fTwin:
    out: np.ndarray                 # longdouble [E, n]: the balanced message
    live: np.ndarray                # bool [E, n]: written by a sweep (j < np of a hidden variable's edge); everything else must not be
    bound: np.ndarray               # float64 [E, n]
    max_rule: np.ndarray            # bool [E]: the shift is max - max_log_value
    margin: np.ndarray              # float64 [E]: the shift rule's margin in bounds (inf on rows nothing writes)
    clamped: np.ndarray             # bool [V, n]: log w sits at +log 1e200
    penalised: np.ndarray           # bool [V, n]: log w is -log 1e200 (a bound, or one of the first two states)


def log_weight(st, v, mutant=None):
    """(log w [np] longdouble, its error bound [np], clamped, penalised) of variable v's particles (``important_weight``)"""
    fl = st.flat
    npv = int(st.counts[v])
    x = st.particles[v, :npv]
    d = fl.var_dom[v]
    pen = np.zeros(npv, dtype=bool)
    if fl.dom_cont[d]:
        pen = (x == fl.dom_lo[d]) | (x == fl.dom_hi[d])
    elif not st.epbp:
        return np.zeros(npv, dtype=LD), np.zeros(npv), np.zeros(npv, dtype=bool), pen
    else:
        vals = st.grid(v)
        pen = (x == vals[0]) | ((x == vals[1]) if vals.size > 1 else False)
    if mutant == 'no_bound_penalty':
        pen = np.zeros(npv, dtype=bool)
    mu, sd = LD(st.q[v, 0]), np.sqrt(LD(st.q[v, 1]))
    u = (x.astype(LD) - mu) / sd
    pdf = np.exp(-u * u / 2) / (LD(SQRT_2PI) * sd)
    U, log_norm = (u * u / 2).astype(np.float64), float(np.log(LD(SQRT_2PI) * sd))
    free = u * u / 2 + np.log(LD(SQRT_2PI) * sd)            # -log(pdf), which underflows even the longdouble range at U > 11356
    lw = free if mutant == 'no_clamp' else np.log(1 / np.maximum(pdf, LD(TINY)))
    clamped = (pdf < LD(TINY)) & ~pen
    lw = np.where(pen, np.log(LD(TINY)), lw)
    err = EPS * np.where(pen, np.abs(lw), 15 * U + 5 * abs(log_norm) + 3 + np.abs(lw)).astype(np.float64)
    return lw, err, clamped, pen


def v2f_twin(st, mutant=None):
    fl, n = st.flat, st.n
    out = np.zeros((fl.E, n), dtype=LD)
    live = np.zeros((fl.E, n), dtype=bool)
    bound = np.zeros((fl.E, n))
    max_rule = np.zeros(fl.E, dtype=bool)
    margin = np.full(fl.E, np.inf)
    clamped = np.zeros((fl.V, n), dtype=bool)
    penalised = np.zeros((fl.V, n), dtype=bool)
    mlv = LD(st.max_log_value)
    for v in st.hidden():
        rows, npv = st.rows(v), int(st.counts[v])
        deg = rows.size
        if deg == 0:
            continue
        M = st.f2v[rows, :npv].astype(LD)
        c = (fl.edge_count[rows] if fl.lifted else np.ones(deg)).astype(LD)[:, None]
        CM = c * M
        zero = np.zeros((1, npv), dtype=LD)
        before = np.concatenate([zero, np.cumsum(CM, axis=0)[:-1]])                      # sum_{k < e}
        after = np.concatenate([np.cumsum(CM[::-1], axis=0)[::-1][1:], zero])            # sum_{k > e}
        own = (c - 1) * M
        if mutant == 'own_kept':
            own = CM
        elif mutant == 'own_count':
            own = 0 * M
        lw, e_lw, clamped[v, :npv], penalised[v, :npv] = log_weight(st, v, mutant)
        res = (before + after) + own + lw[None, :]
        A = np.abs(CM).sum(axis=0).astype(np.float64)
        e_res = EPS * ((deg + 1) * A + 2 * (A + np.abs(lw).astype(np.float64))) + e_lw           # [np]
        uq = st.uniq[v, :npv].astype(bool)
        in_mean = np.ones(npv, dtype=bool) if mutant == 'mean_all' else uq
        in_max = np.ones(npv, dtype=bool) if mutant == 'max_all' else uq
        cnt = int(in_mean.sum())
        mean = res[:, in_mean].sum(axis=1) / cnt
        mx = res[:, in_max].max(axis=1)
        spread = mx if mutant == 'rule_max' else mx - mean
        use_max = spread > mlv
        shift = np.where(use_max, mx - mlv, mean)
        o = res - shift[:, None]
        R = np.abs(res[:, uq]).sum(axis=1).astype(np.float64) / cnt
        e_max = float(e_res[uq].max())
        e_shift = e_max + EPS * ((cnt + 2) * R + np.abs(shift).astype(np.float64))
        out[rows, :npv], live[rows, :npv] = o, True
        bound[rows, :npv] = e_res[None, :] + e_shift[:, None] + EPS * np.abs(o).astype(np.float64)
        max_rule[rows] = use_max
        margin[rows] = np.abs((mx - mean) - mlv).astype(np.float64) / (2 * e_max + EPS * ((cnt + 2) * R + np.abs(mx - mean).astype(np.float64)))
    return V2fTwin(out, live, bound, max_rule, margin, clamped, penalised)


# ---- proposal ------------------------------------------------------------------------------------------------------------------------
@dataclass
class ProposalTwin:
    eta: np.ndarray                 # longdouble [E, 2]: the sites after the update (the old ones where nothing is written)
    eta_bound: np.ndarray           # float64 [E, 2]; 0: bit for bit (kept, floored variance, rows nothing writes)
    owned: np.ndarray               # bool [E]: an edge of a hidden continuous variable
    kept: np.ndarray                # bool [E]: the accept test failed -- the old site stays
    why_kept: list                  # per edge: '', 'z=0', 'zero', 'negative'
    floored: np.ndarray             # bool [E]
    cavity: np.ndarray              # bool [E]: the moments were taken under the cavity density
    q: np.ndarray                   # longdouble [V, 2] (the old q where nothing is written)
    q_bound: np.ndarray             # float64 [V, 2]
    q_live: np.ndarray              # bool [V]
    margin: dict                    # 'accept', 'floor', 'cavity': float64 [E] in bounds (inf where there is no such decision, and for the
                                    # cavity switch everywhere: it compares two inputs)
    ps: np.ndarray                  # longdouble [V, 2]: the information-form sums (sum c / sig, sum c mu / sig)


def gaussian_division(a0, a1, b0, b1):
    sig = a1 * b1 / (b1 - a1)
    return (a0 * (b1 + sig) - b0 * sig) / b1, sig


def proposal_twin(st, mutant=None):
    fl, n = st.flat, st.n
    E, V = fl.E, fl.V
    eta, eta_bound = st.eta.astype(LD), np.zeros((E, 2))
    owned, kept, floored, cavity = (np.zeros(E, dtype=bool) for _ in range(4))
    why = [''] * E
    q, q_bound, q_live = st.q.astype(LD), np.zeros((V, 2)), np.zeros(V, dtype=bool)
    ps_out = np.zeros((V, 2), dtype=LD)
    margin = {'accept': np.full(E, np.inf), 'floor': np.full(E, np.inf), 'cavity': np.full(E, np.inf)}
    u = EPS
    with np.errstate(all='ignore'):
        for v in st.cont():
            rows, x = st.rows(v), st.grid(v).astype(LD)
            deg, T = rows.size, x.size
            if mutant == 'last_point' and T > 1:
                x, T = x[:-1], T - 1
            G = st.f2v[rows, n:n + T]
            assert ((G >= FLOOR) | (G <= DEAD)).all(), 'a message between the classes'
            c = (fl.edge_count[rows] if fl.lifted else np.ones(deg)).astype(LD)
            total = LD(st.var_degree[v]) if st.var_degree is not None else c.sum()
            if mutant == 'floor_degree':
                total = LD(deg)
            min_sig = LD(np.float64(total) * np.float64(st.var_threshold))      # (the floor IS the fp64 product: a floored site compares bit for bit)
            q0, q1 = LD(st.q[v, 0]), LD(st.q[v, 1])
            b0, b1 = st.eta[rows, 0].astype(LD), st.eta[rows, 1].astype(LD)
            cav = np.full(deg, st.ep) & ~(q1 >= b1)
            if mutant == 'cavity_inverted':
                cav = np.full(deg, st.ep) & (q1 >= b1)
            c0, c1 = gaussian_division(q0, q1, b0, b1)
            csd = np.sqrt(c1)
            vt = (x[None, :] - c0[:, None]) / csd[:, None]
            pdf = np.exp(-vt * vt / 2) / (LD(SQRT_2PI) * csd[:, None])
            w = np.where(G <= DEAD, LD(0), np.exp(G.astype(LD)))
            w = np.where(cav[:, None], w * pdf, w)
            z, a, b = w.sum(axis=1), (w * x).sum(axis=1), (w * (x * x)).sum(axis=1)
            mu, sig = a / z, b / z - (a / z) ** 2
            # ---- the moments' error
            K0 = ((abs(q0) * (b1 + c1) + np.abs(b0) * c1) / b1).astype(np.float64)
            v64 = np.abs(vt).astype(np.float64)
            rho = np.where(cav[:, None], u * (6 * v64 ** 2 + 8 * K0[:, None] * v64 / csd.astype(np.float64)[:, None] + 10), 2 * u)
            w64, x64 = w.astype(np.float64), np.abs(x).astype(np.float64)[None, :]
            rho = np.where(w64 > 0, rho, 0.0)
            z64, mu64 = z.astype(np.float64), np.abs(mu).astype(np.float64)
            e_z = (w64 * rho).sum(axis=1) + (T - 1) * u * z64
            e_a = (w64 * x64 * (rho + u)).sum(axis=1) + (T - 1) * u * (w64 * x64).sum(axis=1)
            e_b = (w64 * x64 ** 2 * (rho + 2 * u)).sum(axis=1) + (T - 1) * u * (w64 * x64 ** 2).sum(axis=1)
            E2 = (b / z).astype(np.float64)
            e_mu = (e_a + mu64 * e_z) / z64 + 3 * u * mu64
            e_sig = (e_b + E2 * e_z) / z64 + 3 * u * E2 + 2 * mu64 * e_mu + u * mu64 ** 2 + u * np.maximum(E2, mu64 ** 2)
            # one grid point with weight exactly 1 and an exactly representable square: the variance is 0 in any order
            one = (w64 > 0).sum(axis=1) == 1
            at = np.argmax(w64 > 0, axis=1)
            exact0 = one & ~cav & (w64[np.arange(deg), at] == 1.0) & (x[at] * x[at] == (x[at].astype(np.float64) ** 2).astype(LD))
            # ---- the division by the cavity
            mu_d, sig_d = gaussian_division(mu, sig, c0, c1)
            s64, c164 = np.abs(sig).astype(np.float64), c1.astype(np.float64)
            rel = e_sig / s64 + (3 * u * c164 + e_sig) / np.abs(c1 - sig).astype(np.float64) + 6 * u
            e_sd = np.abs(sig_d).astype(np.float64) * rel
            m_big, c_big = np.abs(mu * (c1 + sig_d)).astype(np.float64), np.abs(c0 * sig_d).astype(np.float64)
            e_c0 = 8 * u * K0
            e_mud = (e_mu * np.abs(c1 + sig_d).astype(np.float64) + mu64 * (3 * u * c164 + e_sd) + e_c0 * np.abs(sig_d).astype(np.float64)
                     + np.abs(c0).astype(np.float64) * e_sd + 3 * u * (m_big + c_big)) / c164 + 5 * u * np.abs(mu_d).astype(np.float64)
            mu, sig = np.where(cav, mu_d, mu), np.where(cav, sig_d, sig)
            e_mu, e_sig = np.where(cav, e_mud, e_mu), np.where(cav, e_sd, e_sig)
            ok = (z > 0) & (sig > 0) & np.isfinite(sig.astype(np.float64))
            for i, e in enumerate(rows):
                if z[i] == 0 or not np.isfinite(z64[i]):
                    why[e] = 'z=0'
                elif not ok[i]:
                    why[e] = 'zero' if exact0[i] else 'negative'
                if z[i] > 0:
                    assert z64[i] > 1e-280, 'a denormal sum of weights'
                    if not exact0[i]:
                        margin['accept'][e] = abs(float(sig[i])) / e_sig[i]
                    if ok[i]:
                        margin['floor'][e] = abs(float(sig[i] - min_sig)) / e_sig[i]
            fl_ = ok & (sig <= min_sig)
            new_mu, new_sig = np.where(ok, mu, b0), np.where(ok, np.maximum(sig, min_sig), b1)
            if mutant == 'overwrite_failed':
                new_mu, new_sig = np.where(ok, mu, LD(0)), np.where(ok, new_sig, min_sig)
            eta[rows, 0], eta[rows, 1] = new_mu, new_sig
            e_mu, e_sig = np.where(ok, e_mu, 0.0), np.where(ok & ~fl_, e_sig, 0.0)
            eta_bound[rows, 0], eta_bound[rows, 1] = e_mu, e_sig
            owned[rows], kept[rows], floored[rows], cavity[rows] = True, ~ok, fl_, cav
            # ---- q
            cc = np.ones(deg, dtype=LD) if mutant == 'no_counts' else c
            ps, pm = (cc / new_sig).sum(), (cc * new_mu / new_sig).sum()
            q[v, 1], q[v, 0] = 1 / ps, pm / ps
            ps_out[v] = ps, pm
            s_, m_, c_ = new_sig.astype(np.float64), np.abs(new_mu).astype(np.float64), c.astype(np.float64)
            ps64 = float(ps)
            e_ps = (c_ * (e_sig / s_ + 4 * u) / s_).sum() + deg * u * ps64
            e_pm = (c_ * ((e_sig / s_ + 5 * u) * m_ + e_mu) / s_).sum() + deg * u * (c_ * m_ / s_).sum()
            q_bound[v, 1] = (e_ps / ps64 + 2 * u) / ps64
            q_bound[v, 0] = abs(float(pm / ps)) * (e_ps / ps64 + 3 * u) + e_pm / ps64
            q_live[v] = True
    return ProposalTwin(eta, eta_bound, owned, kept, why, floored, cavity, q, q_bound, q_live, margin, ps_out)


def ratio(got, want, bound):
    """|got - want| / bound elementwise; 0 where both agree exactly, inf where they differ and the bound is 0 (or got is no number)"""
    with np.errstate(all='ignore'):
        diff = np.abs(np.asarray(got, dtype=LD) - want).astype(np.float64)
        r = np.where(diff == 0, 0.0, diff / bound)
    return np.where(np.isfinite(diff), r, np.inf)


# ---- 50-digit restatements of single values (tests/test_pbp_var_host.py) ----------------------------------------------------------------
def v2f_value_mp(st, e, mp):
    """the balanced message row of edge e at 50 digits, from the definitions, particle by particle"""
    fl = st.flat
    v = int(fl.edge_var[e])
    rows, npv = st.rows(v), int(st.counts[v])
    d = fl.var_dom[v]
    res = []
    for j in range(npv):
        x = st.particles[v, j]
        acc = mp.mpf(0)
        for k in rows:
            cnt = mp.mpf(float(fl.edge_count[k])) if fl.lifted else mp.mpf(1)
            acc += (cnt - 1 if k == e else cnt) * mp.mpf(float(st.f2v[k, j]))
        if fl.dom_cont[d]:
            pen = x == fl.dom_lo[d] or x == fl.dom_hi[d]
        else:
            vals = st.grid(v)
            pen = st.epbp and (x == vals[0] or (vals.size > 1 and x == vals[1]))
        if not fl.dom_cont[d] and not st.epbp:
            w = mp.mpf(1)
        elif pen:
            w = mp.mpf(TINY)
        else:
            sd = mp.sqrt(mp.mpf(float(st.q[v, 1])))
            t = (mp.mpf(float(x)) - mp.mpf(float(st.q[v, 0]))) / sd
            w = 1 / max(mp.exp(-t * t / 2) / (mp.mpf(SQRT_2PI) * sd), mp.mpf(TINY))
        res.append(acc + mp.log(w))
    uq = [r for r, keep in zip(res, st.uniq[v, :npv]) if keep]
    mean, mx = sum(uq) / len(uq), max(uq)
    shift = mx - mp.mpf(st.max_log_value) if mx - mean > st.max_log_value else mean
    return [r - shift for r in res]


def site_mp(st, e, mp):
    """(mu, sig, accepted) of edge e's site before the floor, at 50 digits"""
    fl = st.flat
    v = int(fl.edge_var[e])
    xs = [mp.mpf(float(t)) for t in st.grid(v)]
    msg = st.f2v[e, st.n:st.n + len(xs)]
    q0, q1 = mp.mpf(float(st.q[v, 0])), mp.mpf(float(st.q[v, 1]))
    b0, b1 = mp.mpf(float(st.eta[e, 0])), mp.mpf(float(st.eta[e, 1]))
    cav = st.ep and not q1 >= b1
    if cav:
        c1 = q1 * b1 / (b1 - q1)
        c0 = (q0 * (b1 + c1) - b0 * c1) / b1
        csd = mp.sqrt(c1)
    w = []
    for x, m in zip(xs, msg):
        t = mp.mpf(0) if m <= DEAD else mp.exp(mp.mpf(float(m)))
        if cav:
            t *= mp.exp(-((x - c0) / csd) ** 2 / 2) / (mp.mpf(SQRT_2PI) * csd)
        w.append(t)
    z = sum(w)
    if z == 0:
        return None, None, False
    mu = sum(t * x for t, x in zip(w, xs)) / z
    sig = sum(t * x * x for t, x in zip(w, xs)) / z - mu * mu
    if cav:
        s2 = sig * c1 / (c1 - sig)
        mu, sig = (mu * (c1 + s2) - c0 * s2) / c1, s2
    return mu, sig, sig > 0


# ---- states --------------------------------------------------------------------------------------------------------------------------
def _exact_square_point(grid):
    """a grid point whose square is a double"""
    for t in np.argsort(np.abs(grid))[::-1]:
        x = LD(grid[t])
        if x * x == LD(np.float64(grid[t]) ** 2) and grid[t] != 0:
            return int(t)
    return int(np.argmin(np.abs(grid)))


def var_graph(n, seed):
    """the graph of every family: per (degree, T) a hidden continuous variable -- the degrees of SMALL_DEGREES on every domain of
    T_LIST, those of HUB_DEGREES on HUB_T --, per (degree, states) a hidden discrete one (states <= n), and observed variables of
    every class; each variable owns `degree` unary factors.  Returns (flat, kind per variable)"""
    from lhvi.graph import Domain
    rng = np.random.default_rng(seed)
    doms = [Domain((LO, HI), continuous=True, integral_points=grid_points(T)) for T in T_LIST]
    disc = [k for k in DISCRETE if k <= n]
    doms += [Domain(tuple(float(i) for i in range(k)), continuous=False) for k in disc]
    b = _Builder(doms)
    kinds = []

    def add(dom, deg, value=np.nan):
        v = b.var(dom, value)
        for _ in range(deg):
            if dom < len(T_LIST):
                b.factor((v,), X2, [1.0, float(rng.uniform(2, 10))], 'x2')
            else:
                k = disc[dom - len(T_LIST)]
                b.factor((v,), TABLE, [1, k] + rng.uniform(0.2, 3.0, k).tolist(), 'table')
        kinds.append(('cont' if dom < len(T_LIST) else 'disc') + ('' if np.isnan(value) else ' observed'))
        return v

    for ti, T in enumerate(T_LIST):
        for deg in SMALL_DEGREES + (HUB_DEGREES if T in HUB_T else ()):
            add(ti, deg)
        add(ti, 3, float(rng.uniform(-8, 8)))
    for ki, k in enumerate(disc):
        for deg in DISCRETE_DEGREES:
            add(len(T_LIST) + ki, deg)
        add(len(T_LIST) + ki, 3, float(rng.integers(k)))
    return b.flat(), kinds


MSG_KINDS = ('ordinary', 'peaked', 'flat', 'underflow', 'point', 'floor entries', 'negvar')
ETA_KINDS = ('gt', 'eq', 'lt', 'gt')


def build(n, family='zoo', epbp=True, ep=False, lifted=False, var_threshold=None, var_degree=False, seed=11):
    """a state of `n` particles.  family 'zoo': ordinary rows (|m| <= 5) with the particle rows' spice, the clamp rows and every
    kind of proposal row;  'ranges': the v -> f rows that decide the shift rule (a spread just under / just over max_log_value, FLOOR
    entries, a duplicate that carries the row's maximum);  'init': eta and q as ``pbp_init_kernel`` leaves them.
    `lifted`: multiplicities 1..6 in ``edge_count``; `var_degree`: the count totals handed over instead of summed (+ 2, so that a
    kernel that ignored them would show)."""
    import dataclasses
    from oracle import oracle
    flat, kinds = var_graph(n, seed)
    rng = np.random.default_rng(seed + 7919 * n + (1 if lifted else 0) + (2 if ep else 0) + (4 if epbp else 0))
    if lifted:
        flat = dataclasses.replace(flat, edge_count=rng.integers(1, 7, flat.E).astype(np.float64), lifted=True)
    thr = float(var_threshold if var_threshold is not None else (3 if epbp else 5))
    counts = oracle.pbp_counts(flat, n)
    Tmax = max(T_LIST)
    f2v = rng.uniform(-5, 5, (flat.E, n + Tmax))
    particles = rng.uniform(LO, HI, (flat.V, n))
    q = np.stack([rng.uniform(-3, 3, flat.V), rng.uniform(0.5, 8.0, flat.V)], axis=1)
    eta = np.stack([rng.uniform(-3, 3, flat.E), rng.uniform(0.5, 20.0, flat.E)], axis=1)
    tags = {}
    hidden = np.flatnonzero(flat.var_hidden)
    if not epbp:
        q[~flat.var_cont] = np.nan                 # (HybridLBP keeps no proposal for a discrete variable)
    for v in np.flatnonzero(flat.var_hidden & ~flat.var_cont):
        vals = flat.dom_val[flat.dom_ptr[flat.var_dom[v]]:flat.dom_ptr[flat.var_dom[v] + 1]]
        particles[v, :vals.size] = vals
    total = np.array([flat.edge_count[flat.var_edge[flat.var_ptr[v]:flat.var_ptr[v + 1]]].sum() for v in range(flat.V)])
    # ---- particle rows: both bounds, +-0, duplicates, and a particle far from mu at a small variance (the clamp)
    for i, v in enumerate(np.flatnonzero(flat.var_hidden & flat.var_cont)):
        t = tags.setdefault(int(v), set())
        special = [LO, HI, 0.0, -0.0, None]
        cols = rng.permutation(n)[:len(special) + 1]
        for col, s in zip(cols[1:], special):
            particles[v, col] = particles[v, cols[0]] if s is None else s
        t.add('spice')
        if i % 3 == 0:
            q[v] = rng.uniform(-3, 3), rng.uniform(0.005, 0.02)
            t.add('clamp')
    uniq = first_occurrence(particles, counts).astype(np.uint8)
    rows_of = lambda v: flat.var_edge[flat.var_ptr[v]:flat.var_ptr[v + 1]]
    if family == 'ranges':
        # ---- the rows that decide the shift rule: one row of the variable carries D on one DISTINCT particle, so that every other
        # edge's max - mean is D (1 - 1 / cnt) + ordinary noise: 15 under / 15 over 700; FLOOR entries in some particles; a duplicate
        # particle with +2000 in one row: it is no key of the reference's dictionary and must not drive the shift
        for i, v in enumerate(hidden):
            rows, npv = rows_of(v), int(counts[v])
            t = tags.setdefault(int(v), set())
            uq = np.flatnonzero(uniq[v, :npv])
            if rows.size < 2:
                continue
            kind = ('under', 'over', 'floor entries', 'dup max')[i % 4]
            mult = flat.edge_count[rows[0]]
            if kind in ('under', 'over'):
                D = (700.0 + (-15.0 if kind == 'under' else 15.0)) / (1.0 - 1.0 / uq.size) / mult
                f2v[rows[0], uq[int(rng.integers(uq.size))]] += D
            elif kind == 'floor entries':
                f2v[rows[int(rng.integers(rows.size))], rng.permutation(npv)[:max(1, npv // 3)]] = FLOOR
            else:
                dup = np.flatnonzero(~uniq[v, :npv].astype(bool))
                if dup.size == 0:
                    continue
                f2v[rows[0], dup[0]] = 2000.0
            t.add(kind)
    # ---- proposal rows
    for v in np.flatnonzero(flat.var_hidden & flat.var_cont):
        rows = rows_of(v)
        grid = flat.dom_val[flat.dom_ptr[flat.var_dom[v]]:flat.dom_ptr[flat.var_dom[v] + 1]]
        T = grid.size
        t = tags.setdefault(int(v), set())
        f2v[rows, n + T:] = np.nan                              # beyond the domain's points: read by nothing
        for i, e in enumerate(rows):
            if family == 'init':
                eta[e] = 0.0, 5.0 * total[v]
                if T == 1:
                    f2v[e, n] = DEAD if ep else 0.0          # (one live point under the cavity's weight: a variance of rounding noise)
                continue
            kind = MSG_KINDS[(i + v) % len(MSG_KINDS)]
            ek = ETA_KINDS[(i // len(MSG_KINDS) + v) % len(ETA_KINDS)] if ep else 'lt'
            if T == 1 or kind == 'point' or 'clamp' in t:
                # a single live point is exact only without the cavity's weight; a cavity of variance ~0.01 leaves every weight
                # on a grid of step >= 0.15 denormal
                ek = 'lt' if ek == 'gt' else ek
            eta[e, 1] = q[v, 1] * {'gt': rng.uniform(1.5, 4.0), 'eq': 1.0, 'lt': rng.uniform(0.3, 0.8)}[ek]
            if ek == 'gt':
                eta[e, 0] = q[v, 0] + rng.uniform(-1, 1)          # (the cavity's mean stays within 2 of q's: inside the domain)
            if T == 1:
                f2v[e, n] = DEAD if kind == 'underflow' else 0.0
                kind = 'underflow' if kind == 'underflow' else 'point'
            elif kind == 'peaked':
                f2v[e, n:n + T] = -(grid - rng.uniform(-6, 6)) ** 2 / (2 * rng.uniform(0.3, 1.5))
            elif kind == 'flat':
                f2v[e, n:n + T] = rng.uniform(-0.01, 0.01, T)
            elif kind == 'underflow':
                f2v[e, n:n + T] = DEAD
            elif kind == 'point':
                f2v[e, n:n + T] = DEAD
                f2v[e, n + _exact_square_point(grid)] = 0.0
            elif kind == 'floor entries':
                f2v[e, n + rng.permutation(T)[:max(1, T // 3)]] = FLOOR
            elif kind == 'negvar':
                if ek == 'gt':                                  # a convex message: under the cavity the mass moves to the domain's ends
                    c0, c1 = gaussian_division(q[v, 0], q[v, 1], eta[e, 0], eta[e, 1])
                    f2v[e, n:n + T] = 0.75 * (grid - c0) ** 2 / c1
                else:
                    kind = 'ordinary'
            t.update({kind, 'eta ' + ek})
        if family == 'init':
            q[v] = 0.0, 5.0
            t.add('init')
    if family == 'init' and epbp:
        for v in np.flatnonzero(flat.var_hidden & ~flat.var_cont):
            q[v] = 0.0, 5.0
            eta[rows_of(v)] = 0.0, 5.0 * total[v]
    st = VarState(flat=flat, n=int(n), epbp=epbp, ep=ep, var_threshold=thr, particles=np.ascontiguousarray(particles), uniq=uniq,
                  f2v=np.ascontiguousarray(f2v), q=np.ascontiguousarray(q), eta=np.ascontiguousarray(eta), counts=counts,
                  var_degree=(total + 2.0) if var_degree else None, tags=tags)
    st.kinds = kinds
    check_decisions(st)
    return st


def check_decisions(st):
    """no decision of the twin within MARGIN bounds of its threshold"""
    tw, pr = st.v2f(), st.proposal()
    assert (tw.margin >= MARGIN).all(), ('shift rule', np.flatnonzero(~(tw.margin >= MARGIN))[:5], tw.margin.min())
    for name in ('accept', 'floor', 'cavity'):
        m = pr.margin[name]
        assert (m >= MARGIN).all(), (name, np.flatnonzero(~(m >= MARGIN))[:5], float(np.nanmin(m)))
    return st


def coverage(st):
    """counts of the branches the state's rows reach"""
    fl = st.flat
    tw, pr = st.v2f(), st.proposal()
    hid = st.hidden()
    deg = np.diff(fl.var_ptr)
    cont = st.cont()
    out = {
        'live v2f': int(tw.live.sum()), 'untouched v2f': int((~tw.live).sum()),
        'max rule': int(tw.max_rule.sum()), 'mean rule': int((~tw.max_rule & tw.live.any(axis=1)).sum()),
        'duplicates': int(((st.uniq == 0) & (np.arange(st.n)[None, :] < st.counts[:, None]))[hid].sum()),
        'penalised': int(tw.penalised.sum()), 'clamped': int(tw.clamped.sum()),
        'degrees': sorted(set(deg[hid].tolist())), 'degree 4': int((deg[hid] == 4).sum()), 'degree 5': int((deg[hid] == 5).sum()), 'hub': int((deg[hid] > 64).sum()),
        'kept z=0': pr.why_kept.count('z=0'), 'kept zero': pr.why_kept.count('zero'), 'kept negative': pr.why_kept.count('negative'),
        'floored': int(pr.floored.sum()), 'unfloored': int((pr.owned & ~pr.kept & ~pr.floored).sum()),
        'cavity': int(pr.cavity.sum()), 'no cavity': int((pr.owned & ~pr.cavity).sum()),
        'eta eq': int(sum((st.eta[st.rows(v), 1] == st.q[v, 1]).sum() for v in cont)),
        'sites': int(pr.owned.sum()), 'untouched sites': int((~pr.owned).sum()),
        'T': sorted({int(st.grid(v).size) for v in cont}),
        'counts': sorted(set(fl.edge_count.tolist())) if fl.lifted else [1.0],
    }
    return out
