"""NumPy restatement of ``KL(p || q)`` with ``p`` a scalar Gaussian mixture and ``q`` ANY log density (docs/kernels_pbkl.md:
``lhvi_gm_kl_fn_host`` on the host, ``lhvi_pbp_kl`` with a particle belief on the device), and what its tests share.

``kl_logq`` follows the method of docs/kernels_gmkl.md step by step -- the range and the panels from ``p`` alone, QUADPACK's
21-point Gauss-Kronrod rule on every panel, the bound from their sum, depth-first bisection left to right, the two guards --
and takes ``log_q`` as a function of the 21 points of a rule at once.  It shares no code with the library, and takes nothing
from tests/gmkl_models.py but the row generators."""
import numpy as np

from gmkl_models import FAMILIES, family_rows, rand_gm     # noqa: F401  (the row generators, re-exported for the tests)

RANGE_SD, PANEL_SD, PANEL_CAP, DEPTH_CAP, BISECT_CAP = 10.0, 8.0, 1024, 40, 4096
ST_TOLERANCE, ST_CAP, ST_INVALID = 1, 2, 4
HALF_LOG_2PI = 0.5 * float(np.log(2.0 * np.pi))

# dqk21: the ten positive Kronrod abscissae in ascending order with their weights, the centre weight, and the Gauss weights of
# the five abscissae that are Gauss nodes too (the second, fourth, ... counted from the outside)
_X = np.array([0.148874338981631210884826001129720, 0.294392862701460198131126603103866, 0.433395394129247190799265943165784,
               0.562757134668604683339000099272694, 0.679409568299024406234327365114874, 0.780817726586416897063717578345042,
               0.865063366688984510732096688423493, 0.930157491355708226001207180059508, 0.973906528517171720077964012084452,
               0.995657163025808080735527280689003])
_WK = np.array([0.147739104901338491374841515972068, 0.142775938577060080797094273138717, 0.134709217311473325928054001771707,
                0.123491976262065851077958109585166, 0.109387158802297641899210590325805, 0.093125454583697605535065465083366,
                0.075039674810919952767043140916190, 0.054755896574351996031381300244580, 0.032558162307964727478818972459390,
                0.011694638867371874278064396062192])
_WK0 = 0.149445554002916905664936468389821
_WG = {8: 0.066671344308688137593568809893332, 6: 0.149451349150580593145776339657697, 4: 0.219086362515982043995534934228163,
       2: 0.269266719309996355091226921569469, 0: 0.295524224714752870173815619188769}       # by index into _X
_EPS, _TINY = float(np.finfo(float).eps), float(np.finfo(float).tiny)


def nodes(lo, hi):
    """the 21 points of the rule on [lo, hi], ascending"""
    c, h = 0.5 * (lo + hi), 0.5 * (hi - lo)
    return np.concatenate([c - h * _X[::-1], [c], c + h * _X])


def rule(values, lo, hi):
    """(result, estimate) of dqk21 from the integrand's 21 values at ``nodes(lo, hi)``, the sums in QUADPACK's order: the centre,
    the Gauss pairs from the outside in, then the other Kronrod pairs from the outside in"""
    h = 0.5 * (hi - lo)
    left, mid, right = values[9::-1], float(values[10]), values[11:]          # left[i], right[i]: the pair at -+ _X[i]
    kron, gauss, mag = _WK0 * mid, 0.0, abs(_WK0 * mid)
    for i in (8, 6, 4, 2, 0):
        pair = left[i] + right[i]
        gauss += _WG[i] * pair
        kron += _WK[i] * pair
        mag += _WK[i] * (abs(left[i]) + abs(right[i]))
    for i in (9, 7, 5, 3, 1):
        kron += _WK[i] * (left[i] + right[i])
        mag += _WK[i] * (abs(left[i]) + abs(right[i]))
    mean = 0.5 * kron
    dev = _WK0 * abs(mid - mean)
    for i in range(9, -1, -1):
        dev += _WK[i] * (abs(left[i] - mean) + abs(right[i] - mean))
    mag, dev = mag * abs(h), dev * abs(h)
    est = abs((kron - gauss) * h)
    if dev != 0.0 and est != 0.0:
        est = dev * min(1.0, (200.0 * est / dev) ** 1.5)
    if mag > _TINY / (50.0 * _EPS):
        est = max(50.0 * _EPS * mag, est)
    return float(kron * h), float(est)


def log_p(x, w, mu, var):
    """log density of the mixture at the points x; components of weight 0 are left out"""
    on = w > 0
    w, mu, var = w[on], mu[on], var[on]
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))[:, None]
    terms = np.log(w) - HALF_LOG_2PI - 0.5 * np.log(var) - (x - mu) ** 2 / (2.0 * var)
    top = terms.max(axis=1)
    with np.errstate(invalid='ignore', divide='ignore'):
        out = top + np.log(np.exp(terms - top[:, None]).sum(axis=1))
    return np.where(np.isneginf(top), -np.inf, out)


def panels(p, a, b):
    """(L, U, P, capped): the range and the panel count of the row; P = 0: nothing to integrate"""
    w, mu, var = p
    sd = np.sqrt(var[w > 0])
    m = mu[w > 0]
    L, U = max(a, float(np.min(m - RANGE_SD * sd))), min(b, float(np.max(m + RANGE_SD * sd)))
    if not U > L:
        return L, U, 0, False
    want = float(np.ceil((U - L) / (PANEL_SD * float(sd.min()))))
    return L, U, int(min(max(want, 1.0), PANEL_CAP)), want > PANEL_CAP


def p_invalid(p):
    w, mu, var = p
    ok = np.isfinite(w).all() and np.isfinite(mu).all() and np.isfinite(var).all() and (var > 0).all() and (w >= 0).all() and (w > 0).any()
    return not ok


def kl_logq(p, log_q, a=-np.inf, b=np.inf, epsabs=1.49e-8, epsrel=1.49e-8, stats=None):
    """(kl, abserr, status, neval) of one row: p = (w, mu, var) [K]; ``log_q(x)`` takes the 21 points of a rule and returns
    their log densities.  ``stats`` (a dict) receives the panel count ``P`` and the deepest accepted interval ``depth``."""
    p = tuple(np.asarray(t, dtype=np.float64) for t in p)
    if p_invalid(p) or np.isnan(a) or np.isnan(b):
        return np.nan, np.nan, ST_INVALID, 0
    L, U, P, capped = panels(p, a, b)
    if stats is not None:
        stats.update(P=P, depth=0)
    if P == 0:
        return 0.0, 0.0, 0, 0

    def on(lo, hi):
        x = nodes(lo, hi)
        lp, lq = log_p(x, *p), np.asarray(log_q(x), dtype=np.float64)
        dens = np.exp(lp)
        with np.errstate(invalid='ignore', over='ignore'):
            return rule(np.where(dens == 0.0, 0.0, dens * (lp - lq)), lo, hi)
    width = (U - L) / P
    cut = [L + i * width for i in range(P)] + [U]
    with np.errstate(invalid='ignore', over='ignore'):
        first = [on(cut[i], cut[i + 1]) for i in range(P)]
        area = 0.0
        for res, _ in first:
            area += res
        bound = max(epsabs, epsrel * abs(area))
        total = esum = 0.0
        status, neval, splits, deepest = (ST_CAP if capped else 0), 21 * P, 0, 0
        for i in range(P):
            todo = [(cut[i], cut[i + 1], first[i], 0)]
            while todo:
                lo, hi, (res, est), depth = todo.pop()
                met = bool(np.isfinite(est) and est <= bound * ((hi - lo) / (U - L)))      # (a non-finite estimate meets nothing)
                if met or depth >= DEPTH_CAP or splits >= BISECT_CAP or not np.isfinite(est):       # the two guards
                    status |= 0 if met else ST_TOLERANCE
                    total, esum, deepest = total + res, esum + est, max(deepest, depth)
                    continue
                mid = 0.5 * (lo + hi)
                halves = on(lo, mid), on(mid, hi)
                splits, neval = splits + 1, neval + 42
                todo.append((mid, hi, halves[1], depth + 1))
                todo.append((lo, mid, halves[0], depth + 1))
    if stats is not None:
        stats['depth'] = deepest
    return total, esum, status, neval


def kl_logq_rows(p, log_q, a=-np.inf, b=np.inf, **kw):
    """``kl_logq`` over the rows of padded [R, K] arrays; ``log_q(x, r)`` is row r's vectorised log density"""
    R = p[1].shape[0]
    a, b = np.broadcast_to(a, (R,)), np.broadcast_to(b, (R,))
    out = [kl_logq(tuple(t[r] for t in p), lambda x, r=r: log_q(x, r), float(a[r]), float(b[r]), **kw) for r in range(R)]
    kl, err, st, ne = zip(*out)
    return np.array(kl), np.array(err), np.array(st, dtype=np.int32), np.array(ne, dtype=np.int32)


# ---- log densities that are no mixtures (T2) -----------------------------------------------------------------------------------------
def laplace(loc, scale):
    return lambda x: -np.abs(np.asarray(x, dtype=np.float64) - loc) / scale - np.log(2.0 * scale)


def student_t3(loc, scale):
    """Student's t with 3 degrees of freedom: density 2 / (pi sqrt(3) s (1 + u^2 / 3)^2), u = (x - loc) / s"""
    c = np.log(2.0) - np.log(np.pi) - 0.5 * np.log(3.0) - np.log(scale)
    return lambda x: c - 2.0 * np.log1p(((np.asarray(x, dtype=np.float64) - loc) / scale) ** 2 / 3.0)


def rippled_normal(loc, sd, amp, freq):
    """a Gaussian log density plus a bounded ripple (not normalised: a constant offset of log q shifts the KL by that constant
    and changes nothing in how hard the integrand is)"""
    return lambda x: (-0.5 * ((np.asarray(x, dtype=np.float64) - loc) / sd) ** 2 - np.log(sd) - HALF_LOG_2PI
                      + amp * np.sin(freq * np.asarray(x, dtype=np.float64)))
