"""NumPy restatement of the mixture KL of docs/kernels_gmkl.md (``lhvi_gm_kl``), and the generators its tests share.

``kl_twin`` follows the method step by step -- range, panels, QUADPACK's 21-point Gauss-Kronrod rule on every panel, the bound
from their sum, depth-first bisection left to right -- with the log densities formed by NumPy's own log-sum-exp, so it shares
no code with ``csrc/gmkl.hpp``."""
import numpy as np

Z_RANGE, C_PANEL, MAX_PANELS, MAX_DEPTH, MAX_BISECT = 10.0, 8.0, 1024, 40, 4096
LOG_2PI = float(np.log(2 * np.pi))

# QUADPACK dqk21: abscissae and Kronrod weights by magnitude (outermost first, the centre last), Gauss weights of the odd ones
XGK = np.array([0.995657163025808080735527280689003, 0.973906528517171720077964012084452, 0.930157491355708226001207180059508,
                0.865063366688984510732096688423493, 0.780817726586416897063717578345042, 0.679409568299024406234327365114874,
                0.562757134668604683339000099272694, 0.433395394129247190799265943165784, 0.294392862701460198131126603103866,
                0.148874338981631210884826001129720, 0.0])
WGK = np.array([0.011694638867371874278064396062192, 0.032558162307964727478818972459390, 0.054755896574351996031381300244580,
                0.075039674810919952767043140916190, 0.093125454583697605535065465083366, 0.109387158802297641899210590325805,
                0.123491976262065851077958109585166, 0.134709217311473325928054001771707, 0.142775938577060080797094273138717,
                0.147739104901338491374841515972068, 0.149445554002916905664936468389821])
WG = np.array([0.066671344308688137593568809893332, 0.149451349150580593145776339657697, 0.219086362515982043995534934228163,
               0.269266719309996355091226921569469, 0.295524224714752870173815619188769])
EPMACH, UFLOW = 2.220446049250313e-16, 2.2250738585072014e-308

FAMILIES = {'mild': (3.0, 0.25, 4.0), 'wide': (10.0, 0.05, 9.0), 'narrow': (8.0, 1e-3, 1.0)}      # spread, vlo, vhi


def rand_gm(rng, K, spread, vlo, vhi):
    w = rng.dirichlet(2.0 * np.ones(K))
    mu = rng.uniform(-spread, spread, K)
    var = np.exp(rng.uniform(np.log(vlo), np.log(vhi), K))
    return w, mu, var


def family_rows(family, n, seed, kmax=5):
    """n rows of the family as padded arrays: (wp, mup, varp [n, kmax], wq, muq, varq [n, kmax]); K of each side in 1 .. kmax,
    the padding has weight 0, mean 0 and variance 1"""
    rng = np.random.default_rng(seed)
    out = [np.zeros((n, kmax)), np.zeros((n, kmax)), np.ones((n, kmax)), np.zeros((n, kmax)), np.zeros((n, kmax)), np.ones((n, kmax))]
    for r in range(n):
        for s in (0, 3):
            K = int(rng.integers(1, kmax + 1))
            w, mu, var = rand_gm(rng, K, *FAMILIES[family])
            out[s][r, :K], out[s + 1][r, :K], out[s + 2][r, :K] = w, mu, var
    return out


def normal_pairs(n, seed):
    """(m1, sd1, m2, sd2) [n]: m ~ U(-10, 10), sd log-uniform in [0.03, 3]; row 0 is the pair plain adaptive quadrature misses"""
    rng = np.random.default_rng(seed)
    m1, m2 = rng.uniform(-10, 10, n), rng.uniform(-10, 10, n)
    s1, s2 = (np.exp(rng.uniform(np.log(0.03), np.log(3.0), n)) for _ in range(2))
    m1[0], s1[0], m2[0], s2[0] = 5.2134, np.sqrt(0.0041), 3.1414, np.sqrt(0.0018)
    return m1, s1, m2, s2


def log_mixture(x, w, mu, var):
    """log sum_k w_k N(x; mu_k, var_k) at the points x [n]; components of weight 0 are left out"""
    keep = w != 0
    w, mu, var = w[keep], mu[keep], var[keep]
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    t = np.log(w) - 0.5 * (LOG_2PI + np.log(var)) - 0.5 * (x[:, None] - mu) ** 2 / var
    m = t.max(axis=1)
    with np.errstate(invalid='ignore', divide='ignore'):
        out = m + np.log(np.exp(t - m[:, None]).sum(axis=1))
    return np.where(m == -np.inf, -np.inf, out)


def integrand(x, p, q):
    lp, lq = log_mixture(x, *p), log_mixture(x, *q)
    ep = np.exp(lp)
    with np.errstate(invalid='ignore'):
        return np.where(ep == 0.0, 0.0, ep * (lp - lq))


def gk21(f, a, b):
    """(result, abserr) of dqk21 on [a, b]; f takes the 21 points at once"""
    centr, hlgth = 0.5 * (a + b), 0.5 * (b - a)
    absc = hlgth * XGK[:10]
    fv = f(np.concatenate([centr - absc, [centr], centr + absc]))
    fc, f1, f2 = float(fv[10]), fv[:10], fv[11:]
    resk = WGK[10] * fc
    resabs, resg = abs(resk), 0.0
    for j in range(5):
        k = 2 * j + 1
        resg += WG[j] * (f1[k] + f2[k])
        resk += WGK[k] * (f1[k] + f2[k])
        resabs += WGK[k] * (abs(f1[k]) + abs(f2[k]))
    for j in range(5):
        k = 2 * j
        resk += WGK[k] * (f1[k] + f2[k])
        resabs += WGK[k] * (abs(f1[k]) + abs(f2[k]))
    reskh = resk * 0.5
    resasc = WGK[10] * abs(fc - reskh)
    for k in range(10):
        resasc += WGK[k] * (abs(f1[k] - reskh) + abs(f2[k] - reskh))
    result, resabs, resasc = resk * hlgth, resabs * abs(hlgth), resasc * abs(hlgth)
    abserr = abs((resk - resg) * hlgth)
    if resasc != 0.0 and abserr != 0.0:
        abserr = resasc * min(1.0, (200.0 * abserr / resasc) ** 1.5)
    if resabs > UFLOW / (50.0 * EPMACH):
        abserr = max((EPMACH * 50.0) * resabs, abserr)
    return float(result), float(abserr)


def plan(p, a, b):
    """(L, U, P, capped) of the row; P = 0 when there is nothing to integrate"""
    w, mu, var = p
    keep = w > 0
    sd = np.sqrt(var[keep])
    L = max(a, float((mu[keep] - Z_RANGE * sd).min()))
    U = min(b, float((mu[keep] + Z_RANGE * sd).max()))
    if not U > L:
        return L, U, 0, False
    want = np.ceil((U - L) / (C_PANEL * float(sd.min())))
    return L, U, int(min(max(want, 1.0), MAX_PANELS)), bool(want > MAX_PANELS)


def kl_twin(p, q, a=-np.inf, b=np.inf, epsabs=1.49e-8, epsrel=1.49e-8, stats=None):
    """(kl, abserr, status, neval) of one row; p, q = (w, mu, var) [K].  ``stats``: a dict that receives the panel count ``P``
    and the deepest accepted interval ``depth``"""
    p, q = tuple(np.asarray(t, dtype=np.float64) for t in p), tuple(np.asarray(t, dtype=np.float64) for t in q)
    for w, mu, var in (p, q):
        if not (np.isfinite(w).all() and np.isfinite(mu).all() and np.isfinite(var).all() and (var > 0).all() and (w >= 0).all()
                and (w > 0).any()):
            return np.nan, np.nan, 4, 0
    if np.isnan(a) or np.isnan(b):
        return np.nan, np.nan, 4, 0
    L, U, P, capped = plan(p, a, b)
    if P == 0:
        return 0.0, 0.0, 0, 0
    f = lambda x: integrand(x, p, q)                # noqa: E731
    h = (U - L) / P
    edge = lambda i: U if i >= P else L + i * h     # noqa: E731
    first = [gk21(f, edge(i), edge(i + 1)) for i in range(P)]
    area0 = 0.0
    for res, _ in first:
        area0 += res
    bound = max(epsabs, epsrel * abs(area0))
    total, esum, status, neval, nbis, deepest = 0.0, 0.0, 2 if capped else 0, 21 * P, 0, 0
    for i in range(P):
        stack = [(edge(i), edge(i + 1), first[i][0], first[i][1], 0)]
        while stack:
            lo, hi, res, err, depth = stack.pop()
            ok = err <= bound * ((hi - lo) / (U - L))
            if ok or depth >= MAX_DEPTH or nbis >= MAX_BISECT or not np.isfinite(err):
                if not ok:
                    status |= 1
                total += res
                esum += err
                deepest = max(deepest, depth)
                continue
            mid = 0.5 * (lo + hi)
            left, right = gk21(f, lo, mid), gk21(f, mid, hi)
            nbis, neval = nbis + 1, neval + 42
            stack.append((mid, hi, right[0], right[1], depth + 1))
            stack.append((lo, mid, left[0], left[1], depth + 1))
    if stats is not None:
        stats.update(P=P, depth=deepest)
    return total, esum, status, neval


def kl_twin_rows(p, q, a, b, **kw):
    """kl_twin over the rows of padded [R, K] arrays: (kl, abserr, status, neval) [R]"""
    R = p[1].shape[0]
    a, b = np.broadcast_to(a, (R,)), np.broadcast_to(b, (R,))
    out = [kl_twin(tuple(t[r] for t in p), tuple(t[r] for t in q), float(a[r]), float(b[r]), **kw) for r in range(R)]
    kl, err, st, ne = zip(*out)
    return np.array(kl), np.array(err), np.array(st, dtype=np.int32), np.array(ne, dtype=np.int32)
