"""Evaluation helpers kept for API parity with the reference's ``utils.py`` (host-side, not on the hot path)."""
from math import log

import numpy as np


def log_likelihood(g, assignment):
    """negative log of the unnormalised joint at `assignment` (``utils.py:6-15``)"""
    from .flat import ground_order
    res = 0
    for f in ground_order(g.factors):        # (a set in the reference: creation order here, so the sum does not change from process to process)
        value = f.potential.get([assignment[rv] for rv in f.nb])
        if value == 0:
            return -np.inf
        res += log(value)
    return -res


def KL(q, p, domain):
    """``utils.KL`` (utils.py:18-31): sum over the domain's integral points (or states) of qx log(qx / px) with
    qx = q(x) w + 1e-8, px = p(x) w + 1e-8, w = the grid spacing (1 for a discrete domain)"""
    if domain.continuous:
        pts = domain.integral_points
        w = (domain.values[1] - domain.values[0]) / (len(pts) - 1)
    else:
        pts, w = domain.values, 1
    total = 0
    for x in pts:
        qx, px = q(x) * w + 1e-8, p(x) * w + 1e-8
        total += qx * np.log(qx / px)
    return total


def softmax(a, axis=None):
    """``osi/utils.py:21-34``: exp(a) / sum exp(a) along ``axis`` through scipy's logsumexp"""
    from scipy.special import logsumexp
    lse = logsumexp(a, axis=axis)
    if axis is not None:
        lse = np.expand_dims(lse, axis)
    return np.exp(a - lse)


def get_scalar_gm_mode(w, mu, var, bds, best_log_pdf=False, host=False):
    """``osi/utils.py:66-98`` on the device: the mode of the scalar Gaussian mixture (w, mu, var) inside ``bds`` = (lb, ub), and
    its log density with ``best_log_pdf``.  A safeguarded Newton iteration from every component mean instead of one bounded
    ``scipy.optimize.minimize`` per mean (``lhvi_mix_marginal_map``, docs/kernels_mixture.md): a deviation in method, not in
    result.  ``lhvi.mixture.MixtureBelief.marginal_map_all`` is the batched form."""
    from .mixture import MixtureBelief
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    belief = MixtureBelief(w, np.asarray(mu, dtype=np.float64).reshape(1, -1), np.asarray(var, dtype=np.float64).reshape(1, -1),
                           bds=np.asarray(bds, dtype=np.float64).reshape(2, 1))
    x, f = belief.map_weights(w, [0], host=host)
    return (float(x[0]), float(f[0])) if best_log_pdf else float(x[0])


def get_multivar_gm_mode(log_w, Mu, Var, bds, init_xs=None, diagonal_cov=True, best_log_pdf=False, grad_lr=0.01, grad_its=500,
                         tol=1e-7, host=False):
    """``osi/utils.py:101-161`` on the device: the approximate mode of a Gaussian mixture with diagonal covariances (``Mu``, ``Var``
    [N, K], log weights ``log_w``, ``bds`` [2, N]) by projected gradient ascent with Polyak averaging from each of ``init_xs``
    [M, N] (default: the K component means), the best one kept, with its log density under ``best_log_pdf``
    (``lhvi_mix_joint_map`` without discrete rows and one coordinate iteration, docs/kernels_mixture.md)."""
    from .mixture import MixtureBelief
    assert diagonal_cov, 'Currently assume diagonal covariance matrices!!!'
    log_w = np.asarray(log_w, dtype=np.float64).reshape(-1)
    belief = MixtureBelief(np.full(log_w.size, 1.0 / log_w.size), Mu, Var, bds=bds)
    r = belief.joint_map(log_w=log_w, init_xs=init_xs, coord_its=1, grad_lr=grad_lr, grad_its=grad_its, tol=tol, host=host)
    return (r['xc'], float(np.max(r['objs']))) if best_log_pdf else r['xc']


def kl_discrete(p, q):
    """KL(p || q) of two probability tables of the same shape (utils.py:34-44)"""
    return np.sum(p * (np.log(p) - np.log(q)))


def _quad(integrand, a, b, args, kwargs):
    from scipy.integrate import quad
    res = quad(integrand, a, b, *args, **kwargs)
    return res if kwargs.get('full_result') else res[0]


def kl_continuous_no_add_const(p, q, a, b, *args, **kwargs):
    """KL(p || q) on [a, b] by adaptive quadrature, integrand log(p^p) - log(q^p) (utils.py:47-67)"""
    def integrand(x):
        px, qx = p(x), q(x)
        return log(px ** px) - log(qx ** px)
    return _quad(integrand, a, b, args, kwargs)


def kl_continuous(p, q, a, b, *args, **kwargs):
    """KL(p || q) on [a, b] by adaptive quadrature; both densities are offset by 1e-100 (utils.py:70-89)"""
    def integrand(x):
        px, qx = p(x) + 1e-100, q(x) + 1e-100
        return px * (log(px) - log(qx))
    return _quad(integrand, a, b, args, kwargs)


def kl_continuous_logpdf(log_p, log_q, a, b, *args, **kwargs):
    """KL(p || q) on [a, b] from the log densities (utils.py:92-113)"""
    from math import exp

    def integrand(x):
        lp = log_p(x)
        return exp(lp) * (lp - log_q(x))
    return _quad(integrand, a, b, args, kwargs)


def kl_normal(mu1, mu2, sig1, sig2):
    """KL(N(mu1, sig1^2) || N(mu2, sig2^2)) -- argument order of the reference (utils.py:116-128)"""
    return log(sig2) - log(sig1) + (sig1 ** 2 + (mu1 - mu2) ** 2) / (2 * sig2 ** 2) - 0.5


def kl_tables(p, q, a, b):
    """Batched ``kl_continuous`` on tabulated densities: ``p``, ``q`` are (V, m) device
    tensors (or arrays) of the two densities of every variable on its own uniform m-point grid over [a[v], b[v]] -- e.g.
    two solvers' ``belief_all`` on the same query grid -- and the result is the (V,) tensor of trapezoid sums of
    (p + 1e-100) (log(p + 1e-100) - log(q + 1e-100)), the integrand of ``kl_continuous``."""
    from . import _abi
    torch = _abi.require_gpu()

    def dev(t):
        return t if torch.is_tensor(t) else _abi.to_dev(np.ascontiguousarray(t, dtype=np.float64))
    p, q = dev(p), dev(q)
    a = dev(np.broadcast_to(np.asarray(a, dtype=np.float64), (p.shape[0],)).copy()) if not torch.is_tensor(a) else a
    b = dev(np.broadcast_to(np.asarray(b, dtype=np.float64), (p.shape[0],)).copy()) if not torch.is_tensor(b) else b
    pp, qq = p + 1e-100, q + 1e-100
    f = pp * (torch.log(pp) - torch.log(qq))
    h = (b - a) / (p.shape[1] - 1)
    return (f[:, 1:] + f[:, :-1]).sum(dim=1) * h * 0.5


def log_likelihood_flat(dg, x):
    """``log_likelihood`` of the assignment ``x`` (array of length V, variable-index order) on a device-resident graph
    (``_abi.DeviceGraph``): one thread per factor, two-stage reduction (``lhvi_log_likelihood``)."""
    from . import _abi
    torch = _abi.require_gpu()
    l = _abi.lib()
    xd = x if torch.is_tensor(x) else _abi.to_dev(np.ascontiguousarray(x, dtype=np.float64))
    nbytes = int(l.lhvi_log_likelihood_workspace_bytes(dg.g))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dg.device)
    out = torch.empty(1, dtype=torch.float64, device=dg.device)
    _abi.check(l.lhvi_log_likelihood(dg.g, dg.p, _abi.ptr(xd), _abi.ptr(out), _abi.ptr(ws), nbytes, _abi.stream_ptr()))
    return float(out.item())


def eval_joint_assignment_energy(factors, rvs2vals):
    """``osi/utils.py:164-169``: the sum of ``factor.log_potential_fun`` over the factors at the assignment ``rvs2vals``
    ({rv: value}; a discrete variable of a LogTable / LogHybridQuadratic by its state index, as the reference passes it).  Pure
    host code for any ``log_potential_fun``; the batched form on the exact baseline's model is
    ``ExactHybridGaussian.energy`` (``lhvi/hg_energy.py``)."""
    energy = 0
    for f in factors:           # in factor order, like the reference's loop
        energy = energy + f.log_potential_fun([rvs2vals[rv] for rv in f.nb])
    return energy


def set_log_potential_funs(factors, skip_existing=True):
    """``osi/utils.py:188-205``: set ``factor.log_potential_fun`` from ``factor.potential.to_log_potential()``, one object per
    distinct potential (the potentials' own hash / eq), skipping a group whose factors all have one unless told otherwise"""
    groups = {}
    for f in factors:
        groups.setdefault(f.potential, []).append(f)
    for pot, like in groups.items():
        if skip_existing and all(f.log_potential_fun is not None for f in like):
            continue
        lp = pot.to_log_potential()
        for f in like:
            f.log_potential_fun = lp


def set_nbrs_idx_in_factors(factors, Vd_idx, Vc_idx):
    """``osi/utils.py:417-429``: ``factor.disc_nb_idx / cont_nb_idx`` = positions of the factor's discrete / continuous
    neighbours in Vd / Vc, in scope order"""
    for f in factors:
        f.disc_nb_idx = tuple(Vd_idx[rv] for rv in f.nb if rv.domain_type[0] == 'd')
        f.cont_nb_idx = tuple(Vc_idx[rv] for rv in f.nb if rv.domain_type[0] == 'c')


def get_conditional_quadratic(A, b, c, obs_args_vals):
    """``osi/utils.py:249-276``: the quadratic over the remaining arguments x of [x y]'A[x y] + b'[x y] + c with the arguments
    ``obs_args_vals`` = {index: value} fixed: (A_xx, A_xy y + A_yx' y + b_x, y'A_yy y + b_y'y + c)"""
    A, b = np.asarray(A, dtype=np.float64), np.asarray(b, dtype=np.float64)
    yi = np.array(list(obs_args_vals.keys()), dtype=int)
    y = np.array([obs_args_vals[i] for i in yi], dtype=np.float64)
    xi = np.setdiff1d(np.arange(len(b)), yi)
    b_cond = A[np.ix_(xi, yi)] @ y + A[np.ix_(yi, xi)].T @ y + b[xi]
    c_cond = np.dot(y, A[np.ix_(yi, yi)] @ y) + np.dot(b[yi], y) + c
    return A[np.ix_(xi, xi)], b_cond, c_cond


def get_conditional_gaussian(mu, Sig, obs_args_vals):
    """``osi/utils.py:279-303``: mean and covariance of p(x_a | x_b) from the joint (mu, Sig) with x_b = ``obs_args_vals``
    {index: value} (PRML 2.81, 2.82)"""
    mu, Sig = np.asarray(mu, dtype=np.float64), np.asarray(Sig, dtype=np.float64)
    bi = np.array(list(obs_args_vals.keys()), dtype=int)
    bv = np.array([obs_args_vals[i] for i in bi], dtype=np.float64)
    ai = np.setdiff1d(np.arange(len(mu)), bi)
    Sbb_inv = np.linalg.inv(Sig[np.ix_(bi, bi)])
    Sab = Sig[np.ix_(ai, bi)]
    return mu[ai] + Sab @ (Sbb_inv @ (bv - mu[bi])), Sig[np.ix_(ai, ai)] - Sab @ Sbb_inv @ Sab.T


def _quadratic_family():
    from .potentials import GaussianPotential, LinearGaussianPotential, QuadraticPotential, X2Potential, XYPotential
    return (QuadraticPotential, GaussianPotential, LinearGaussianPotential, X2Potential, XYPotential)


def condition_factors_on_evidence(factors, evidence):
    """``osi/utils.py:306-361`` for the quadratic family: a new list of factors reduced to the context of ``evidence`` {rv: value}
    (the given factors are not modified).  A partly observed factor becomes a ``QuadraticPotential`` over its remaining
    arguments (``get_conditional_quadratic``), a fully observed one a constant ``log_potential_fun`` with ``potential`` None.
    An MLN or generic potential that the evidence touches raises ``NotImplementedError``."""
    from copy import copy
    from .potentials import QuadraticPotential
    out = []
    for factor in factors:
        if not any(rv in evidence for rv in factor.nb):
            out.append(factor)
            continue
        partial = {i: evidence[rv] for i, rv in enumerate(factor.nb) if rv in evidence}
        f = copy(factor)
        f.uncond_factor = factor
        f.nb = [rv for rv in factor.nb if rv not in evidence]
        potential = factor.potential
        if not f.nb:
            f.potential = None
            f.log_potential_fun = (lambda fac: lambda x: fac.log_potential_fun([evidence[rv] for rv in fac.nb]))(factor)
        elif isinstance(potential, _quadratic_family()):
            pot = QuadraticPotential(*get_conditional_quadratic(*potential.get_quadratic_params(), partial))
            if hasattr(potential, 'symmetric'):
                pot.symmetric = potential.symmetric
            f.potential = pot
            f.log_potential_fun = pot.to_log_potential()
        else:
            raise NotImplementedError('%s: conditioning a %s on evidence is not supported (quadratic family only)'
                                      % (factor, type(potential).__name__))
        out.append(f)
    return out


def get_conditional_mrf(factors, rvs, evidence, update_rv_nbs=False):
    """``osi/utils.py:432-455``: a ``Graph`` of the unobserved rvs and the conditioned, non-empty factors.  The rv objects are
    shared with the caller's graph; ``update_rv_nbs`` runs ``init_nb`` on the result (which rewrites their ``nb``)."""
    from .graph import Graph
    cond = [f for f in condition_factors_on_evidence(factors, evidence) if len(f.nb) > 0]
    g = Graph()
    g.rvs = [rv for rv in rvs if rv not in evidence]
    g.factors = cond
    if update_rv_nbs:
        g.init_nb()
    return g


def get_joint_quadratic_params(factor_params, factor_scopes, N=None):
    """``osi/utils.py:458-488``: (A, b, c) of x'Ax + b'x + c from quadratic factors [(A1, b1, c1), ...] over the index tuples
    ``factor_scopes``, summed in the reference's factor, i, j order"""
    flat = np.array([i for scope in factor_scopes for i in scope], dtype=int)
    assert np.all(flat >= 0)
    if N is None:
        N = int(flat.max()) + 1
    A, b, c = np.zeros([N, N], dtype='float'), np.zeros(N, dtype='float'), 0
    for (A_, b_, c_), scope in zip(factor_params, factor_scopes):
        n = len(scope)
        for i in range(n):
            for j in range(n):
                A[scope[i], scope[j]] += A_[i, j]
            b[scope[i]] += b_[i]
        c += c_
    return A, b, c


def get_quadratic_params_from_factor_graph(factors, rvs_list):
    """``osi/utils.py:491-522``: ((A, b, c), rvs_idx) of the joint quadratic of exp-quadratic factors; a factor's
    ``log_potential_fun`` (a ``LogQuadratic``) is read when set, else its potential's ``get_quadratic_params``"""
    from .potentials import LogQuadratic
    rvs_idx = {rv: i for i, rv in enumerate(rvs_list)}
    params, scopes = [], []
    for factor in factors:
        lp = getattr(factor, 'log_potential_fun', None)
        if lp is not None:
            assert isinstance(lp, LogQuadratic)
            params.append((np.asarray(lp.A), np.asarray(lp.b), lp.c))
        else:
            assert isinstance(factor.potential, _quadratic_family())
            params.append(factor.potential.get_quadratic_params())
        scopes.append(tuple(rvs_idx[rv] for rv in factor.nb))
    return get_joint_quadratic_params(params, scopes, len(rvs_list)), rvs_idx


def get_prec_mat_from_gaussian_mrf(factors, rvs_list):
    """``osi/utils.py:544-564``: (precision matrix, rvs_idx) of a Gaussian MRF of ``GaussianPotential`` factors"""
    from .potentials import GaussianPotential
    rvs_idx = {rv: i for i, rv in enumerate(rvs_list)}
    prec = np.zeros([len(rvs_list), len(rvs_list)], dtype='float')
    for factor in factors:
        assert isinstance(factor.potential, GaussianPotential)
        J = np.linalg.inv(factor.potential.sig)
        pos = [rvs_idx[rv] for rv in factor.nb]
        for i in range(len(pos)):
            for j in range(len(pos)):
                prec[pos[i], pos[j]] += J[i, j]
    return prec, rvs_idx


def get_gaussian_mean_params_from_quadratic_params(A, b, mu_only=True):
    """``osi/utils.py:525-541`` on the device: mu (and Sig unless ``mu_only``) with -1/2 (x - mu)' Sig^-1 (x - mu) = x'Ax + b'x +
    const.  ``A``, ``b``: arrays or device tensors (the results are of the same kind).  A blocked fp64 Cholesky of
    J = -(A + A^T) (csrc/gauss_exact.hip) instead of ``np.linalg.solve`` / ``inv``; a J that is not positive definite raises
    ``ValueError``; without a GPU the call raises ``LhviError``."""
    from . import gauss_exact
    return gauss_exact.mean_params_from_quadratic(A, b, mu_only)
