"""Record the reference's exact hybrid-Gaussian baseline as fixtures (tests/golden/exact_*.npz, data only).

Imports the reference's gibbs/hybrid_gaussian_mrf.py (path given by --reference; path order osi/, gibbs/, root, so that its
`import utils` is osi/utils.py) and runs convert_to_bn, get_drv_marg, get_rv_marg_map_from_bn_params and
utils.get_scalar_gm_log_prob over the models of tests/exact_models.py built from the reference's own classes.

Per model: table, logZ, means, variances, the lower triangle of the covariances (every configuration, or the seeded sample of
rand_12_16, without covariances), every discrete marginal, marginal MAPs, log densities at the query points, and max cond(J).  It ASSERTS
cond(J) <= 500 and that every recorded continuous marginal MAP is interior to its bounds and unique (the best optimum of
another mode is lower in log density by more than 1e-6); a model that fails is to be regenerated with another seed.

rand_8_8_ev (evidence): the reference's condition_factors_on_evidence turns a table or hybrid factor into a plain function,
which its convert_to_bn cannot read, so the conditional model is derived from the unconditioned network instead:
p(x_d') ~ p(x_d', x_d^obs) N(x_c^obs; mu, Sig) and utils.get_conditional_gaussian per configuration.

Usage: python scripts/capture_exact.py --reference PATH [--only NAME] [--maps-12-16 N]
"""
import argparse
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def reference_ns(path):
    sys.path[:0] = [os.path.join(path, 'osi'), os.path.join(path, 'gibbs'), path]
    import Graph
    import MLNPotential
    import Potential
    import hybrid_gaussian_mrf as hgm
    import utils
    ns = types.SimpleNamespace(
        F=Graph.F, RV=Graph.RV, Domain=Graph.Domain, LogTable=Potential.LogTable, LogQuadratic=Potential.LogQuadratic,
        LogHybridQuadratic=Potential.LogHybridQuadratic, TablePotential=Potential.TablePotential,
        QuadraticPotential=Potential.QuadraticPotential, HybridQuadraticPotential=Potential.HybridQuadraticPotential,
        MLNPotential=MLNPotential.MLNPotential, eq_op=MLNPotential.eq_op, and_op=MLNPotential.and_op)
    return ns, hgm, utils


def tril(covs):
    n = covs.shape[-1]
    i, j = np.tril_indices(n)
    return covs[..., i, j]


def marginal_map(hgm, utils, bn, Vd_idx, Vc_idx, rv):
    """get_rv_marg_map_from_bn_params plus, for a continuous variable, the log density there and the checks on the optimum"""
    if rv in Vd_idx:
        return float(hgm.get_rv_marg_map_from_bn_params(*bn, Vd_idx, Vc_idx, rv)), np.nan
    import scipy.optimize as so
    runs, orig = [], so.minimize

    def recording(*a, **kw):
        r = orig(*a, **kw)
        runs.append((float(np.ravel(r.x)[0]), float(r.fun)))
        return r
    so.minimize = recording
    try:
        x = float(hgm.get_rv_marg_map_from_bn_params(*bn, Vd_idx, Vc_idx, rv))
    finally:
        so.minimize = orig
    xs, fs = np.array([r[0] for r in runs]), np.array([r[1] for r in runs])
    best = fs.min()
    lo, hi = float(rv.values[0]), float(rv.values[1])
    assert lo + 1e-3 < x < hi - 1e-3, ('marginal MAP on the bounds', x)
    other = fs[np.abs(xs - x) > 1e-3]
    assert other.size == 0 or other.min() - best > 1e-6, ('marginal MAP not unique', x, best, other.min())
    return x, -best


def capture(name, ns, hgm, utils, n_maps_12_16):
    import exact_models as em
    base = 'rand_8_8' if name == 'rand_8_8_ev' else name
    model = em.build(base, ns, **({'hand': True} if name == 'ref_mln0' else {}))
    Vd, Vc = model['Vd'], model['Vc']
    Vd_idx, Vc_idx = em.set_indices(model)
    table, means, covs, logZ = hgm.convert_to_bn(model['factors'], Vd, Vc, return_logZ=True)
    if name == 'rand_8_8_ev':
        ev = em.EVIDENCE_8_8
        rvs = model['rvs']
        obs_d = {Vd_idx[rvs[p]]: int(v) for p, v in ev.items() if rvs[p] in Vd_idx}
        obs_c = {Vc_idx[rvs[p]]: float(v) for p, v in ev.items() if rvs[p] in Vc_idx}
        sel = tuple(obs_d.get(i, slice(None)) for i in range(len(Vd)))
        t, mu, Sig = table[sel], means[sel], covs[sel]
        oi = np.array(sorted(obs_c))
        ov = np.array([obs_c[i] for i in oi])
        nc = len(Vc) - len(oi)
        logw, means, covs = np.empty(t.shape), np.empty(t.shape + (nc,)), np.empty(t.shape + (nc, nc))
        for idx in np.ndindex(*t.shape):
            S = Sig[idx][np.ix_(oi, oi)]
            d = ov - mu[idx][oi]
            logw[idx] = np.log(t[idx]) - 0.5 * (len(oi) * np.log(2 * np.pi) + np.linalg.slogdet(S)[1] + d @ np.linalg.solve(S, d))
            means[idx], covs[idx] = utils.get_conditional_gaussian(mu[idx], Sig[idx], obs_c)
        lse = utils.logsumexp(logw)
        table, logZ = np.exp(logw - lse), logZ + lse
        Vd = [rv for rv in Vd if Vd_idx[rv] not in obs_d]
        Vc = [rv for rv in Vc if Vc_idx[rv] not in obs_c]
        Vd_idx, Vc_idx = {rv: i for i, rv in enumerate(Vd)}, {rv: i for i, rv in enumerate(Vc)}
    Nd, Nc, M = len(Vd), len(Vc), int(table.size)
    conds = np.array([np.linalg.cond(c) for c in covs.reshape(M, Nc, Nc)])
    assert conds.max() <= 500, ('cond(J) above 500', name, conds.max())
    assert abs(table.sum() - 1) < 1e-12
    variances = np.diagonal(covs, axis1=-2, axis2=-1)
    bn = (table, means, covs)
    out = dict(logZ=np.float64(logZ), max_cond=np.float64(conds.max()), dstates=np.array([rv.dstates for rv in Vd]),
               marg=np.concatenate([hgm.get_drv_marg(table, i) for i in range(Nd)]))
    hidden = Vd + Vc
    n_map = len(hidden) if name != 'rand_12_16' else Nd + n_maps_12_16
    maps, map_logpdf = np.full(len(hidden), np.nan), np.full(len(hidden), np.nan)
    for v, rv in enumerate(hidden[:n_map]):
        maps[v], map_logpdf[v] = marginal_map(hgm, utils, bn, Vd_idx, Vc_idx, rv)
    out.update(maps=maps, map_logpdf=map_logpdf, maps_recorded=np.arange(len(hidden)) < n_map)
    bel_x = np.array([em.query_points(rv) for rv in Vc])
    out['bel_x'] = bel_x
    out['bel_logp'] = np.array([utils.get_scalar_gm_log_prob(bel_x[j], *hgm.get_crv_marg(*bn, j)) for j in range(Nc)])
    rows = np.arange(M) if name in em.FULL else em.sampled_configs(M)
    out.update(cfg=rows, table=table.reshape(M)[rows], means=means.reshape(M, Nc)[rows],
               variances=variances.reshape(M, Nc)[rows])
    if name in em.FULL:
        out['covs_tril'] = tril(covs.reshape(M, Nc, Nc))
    return out


def main():
    import exact_models as em
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True)
    ap.add_argument('--only')
    ap.add_argument('--maps-12-16', type=int, default=1, help='continuous variables of rand_12_16 whose marginal MAP is recorded')
    args = ap.parse_args()
    ns, hgm, utils = reference_ns(os.path.abspath(args.reference))
    for name in em.NAMES:
        if args.only and name != args.only:
            continue
        out = capture(name, ns, hgm, utils, args.maps_12_16)
        path = os.path.join(ROOT, 'tests', 'golden', 'exact_%s.npz' % name)
        np.savez(path, **out)
        print('%s: %d configurations recorded, max cond(J) = %.3g, logZ = %.12g, %d bytes'
              % (name, out['cfg'].size, out['max_cond'], out['logZ'], os.path.getsize(path)))


if __name__ == '__main__':
    main()
