"""Record the NumPy half of the reference's osi/mixture_beliefs.py as fixtures (tests/golden/mixture_*.npz, data only).

Imports the reference's osi/mixture_beliefs.py (path given by --reference) with an empty module named `tensorflow` in
sys.modules -- the NumPy half (:505-746) never touches it -- and runs _calc_marg_comp_log_prob, calc_marg_log_prob,
calc_cond_mixture_weights, drv_belief_map, marginal_map and utils.get_scalar_gm_mode on the cases of tests/mixture_models.py
(without NaN holes, which the reference does not know; its rvs are plain objects with domain_type / belief_params / values).

  mixture_cond_k{K}.npz   per N_o in 1, 63, 64, 65: obs, X [5, N_o], comp, logp, condw, the same for the first row given as a
                          vector, drv_belief_map of every discrete row under condw; for N_o = 1: marginal_map of every row
                          the evidence does not observe, given the first evidence row
  mixture_joint.npz       joint_map_from_belief_params (xd, xc) on joint_case(shape) for every shape of JOINT_SHAPES, and
                          get_multivar_gm_mode from the component means (x, log density) on the shapes with continuous rows
  mixture_modes.npz       get_scalar_gm_mode (x, log density) on mode_case(0 .. 47), parameters padded to 8 components

Usage: python scripts/capture_mixture.py --reference PATH
"""
import argparse
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def reference_modules(path):
    sys.modules.setdefault('tensorflow', types.ModuleType('tensorflow'))
    sys.path[:0] = [os.path.join(path, 'osi'), path]
    import mixture_beliefs
    import utils
    return mixture_beliefs, utils


def rvs_of(case):
    Nc = len(case['Mu'])
    rvs = []
    for v in range(Nc):
        rvs.append(types.SimpleNamespace(domain_type='c-g', belief_params={'mu': case['Mu'][v], 'var': case['Var'][v]},
                                         values=np.array(case['bds'][:, v])))
    for pi in case['Pi']:
        rvs.append(types.SimpleNamespace(domain_type='d-%d' % pi.shape[1], belief_params={'pi': pi},
                                         values=np.arange(pi.shape[1], dtype=float)))
    return rvs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True)
    args = ap.parse_args()
    import mixture_models as mm
    mb, utils = reference_modules(args.reference)
    out_dir = os.path.join(ROOT, 'tests', 'golden')
    for K in mm.KS:
        rec = {}
        for N_o in mm.NOS[1:]:
            case = mm.condition_case(K, N_o, 5, holes=False)
            rvs = rvs_of(case)
            obs_rvs = [rvs[v] for v in case['obs']]
            X, w, pre = case['X'], case['w'], 'no%d_' % N_o
            rec[pre + 'obs'], rec[pre + 'X'] = case['obs'], X
            types_, params = mb.get_obs_rvs_domain_types_and_params(obs_rvs)
            rec[pre + 'comp'] = mb._calc_marg_comp_log_prob(X, types_, params)
            rec[pre + 'logp'] = mb.calc_marg_log_prob(X, obs_rvs, w)
            rec[pre + 'condw'] = condw = mb.calc_cond_mixture_weights(X, obs_rvs, w)
            rec[pre + 'comp1'] = mb._calc_marg_comp_log_prob(X[0], types_, params)
            rec[pre + 'logp1'] = mb.calc_marg_log_prob(X[0], obs_rvs, w)
            rec[pre + 'condw1'] = mb.calc_cond_mixture_weights(X[0], obs_rvs, w)
            rec[pre + 'dmap'] = np.array([mb.drv_belief_map(condw, pi)[0] for pi in case['Pi']])
            rec[pre + 'dmap1'] = np.array([mb.drv_belief_map(condw[0], pi)[0] for pi in case['Pi']])
            if N_o == 1:
                query = [v for v in range(len(rvs)) if v not in case['obs']]
                rec[pre + 'query'] = np.array(query)
                rec[pre + 'mmap'] = np.array([float(mb.marginal_map(X[0], obs_rvs, rvs[v], w)) for v in query])
        np.savez_compressed(os.path.join(out_dir, 'mixture_cond_k%d.npz' % K), **rec)
    rec = {}
    for shape in mm.JOINT_SHAPES:
        case = mm.joint_case(shape)
        pre = 'j%d_%d_%d_%d_' % shape
        val = mb.joint_map_from_belief_params(case['w'], case['Pi'], case['Mu'], case['Var'], case['bds'])
        for key in ('xd', 'xc'):
            if val[key] is not None:
                rec[pre + key] = np.array(val[key])
        if case['Mu'] is not None:
            x, f = utils.get_multivar_gm_mode(np.log(case['w']), case['Mu'], case['Var'], case['bds'], best_log_pdf=True)
            rec[pre + 'gm_x'], rec[pre + 'gm_f'] = np.array(x), float(f)
    np.savez_compressed(os.path.join(out_dir, 'mixture_joint.npz'), **rec)
    n = 48
    W, MU, VAR, KK, XM, FM = np.zeros((n, 8)), np.zeros((n, 8)), np.ones((n, 8)), np.zeros(n, dtype=int), np.zeros(n), np.zeros(n)
    for i in range(n):
        w, mu, var, bds = mm.mode_case(i)
        k = KK[i] = len(w)
        W[i, :k], MU[i, :k], VAR[i, :k] = w, mu, var
        XM[i], FM[i] = utils.get_scalar_gm_mode(w, mu, var, bds, best_log_pdf=True)
    np.savez_compressed(os.path.join(out_dir, 'mixture_modes.npz'), w=W, mu=MU, var=VAR, K=KK, x=XM, f=FM, bds=np.array(bds))


if __name__ == '__main__':
    main()
