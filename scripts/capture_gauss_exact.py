"""Record the reference's exact Gaussian answer on its RGM datasets as fixtures (tests/golden/gauss_exact_rgm{0..4}.npz, data
only).

Imports the reference (path given by --reference), builds the RGM with its generate_rel_graph, loads Demo/Data/RGM/0..4 and runs
the three calls of Demo/RGM/RGMKLDivergence.py: osi/utils.py get_conditional_mrf, get_quadratic_params_from_factor_graph and
get_gaussian_mean_params_from_quadratic_params(A, b, mu_only=False).

Per dataset: the evidence as (key, value) pairs, the hidden variables' keys in matrix order (the reference numbers them by set
iteration, so the keys are what identifies a row), mu, diag(Sig), 256 seeded off-diagonal entries of Sig as (i, j, value),
log det J by slogdet, the extreme eigenvalues and cond(J).  It ASSERTS that J = -2A is symmetric and cond(J) <= 500.  Full
covariance matrices are not recorded.

Usage: python scripts/capture_gauss_exact.py --reference PATH [--only I]
"""
import argparse
import collections
import collections.abc
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_COV = 256


def reference_modules(path):
    # the reference predates NumPy 2 and Python 3.10
    if not hasattr(np, 'Inf'):
        np.Inf = np.inf
    if not hasattr(collections, 'MutableSet'):
        collections.MutableSet = collections.abc.MutableSet
    sys.path[:0] = [path]
    os.chdir(path)
    import osi.utils as utils
    from Demo.Data.RGM.Generator import generate_rel_graph, load_data
    return utils, generate_rel_graph, load_data


def capture(i, utils, rel_g, load_data):
    data = load_data(os.path.join('Demo', 'Data', 'RGM', str(i)))
    g, rvs_dict = rel_g.add_evidence(data)
    key_of = {rv: key for key, rv in rvs_dict.items()}
    evidence = {rv: rv.value for rv in g.rvs if rv.value is not None}
    cond_g = utils.get_conditional_mrf(g.factors_list, g.rvs, evidence)
    (A, b, c), rvs_idx = utils.get_quadratic_params_from_factor_graph(cond_g.factors, cond_g.rvs_list)
    mu, Sig = utils.get_gaussian_mean_params_from_quadratic_params(A=A, b=b, mu_only=False)
    J = -2.0 * A
    assert np.array_equal(J, J.T), 'J is not symmetric'
    eig = np.linalg.eigvalsh(J)
    cond = eig[-1] / eig[0]
    assert eig[0] > 0 and cond <= 500, ('cond(J) above 500', i, cond)
    N = len(mu)
    hidden = [None] * N
    for rv, k in rvs_idx.items():
        hidden[k] = repr(key_of[rv])
    rng = np.random.default_rng(1000 + i)
    ci = rng.integers(0, N, size=N_COV)
    cj = (ci + 1 + rng.integers(0, N - 1, size=N_COV)) % N
    ev = sorted((repr(key_of[rv]), float(v)) for rv, v in evidence.items())
    return dict(ev_keys=np.array([k for k, _ in ev]), ev_vals=np.array([v for _, v in ev]), hidden_keys=np.array(hidden),
                mu=np.asarray(mu, dtype=np.float64), var=np.diag(Sig).copy(), cov_i=ci, cov_j=cj, cov_v=Sig[ci, cj],
                logdet=np.float64(np.linalg.slogdet(J)[1]), eig_min=np.float64(eig[0]), eig_max=np.float64(eig[-1]),
                cond=np.float64(cond), n_factors=np.int64(len(cond_g.factors)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True)
    ap.add_argument('--only', type=int)
    args = ap.parse_args()
    utils, generate_rel_graph, load_data = reference_modules(os.path.abspath(args.reference))
    rel_g = generate_rel_graph()
    rel_g.ground_graph()
    for i in range(5):
        if args.only is not None and i != args.only:
            continue
        out = capture(i, utils, rel_g, load_data)
        path = os.path.join(ROOT, 'tests', 'golden', 'gauss_exact_rgm%d.npz' % i)
        np.savez_compressed(path, **out)
        print('rgm%d: N = %d hidden, %d conditioned factors, cond(J) = %.4g, log det J = %.12g, %d bytes'
              % (i, out['mu'].size, out['n_factors'], out['cond'], out['logdet'], os.path.getsize(path)))


if __name__ == '__main__':
    main()
