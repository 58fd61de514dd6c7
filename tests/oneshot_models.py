"""The yardstick of the OneShot tests: a torch (CPU, float64) restatement of the reference's TensorFlow graph -- ``osi/OneShot.py``
with ``osi/mixture_beliefs.py`` (``hfactors_bfe_obj`` / ``dfactors_bfe_obj`` with ``neg_lpot_only=False``, ``drvs_bfe_obj``,
``crvs_bfe_obj``) -- differentiated by autograd, on top of tests/npvi_models.py: the parameters, the Adam step and the graphs are
that file's, ``objectives()`` is the Bethe free energy.  Purely discrete factors go through ``dfactor_bfe_obj`` (a sum over the
states of ``b F``) as in the reference, where the kernels use the K-grid form for every factor: the tests show the two agree.

``deg`` is ``len(rv.nb)`` of the flat graph's rows, or what the caller passes (a lifted graph: the ground degree of a member).
Plus the graphs the variable term needs and the symmetric relational graph of the lifted test.
"""
import numpy as np
import torch

import npvi_models as nm
from lhvi.graph import RV, F
from lhvi.potentials import QuadraticPotential, TablePotential, HybridQuadraticPotential

dtype = nm.dtype


class Twin(nm.Twin):
    def __init__(self, g, K, T, Var_bds=None, var_count=None, fac_count=None, deg=None):
        nm.Twin.__init__(self, g, K, T, Var_bds=Var_bds, var_count=var_count, fac_count=fac_count)
        self.deg = np.array([len(rv.nb) for rv in self.rvs], dtype=float) if deg is None else np.asarray(deg, dtype=float)

    # ---- the graph of OneShot.__init__ --------------------------------------------------------------------------------------
    def objectives(self):
        w = torch.softmax(self.tau, dim=0)
        Var = torch.exp(self.lVar)
        Pi = {v: torch.softmax(self.Rho[v, :, :self.nst[v]], dim=-1) for v in range(len(self.rvs)) if self.hidden[v] and not self.cont[v]}
        bfe = aux_obj = 0
        for v in sorted(Pi):
            d_bfe, d_aux = self.drv_bfe_obj(v, w, Pi[v])
            bfe = bfe + self.var_count[v] * d_bfe
            aux_obj = aux_obj + self.var_count[v] * d_aux
        cv = np.flatnonzero(self.hidden & self.cont)
        if cv.size:
            d_bfe, d_aux = self.crvs_bfe_obj(cv, w, self.Mu[cv], Var[cv])
            bfe = bfe + d_bfe
            aux_obj = aux_obj + d_aux
        for fi, f in enumerate(self.factors):
            hid = [rv.value is None for rv in f.nb]
            if any(h and rv.domain.continuous for h, rv in zip(hid, f.nb)) or not all(hid):
                d_bfe, d_aux = self.hfactor_bfe_obj(fi, f, w, Var, Pi)
            else:
                d_bfe, d_aux = self.dfactor_bfe_obj(fi, f, w, Pi)
            bfe = bfe + self.fac_count[fi] * d_bfe
            aux_obj = aux_obj + self.fac_count[fi] * d_aux
        return bfe, aux_obj

    def drv_bfe_obj(self, v, w, Pi_v):
        """mixture_beliefs.drvs_bfe_obj (:441-464) for one variable (the state counts differ); the sharing count is the caller's"""
        belief = torch.sum(w[:, None] * Pi_v, dim=0)
        log_belief = torch.log(belief)
        prod = (belief * log_belief).detach()
        coef = 1 - self.deg[v]
        return coef * torch.sum(prod), coef * torch.sum(prod * log_belief)

    def crvs_bfe_obj(self, rows, w, Mu, Var):
        """mixture_beliefs.crvs_bfe_obj (:467-502) with eval_crvs_belief"""
        N, K = Mu.shape
        w_1K1 = w[None, :, None]
        QY = self.ghq_points * (2 * Var.reshape(N, K, 1)) ** 0.5 + Mu.reshape(N, K, 1)          # N x K x T; all eval points
        QY = QY.detach()
        X = QY.reshape(N, 1, K * self.T)
        Var_inv = (1 / Var).reshape(N, K, 1)
        comp = (2 * np.pi) ** (-0.5) * torch.sqrt(Var_inv) * torch.exp(-0.5 * (X - Mu.reshape(N, K, 1)) ** 2 * Var_inv)
        belief = torch.sum(w_1K1 * comp, dim=1).reshape(N, K, self.T)
        log_belief = torch.log(belief)
        prod = (w_1K1 * self.ghq_weights * log_belief).detach()
        expect_coefs = torch.tensor(self.var_count[rows] * (1 - self.deg[rows]), dtype=dtype)
        bfe = torch.sum(expect_coefs * torch.sum(prod, dim=[1, 2]))
        aux_obj = torch.sum(expect_coefs * torch.sum(prod * log_belief, dim=[1, 2]))
        return bfe, aux_obj

    def hfactor_bfe_obj(self, fi, f, w, Var, Pi):
        """mixture_beliefs.hfactors_bfe_obj (:160-256) for one factor, neg_lpot_only=False"""
        K, n = self.K, len(f.nb)
        coefs, axes, comp_probs = [], [], []
        for rv in f.nb:
            v = self.idx[rv]
            if rv.value is not None:                 # evidence: a one-point axis with coefficient 1
                c = torch.ones(K, 1, dtype=dtype)
                a = torch.full((K, 1), float(rv.value), dtype=dtype)
                comp_prob = torch.ones(K, K, 1, dtype=dtype)
            elif not rv.domain.continuous:
                c = Pi[v]
                a = torch.tensor(np.tile(np.reshape(np.array(rv.domain.values, dtype=float), [1, -1]), [K, 1]), dtype=dtype)
                comp_prob = c[:, None, :].repeat(1, K, 1)
            else:
                c = self.ghq_weights.reshape(1, -1).repeat(K, 1)
                a = ((2 * Var[v][:, None]) ** 0.5 * self.ghq_points + self.Mu[v][:, None]).detach()
                Mu_K11 = self.Mu[v][:, None, None]
                Var_inv_K11 = (1 / Var[v])[:, None, None]
                comp_prob = (2 * np.pi) ** (-0.5) * torch.sqrt(Var_inv_K11) * torch.exp(-0.5 * (a - Mu_K11) ** 2 * Var_inv_K11)
            coefs.append(c)
            axes.append(a)
            comp_probs.append(comp_prob)
        joint_comp_probs = torch.einsum(nm.outer_prod_einsum_equation(n, 2), *comp_probs)   # K x M x V1 x ... x Vn
        belief = torch.sum(w.reshape([K] + [1] * (n + 1)) * joint_comp_probs, dim=0)        # M x V1 x ... x Vn
        coefs = torch.einsum(nm.outer_prod_einsum_equation(n, 1), *coefs)
        lpot = self.eval_lpot(fi, f, axes)
        log_belief = torch.log(belief)
        F_ = -lpot + log_belief
        prod = (w.reshape([-1] + [1] * n) * coefs * F_).detach()
        return torch.sum(prod), torch.sum(prod * log_belief)

    def dfactor_bfe_obj(self, fi, f, w, Pi):
        """mixture_beliefs.dfactors_bfe_obj (:293-340) for one factor, neg_lpot_only=False"""
        K, n = self.K, len(f.nb)
        comp_probs = [Pi[self.idx[rv]] for rv in f.nb]
        joint_comp_probs = torch.einsum(nm.outer_prod_einsum_equation(n, 1), *comp_probs)
        belief = torch.sum(w.reshape([-1] + [1] * n) * joint_comp_probs, dim=0)
        axes = [torch.tensor(np.array(rv.domain.values, dtype=float), dtype=dtype).reshape(1, -1).repeat(K, 1) for rv in f.nb]
        lpot = self.eval_lpot(fi, f, axes)[0]
        log_belief = torch.log(belief)
        F_ = -lpot + log_belief
        prod = (belief * F_).detach()
        return torch.sum(prod), torch.sum(prod * log_belief)


# ---- graphs the variable term needs -------------------------------------------------------------------------------------------
def _pair(rng):
    c = 0.25 * rng.randn()
    return QuadraticPotential(np.array([[-0.5, c], [c, -0.6]]), rng.randn(2) * 0.2, 0.0)


def degree_graph(seed=13):
    """hidden variables of degree 1 (kappa = 0: a continuous and a discrete leaf) next to ones of degree 3"""
    rng, d2, d3 = nm._hybrid_parts(seed)
    x, leaf, y = RV(nm.cdom()), RV(nm.cdom()), RV(nm.cdom())
    a, dleaf = RV(d3), RV(d2)
    fs = [
        F(_pair(rng), nb=[x, leaf]),
        F(_pair(rng), nb=[x, y]),
        F(QuadraticPotential(np.array([[-0.6]]), np.array([0.3]), 0.0), nb=[x]),
        F(HybridQuadraticPotential(-np.abs(rng.randn(3, 1, 1)) - 0.3, rng.randn(3, 1), rng.randn(3) * 0.3), nb=[a, y]),
        F(TablePotential(np.exp(rng.randn(3, 2))), nb=[a, dleaf]),
        F(TablePotential(np.exp(rng.randn(3))), nb=[a]),
    ]
    return nm._graph([x, leaf, y, a, dleaf], fs)


def isolated_graph(seed=14):
    """an isolated hidden continuous and an isolated hidden discrete variable (kappa = +c_v, no edges) beside a small connected part"""
    rng, d2, d3 = nm._hybrid_parts(seed)
    x, y = RV(nm.cdom()), RV(nm.cdom())
    a = RV(d2)
    lone_c, lone_d = RV(nm.cdom()), RV(d3)
    fs = [
        F(_pair(rng), nb=[x, y]),
        F(HybridQuadraticPotential(-np.abs(rng.randn(2, 1, 1)) - 0.3, rng.randn(2, 1), rng.randn(2) * 0.3), nb=[a, x]),
        F(QuadraticPotential(np.array([[-0.4]]), np.array([0.1]), 0.0), nb=[y]),
    ]
    return nm._graph([x, lone_c, y, a, lone_d], fs)


def leaves_only_graph(seed=15):
    """every hidden variable has degree 1: the variable term skips every row"""
    rng, d2, d3 = nm._hybrid_parts(seed)
    x, y, z = RV(nm.cdom()), RV(nm.cdom()), RV(nm.cdom())
    a = RV(d3)
    o = RV(nm.cdom(), value=0.4)
    fs = [
        F(_pair(rng), nb=[x, y]),
        F(HybridQuadraticPotential(-np.abs(rng.randn(3, 1, 1)) - 0.3, rng.randn(3, 1), rng.randn(3) * 0.3), nb=[a, z]),
        F(QuadraticPotential(np.array([[-0.3]]), np.array([0.2]), 0.0), nb=[o]),
    ]
    return nm._graph([x, y, z, a, o], fs)


def symmetric_rgm():
    """three exchangeable continuous variables tied to one template variable, one evidence value: colour passing puts the three in
    one cluster.  Ground degrees: hub 4, leaves 2 -- the cluster of the leaves has one edge of count 1 to each of two factor clusters,
    the hub's cluster an edge of count 3"""
    dom = nm.cdom()                     # one domain object: colour passing starts from domain identity
    hub, ev = RV(dom), RV(dom, value=0.3)
    leaves = [RV(dom) for _ in range(3)]
    pair = QuadraticPotential(np.array([[-0.5, 0.3], [0.3, -0.6]]), np.array([0.1, -0.2]), 0.0)
    unary = QuadraticPotential(np.array([[-0.4]]), np.array([0.2]), 0.0)
    fs = [F(pair, nb=[hub, x]) for x in leaves] + [F(unary, nb=[x]) for x in leaves] + [F(pair, nb=[ev, hub])]
    return nm._graph([hub, ev] + leaves, fs), ([0, 1, 2, 2, 2], [0, 0, 0, 1, 1, 1, 2])
