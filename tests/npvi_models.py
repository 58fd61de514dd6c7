"""The yardstick of the NPVI tests: a torch (CPU, float64) restatement of the reference's TensorFlow graph -- ``osi/NPVI.py`` with
``osi/mixture_beliefs.py`` (``hfactors_bfe_obj`` / ``dfactors_bfe_obj`` with ``neg_lpot_only=True``, ``get_hybrid_mixture_entropy_lb``)
-- differentiated by autograd, plus the test graphs.  ``tf.stop_gradient`` is ``.detach()``, ``tf.einsum`` is ``torch.einsum``, the
gradients are ``torch.autograd.grad(aux_obj, params)`` and TensorFlow's Adam is written out by hand.

The twin keeps the parameters by ROW of the flat graph (``Mu`` / ``lVar`` [V, K], ``Rho`` [V, K, Dmax]) so that its arrays compare
with the solver's directly; rows of observed variables and entries beyond a variable's states take no part.  Unlike the reference it
keeps observed variables in the factors, as one-point axes with coefficient 1 (the reference conditions the graph first), and lets
the discrete variables differ in their number of states.
"""
import string

import numpy as np
import torch
from numpy.polynomial.hermite import hermgauss

from lhvi.flat import flatten
from lhvi.graph import RV, F, Graph, Domain
from lhvi.potentials import QuadraticPotential, TablePotential, HybridQuadraticPotential
from lhvi.mln import MLNPotential, eq_op

dtype = torch.float64


def outer_prod_einsum_equation(n, common_first_ndims):
    """osi/utils.py: 'abc,abd,abe->abcde' for n = 3, common_first_ndims = 2"""
    letters = string.ascii_lowercase
    common = letters[:common_first_ndims]
    rest = letters[common_first_ndims:common_first_ndims + n]
    return ','.join(common + r for r in rest) + '->' + common + rest


def log_potential_of(pot):
    to_log = getattr(pot, 'to_log_potential', None)
    if to_log is not None:
        lp = to_log()
        return lambda args: float(lp(args))
    return lambda args: float(np.log(pot.get(args)))


class Twin:
    def __init__(self, g, K, T, Var_bds=None, var_count=None, fac_count=None):
        self.flat = flat = flatten(g)
        self.K, self.T = K, T
        self.rvs, self.factors = flat.rvs, flat.factors
        self.idx = {rv: i for i, rv in enumerate(self.rvs)}
        V = len(self.rvs)
        self.hidden = np.array([rv.value is None for rv in self.rvs])
        self.cont = np.array([bool(rv.domain.continuous) for rv in self.rvs])
        self.nst = np.array([0 if rv.domain.continuous else len(rv.domain.values) for rv in self.rvs])
        disc = self.hidden & ~self.cont
        self.Dmax = int(self.nst[disc].max()) if disc.any() else 1
        self.var_count = np.ones(V) if var_count is None else np.asarray(var_count, dtype=float)
        self.fac_count = np.ones(len(self.factors)) if fac_count is None else np.asarray(fac_count, dtype=float)
        self.Var_bds = [5e-3, 10] if Var_bds is None else Var_bds
        x, w = hermgauss(T)
        self.ghq_points = torch.tensor(x, dtype=dtype)
        self.ghq_weights = torch.tensor(w * np.pi ** -0.5, dtype=dtype)
        self.lpots = [log_potential_of(f.potential) for f in self.factors]

    # ---- parameters ---------------------------------------------------------------------------------------------------------
    def set_params(self, tau, Mu, lVar, Rho):
        mk = lambda a: torch.tensor(np.array(a, dtype=np.float64), dtype=dtype, requires_grad=True)
        self.tau, self.Mu, self.lVar, self.Rho = mk(tau), mk(Mu), mk(lVar), mk(Rho)
        self.adam = [[torch.zeros_like(p), torch.zeros_like(p)] for p in self.params()]
        self.t = 0

    def params(self):
        return [self.tau, self.Mu, self.lVar, self.Rho]

    # ---- the graph of NPVI.__init__ -----------------------------------------------------------------------------------------
    def objectives(self):
        K = self.K
        w = torch.softmax(self.tau, dim=0)
        Var = torch.exp(self.lVar)
        Pi = {v: torch.softmax(self.Rho[v, :, :self.nst[v]], dim=-1) for v in range(len(self.rvs)) if self.hidden[v] and not self.cont[v]}
        neg_elbo = aux_obj = 0
        for fi, f in enumerate(self.factors):
            hid = [rv.value is None for rv in f.nb]
            if any(h and rv.domain.continuous for h, rv in zip(hid, f.nb)) or not all(hid):
                d_bfe, d_aux = self.hfactor_bfe_obj(fi, f, w, Var, Pi)
            else:
                d_bfe, d_aux = self.dfactor_bfe_obj(fi, f, w, Pi)
            neg_elbo = neg_elbo + self.fac_count[fi] * d_bfe
            aux_obj = aux_obj + self.fac_count[fi] * d_aux
        neg_ent_lb = -self.get_hybrid_mixture_entropy_lb(w, Var, Pi)
        return neg_elbo + neg_ent_lb, aux_obj + neg_ent_lb

    def eval_lpot(self, fi, f, axes):
        """utils.eval_fun_grid per component grid: K x V1 x ... x Vn (a constant of the graph: it only enters stop_gradient)"""
        K = self.K
        shape = [int(a.shape[1]) for a in axes]
        out = np.zeros([K] + shape)
        ax = [a.detach().numpy() for a in axes]
        for k in range(K):
            for ind in np.ndindex(*shape):
                args = []
                for i, rv in enumerate(f.nb):
                    val = ax[i][k, ind[i]]
                    if not rv.domain.continuous:
                        val = next(s for s in rv.domain.values if s == val)      # the domain's own (integer) state
                    args.append(val)
                out[(k,) + ind] = self.lpots[fi](tuple(args))
        return torch.tensor(out, dtype=dtype)

    def hfactor_bfe_obj(self, fi, f, w, Var, Pi):
        """mixture_beliefs.hfactors_bfe_obj (:160-256) for one factor, neg_lpot_only=True"""
        K, n = self.K, len(f.nb)
        coefs, axes, comp_probs = [], [], []
        for rv in f.nb:
            v = self.idx[rv]
            if rv.value is not None:                 # evidence: a one-point axis with coefficient 1
                c = torch.ones(K, 1, dtype=dtype)
                a = torch.full((K, 1), float(rv.value), dtype=dtype)
                comp_prob = torch.ones(K, K, 1, dtype=dtype)
            elif not rv.domain.continuous:
                c = Pi[v]                            # K x Vi
                a = torch.tensor(np.tile(np.reshape(np.array(rv.domain.values, dtype=float), [1, -1]), [K, 1]), dtype=dtype)
                comp_prob = c[:, None, :].repeat(1, K, 1)       # K x M(=K) x Vi; same for all M axes
            else:
                c = self.ghq_weights.reshape(1, -1).repeat(K, 1)
                a = (2 * Var[v][:, None]) ** 0.5 * self.ghq_points + self.Mu[v][:, None]        # K x T
                a = a.detach()                       # don't want to differentiate w.r.t. evaluation points
                Mu_K11 = self.Mu[v][:, None, None]
                Var_inv_K11 = (1 / Var[v])[:, None, None]
                comp_prob = (2 * np.pi) ** (-0.5) * torch.sqrt(Var_inv_K11) * torch.exp(-0.5 * (a - Mu_K11) ** 2 * Var_inv_K11)
            coefs.append(c)
            axes.append(a)
            comp_probs.append(comp_prob)
        joint_comp_probs = torch.einsum(outer_prod_einsum_equation(n, 2), *comp_probs)      # K x M x V1 x ... x Vn
        belief = torch.sum(w.reshape([K] + [1] * (n + 1)) * joint_comp_probs, dim=0)        # M x V1 x ... x Vn
        coefs = torch.einsum(outer_prod_einsum_equation(n, 1), *coefs)                      # K x V1 x ... x Vn
        lpot = self.eval_lpot(fi, f, axes)
        log_belief = torch.log(belief)
        F_ = -lpot
        prod = (w.reshape([-1] + [1] * n) * coefs * F_).detach()
        return torch.sum(prod), torch.sum(prod * log_belief)

    def dfactor_bfe_obj(self, fi, f, w, Pi):
        """mixture_beliefs.dfactors_bfe_obj (:293-340) for one factor, neg_lpot_only=True"""
        K, n = self.K, len(f.nb)
        comp_probs = [Pi[self.idx[rv]] for rv in f.nb]
        joint_comp_probs = torch.einsum(outer_prod_einsum_equation(n, 1), *comp_probs)      # K x V1 x ... x Vn
        belief = torch.sum(w.reshape([-1] + [1] * n) * joint_comp_probs, dim=0)
        axes = [torch.tensor(np.array(rv.domain.values, dtype=float), dtype=dtype).reshape(1, -1).repeat(K, 1) for rv in f.nb]
        lpot = self.eval_lpot(fi, f, axes)[0]
        log_belief = torch.log(belief)
        F_ = -lpot
        prod = (belief * F_).detach()
        return torch.sum(prod), torch.sum(prod * log_belief)

    def get_hybrid_mixture_entropy_lb(self, w, Var, Pi):
        """mixture_beliefs.get_hybrid_mixture_entropy_lb (:903-942); discrete variables one by one (their state counts differ)"""
        K = self.K
        all_log_comp_integrals = torch.zeros(K, K, dtype=dtype)
        cv = np.flatnonzero(self.hidden & self.cont)
        if cv.size:
            Mu, Sigs = self.Mu[cv], Var[cv]
            N = cv.size
            conv_Mu_diffs = Mu.reshape(N, K, 1) - Mu.reshape(N, 1, K)
            conv_Sigs = Sigs.reshape(N, K, 1) + Sigs.reshape(N, 1, K)
            conv_Sigs_inv = 1 / conv_Sigs
            log_comp_integrals = (-0.5 * np.log(2 * np.pi)) - 0.5 * torch.log(conv_Sigs) - 0.5 * conv_Mu_diffs ** 2 * conv_Sigs_inv
            log_comp_integrals = log_comp_integrals * torch.tensor(self.var_count[cv], dtype=dtype).reshape(N, 1, 1)
            all_log_comp_integrals = all_log_comp_integrals + torch.sum(log_comp_integrals, dim=0)
        for v in sorted(Pi):
            S = int(self.nst[v])
            comp_integrals = torch.sum(Pi[v].reshape(K, 1, S) * Pi[v].reshape(1, K, S), dim=-1)
            all_log_comp_integrals = all_log_comp_integrals + self.var_count[v] * torch.log(comp_integrals)
        inner_integrals = torch.logsumexp(all_log_comp_integrals + torch.log(w), dim=1)
        return -torch.sum(w * inner_integrals)

    # ---- what the tests compare ---------------------------------------------------------------------------------------------
    def obj_and_grads(self):
        """(obj, g_tau [K], g_c [V, K, 2], g_rho [V, K, Dmax]) in the solver's layout"""
        obj, aux = self.objectives()
        gs = torch.autograd.grad(aux, self.params(), allow_unused=True)
        g_tau, g_mu, g_lv, g_rho = [torch.zeros_like(p) if g is None else g for g, p in zip(gs, self.params())]
        return float(obj.detach()), g_tau.numpy(), np.stack([g_mu.numpy(), g_lv.numpy()], axis=2), g_rho.numpy()

    def adam_step(self, lr, fix_mix, beta1=0.9, beta2=0.999, eps=1e-8):
        """one round of NPVI.run's loop (:230-263): tf.train.AdamOptimizer on aux_obj, the clips, the fix_mix reset"""
        obj, aux = self.objectives()
        gs = torch.autograd.grad(aux, self.params(), allow_unused=True)
        self.t += 1
        lr_t = lr * np.sqrt(1 - beta2 ** self.t) / (1 - beta1 ** self.t)
        with torch.no_grad():
            for p, g, (m, v) in zip(self.params(), gs, self.adam):
                if g is None:
                    continue
                m.mul_(beta1).add_((1 - beta1) * g)
                v.mul_(beta2).add_((1 - beta2) * (g * g))
                p.sub_(lr_t * m / (torch.sqrt(v) + eps))
            lo = torch.tensor([rv.domain.values[0] if rv.domain.continuous else 0.0 for rv in self.rvs], dtype=dtype)[:, None]
            hi = torch.tensor([rv.domain.values[1] if rv.domain.continuous else 0.0 for rv in self.rvs], dtype=dtype)[:, None]
            cont = torch.tensor(self.hidden & self.cont)[:, None]
            self.Mu.copy_(torch.where(cont, torch.minimum(torch.maximum(self.Mu, lo), hi), self.Mu))
            lb = np.log(self.Var_bds)
            self.lVar.copy_(torch.where(cont, torch.clamp(self.lVar, lb[0], lb[1]), self.lVar))
            if fix_mix:
                self.tau.zero_()
        return float(obj.detach())


# ---- test graphs --------------------------------------------------------------------------------------------------------------
def _graph(rvs, factors):
    g = Graph()
    g.rvs, g.factors = list(rvs), list(factors)
    g.init_nb()
    return g


def cdom(lo=-4.0, hi=4.0):
    return Domain([lo, hi], continuous=True)


def dense_gaussian_mrf(n=4, seed=0):
    """unary plus all pairwise quadratic factors on n continuous variables; returns (graph, J, h): p(x) ~ exp(-x'Jx/2 + h'x)"""
    rng = np.random.RandomState(seed)
    B = rng.randn(n, n) * 0.4
    J = B @ B.T + np.eye(n)
    h = rng.randn(n)
    rvs = [RV(cdom(-10.0, 10.0)) for _ in range(n)]
    fs = [F(QuadraticPotential(np.array([[-0.5 * J[i, i]]]), np.array([h[i]]), 0.0), nb=[rvs[i]]) for i in range(n)]
    for i in range(n):
        for j in range(i + 1, n):
            fs.append(F(QuadraticPotential(np.array([[0.0, -0.5 * J[i, j]], [-0.5 * J[i, j], 0.0]]), np.zeros(2), 0.0), nb=[rvs[i], rvs[j]]))
    return _graph(rvs, fs), J, h


def gaussian_chain(n=5, seed=1):
    rng = np.random.RandomState(seed)
    rvs = [RV(cdom()) for _ in range(n)]
    fs = [F(QuadraticPotential(np.array([[-0.5 - 0.1 * i]]), np.array([rng.randn()]), 0.1), nb=[rvs[i]]) for i in range(n)]
    for i in range(n - 1):
        a = 0.3 * rng.randn()
        fs.append(F(QuadraticPotential(np.array([[-0.4, a], [a, -0.6]]), rng.randn(2) * 0.2, -0.2), nb=[rvs[i], rvs[i + 1]]))
    return _graph(rvs, fs)


def _hybrid_parts(seed=2):
    rng = np.random.RandomState(seed)
    d2, d3 = Domain([0, 1], continuous=False), Domain([0, 1, 2], continuous=False)
    return rng, d2, d3


def hybrid_graph(seed=2, observe=False):
    """HybridQuadraticPotential, TablePotential and an MLNPotential over discrete variables of 2 and 3 states and continuous ones;
    ``observe``: one continuous and one discrete argument are evidence"""
    rng, d2, d3 = _hybrid_parts(seed)
    a, b = RV(d2), RV(d3)
    x, y = RV(cdom()), RV(cdom())
    z, c = RV(cdom(), value=0.7 if observe else None), RV(d3, value=2 if observe else None)
    A = -np.abs(rng.randn(3, 1, 1)) - 0.3
    fs = [
        F(HybridQuadraticPotential(A, rng.randn(3, 1), rng.randn(3) * 0.3), nb=[b, x]),
        F(HybridQuadraticPotential(A[:2] * 0.7, rng.randn(2, 1), rng.randn(2) * 0.3), nb=[a, y]),
        F(TablePotential(np.exp(rng.randn(2, 3))), nb=[a, b]),
        F(TablePotential(np.exp(rng.randn(3, 3))), nb=[b, c]),
        F(MLNPotential(lambda v: v[0] * eq_op(v[1], v[2]), w=0.8), nb=[a, x, y]),
        F(QuadraticPotential(np.array([[-0.5, 0.2], [0.2, -0.7]]), np.array([0.1, -0.3]), 0.0), nb=[y, z]),
        F(HybridQuadraticPotential(A * 0.5, rng.randn(3, 1), rng.randn(3) * 0.3), nb=[c, z]),
        F(QuadraticPotential(np.array([[-0.6]]), np.array([0.4]), 0.0), nb=[x]),
    ]
    return _graph([a, b, x, y, z, c], fs)


def arity3_graph(seed=3):
    rng = np.random.RandomState(seed)
    rvs = [RV(cdom()) for _ in range(3)]
    B = rng.randn(3, 3) * 0.3
    A = -(B @ B.T + 0.5 * np.eye(3))
    fs = [F(QuadraticPotential(A, rng.randn(3) * 0.3, 0.05), nb=rvs)]
    fs += [F(QuadraticPotential(np.array([[-0.3]]), np.array([0.1 * i]), 0.0), nb=[rvs[i]]) for i in range(3)]
    return _graph(rvs, fs)


def observed_factor_graph(seed=4):
    """a factor all of whose arguments are evidence (a constant of the objective), beside a small hidden part"""
    rng, d2, d3 = _hybrid_parts(seed)
    x, y = RV(cdom()), RV(cdom(), value=-0.4)
    a, b = RV(d2), RV(d3, value=1)
    fs = [
        F(HybridQuadraticPotential(-np.abs(rng.randn(3, 1, 1)) - 0.2, rng.randn(3, 1), rng.randn(3)), nb=[b, y]),
        F(QuadraticPotential(np.array([[-0.5, 0.1], [0.1, -0.5]]), np.zeros(2), 0.3), nb=[x, y]),
        F(TablePotential(np.exp(rng.randn(2, 3))), nb=[a, b]),
        F(HybridQuadraticPotential(-np.abs(rng.randn(2, 1, 1)) - 0.2, rng.randn(2, 1), rng.randn(2)), nb=[a, x]),
    ]
    return _graph([x, y, a, b], fs)


def interpreted_graph(seed=6):
    """formulas the device has to interpret (no conditional-quadratic view: |x - y| and a cube), one of them over four arguments, on a
    hybrid scope -- the factor kernel's interpreter build"""
    rng, d2, d3 = _hybrid_parts(seed)
    a, b = RV(d2), RV(d3)
    x, y, z = RV(cdom()), RV(cdom()), RV(cdom())
    fs = [
        F(MLNPotential(lambda v: -v[0] * abs(v[1] - v[2]), w=0.7), nb=[a, x, y]),
        F(MLNPotential(lambda v: -abs(v[1] - 0.3 * v[2]) * (1 + v[0]) - 0.1 * abs(v[3]) ** 3, w=0.5), nb=[b, y, z, x]),
        F(TablePotential(np.exp(rng.randn(2, 3))), nb=[a, b]),
    ]
    fs += [F(QuadraticPotential(np.array([[-0.5]]), np.array([0.2 * i]), 0.0), nb=[r]) for i, r in enumerate((x, y, z))]
    return _graph([a, b, x, y, z], fs)


def high_arity_graph(seed=9):
    """an arity-4 factor (3 continuous + 1 discrete argument) and an arity-6 factor (2 discrete, 4 continuous arguments, two of the
    continuous ones observed): the arity-6 loops of the factor kernel, with discrete partials"""
    rng, d2, d3 = _hybrid_parts(seed)
    a, b = RV(d2), RV(d2)
    x, y, z = RV(cdom()), RV(cdom()), RV(cdom())
    o1, o2 = RV(cdom(), value=0.5), RV(cdom(), value=-0.8)

    def neg_def(n, scale):
        B = rng.randn(n, n) * 0.3
        return -(B @ B.T + 0.5 * np.eye(n)) * scale
    A6 = np.stack([np.stack([neg_def(4, 0.6 + 0.2 * (i + j)) for j in range(2)]) for i in range(2)])       # [2, 2, 4, 4]
    fs = [
        F(QuadraticPotential(neg_def(4, 0.5), rng.randn(4) * 0.2, 0.1), nb=[x, a, y, z]),
        F(HybridQuadraticPotential(A6, rng.randn(2, 2, 4) * 0.3, rng.randn(2, 2) * 0.3), nb=[a, b, x, o1, y, o2]),
        F(TablePotential(np.exp(rng.randn(2, 2))), nb=[a, b]),
        F(QuadraticPotential(np.array([[-0.4]]), np.array([0.1]), 0.0), nb=[z]),
    ]
    return _graph([a, b, x, y, z, o1, o2], fs)


def long_chain(n=1025):
    """n continuous variables of degree 2 and 3.  At n = 1 025 the reductions over the variables take five blocks of 256, the last one
    holding a single variable; at K = 2 OneShot's variable kernel takes 128 variables a block -- nine blocks, the last one holding a
    single group"""
    rvs = [RV(cdom()) for _ in range(n)]
    unary = [QuadraticPotential(np.array([[-0.5 - 0.05 * i]]), np.array([0.3 * i - 0.6]), 0.0) for i in range(5)]
    pair = [QuadraticPotential(np.array([[-0.4, a], [a, -0.6]]), np.array([0.1, -0.1]), 0.0) for a in (0.25, -0.2, 0.1)]
    fs = [F(unary[i % 5], nb=[rvs[i]]) for i in range(n)] + [F(pair[i % 3], nb=[rvs[i], rvs[i + 1]]) for i in range(n - 1)]
    return _graph(rvs, fs)


def hub_graph(deg=70):
    """one variable of degree 70 (> LHVI_HUB_DEGREE = 64; OneShot's kappa = -69): its gather takes the wavefront path; the leaves
    have degree 1 (OneShot's variable kernel skips them)"""
    hub = RV(cdom())
    leaves = [RV(cdom()) for _ in range(deg - 1)]
    pair = QuadraticPotential(np.array([[-0.05, 0.02], [0.02, -0.6]]), np.array([0.01, -0.2]), 0.0)
    fs = [F(pair, nb=[hub, x]) for x in leaves] + [F(QuadraticPotential(np.array([[-0.4]]), np.array([0.2]), 0.0), nb=[hub])]
    return _graph([hub] + leaves, fs)


def start_params(tw, seed, spread=1.0):
    """a random start in the solver's layout: (tau [K], Mu [V, K], lVar [V, K], Rho [V, K, Dmax])"""
    rng = np.random.RandomState(seed)
    V, K = len(tw.rvs), tw.K
    return rng.randn(K) * 0.5, rng.randn(V, K) * spread, np.log(rng.uniform(0.2, 2.0, size=(V, K))), rng.randn(V, K, tw.Dmax)


# ---- comparisons the host and the GPU modules of NPVI and OneShot share ---------------------------------------------------------
def assert_close(got, want, tol, what):
    scale = max(float(np.max(np.abs(want))), 1e-300)
    err = float(np.max(np.abs(np.asarray(got) - np.asarray(want)))) / scale
    assert err <= tol, '%s: %.3g of the largest entry %.3g' % (what, err, scale)


def param_diff(s, tw):
    h = s._h
    cont, mask = s._cont[:, None], s._mask_d[:, None, :]
    return max(float(np.max(np.abs(h['tau'] - tw.tau.detach().numpy()))),
               float(np.max(np.abs(np.where(cont, h['theta_c'][:, :, 0] - tw.Mu.detach().numpy(), 0.0)))),
               float(np.max(np.abs(np.where(cont, h['theta_c'][:, :, 1] - tw.lVar.detach().numpy(), 0.0)))),
               float(np.max(np.abs(np.where(mask, h['rho'] - tw.Rho.detach().numpy(), 0.0)))))


def device_bits(s):
    """the bytes of every device array of a solver, the workspace included, of its host copies, and its update count"""
    dev = {n: a.cpu().numpy().tobytes() for n, a in s._dev.items() if isinstance(a, torch.Tensor)}
    return dev, {n: a.tobytes() for n, a in s._h.items()}, s.t
