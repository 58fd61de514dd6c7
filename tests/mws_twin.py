"""The free-running HybridMaxWalkSAT search restated on the host: one try, plain Python / NumPy, written from
docs/kernels_mws.md ("Semantics kept from the reference", "Deliberate deviations") and the comments of csrc/mws.hip.

What it shares with the device: the Philox round (``gibbs_models.philox4``, checked against the Random123 vectors) and the
L-BFGS-B source (``lhvi_lbfgsb_host``, the device's optimiser built for the host; the objective is evaluated here).  Everything
else is its own: phi comes from the factor objects (``f.potential.get(tuple(values))``, as ``HybridMaxWalkSAT.score`` does), a
score term is ``log(phi)`` or -700 where ``phi == 0``, and sums run in a selectable order (``ORDERS``).

The device sums a set of factors lane-strided and then across lanes, so its scores differ from any host order in the last
bits.  ``step`` therefore records the margin |a - b| / max(1, |a|, |b|) of every strict comparison whose outcome the flip
depends on, and can produce what the flip would have done had comparisons gone the other way (``Step.alt``,
``Step.reachable``).  A flip is *tight* when one of its margins is <= ``TOL`` (1e-9, the project's score tolerance), and
*ambiguous* when it is tight and the other outcome of a tight comparison leads to another state.  Three things are not
counted, each because the outcome cannot differ between two correct implementations: the accept test of a discrete clause
(``bsc > cur_local or c is discrete``: its outcome changes nothing); a comparison of two sums whose terms are equal one by
one and that stem from discrete candidates (the same bits under every summation order: "equal scores compare equal"); and a
tight flip all of whose alternatives end in the same state.  Flips that are not ambiguous are held to the twin's one result.

``check_trajectory`` / ``check_best`` / ``likelihood_log`` are the comparison rules of tests/test_gpu_mws_twin.py, kept here
so that tests/test_mws_twin_host.py can run them without a device (against the twin's own runs, and against mutated twins).
"""
import ctypes as C
import math

import numpy as np

from gibbs_models import philox4
from lhvi import _abi
from lhvi.flat import flatten
from lhvi.mln import MLNHardPotential, MLNPotential

TAG_FLIP, TAG_INIT = (int.from_bytes(t, 'big') for t in (b'MWSF', b'MWSI'))      # the fourth counter word
TOL = 1e-9                  # score tolerance: a comparison with a margin this small is ambiguous
ORDERS = ('forward', 'reversed', 'fsum')
VAL_TIGHT, VAL_LOOSE, TIGHT_SHARE = 1e-7, 1e-4, 0.95     # the replay tolerances on continuous values
AMBIGUOUS_CAP = 0.02


# ---- draws -------------------------------------------------------------------------------------------------------------------
def uniform2(seed, a, b, draw, tag):
    """the two 53-bit uniforms in [0, 1) of counter (a, b, draw, tag): words (0, 1) and (2, 3), high word first"""
    c = [int(w) for w in philox4(a, b, draw, tag, seed)]
    r0, r1 = (c[0] << 32) | c[1], (c[2] << 32) | c[3]
    return (r0 >> 11) * 2.0 ** -53, (r1 >> 11) * 2.0 ** -53


def pick(u, n):
    """floor(u n) for u in [0, 1), never n"""
    return min(int(u * n), n - 1)


def flip_draws(seed, flip, try_id):
    """(u0 .. u5) of a flip: draw pairs 0, 1, 2 of counter (flip, try, draw, "MWSF")"""
    out = []
    for draw in range(3):
        out.extend(uniform2(seed, flip, try_id, draw, TAG_FLIP))
    return tuple(out)


def init_draw(seed, v, try_id):
    """the uniform that places hidden variable v: the first of counter (v, try, 0, "MWSI")"""
    return uniform2(seed, v, try_id, 0, TAG_INIT)[0]


def box_muller(noise_std, u4, u5):
    return noise_std * (math.sqrt(-2.0 * math.log(1.0 - u4)) * math.cos(6.283185307179586 * u5))


def margin(a, b):
    return abs(a - b) / max(1.0, abs(a), abs(b))


def host_lbfgsb(fun, x0):
    """lhvi_lbfgsb_host (csrc/scipy_opt.hpp built for the host) on fun(list of n floats)"""
    n = len(x0)
    cb = _abi.LBFGSB_FUN(lambda p, ctx: float(fun([p[i] for i in range(n)])))
    x = np.array(x0, dtype=np.float64)
    _abi.check(_abi.lib().lhvi_lbfgsb_host(n, x.ctypes.data, cb, None, None, None, None, None))
    return [float(v) for v in x]


class _Decider:
    """the strict comparisons of one flip, in the order they are made; `forced` overrides the first len(forced) outcomes"""

    def __init__(self, forced, total):
        self.forced, self.log, self.total = tuple(forced), [], total

    def gt(self, a, b, kind, exact=False):
        """a > b of two sums of score terms (term lists).  exact: the two lists are equal term by term and belong to discrete
        candidates, so the sums are the same bits under every summation order: a tie by construction, not an ambiguity"""
        exact = exact and a == b
        a, b = self.total(a), self.total(b)
        natural = bool(a > b)
        i = len(self.log)
        out = self.forced[i] if i < len(self.forced) else natural
        self.log.append((kind, margin(a, b), out, exact))
        return out


class Step:
    """one flip: hard / soft (unsatisfied factor indices, factor order), clause, c_disc, branch ('walk' / 'greedy'); a walk's
    walk_var / walk_val; a greedy move's cands [(variable, candidate, score on the clause's neighbourhood)], winner (index
    among the hidden variables), cur_local, accept, numeric ('joint' / 'noop' / None); changed (the variables the flip may
    write), post (the state after it), cmp [(kind, margin, outcome)]."""

    def __init__(self, run, **kw):
        self._run = run
        self.__dict__.update(kw)

    @property
    def min_margin(self):
        return min((m for _, m, _, exact in self.cmp if not exact), default=np.inf)

    @property
    def tight(self):
        """some comparison of the flip has a margin <= TOL"""
        return self.min_margin <= TOL

    @property
    def ambiguous(self):
        """tight, and deciding the tight comparisons the other way leads to another state: a discrete value differs, or a
        continuous one by more than VAL_TIGHT.  (A greedy move on a variable that already sits at its optimum ties the current
        score by construction; accepted or not, it usually leaves the state where it was, and such a flip is compared with
        the device like any other.)"""
        if not self.tight:
            return False
        if '_ambiguous' not in self.__dict__:
            self._ambiguous = any(not same_state(self.cont, r.post, self.post) for r in self.reachable()[1:])
        return self._ambiguous

    def alt(self, i):
        """the flip with comparison i decided the other way (and the earlier ones as they were)"""
        return self._run(tuple(c[2] for c in self.cmp[:i]) + (not self.cmp[i][2],))

    def reachable(self, tol=TOL):
        """every outcome of the flip under any combination of reversed comparisons of margin <= tol; [0] is this one"""
        out, stack = [], [(self, 0)]
        while stack:
            r, start = stack.pop()
            out.append(r)
            for i in range(start, len(r.cmp)):
                if r.cmp[i][1] <= tol and not r.cmp[i][3]:
                    stack.append((r.alt(i), i + 1))
        return out


def same_state(cont, a, b):
    """discrete values equal, continuous ones to VAL_TIGHT"""
    d = np.abs(a - b)
    return bool(np.all(np.where(cont, d <= VAL_TIGHT * np.maximum(1.0, np.abs(b)), d == 0)))


class Twin:
    def __init__(self, g, order='forward'):
        assert order in ORDERS
        self.order = order
        fl = flatten(g, require_device_potentials=True)          # only for the numbering: rvs and factors in id order
        self.rvs, self.factors = fl.rvs, fl.factors
        self.V, self.F = len(self.rvs), len(self.factors)
        vi, fi = fl.var_index, fl.fac_index
        self.scope = [[vi[rv] for rv in f.nb] for f in self.factors]
        self.rows = [[fi[f] for f in rv.nb] for rv in self.rvs]                  # rv.nb order
        self.cont = [bool(rv.domain.continuous) for rv in self.rvs]
        self.cont_mask = np.array(self.cont, dtype=bool)
        self.hidden = [rv.value is None for rv in self.rvs]
        self.states = [None if rv.domain.continuous else tuple(float(s) for s in rv.domain.values) for rv in self.rvs]
        self.bounds = [(float(rv.domain.values[0]), float(rv.domain.values[1])) if rv.domain.continuous else None
                       for rv in self.rvs]
        has_cont = [any(self.cont[v] for v in sc) for sc in self.scope]
        has_hid = [any(self.hidden[v] for v in sc) for sc in self.scope]
        self.numeric = [f for f in range(self.F) if has_cont[f] and has_hid[f]]
        self.discrete = [f for f in range(self.F) if not has_cont[f] and has_hid[f]]
        self._is_disc = set(self.discrete)
        self.cls = [1 if type(f.potential) is MLNHardPotential else 2 if type(f.potential) is MLNPotential else 0
                    for f in self.factors]

    # ---- phi, terms, sums ------------------------------------------------------------------------------------------------------
    def _arg(self, v, val):
        val = float(val)
        return val if self.cont[v] or not val.is_integer() else int(val)

    def phi(self, f, x, sub=None):
        sub = sub or {}
        return self.factors[f].potential.get(tuple(self._arg(v, sub[v] if v in sub else x[v]) for v in self.scope[f]))

    @staticmethod
    def term(phi):
        return -700.0 if phi == 0 else math.log(phi)

    def _sum(self, terms, order=None):
        order = order or self.order
        if order == 'fsum':
            return math.fsum(terms)
        total = 0.0
        for t in (reversed(terms) if order == 'reversed' else terms):
            total += t
        return total

    def score(self, x, order=None):
        """(sum of the score terms of all factors, number of factors with phi == 0)"""
        phis = [self.phi(f, x) for f in range(self.F)]
        return self._sum([self.term(p) for p in phis], order), sum(1 for p in phis if p == 0)

    def union(self, vs):
        """the factors of the variables vs, each once, listed under the first variable that has it"""
        out = []
        for a, v in enumerate(vs):
            out.extend(f for f in self.rows[v] if not any(u in self.scope[f] for u in vs[:a]))
        return out

    def local_terms(self, x, vs, sub=None):
        return [self.term(self.phi(f, x, sub)) for f in self.union(vs)]

    def local_score(self, x, vs, sub=None):
        return self._sum(self.local_terms(x, vs, sub))

    def unsatisfied(self, x):
        hard = [f for f in self.discrete if self.cls[f] == 1 and self.phi(f, x) == 0]
        soft = [f for f in self.discrete if self.cls[f] == 2 and self.phi(f, x) == 1]
        return hard, soft

    # ---- the search -------------------------------------------------------------------------------------------------------------
    def init(self, seed, try_id):
        x = np.empty(self.V)
        for v, rv in enumerate(self.rvs):
            if not self.hidden[v]:
                x[v] = float(rv.value)
            elif self.cont[v]:
                lo, hi = self.bounds[v]
                x[v] = lo + (hi - lo) * init_draw(seed, v, try_id)
            else:
                x[v] = self.states[v][pick(init_draw(seed, v, try_id), len(self.states[v]))]
        return x

    @staticmethod
    def _kth(lst, k):
        return lst[k]

    @staticmethod
    def _roles(u):
        """(class draw, index draw, branch draw, walk-variable draw, radius draw, angle draw) = u0 .. u5"""
        return u

    def choose(self, x, flip, try_id, seed, epsilon, noise_std):
        """the drawn decisions of a flip: (hard, soft, clause, c_disc, walk, walk_k, noise, took_soft)"""
        hard, soft = self.unsatisfied(x)
        u_cls, u_idx, u_branch, u_var, u_rad, u_ang = self._roles(flip_draws(seed, flip, try_id))
        took_soft = None
        if hard:
            c, c_disc = self._kth(hard, pick(u_idx, len(hard))), True
        else:
            if len(soft) + len(self.numeric) == 0:
                raise ZeroDivisionError('try %d, flip %d: nothing to pick' % (try_id, flip))
            took_soft = u_cls < len(soft) / (len(soft) + len(self.numeric))
            if took_soft:
                c, c_disc = self._kth(soft, pick(u_idx, len(soft))), True
            else:
                c, c_disc = self._kth(self.numeric, pick(u_idx, len(self.numeric))), False
        nhv = sum(1 for v in self.scope[c] if self.hidden[v])
        walk = u_branch < epsilon
        return hard, soft, c, c_disc, walk, (pick(u_var, nhv) if walk else -1), box_muller(noise_std, u_rad, u_ang), took_soft

    def step(self, x, flip, try_id, seed, epsilon, noise_std):
        x = np.array(x, dtype=np.float64)
        hard, soft, c, c_disc, walk, walk_k, noise, took_soft = self.choose(x, flip, try_id, seed, epsilon, noise_std)
        return self._flip(x, hard, soft, c, c_disc, walk, walk_k, noise, took_soft)

    def replay_step(self, x, clause, walk, walk_k, noise):
        x = np.array(x, dtype=np.float64)
        hard, soft = self.unsatisfied(x)
        return self._flip(x, hard, soft, int(clause), int(clause) in self._is_disc, bool(walk), int(walk_k), float(noise), None)

    def _flip(self, x, hard, soft, c, c_disc, walk, walk_k, noise, took_soft):
        cache = {}

        def opt(key, fun, x0):
            if key not in cache:
                cache[key] = host_lbfgsb(fun, x0)
            return cache[key]

        def run(forced):
            dec = _Decider(forced, self._sum)
            nb = self.scope[c]
            hv = [v for v in nb if self.hidden[v]]
            hid_disc = any(not self.cont[v] for v in hv)
            post = x.copy()
            out = dict(hard=hard, soft=soft, clause=c, c_disc=c_disc, took_soft=took_soft, hv=hv, branch='walk' if walk else 'greedy',
                       walk_var=None, walk_val=None, cands=None, winner=-1, cur_local=None, accept=-1, numeric=None)
            if walk:
                v = hv[walk_k]
                if self.cont[v]:
                    val = opt(('phi', v), lambda z: -self.phi(c, x, {v: z[0]}), [x[v]])[0] + noise
                else:
                    val = 1.0 - x[v]
                post[v] = val
                out.update(walk_var=v, walk_val=val, changed=[v])
            else:
                cands, terms, best = [], [], None
                for k, v in enumerate(hv):
                    if self.cont[v]:
                        cand = opt(('local', v), lambda z, v=v: -self.local_score(x, [v], {v: z[0]}), [x[v]])[0]
                    else:
                        # the value of largest negated local score (the worst one), the first winning ties
                        cand = bn = None
                        for s in self.states[v]:
                            neg = [-t for t in self.local_terms(x, [v], {v: s})]
                            if bn is None or dec.gt(neg, bn, 'state', exact=True):
                                bn, cand = neg, s
                    terms.append(self.local_terms(x, nb, {v: cand}))
                    cands.append((v, cand, self._sum(terms[k])))
                    if best is None or dec.gt(terms[k], terms[best], 'cand', exact=not self.cont[v] and not self.cont[hv[best]]):
                        best = k
                bv, bval, bsc = cands[best]
                cur_terms = self.local_terms(x, nb)
                cur_local = self._sum(cur_terms)
                accept = c_disc or dec.gt(terms[best], cur_terms, 'accept', exact=not self.cont[bv])
                out.update(cands=cands, winner=best, cur_local=cur_local, accept=int(accept))
                if accept:
                    post[bv] = bval
                    out.update(changed=[bv])
                elif hid_disc:
                    out.update(numeric='noop', changed=[])
                else:
                    z = opt(('joint',), lambda z: -self.local_score(x, hv, dict(zip(hv, z))), [x[v] for v in hv])
                    post[hv] = z
                    out.update(numeric='joint', changed=list(hv))
            return Step(run, cont=self.cont_mask, pre=x, post=post, cmp=dec.log, **out)

        return run(())

    def run(self, seed, try_id, flips, epsilon, noise_std):
        """a free try: dict(init, steps, states [flips + 1, V], scores [flips + 1] (of states, own order), zeros)"""
        x = self.init(seed, try_id)
        states, steps = [x], []
        for j in range(flips):
            s = self.step(x, j, try_id, seed, epsilon, noise_std)
            steps.append(s)
            x = s.post
            states.append(x)
        sz = [self.score(s) for s in states]
        return dict(init=states[0], steps=steps, states=np.array(states), scores=np.array([a for a, _ in sz]),
                    zeros=np.array([b for _, b in sz]))


# ---- the rules of the comparison with a recorded trajectory ---------------------------------------------------------------------
def best_of(start_scores, start_states):
    """the best state of a try, the reference's way: the state at the START of a flip is taken when its score is strictly
    greater, so the first maximum wins and the state after the last flip is never looked at.  start_scores [flips]: the score at
    the start of each flip (init first)."""
    best, best_x = -np.inf, None
    for sc, st in zip(start_scores, start_states):
        if sc > best:
            best, best_x = sc, st
    return best, best_x


def likelihood_log(init, post, zero):
    """the likelihood column of time_log: tries in sequence; at the start of a flip the best score takes the start score if
    strictly greater; after the flip a row is logged if the new score beats the best: -score, or -inf where a factor vanishes"""
    out, best = [], -np.inf
    for i in range(post.shape[0]):
        for j in range(post.shape[1]):
            start = init[i] if j == 0 else post[i, j - 1]
            if start > best:
                best = start
            if post[i, j] > best:
                out.append(-np.inf if zero[i, j] > 0 else -float(post[i, j]))
    return out


def value_error(twin, v, got, want):
    """0 / inf for a discrete variable (exact), the relative error for a continuous one"""
    if not twin.cont[v]:
        return 0.0 if got == want else np.inf
    return abs(got - want) / max(1.0, abs(want))


def match_post(twin, pre, post, step):
    """None if post differs from pre outside the step's variables or misses a value by more than VAL_LOOSE (a discrete one at
    all); else the list of continuous errors of the moved variables"""
    same = np.ones(twin.V, dtype=bool)
    same[step.changed] = False
    if not np.array_equal(post[same], pre[same]):
        return None
    errs = []
    for v in step.changed:
        err = value_error(twin, v, post[v], step.post[v])
        if not err <= VAL_LOOSE:
            return None
        if twin.cont[v]:
            errs.append(err)
    return errs


def check_trajectory(twin, traj, seed, try_id, epsilon, noise_std):
    """traj: dict(x [flips + 1, V] the recorded states (init first), init_score, rec_score [flips], rec_zero [flips]).
    Every flip starts from the recorded pre-state.  Returns dict(flips, ambiguous, errs [continuous errors])."""
    xs = np.asarray(traj['x'])
    flips = xs.shape[0] - 1
    init = twin.init(seed, try_id)
    assert np.array_equal(xs[0], init), ('init', try_id, np.flatnonzero(xs[0] != init).tolist())
    obs = np.flatnonzero(~np.array(twin.hidden))
    assert np.array_equal(xs[:, obs], np.broadcast_to(init[obs], (flips + 1, obs.size))), ('observed value written', try_id)
    sc0, _ = twin.score(xs[0], 'fsum')
    assert abs(traj['init_score'] - sc0) <= 1e-9 * max(1.0, abs(sc0)), ('init score', try_id, traj['init_score'], sc0)
    ambiguous, tight, errs = 0, 0, []
    for j in range(flips):
        sc, nz = twin.score(xs[j + 1], 'fsum')
        assert abs(traj['rec_score'][j] - sc) <= 1e-9 * max(1.0, abs(sc)), ('rec_score', try_id, j, traj['rec_score'][j], sc)
        assert int(traj['rec_zero'][j]) == nz, ('rec_zero', try_id, j, int(traj['rec_zero'][j]), nz)
        s = twin.step(xs[j], j, try_id, seed, epsilon, noise_std)
        tight += s.tight
        if not s.tight:
            e = match_post(twin, xs[j], xs[j + 1], s)
            assert e is not None, ('flip', try_id, j, s.clause, s.branch, s.changed, xs[j + 1][s.changed].tolist(),
                                   s.post[s.changed].tolist(), np.flatnonzero(xs[j + 1] != xs[j]).tolist())
        else:
            # a tight flip may go either way at its tight comparisons; it counts as ambiguous only if that matters
            ambiguous += s.ambiguous
            e = None
            for r in s.reachable():
                e = match_post(twin, xs[j], xs[j + 1], r)
                if e is not None:
                    break
            assert e is not None, ('flip', 'tight: matches no alternative', try_id, j, s.clause, s.cmp)
        errs.extend(e)
    return dict(flips=flips, ambiguous=ambiguous, tight=tight, errs=errs)


def check_model_totals(stats):
    """over all tries of a model: ambiguous share <= 2 %, continuous values to 1e-7 in >= 95 % of the moves (1e-4 in all is
    asserted per flip).  Returns (ambiguous share, worst continuous error)."""
    flips = sum(s['flips'] for s in stats)
    amb = sum(s['ambiguous'] for s in stats)
    errs = np.array([e for s in stats for e in s['errs']])
    assert amb <= AMBIGUOUS_CAP * flips, ('ambiguous share', amb, flips)
    if errs.size:
        assert (errs <= VAL_TIGHT).mean() >= TIGHT_SHARE, ('continuous values', float((errs <= VAL_TIGHT).mean()), float(errs.max()))
    return amb / max(flips, 1), float(errs.max()) if errs.size else 0.0


def check_best(traj, best_score, best_x):
    """best_score / best_x of a try equal, bit for bit, best_of over the recorded scores and states"""
    xs = np.asarray(traj['x'])
    flips = xs.shape[0] - 1
    starts = [traj['init_score']] + [traj['rec_score'][j] for j in range(flips - 1)]
    want, want_x = best_of(starts[:flips], xs[:flips])
    assert best_score == want, ('best_score', best_score, want)
    assert want_x is not None and np.array_equal(best_x, want_x), ('best_x', np.flatnonzero(best_x != want_x).tolist())


# ---- the runs of the free-running check: the same on the CPU (ambiguity cap, coverage) and on the device ----------------------
SEED, TRY_IDS, EPSILON, NOISE_STD = 5, (0, 3, 4, 9, 1000), 0.5, 0.7
# name -> (builder in tests/mws_models.py, its arguments, flips per try)
CASES = {'many_63': ('many_clauses', (63,), 40), 'many_64': ('many_clauses', (64,), 40), 'many_65': ('many_clauses', (65,), 40),
         'many_130': ('many_clauses', (130,), 25), 'wide_hub': ('wide_hub', (), 25), 'multi_state': ('multi_state', (), 40),
         'shared_scope': ('shared_scope', (), 40), 'every_kind': ('every_kind', (), 40), 'small_hybrid': ('small_hybrid', (), 40),
         'robot_mapping': ('robot_mapping', (), 40)}
CPU_ONLY_CASES = {'paper_popularity': ('paper_popularity', (), 40)}          # its device run is the replay fixtures'


def build_case(name):
    import mws_models
    builder, args, flips = {**CASES, **CPU_ONLY_CASES}[name]
    return getattr(mws_models, builder)(*args), flips


def trajectory_of(run):
    """a twin's own free run in the shape check_trajectory / check_best take"""
    return dict(x=run['states'], init_score=run['scores'][0], rec_score=run['scores'][1:], rec_zero=run['zeros'][1:])
