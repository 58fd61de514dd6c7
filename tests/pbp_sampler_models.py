"""Host twin of the particle sampler of csrc/pbp.hip (``philox_normal_pair`` / ``philox_normal``, ``pbp_resample_kernel``,
``pbp_resample_uniq_kernel`` and step 3 of ``pbp_var_fused_kernel``), shared by tests/test_pbp_sampler_host.py and
tests/test_gpu_pbp_sampler.py.  Plain NumPy, vectorised over (variable, particle), written from the stream's specification and not
from the kernels:

  uniforms   Philox4x32-10 (``gibbs_models.philox4``, itself checked against the Random123 vectors), key = seed, counter words
             (gid & 0xffffffff, gid >> 32, block, iteration); r0 = words 0 and 1, r1 = words 2 and 3, high word first;
             u = (float64(r >> 11) + 0.5) * 2**-53 in float64 (for r >> 11 >= 2**52 the addition rounds to even: u is in (0, 1] and
             u = 1 at r >> 11 = 2**53 - 1 alone)
  block      particle j takes block (j & 31) | (j >> 6 << 5); bit 5 of j clear: the cosine normal, set: the sine normal
  normals    rad = sqrt(-2 ln u1), z = rad cos(2 pi u2) or rad sin(2 pi u2) = rad cos(2 pi (u2 - 1/4)), in ``np.longdouble`` with
             2 pi carried as the sum of two doubles
  particle   x = clip(mu + sqrt(var) z, lo, hi) + 0.0 for a hidden continuous variable; a hidden discrete variable's particles
             are its states; an observed variable (np = 0) has none; entries j >= np[v] are not written
  mask       uniq[v][j] = j < np[v] and no i < j with x[v][i] == x[v][j] (numeric equality)

The error bound ``z_bound``
---------------------------
The device forms z = fl(rad_dev * c_dev) with l_dev = log_table(u1) or log_pos(u1), rad_dev = sqrt_pos(-2 l_dev) and
c_dev = cos_turns(t), t = u2 or u2 - 1/4.  u1, u2 and t are exact (u2 is a multiple of 2**-54, so u2 - 1/4 is representable for
every u2 in (0, 1]).  With u = 2**-53:

* logarithm.  |l_dev - ln u1| <= dl, the bound tests/test_gpu_pbp.py::test_device_log_accuracy asserts for the routine:
  2.25 spacing(max(|l|, 1)) for the table log, 2 spacing(|l|) for the series log.  -2 l is exact, so the radicand is off by at
  most 2 dl and its exact square root by at most  drad = rad - sqrt(rad^2 - 2 dl)  (the downward case, the larger one), which is
  dl / rad (1 + O(dl / rad^2)): the "|dl| / rad" of the bound.  For small radii this term dominates -- next to u1 = 1 the table log
  is only absolutely accurate (dl = 5e-16), and the error of z is that divided by the radius.
* sqrt_pos.  The v_rsq_f64 seed has a relative error e <= 2**-23 (documented for the instruction: 2**29 ulp).  The coupled step
  gives g1 = s (1 - 3/2 e^2 + O(e^3)) and h1 = (1 - 3/2 e^2) / (2 s); the residual x - g1^2 is formed by one fma (relative rounding
  u of a quantity of relative size 3 e^2), so the correction leaves a relative error of O(e^4) + 3 e^2 u < 1e-27 before the last
  fma rounds: one rounding, relative error <= u (1 + 1e-9).
* cos_turns.  rint, the subtraction t - rint(t) (Sterbenz for t >= 1/2, else rint = 0) and 0.5 - tt (tt in (1/4, 1/2]) are exact:
  w in [0, 1/4] is exact and the true value is +- cos(a), a = 2 pi w <= pi / 2.  The kernel's a_dev = fl(w * fl(2 pi)) has a relative
  error <= u + rho, rho = 3.9e-17 the relative error of the double nearest 2 pi; z = fl(a_dev^2) adds u to the relative error of
  a^2, i.e. u / 2 to that of a.  d cos / da = -sin a, so the argument costs  a sin(a) (3/2 u + rho).  The series stops at a^22; the
  code states the remainder as < 2e-17 (the first omitted term, a^24 / 24! <= 8.3e-20, is smaller still).  Horner in fma form:
  step k (k = 11 .. 1) rounds p_k, |p_k| <= |c_k| = 1 / (2k)! (alternating, decreasing since a^2 / 12 < 1), and that error reaches the
  result multiplied by a^(2k): in all u sum_{k >= 1} a^(2k) / (2k)! <= u (cosh a - 1).  The coefficients from 1/4! on are rounded
  constants: u (cosh a - 1 - a^2 / 2) <= u a^4 cosh(a) / 24.  Together
      E_cos(a) = a sin(a) (3/2 u + rho) + 2e-17 + u ((cosh a - 1) + a^4 cosh(a) / 24)
  absolute, 5.4e-16 at a = pi / 2 and 2e-17 at a = 0, plus the rounding of the last Horner step, relative u.
* product.  z_dev = (rad + dr)(1 + e_s) (c + dc)(1 + e_f)(1 + e_m) with |dr| <= drad, |dc| <= E_cos and three relative roundings
  (sqrt_pos, the last Horner step, the multiplication) of at most u (1 + 1e-9) each; u |z| <= spacing(|z|).  Hence
      |z_dev - z| <= (|c| + E_cos) drad + rad E_cos + 3 spacing(|z|)                (k = 3)
  times (1 + 2**-40) for the products of two error terms.  (|c| <= 1 gives the coarser "dl / rad + rad E_cos + k spacing(|z|)".)
* reference.  The longdouble evaluation takes six operations of relative error 2**-64 or (the cosine) absolute error 2**-64 plus
  the error of the angle, 2 pi 2**-64 after the period is taken off: at most 2**-60 rad, which the bound includes and
  tests/test_pbp_sampler_host.py checks against mpmath at 200 bits.

The constants come from this argument alone; none is fitted to what a device returns.

For a general proposal the kernels form fma(sd, z, mu), sd = sqrt_pos(var) (or mu + sqrt(var) z, with or without contraction):
|x_dev - x| <= sqrt(var) z_bound + 2 spacing(|mu| + sqrt(var) |z|)  (``x_bound``; the 2 covers the rounding of sd, relative u, the
product's and the sum's).  Clipping is 1-Lipschitz, so the clipped values differ by no more; where the unclipped reference lies
further than the bound outside (inside) the domain, both are the bound itself (both are inside)."""
from collections import namedtuple

import numpy as np

from gibbs_models import philox4

LD = np.longdouble
U = 2.0 ** -53
TWO_PI_HI, TWO_PI_LO = 6.283185307179586, 2.4492935982947064e-16       # 2 pi = hi + lo to 107 bits
RHO_2PI = TWO_PI_LO / TWO_PI_HI
COS_REMAINDER = 2e-17
K_ROUNDINGS = 3.0
REF_ERROR = 2.0 ** -60              # of the longdouble reference, relative to the radius
SLOP = 1.0 + 2.0 ** -40
PATHS = ('table', 'series')
SENTINEL = -77.0                    # what the GPU tests fill the output buffers with
MASK_SENTINEL = 9


def block_of(j):
    j = np.asarray(j, dtype=np.int64)
    return (j & 31) | ((j >> 6) << 5)


def sine_of(j):
    return (np.asarray(j, dtype=np.int64) & 32) != 0


def uniform_of_bits(r):
    """the uniform of a 64-bit Philox output: float64 arithmetic throughout, the addition rounds to nearest even"""
    k = (np.asarray(r, dtype=np.uint64) >> np.uint64(11)).astype(np.float64)
    return (k + 0.5) * 2.0 ** -53


def uniforms(seed, gid, block, iteration):
    gid = np.asarray(gid).astype(np.uint64)
    c = philox4(gid & np.uint64(0xffffffff), gid >> np.uint64(32), np.asarray(block, dtype=np.uint64),
                np.asarray(int(iteration) & 0xffffffff, dtype=np.uint64), seed)
    return uniform_of_bits((c[0] << np.uint64(32)) | c[1]), uniform_of_bits((c[2] << np.uint64(32)) | c[3])


def box_muller(u1, u2, sine):
    """(rad, c, z) in longdouble: c = cos(2 pi u2), or sin(2 pi u2) taken as cos(2 pi (u2 - 1/4)); whole turns are taken off the
    exact argument first, which changes nothing but the rounding of the angle"""
    u1, u2 = np.asarray(u1, dtype=np.float64), np.asarray(u2, dtype=np.float64)
    rad = np.sqrt(LD(-2.0) * np.log(u1.astype(LD)))
    t = u2 - np.where(sine, 0.25, 0.0)              # exact
    t = (t - np.rint(t)).astype(LD)                 # exact, [-1/2, 1/2]
    c = np.cos(LD(TWO_PI_HI) * t + LD(TWO_PI_LO) * t)
    return rad, c, rad * c


Normals = namedtuple('Normals', 'u1 u2 sine rad c z')


def normals(seed, gid, n, iteration):
    """the n standard normals of every variable: arrays [V, n] (z, rad, c longdouble)"""
    gid = np.asarray(gid).reshape(-1, 1)
    j = np.arange(n)[None, :]
    u1, u2 = uniforms(seed, gid, block_of(j), iteration)
    sine = np.broadcast_to(sine_of(j), u1.shape)
    return Normals(u1, u2, sine, *box_muller(u1, u2, sine))


def folded_angle(u2, sine):
    """a = 2 pi w, w the distance of the argument to the nearest multiple of a half turn ... folded into [0, 1/4] (float64, exact up
    to the last product: it only feeds the bound)"""
    t = np.asarray(u2, dtype=np.float64) - np.where(sine, 0.25, 0.0)
    tt = np.abs(t - np.rint(t))
    return TWO_PI_HI * np.where(tt > 0.25, 0.5 - tt, tt)


def log_bound(l, path):
    l = np.abs(np.asarray(l, dtype=np.float64))
    if path == 'table':
        return 2.25 * np.spacing(np.maximum(l, 1.0))
    if path == 'series':
        return 2.0 * np.spacing(l)
    raise ValueError(path)


def cos_error(a):
    a = np.asarray(a, dtype=np.float64)
    cosh_m1 = 2.0 * np.sinh(0.5 * a) ** 2
    return a * np.sin(a) * (1.5 * U + RHO_2PI) + COS_REMAINDER + U * (cosh_m1 + a ** 4 * np.cosh(a) / 24.0)


def z_bound(u1, u2, path, sine=False):
    """bound on |z_dev - z| (module docstring); `path`: which logarithm the kernel took; `sine`: which normal of the block"""
    u1, u2 = np.asarray(u1, dtype=np.float64), np.asarray(u2, dtype=np.float64)
    rad, c, z = box_muller(u1, u2, sine)
    rad, c, z = rad.astype(np.float64), np.abs(c.astype(np.float64)), np.abs(z.astype(np.float64))
    dl = log_bound(0.5 * rad * rad * (1.0 + 2.0 ** -50), path)      # (the factor: |l| from the rounded radius must not fall into the binade below)
    with np.errstate(invalid='ignore', divide='ignore'):
        # rad - sqrt(rad^2 - 2 dl), in the form without cancellation
        drad = np.where(rad * rad > 2.0 * dl, 2.0 * dl / (rad + np.sqrt(np.maximum(rad * rad - 2.0 * dl, 0.0))), np.inf)
    e = cos_error(folded_angle(u2, sine))
    return ((c + e) * drad + rad * e + K_ROUNDINGS * np.spacing(z) + REF_ERROR * rad) * SLOP


def x_bound(zb, z, mu, var):
    sd = np.sqrt(np.asarray(var, dtype=np.float64))
    return sd * zb + 2.0 * np.spacing(np.abs(mu) + sd * np.abs(np.asarray(z, dtype=np.float64)))


def first_occurrence(x, npv):
    """uniq [V, n] by the definition, for every row: stable sort, then 'equal to the entry before' marks all but the first of a
    group of numerically equal particles (-0.0 == 0.0)"""
    x = np.array(x, dtype=np.float64)
    V, n = x.shape
    live = np.arange(n)[None, :] < np.asarray(npv).reshape(-1, 1)
    x[~live] = np.nan                                   # equal to nothing
    order = np.argsort(x, axis=1, kind='stable')
    xs = np.take_along_axis(x, order, axis=1)
    dup_sorted = np.zeros((V, n), dtype=bool)
    dup_sorted[:, 1:] = xs[:, 1:] == xs[:, :-1]
    dup = np.zeros((V, n), dtype=bool)
    np.put_along_axis(dup, order, dup_sorted, axis=1)
    return live & ~dup


def first_occurrence_by_loops(x, npv):
    return np.array([[j < npv[v] and not any(x[v, i] == x[v, j] for i in range(j)) for j in range(x.shape[1])]
                     for v in range(x.shape[0])], dtype=bool).reshape(x.shape)


# ---- hand-built variable layouts ---------------------------------------------------------------------------------------------
class Layout:
    """variables in a chosen order.  `classes [V]`: index into `domains`, or -1 - index for a variable observed on that domain;
    `domains`: (lo, hi) of a continuous domain or the states of a discrete one; `dom_cont`: which are continuous (default: the
    tuples of length two)"""

    def __init__(self, domains, classes, dom_cont=None):
        self.domains, self.classes = list(domains), np.asarray(classes, dtype=np.int64)
        self.V = self.classes.size
        self.var_dom = np.where(self.classes >= 0, self.classes, -1 - self.classes).astype(np.int32)
        self.dom_cont = np.array([len(d) == 2 for d in self.domains]) if dom_cont is None else np.asarray(dom_cont, dtype=bool)
        self.observed = self.classes < 0
        self.cont = self.dom_cont[self.var_dom] & ~self.observed           # hidden continuous
        self.disc = ~self.dom_cont[self.var_dom] & ~self.observed
        self.lo = np.array([d[0] if c else 0.0 for d, c in zip(self.domains, self.dom_cont)])[self.var_dom]
        self.hi = np.array([d[1] if c else 0.0 for d, c in zip(self.domains, self.dom_cont)])[self.var_dom]

    def np_of(self, n):
        nst = np.array([len(d) for d in self.domains])[self.var_dom]
        return np.where(self.observed, 0, np.where(self.cont, n, nst)).astype(np.int32)

    def var_value(self):
        first = np.array([0.5 * (d[0] + d[1]) if c else d[0] for d, c in zip(self.domains, self.dom_cont)])[self.var_dom]
        return np.where(self.observed, first, np.nan)


Draw = namedtuple('Draw', 'x ref tol written undecided exact z zb')


def draw(layout, n, seed, iteration, q, gid=None, path='table', rows=None):
    """what a sampler call leaves in a sentinel-filled particle buffer [V, n].
    ref: the expected value in longdouble (the sentinel where nothing is written), x: ref rounded to float64 (exact where
    `exact`), tol: the bound on |x_dev - ref| (0 where exact), written: entries the call writes, undecided: drawn entries whose unclipped reference lies within
    the bound of lo or hi (either side may clip; the tolerance still holds).  `rows`: the variables the call covers (default all)."""
    V = layout.V
    gid = np.arange(V) if gid is None else np.asarray(gid)
    npv = layout.np_of(n)
    q = np.asarray(q, dtype=np.float64)
    nm = normals(seed, gid, n, iteration)
    zb = z_bound(nm.u1, nm.u2, path, nm.sine)
    mu, var = q[:, 0:1], q[:, 1:2]
    raw = mu.astype(LD) + np.sqrt(var.astype(LD)) * nm.z
    xb = x_bound(zb, nm.z, mu, var)
    lo, hi = layout.lo[:, None], layout.hi[:, None]
    below, above = raw < lo - xb, raw > hi + xb
    inside = (raw > lo + xb) & (raw < hi - xb)
    cont = np.broadcast_to(layout.cont[:, None], raw.shape)
    x = np.clip(raw, lo.astype(LD), hi.astype(LD)) + LD(0.0)
    tol = np.where(below | above, 0.0, xb)
    exact = ~cont | below | above
    for v in np.flatnonzero(layout.disc):
        st = np.asarray(layout.domains[layout.var_dom[v]], dtype=np.float64)
        x[v, :st.size], tol[v] = st, 0.0
    covered = np.zeros(V, dtype=bool)
    covered[np.arange(V) if rows is None else np.asarray(rows)] = True
    written = (np.arange(n)[None, :] < npv[:, None]) & covered[:, None]
    x, tol = np.where(written, x, LD(SENTINEL)), np.where(written, tol, 0.0)
    undecided = written & cont & ~(below | above | inside)
    return Draw(x.astype(np.float64), x, tol, written, undecided, exact | ~written, nm.z, zb)


# ---- the cases of tests/test_gpu_pbp_sampler.py: everything but the device calls, so that the host tests can check the clip
# condition (no drawn entry undecided) for every one of them -----------------------------------------------------------------------
RAW_DOMAIN = (-100.0, 100.0)
RAW_V = 1001
RAW_SEED, RAW_ITERATION = 20261, 3
RAW_FUSED_N, RAW_GENERAL_N, RAW_PLAIN_N = (1, 2, 31, 32, 33, 63, 64), (65, 100, 128, 129), (10, 64, 100)

COUNTER_SEEDS = (0, 1, 2 ** 32, 2 ** 64 - 1)
COUNTER_ITERATIONS = (0, 1, 2 ** 31, 2 ** 32 - 1)
# two variables share gid 1 (rows 1 and 8: with the list or the range starting at 0 the first sits in the second half of its
# wavefront and the other in the first half; a range starting at 1 exchanges them); rows 0 / 3 and 1 / 4 differ in the high word only
COUNTER_GIDS = np.array([0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 7, 2 ** 63 - 1, 5, 1, 2 ** 40 + 7], dtype=np.int64)
COUNTER_SHARED = ((1, 8), (5, 9))
COUNTER_HIGH_ONLY = ((0, 3), (1, 4))
COUNTER_Q = (0.5, 2.0)
COUNTER_DOMAIN = (-10.0, 10.0)

LOOP_SEED, LOOP_ITERATION = 5, 2
LOOP_DOMAIN = (-10.0, 10.0)

PAIR_DOMAINS = [(-10.0, 10.0), (0.0, 1.0), (-1e3, 1e-3), (0.0, 1.0, 2.0), (3.0, 5.0, 7.0, 11.0, 13.0)]
PAIR_CLASSES = (0, 1, 2, 3, 4, -1, -4)          # three continuous, two discrete, observed on domain 0 (continuous) / on domain 3 (discrete)
PAIR_SEED, PAIR_ITERATION = 77, 6
PAIR_N = (64, 33, 6, 100)


def raw_case(n):
    lay = Layout([RAW_DOMAIN], np.zeros(RAW_V, dtype=np.int64))
    return lay, np.tile([0.0, 1.0], (RAW_V, 1))


def counter_case():
    lay = Layout([COUNTER_DOMAIN], np.zeros(COUNTER_GIDS.size, dtype=np.int64))
    return lay, np.tile(COUNTER_Q, (lay.V, 1))


def loop_case(cus):
    V = 160 * cus + 3
    lay = Layout([LOOP_DOMAIN], np.zeros(V, dtype=np.int64))
    rng = np.random.default_rng(11)
    q = np.stack([rng.uniform(-12, 12, V), np.where(rng.random(V) < 0.5, 400.0, 0.01)], axis=1)
    return lay, q


def pair_case():
    """every ordered pair of PAIR_CLASSES as neighbours (2k, 2k + 1), one padding variable, then the same pairs again -- at
    (2k + 1, 2k + 2): a range that starts at an even variable meets the first set as wavefront halves, one that starts at an odd
    variable the second.  Every continuous variable gets a proposal of its own, inside its domain and narrow enough not to clip
    (the clipped rows are test e's)."""
    pairs = [(a, b) for a in PAIR_CLASSES for b in PAIR_CLASSES]
    seq = [c for p in pairs for c in p] + [0] + [c for p in pairs for c in p]
    lay = Layout(PAIR_DOMAINS, seq)
    rng = np.random.default_rng(3)
    width = np.where(lay.cont, lay.hi - lay.lo, 1.0)
    mu = np.where(lay.cont, lay.lo + width * rng.uniform(0.4, 0.6, lay.V), 0.0)
    q = np.stack([mu, (width * rng.uniform(0.01, 0.03, lay.V)) ** 2], axis=1)
    return lay, q, pairs


CLIP_DOMAINS = [(-10.0, 10.0), (-4.0, -0.0), (0.0, 1.0)]
CLIP_SEED, CLIP_ITERATION = 12, 9
CLIP_N = (2, 33, 48, 64, 100)
# (domain, mu, var, what) -- rows 8 .. 11: a pair whose first half is all duplicates and whose second has none, and the reverse
CLIP_ROWS = [
    (0, -60.0, 4.0, 'low'),            # the whole row clipped to lo
    (0, 70.0, 9.0, 'high'),            # ... to hi
    (0, 10.5, 1.0, 'some high'),       # duplicates at hi only
    (0, 0.3, 1e-300, 'point'),         # every draw is mu
    (0, 15.0, 0.25, 'high'),           # mu outside the domain
    (0, -0.0, 1.0, 'none'),            # mu = -0.0
    (1, 3.0, 0.01, 'high'),            # hi = -0.0: the clipped particles are +0.0 in the fused path
    (2, 0.5, 1e-4, 'none'),
    (0, 40.0, 1.0, 'high'), (0, 1.0, 1.0, 'none'),
    (0, -1.0, 2.0, 'none'), (0, -40.0, 1.0, 'low'),
    (2, -7.0, 1.0, 'low'),
]


def clip_case():
    lay = Layout(CLIP_DOMAINS, [r[0] for r in CLIP_ROWS])
    return lay, np.array([[r[1], r[2]] for r in CLIP_ROWS]), [r[3] for r in CLIP_ROWS]


GENERAL_DOMAINS = [(-10.0, 10.0), (0.0, 1.0), (-1e3, 1e-3)]
GENERAL_V = 999
GENERAL_SEED, GENERAL_ITERATION = 2 ** 33 + 5, 40
GENERAL_N = (64, 48, 100)


def general_case():
    """general proposals: every continuous domain, the mean anywhere inside or a little outside, standard deviations from a
    thousandth of the width to twice the width"""
    rng = np.random.default_rng(8)
    lay = Layout(GENERAL_DOMAINS, rng.integers(0, 3, GENERAL_V))
    width = lay.hi - lay.lo
    mu = lay.lo + width * rng.uniform(-0.2, 1.2, lay.V)
    sd = width * np.exp(rng.uniform(np.log(1e-3), np.log(2.0), lay.V))
    return lay, np.stack([mu, sd * sd], axis=1), (np.arange(lay.V, dtype=np.int64) * (2 ** 32 + 3) + 2 ** 45)


FUSED_SEED = 2 ** 32 + 6
FUSED_CASES = {'n16': (16, 3001, 31), 'n32': (32, 3001, 31), 'n64': (64, 3000, 37)}      # n, V, graph seed (synth.hybrid_mrf_flat)
FUSED_Q0 = (0.0, 5.0)                       # lhvi_pbp_init
FUSED_DOMAIN = (-10.0, 10.0)                # synth.hybrid_mrf_flat's continuous domain


def fused_gids(V):
    return np.arange(V, dtype=np.int64) * (2 ** 32 + 1) + (2 ** 40 + 7)


def host_checkable_cases(cus=256):
    """(name, layout, n, seed, iteration, q, gid, path) of every draw of the GPU tests whose inputs are fixed on the host (the
    persistent-loop case for the MI355X's 256 compute units)"""
    out = []
    lay, q = raw_case(0)
    for n in RAW_FUSED_N:
        out.append(('raw uniq n%d' % n, lay, n, RAW_SEED, RAW_ITERATION, q, None, 'table'))
    for n in RAW_GENERAL_N + RAW_PLAIN_N:
        out.append(('raw series n%d' % n, lay, n, RAW_SEED, RAW_ITERATION, q, None, 'series'))
    lay, q = counter_case()
    for seed in COUNTER_SEEDS:
        for it in COUNTER_ITERATIONS:
            out.append(('counter %d %d' % (seed, it), lay, 64, seed, it, q, COUNTER_GIDS, 'table'))
    lay, q = loop_case(cus)
    out.append(('loop', lay, 64, LOOP_SEED, LOOP_ITERATION, q, None, 'table'))
    lay, q, _ = pair_case()
    for n in PAIR_N:
        out.append(('pairs n%d' % n, lay, n, PAIR_SEED, PAIR_ITERATION, q, None, 'table' if n <= 64 else 'series'))
    lay, q, _ = clip_case()
    for n in CLIP_N:
        out.append(('clip n%d' % n, lay, n, CLIP_SEED, CLIP_ITERATION, q, None, 'table' if n <= 64 else 'series'))
    lay, q, gid = general_case()
    for n in GENERAL_N:
        for path in (('table', 'series') if n <= 64 else ('series',)):
            out.append(('general n%d %s' % (n, path), lay, n, GENERAL_SEED, GENERAL_ITERATION, q, gid, path))
    for name, (n, V, _) in FUSED_CASES.items():
        lay = Layout([FUSED_DOMAIN], np.zeros(V, dtype=np.int64))
        out.append(('fused first draw ' + name, lay, n, FUSED_SEED, 0, np.tile(FUSED_Q0, (V, 1)), fused_gids(V), 'table'))
    return out
