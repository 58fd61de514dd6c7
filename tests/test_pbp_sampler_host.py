"""CPU tests of the particle sampler's host twin (tests/pbp_sampler_models.py): that the twin states the stream of include/lhvi.h,
that its longdouble reference is as accurate as its bound assumes, that its normals are normal, that none of the draws the GPU
tests compare is undecided at a domain bound, and that each defect the GPU tests are there to catch moves a draw by more than the
bound."""
import functools

import numpy as np
import pytest

import pbp_sampler_models as sm

LD = np.longdouble


@functools.lru_cache(maxsize=None)
def batch():
    """2.56 M draws: 40 000 variables x 64 particles"""
    return sm.normals(seed=2026, gid=np.arange(40000, dtype=np.int64) + 2 ** 33, n=64, iteration=7)


def test_block_and_branch_of_a_particle():
    j = np.arange(256)
    blk, sine = sm.block_of(j), sm.sine_of(j)
    assert len(set(zip(blk.tolist(), sine.tolist()))) == 256                # distinct draws
    assert blk.max() == 127 and (blk[:32] == np.arange(32)).all() and (blk[64:96] == 32 + np.arange(32)).all()
    for k in range(256):
        if not k & 32:
            assert blk[k] == blk[k + 32] and not sine[k] and sine[k + 32]   # j and j + 32: one block, cosine and sine
    assert (~sine[:32]).all() and sine[32:64].all() and (~sine[64:96]).all()


def test_uniform_of_bits_on_edge_integers():
    top = 2 ** 53 - 1
    ks = [0, 1, 2, 2 ** 51, 2 ** 52 - 1, 2 ** 52, 2 ** 52 + 1, 2 ** 52 + 2, 2 ** 53 - 3, 2 ** 53 - 2, top]
    r = np.array([(k << 11) | low for k in ks for low in (0, 0x7ff)], dtype=np.uint64)
    u = sm.uniform_of_bits(r)
    k = np.repeat(np.array(ks, dtype=object), 2)
    assert (u > 0).all() and (u <= 1).all()
    assert ((u == 1.0) == np.array([x == top for x in k])).all()            # u = 1 at the last integer alone
    assert u[0] == 2.0 ** -54 and u[2] == 1.5 * 2.0 ** -53
    # below 2**52 the sum is exact; from there on it is rounded to even -- as the kernel's float64 addition does, not "corrected"
    for x, got in zip(k, u):
        want = (2 * x + 1) * 2.0 ** -54 if x < 2 ** 52 else float(x + (x & 1)) * 2.0 ** -53
        assert got == want, x
    assert sm.uniform_of_bits(np.uint64((2 ** 52 + 1) << 11)) == (2 ** 52 + 2) * 2.0 ** -53


def test_uniforms_take_all_counter_and_key_words():
    """every word of the counter and of the key changes the block; the block is what gibbs_models.philox4 gives for
    (gid low, gid high, block, iteration) under key = seed"""
    from gibbs_models import philox4
    base = dict(seed=2 ** 40 + 3, gid=np.array([2 ** 35 + 9]), block=5, iteration=17)
    u = sm.uniforms(**base)
    c = philox4(9, 8, 5, 17, 2 ** 40 + 3)
    r0, r1 = (int(c[0]) << 32) | int(c[1]), (int(c[2]) << 32) | int(c[3])
    assert u[0][0] == ((r0 >> 11) + 0.5) * 2.0 ** -53 and u[1][0] == ((r1 >> 11) + 0.5) * 2.0 ** -53
    for name, other in (('seed', 3), ('seed', 2 ** 40 + 2), ('gid', np.array([9])), ('gid', np.array([2 ** 35 + 8])), ('block', 4),
                        ('iteration', 16), ('iteration', 17 + 2 ** 31)):
        v = sm.uniforms(**{**base, name: other})
        assert v[0][0] != u[0][0] and v[1][0] != u[1][0], (name, other)
    assert sm.uniforms(1, np.array([2 ** 63 - 1]), 0, 2 ** 32 - 1)[0].shape == (1,)


def _mp_exact(x):
    import mpmath
    hi = float(x)
    return mpmath.mpf(hi) + mpmath.mpf(float(x - LD(hi)))


def test_longdouble_reference_against_mpmath_on_the_extremes():
    """the 100 smallest and 100 largest radii of the batch and the 100 angles nearest each quarter turn, at 200 bits"""
    import mpmath
    b = batch()
    u1, u2 = b.u1.ravel(), b.u2.ravel()
    pick = [np.argsort(u1)[:100], np.argsort(u1)[-100:]]
    for quarter in (0.0, 0.25, 0.5, 0.75, 1.0):
        pick.append(np.argsort(np.abs(u2 - quarter))[:100])
    pick = np.unique(np.concatenate(pick))
    worst = 0.0
    with mpmath.workprec(200):
        for i in pick:
            rad = mpmath.sqrt(-2 * mpmath.log(mpmath.mpf(float(u1[i]))))
            ang = 2 * mpmath.pi * mpmath.mpf(float(u2[i]))
            want = rad * (mpmath.sin(ang) if b.sine.ravel()[i] else mpmath.cos(ang))
            err = abs(_mp_exact(b.z.ravel()[i]) - want)
            worst = max(worst, float(err))
            assert err <= 1e-17 and err <= sm.REF_ERROR * rad, (i, float(err), float(rad))
    print('longdouble reference: largest error over %d extremes %.3g' % (pick.size, worst))


def test_twin_normals_are_standard_normal():
    b = batch()
    z = b.z.astype(np.float64)
    N = z.size
    assert abs(z.mean()) < 5 / np.sqrt(N) and abs(z.var() - 1) < 5 * np.sqrt(2 / N)
    assert abs((z ** 3).mean()) < 5 * np.sqrt(15 / N) and abs((z ** 4).mean() - 3) < 5 * np.sqrt(96 / N)
    a, s = z[:, :32].ravel(), z[:, 32:].ravel()                                # the cosine and the sine normals of the same blocks
    assert abs(np.corrcoef(a, s)[0, 1]) < 5 / np.sqrt(a.size) and abs(np.corrcoef(a * a, s * s)[0, 1]) < 5 / np.sqrt(a.size)
    assert abs((z > 0).mean() - 0.5) < 5 * 0.5 / np.sqrt(N) and abs((np.abs(z) < 1).mean() - 0.6826894921) < 5 * 0.47 / np.sqrt(N)
    assert abs((z[:, :32] > 0).mean() - 0.5) < 0.002 and abs((z[:, 32:] > 0).mean() - 0.5) < 0.002     # the sign of either branch


def test_bound_is_finite_small_and_largest_at_small_radii():
    """what the bound says about "absolute error < 1e-15 on z": false for small radii, where the table log's absolute error is
    divided by the radius, and not guaranteed at the large ones next to a quarter turn either"""
    b = batch()
    zt, zs = sm.z_bound(b.u1, b.u2, 'table', b.sine), sm.z_bound(b.u1, b.u2, 'series', b.sine)
    for path, zb in zip(sm.PATHS, (zt, zs)):
        assert np.isfinite(zb).all() and zb.min() > 0 and zb.max() < 1e-11, (path, zb.max())
        print('z_bound (%s): median %.3g, largest %.3g at radius %.3g' % (path, np.median(zb), zb.max(), float(b.rad.ravel()[zb.argmax()])))
    small = b.rad.astype(np.float64) < 0.01
    assert small.sum() > 50 and np.median(zt[small]) > 1e-14 and zt[small].max() > 1e-13 and (zs[small] < zt[small]).all()
    assert np.median(zt) < 2e-15 and (zt > 1e-15).mean() > 0.1
    # the coarser form of the bound, with |c| <= 1
    rad = b.rad.astype(np.float64)
    coarse = sm.log_bound(0.5 * rad * rad, 'table') / rad + rad * sm.cos_error(sm.folded_angle(b.u2, b.sine)) + \
        sm.K_ROUNDINGS * np.spacing(np.abs(b.z.astype(np.float64))) + sm.REF_ERROR * rad
    assert (zt <= coarse * (1 + 1e-6)).all()


def test_first_occurrence_equals_the_definition_row_by_row():
    rng = np.random.default_rng(0)
    x = rng.integers(0, 6, (40, 17)).astype(np.float64)
    x[3, 2], x[3, 9] = -0.0, 0.0
    x[5] = 1.5
    npv = rng.integers(0, 18, 40)
    npv[5] = 17
    got = sm.first_occurrence(x, npv)
    assert (got == sm.first_occurrence_by_loops(x, npv)).all()
    assert got[5].tolist() == [True] + [False] * 16 and not got[3, 9] and not got[:, :][npv == 0].any()


def test_layout_and_draw_write_what_the_kernels_write():
    lay, q, pairs = sm.pair_case()
    assert len(pairs) == 49 and lay.V == 197
    # every ordered pair of classes sits at (even, odd) and at (odd, even) positions
    cls = lay.classes
    for start in (0, 1):
        seen = {(int(cls[k]), int(cls[k + 1])) for k in range(start, lay.V - 1, 2)}
        assert seen >= set(pairs), start
    d = sm.draw(lay, 6, sm.PAIR_SEED, sm.PAIR_ITERATION, q)
    npv = lay.np_of(6)
    assert (npv[lay.observed] == 0).all() and (npv[lay.cont] == 6).all() and set(npv[lay.disc]) == {3, 5}
    assert (d.x[lay.observed] == sm.SENTINEL).all() and not d.written[lay.observed].any()
    v = int(np.flatnonzero(lay.disc & (npv == 3))[0])
    assert d.x[v].tolist() == [0.0, 1.0, 2.0] + [sm.SENTINEL] * 3 and (d.tol[v] == 0).all()
    part = sm.draw(lay, 6, sm.PAIR_SEED, sm.PAIR_ITERATION, q, rows=np.arange(1, lay.V))
    assert (part.x[0] == sm.SENTINEL).all() and (part.x[1:] == d.x[1:]).all()
    lay, q, what = sm.clip_case()
    d = sm.draw(lay, 64, sm.CLIP_SEED, sm.CLIP_ITERATION, q)
    for v, w in enumerate(what):
        at_lo, at_hi = d.exact[v] & (d.x[v] == lay.lo[v]), d.exact[v] & (d.x[v] == lay.hi[v])
        assert {'low': at_lo.all(), 'high': at_hi.all(), 'some high': 5 < at_hi.sum() < 60 and not at_lo.any(),
                'point': (d.x[v] == q[v, 0]).all(), 'none': not (at_lo | at_hi).any()}[w], (v, w)
    assert not np.signbit(d.x[6]).any() and (d.x[6] == 0.0).all()            # hi = -0.0: the particles are +0.0


@pytest.mark.parametrize('group', ['raw', 'counter', 'loop', 'pairs', 'clip', 'general', 'fused'])
def test_clip_condition_of_every_gpu_case(group):
    """no draw the GPU tests compare has its unclipped reference within the bound of lo or hi: device and twin clip the same
    entries, so a clipped entry is the bound bit for bit and every other one is inside on both sides"""
    cases = [c for c in sm.host_checkable_cases() if c[0].startswith(group)]
    assert cases
    for name, lay, n, seed, iteration, q, gid, path in cases:
        d = sm.draw(lay, n, seed, iteration, q, gid, path)
        assert int(d.undecided.sum()) == 0, (name, int(d.undecided.sum()))
        assert np.isfinite(d.tol).all()


def _moved(a, b, bound):
    """fraction of entries that differ by more than the bound"""
    return float((np.abs(a - b) > bound).mean())


def test_each_listed_defect_moves_draws_by_more_than_the_bound():
    """the twin with one defect built in against the twin: what the GPU comparison would see if a kernel had that defect"""
    n, seed, it = 128, 2 ** 32 + 9, 5
    gid = np.arange(300, dtype=np.int64) * (2 ** 32 + 1) + 2 ** 40
    good = sm.normals(seed, gid, n, it)
    zb = sm.z_bound(good.u1, good.u2, 'table', good.sine)
    z = good.z
    assert _moved(sm.normals(seed, gid, n, 0).z, z, zb) > 0.999                           # iteration never reaches the counter
    assert _moved(sm.normals(seed, gid & 0xffffffff, n, it).z, z, zb) > 0.999            # the high word of the gid is dropped
    assert _moved(sm.normals(seed & 0xffffffff, gid, n, it).z, z, zb) > 0.999            # ... of the seed
    lost = np.concatenate([z[:, :64], z[:, :64]], axis=1)                                # (j >> 6) << 5 lost: j + 64 repeats j
    assert _moved(lost[:, 64:], z[:, 64:], zb[:, 64:]) > 0.999 and _moved(lost[:, :64], z[:, :64], zb[:, :64]) == 0
    flipped = np.where(good.sine, -z, z)                                                 # the sine with the wrong sign
    assert _moved(flipped[good.sine], z[good.sine], zb[good.sine]) > 0.999
    quadrant = np.where(good.sine, sm.box_muller(good.u1, good.u2 + 0.25, good.sine)[2], z)      # ... in the wrong quadrant
    assert _moved(quadrant[good.sine], z[good.sine], zb[good.sine]) > 0.999
    swapped = np.concatenate([z[:, 32:64], z[:, :32], z[:, 96:], z[:, 64:96]], axis=1)    # cosine and sine exchanged
    assert _moved(swapped, z, zb) > 0.999
    # the two halves of a wavefront take each other's lo / hi
    lay, q, _ = sm.pair_case()
    d = sm.draw(lay, 64, sm.PAIR_SEED, sm.PAIR_ITERATION, q)
    other = np.arange(lay.V) ^ 1
    other[other >= lay.V] = lay.V - 1
    pairs = np.flatnonzero(lay.cont & lay.cont[other] & (lay.var_dom != lay.var_dom[other]))
    assert pairs.size > 10
    raw = q[pairs, 0:1] + np.sqrt(q[pairs, 1:2]) * d.z[pairs].astype(np.float64)
    wrong = np.clip(raw, lay.lo[other[pairs], None], lay.hi[other[pairs], None])
    assert ((np.abs(wrong - d.x[pairs]) > d.tol[pairs]).any(axis=1)).mean() > 0.5
