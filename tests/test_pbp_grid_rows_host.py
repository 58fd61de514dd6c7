"""A NumPy model of the 64 lanes of ``grid_sums32_rows`` (csrc/pbp.hip): the integral-point sums of the heavy f -> v kernel,
S_t = sum_j G0_j q_j^t over a batch of 32 grid points, formed in quarter-wave lane groups.

Lane l = 16 k + c.  Starts: lane = partner j forms its value at batch points 0, 8, 16, 24 with q^4 = (q q)(q q), two
multiplications per eight points.  A 4 x 4 transpose across the four rows (``v_permlane32_swap`` then ``v_permlane16_swap``) and an
all-gather of q leave lane (k, c) with the value at point 8 k and the ratio of partners c, c + 16, c + 32, c + 48.  Eight points
per lane, four folds over lane bits 3, 2, 1, 0, and the lane pair (l, l ^ 1) owns point 8 k + bit3 + 2 bit2 + 4 bit1.

The model moves data exactly as the instructions do (swap: the lanes whose bit is clear end with (own x, partner's x), the others
with (partner's y, own y); fold: own kept value + the partner's copy of the same), in float64 and in the kernel's order of
operations up to the fused multiply-adds the compiler may form, which round once where the model rounds twice (inside the
bound either way).  No device, no ``lhvi`` import."""
import numpy as np
import pytest

import pbp_f2v_models as fm

LANE = np.arange(64)
NJS = (24, 25, 63, 64)


def _bit(b):
    return ((LANE >> b) & 1).astype(bool)


def swap(x, y, b):
    """v_permlane32_swap (b = 5) / v_permlane16_swap (b = 4) of the pair (x, y) [..., 64]"""
    p = LANE ^ (1 << b)
    return np.where(_bit(b), y[..., p], x), np.where(_bit(b), y, x[..., p])


def fold(x, y, b):
    """x is kept by the lanes whose bit b is clear, y by the others: own kept value + the partner's copy of the same"""
    p = LANE ^ (1 << b)
    return np.where(_bit(b), y + y[..., p], x + x[..., p])


def owned_point(lane):
    return 8 * (lane >> 4) + ((lane >> 3) & 1) + 2 * ((lane >> 2) & 1) + 4 * ((lane >> 1) & 1)


def gather_ratios(q):
    lo, hi = swap(q, q, 5)
    a, b = swap(lo, lo, 4)
    c, d = swap(hi, hi, 4)
    return [a, b, c, d]


def sums32_rows(g, q):
    """(the 64 lanes' sums, the lanes' value at the first point of the next batch) from G [..., 64] at the batch's first point"""
    g, q = np.asarray(g, dtype=np.float64), np.asarray(q, dtype=np.float64)
    with np.errstate(over='ignore', invalid='raise'):           # past the grid a product may overflow; nothing may be NaN
        qr = gather_ratios(q)
        q2 = q * q
        q4 = q2 * q2
        s = [g]
        for _ in range(3):
            s.append((s[-1] * q4) * q4)
        nxt = (s[3] * q4) * q4
        s[0], s[2] = swap(s[0], s[2], 5)
        s[1], s[3] = swap(s[1], s[3], 5)
        s[0], s[1] = swap(s[0], s[1], 4)
        s[2], s[3] = swap(s[2], s[3], 4)
        v = []
        for r in range(8):
            v.append((s[0] + s[1]) + (s[2] + s[3]))
            if r < 7:
                s = [a * b for a, b in zip(s, qr)]
        u = [fold(v[2 * i], v[2 * i + 1], 3) for i in range(4)]
        w = [fold(u[0], u[1], 2), fold(u[2], u[3], 2)]
        y = fold(w[0], w[1], 1)
        return fold(y, y, 0), nxt


def padded(nj, g, q):
    """lanes beyond nj contribute G0 = 0, q = 1"""
    keep = LANE < nj
    return np.where(keep, g, 0.0), np.where(keep, q, 1.0)


def test_every_point_is_owned_by_exactly_one_lane_pair():
    t = owned_point(LANE)
    assert sorted(t.tolist()) == sorted(list(range(32)) * 2)
    assert (t == t[LANE ^ 1]).all()
    assert sorted(t[::2].tolist()) == list(range(32))            # the even lanes, which store, cover the batch once


def test_transpose_and_gather_send_partner_16k_plus_c_to_slot_k():
    """the exchange alone, on tags: slot k' of lane (k, c) holds start value k of partner 16 k' + c, and that partner's ratio"""
    s = [1000.0 * LANE + m for m in range(4)]                   # tag: 1000 * partner + start index
    s[0], s[2] = swap(s[0], s[2], 5)
    s[1], s[3] = swap(s[1], s[3], 5)
    s[0], s[1] = swap(s[0], s[1], 4)
    s[2], s[3] = swap(s[2], s[3], 4)
    qr = gather_ratios(LANE.astype(np.float64))
    for kp in range(4):
        partner = 16 * kp + (LANE & 15)
        assert (s[kp] == 1000.0 * partner + (LANE >> 4)).all()
        assert (qr[kp] == partner).all()


@pytest.mark.parametrize('nj', NJS)
def test_every_sum_holds_each_partner_once(nj):
    """one-hot starts with q = 2: partner j alone gives S_t = 2^t exactly in every owning lane (the right power of the right
    partner, once), all partners together give nj 2^t, and a padding lane gives nothing"""
    g = np.eye(64)
    q = np.full((64, 64), 2.0)
    for j in range(64):
        g[j], q[j] = padded(nj, g[j], q[j])
    out, nxt = sums32_rows(g, q)
    t = owned_point(LANE)
    expect = np.where((np.arange(64) < nj)[:, None], 2.0 ** t[None, :], 0.0)
    assert (out == expect).all()
    assert (nxt == np.where(np.arange(64)[:, None] < nj, np.eye(64) * 2.0 ** 32, 0.0)).all()
    allg, allq = padded(nj, np.ones(64), np.full(64, 2.0))
    out, _ = sums32_rows(allg, allq)
    assert (out == nj * 2.0 ** t).all()


def _random_edge(rng, nj, T, scale):
    """records (a_j, b_j) of an edge whose exponents stay inside the range guard's 600 on the grid [-10, 10]"""
    x = np.linspace(-10.0, 10.0, T) if T > 1 else np.array([-10.0])
    a = rng.uniform(-1.0, 1.0, 64) * scale
    b = rng.uniform(-1.0, 1.0, 64) * (scale / 10.0 * 0.8)
    a, b = np.where(LANE < nj, a, 0.0), np.where(LANE < nj, b, 0.0)
    assert (np.abs(a) + np.abs(b) * 10.0 < 600.0).all()
    return a, b, x


@pytest.mark.parametrize('nj', NJS)
@pytest.mark.parametrize('T', [1, 7, 8, 9, 31, 32, 33, 64, 100, 128])
@pytest.mark.parametrize('scale', [3.0, 60.0, 330.0])
def test_error_against_longdouble_sum_stays_inside_the_recurrence_bound(nj, T, scale):
    """all batches of a grid of T points, G carried from batch to batch as the kernel does; points past the grid are formed and
    dropped (they may overflow), every kept sum is finite and within f2v_bound(..., 'recurrence') of the longdouble sum"""
    rng = np.random.default_rng(1000 * nj + T)
    a, b, x = _random_edge(rng, nj, T, scale)
    x0 = x[0]
    h = (x[-1] - x[0]) / (T - 1) if T > 1 else 0.0
    g, q = padded(nj, np.exp(b * x0 + a), np.exp(b * h))
    t_own = owned_point(LANE)
    got = np.full(T, np.nan)
    for t0 in range(0, T, 32):
        out, g = sums32_rows(g, q)
        assert (out == out[LANE ^ 1]).all()
        for lane in range(0, 64, 2):
            if t0 + t_own[lane] < T:
                got[t0 + t_own[lane]] = out[lane]
    assert np.isfinite(got).all() and (got > 0).all()
    LD = fm.LD
    xt = LD(x0) + np.arange(T).astype(LD) * LD(h)
    expo = a[:nj].astype(LD)[None, :] + b[:nj].astype(LD)[None, :] * xt[:, None]
    top = expo.max(axis=1)
    L = top + np.log(np.exp(expo - top[:, None]).sum(axis=1))
    M = float((np.abs(a) + np.abs(b) * np.abs(x).max()).max())
    bound = fm.f2v_bound(M, nj, L, 'recurrence', t=np.arange(T))
    err = np.abs(np.log(got.astype(LD)) - L).astype(np.float64)
    assert (err <= bound).all(), float((err / bound).max())


def test_start_powers_stay_finite_where_q8_would_not():
    """T = 9 on a wide grid: exp(8 b h) leaves the double range for an edge the guard admits (|b| X < 600); the steps of q^4 keep
    every value on the grid finite and accurate"""
    T, nj = 9, 64
    b = np.where(LANE % 2 == 0, 55.0, -55.0)
    a = np.where(LANE % 2 == 0, 20.0, -20.0)
    x = np.linspace(-10.0, 10.0, T)
    h = (x[-1] - x[0]) / (T - 1)
    with np.errstate(over='ignore', under='ignore'):
        assert not np.isfinite(np.exp(8 * 55.0 * h)) and np.exp(-8 * 55.0 * h) == 0.0
    g, q = np.exp(b * x[0] + a), np.exp(b * h)
    out, _ = sums32_rows(g, q)
    t_own = owned_point(LANE)
    LD = fm.LD
    for lane in range(0, 64, 2):
        t = t_own[lane]
        if t < T:
            expo = a.astype(LD) + b.astype(LD) * (LD(x[0]) + LD(t) * LD(h))
            L = expo.max() + np.log(np.exp(expo - expo.max()).sum())
            assert np.isfinite(out[lane])
            assert abs(np.log(LD(out[lane])) - L) <= fm.f2v_bound(570.0, nj, L, 'recurrence', t=t)
