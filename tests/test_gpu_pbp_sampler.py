"""GPU: the particle sampler of csrc/pbp.hip draw by draw against its host twin (tests/pbp_sampler_models.py): the Philox counter
and key words, block and branch of every particle, the Box-Muller normals within the twin's derived bound, the transformed and
clipped particles, the first-occurrence masks by their definition, the persistent loop of ``pbp_resample_uniq_kernel`` beyond one
round, every pairing of variable classes in its two wavefront halves, and the plumbing of gid / seed / iteration into the fused
per-variable kernels.  The graphs are built by hand (``build_flat``, one unary factor per variable) so that the order of the
variables and of their domains is chosen."""
import numpy as np
import pytest

import pbp_sampler_models as sm

pytestmark = pytest.mark.gpu

LD = np.longdouble
X2, TABLE = 6, 1                    # potential kinds (lhvi/potentials.py)


@pytest.fixture(scope='module')
def api():
    from lhvi import _abi
    _abi.require_gpu()
    return _abi


def flat_of(lay):
    from lhvi.flat import build_flat
    from lhvi.graph import Domain
    doms, specs = [], []
    for d, cont in zip(lay.domains, lay.dom_cont):
        if cont:
            doms.append(Domain((float(d[0]), float(d[1])), continuous=True, integral_points=np.linspace(d[0], d[1], 8)))
            specs.append((X2, [1.0, 4.0]))
        else:
            doms.append(Domain(tuple(float(s) for s in d), continuous=False))
            specs.append((TABLE, [1.0, float(len(d))] + [0.0] * len(d)))
    V = lay.V
    return build_flat(np.arange(V + 1), np.arange(V), lay.var_dom, specs, lay.var_value(), lay.var_dom, doms)


class Sampler:
    """a variable-side EPBP state on a hand-built layout with the proposals overwritten; ``call`` runs one sampler entry point
    into sentinel-filled buffers"""

    def __init__(self, api, lay, n, q, gid=None):
        from lhvi.pbp import EPBP
        self.api, self.lay, self.n = api, lay, n
        bp = EPBP(None, n=n, proposal_approximation='simple', sampler='device', seed=0)
        bp._setup(None, flat=flat_of(lay), sides='v')
        assert (bp.np_host == lay.np_of(n)).all()
        bp.q_dev.copy_(api.to_dev(np.ascontiguousarray(q, dtype=np.float64)))
        self.bp = bp
        self.gid = None if gid is None else api.to_dev(np.asarray(gid, dtype=np.int64))
        self.records = None if bp.resample_vars is None else bp.resample_vars.cpu().numpy()
        if self.records is not None:
            assert (self.records[:, 0] == np.flatnonzero(lay.cont)).all()

    def call(self, seed, iteration, entry='uniq', listed=None, var_range=None, flags=0, gid='own'):
        """`entry`: 'uniq' (lhvi_pbp_resample_uniq) or 'plain' (lhvi_pbp_resample); `listed` = (first record, count) of the
        state's list of hidden continuous variables, `var_range` = (var_lo, var_hi); returns (particles, uniq, covered rows)"""
        import torch
        api, bp, V = self.api, self.bp, self.lay.V
        s = bp._struct()
        s.flags |= flags
        rows = np.arange(V)
        if var_range is not None:
            s.var_lo, s.var_hi = int(var_range[0]), int(var_range[1])
            assert 0 <= s.var_lo < s.var_hi <= V
            rows = np.arange(s.var_lo, s.var_hi)
        rec = None
        if listed is not None:
            first, count = listed
            assert 0 <= first and first + count <= self.records.shape[0]
            rec = bp.resample_vars[first:]
            s.resample_vars, s.n_resample_vars = api.ptr(rec), int(count)
            rows = self.records[first:first + count, 0]
        out = torch.full_like(bp.particles, sm.SENTINEL)
        uq = torch.full_like(bp.uniq, sm.MASK_SENTINEL)
        assert out.shape == (V, self.n) and uq.shape == (V, self.n)
        g = self.gid if isinstance(gid, str) else gid
        assert g is None or g.numel() == V
        l, st = api.lib(), api.stream_ptr()
        if entry == 'uniq':
            api.check(l.lhvi_pbp_resample_uniq(bp.dg.g, s, api.ptr(g), int(seed), int(iteration), api.ptr(out), api.ptr(uq), st))
        else:
            api.check(l.lhvi_pbp_resample(bp.dg.g, s, api.ptr(g), int(seed), int(iteration), api.ptr(out), st))
        torch.cuda.synchronize()
        return out.cpu().numpy(), uq.cpu().numpy(), rows


def check_particles(out, d, label, fused=True):
    """every entry of the buffer: within the twin's tolerance of the reference where one is drawn, the reference itself (a bound, a
    state, the sentinel) everywhere else"""
    err = np.abs(out.astype(LD) - d.ref).astype(np.float64)
    drawn = d.tol > 0
    ratio = float((err[drawn] / d.tol[drawn]).max()) if drawn.any() else 0.0
    print('%s: %d drawn entries, largest error / bound %.3f, largest error %.3g; %d exact entries (bounds, states), %d undecided'
          % (label, int(drawn.sum()), ratio, float(err[drawn].max()) if drawn.any() else 0.0,
             int((d.exact & d.written & (d.tol == 0)).sum()), int(d.undecided.sum())))
    bad = np.argwhere(err > d.tol)
    assert bad.size == 0, (label, bad[:5].tolist(), [(float(out[i, j]), float(d.x[i, j]), float(d.tol[i, j])) for i, j in bad[:5]])
    if fused:
        assert not np.signbit(out[out == 0.0]).any(), label            # the fused path stores x + 0.0
    return ratio


def check_mask(uq, out, lay, n, rows, label):
    """covered rows: the first-occurrence mask of the device's own particles by the definition; other rows: untouched"""
    want = np.full(uq.shape, sm.MASK_SENTINEL, dtype=np.uint8)
    want[rows] = sm.first_occurrence(out, lay.np_of(n))[rows]
    bad = np.argwhere(uq != want)
    assert bad.size == 0, (label, bad[:5].tolist())


def by_radius_decade(err, bound, rad):
    rows = []
    dec = np.floor(np.log10(rad)).astype(int)
    for k in np.unique(dec):
        m = dec == k
        rows.append('  radius 1e%+d: %8d draws, largest error %.3g, largest error / bound %.3f' % (k, int(m.sum()), err[m].max(), (err[m] / bound[m]).max()))
    return '\n'.join(rows)


# ---- a. raw normals --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('entry, n', [('uniq', n) for n in sm.RAW_FUSED_N + sm.RAW_GENERAL_N] + [('plain', n) for n in sm.RAW_PLAIN_N])
def test_raw_normals_are_within_the_bound(api, entry, n):
    """q = (0, 1) on [-100, 100]: sqrt_pos(1) = 1, fma(1, z, 0) = z and nothing clips, so the particles are the normals bit for
    bit; every one within ``z_bound`` of the longdouble Box-Muller value of its own Philox block and branch"""
    lay, q = sm.raw_case(n)
    out, uq, rows = Sampler(api, lay, n, q).call(sm.RAW_SEED, sm.RAW_ITERATION, entry)
    path = 'table' if entry == 'uniq' and n <= 64 else 'series'
    nm = sm.normals(sm.RAW_SEED, np.arange(lay.V), n, sm.RAW_ITERATION)
    zb = sm.z_bound(nm.u1, nm.u2, path, nm.sine)
    err = np.abs(out.astype(LD) - nm.z).astype(np.float64)
    print('%s n = %d (%s log): largest error / bound %.3f, largest error %.3g\n%s'
          % (entry, n, path, (err / zb).max(), err.max(), by_radius_decade(err, zb, nm.rad.astype(np.float64))))
    bad = np.argwhere(err > zb)
    assert bad.size == 0, (bad[:5].tolist(), [(float(out[i, j]), float(nm.z[i, j]), float(zb[i, j])) for i, j in bad[:5]])
    if entry == 'uniq':
        check_mask(uq, out, lay, n, rows, 'raw n%d' % n)


# ---- b. counter and key words ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', sm.COUNTER_SEEDS)
def test_counter_and_key_words(api, seed):
    """seeds and iterations with either word set, global ids up to 2**63 - 1: every row equals the twin's draw for its own
    (seed, gid, iteration) in both entry points; two variables with one gid draw the same row whichever half of a wavefront
    they sit in, two whose gids differ in the high word only do not; no gid array means gid = variable index"""
    lay, q = sm.counter_case()
    smp = Sampler(api, lay, 64, q, sm.COUNTER_GIDS)
    V = lay.V
    for it in sm.COUNTER_ITERATIONS:
        d = sm.draw(lay, 64, seed, it, q, sm.COUNTER_GIDS, 'table')
        ds = sm.draw(lay, 64, seed, it, q, sm.COUNTER_GIDS, 'series')
        whole, uq, rows = smp.call(seed, it)
        check_particles(whole, d, 'seed %d iteration %d' % (seed, it))
        check_mask(uq, whole, lay, 64, rows, 'counter')
        shifted, _, _ = smp.call(seed, it, var_range=(1, V))               # every variable in the other half
        assert (shifted[1:] == whole[1:]).all() and (shifted[0] == sm.SENTINEL).all()
        listed, _, _ = smp.call(seed, it, listed=(0, V))
        assert (listed == whole).all()
        plain, _, _ = smp.call(seed, it, entry='plain')
        check_particles(plain, ds, 'seed %d iteration %d plain' % (seed, it), fused=False)
        for got in (whole, shifted, plain):
            for a, b in sm.COUNTER_SHARED:
                assert (got[a] == got[b]).all(), (a, b)
            for a, b in sm.COUNTER_HIGH_ONLY:
                assert (got[a] != got[b]).all(), (a, b)
    own, _, _ = smp.call(seed, 3, gid=None)
    as_index, _, _ = smp.call(seed, 3, gid=api.to_dev(np.arange(V, dtype=np.int64)))
    assert (own == as_index).all()
    check_particles(own, sm.draw(lay, 64, seed, 3, q, None, 'table'), 'no gid array')


# ---- c. the persistent loop ------------------------------------------------------------------------------------------------------
def test_persistent_loop_beyond_two_rounds(api):
    """160 x CUs + 3 variables at n = 64: the grid is 8 x CUs workgroups of four wavefronts, two variables per wavefront and step,
    so every wavefront takes two or three steps (prefetch one step ahead, the LDS bitsets reused); half the rows are clipped to
    the bounds.  Listed and ranged form; all particles against the twin, every mask row against the definition"""
    import torch
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    lay, q = sm.loop_case(cus)
    assert -(-lay.V // 2) > 2 * 32 * cus and lay.V % 2 == 1
    smp = Sampler(api, lay, 64, q)
    d = sm.draw(lay, 64, sm.LOOP_SEED, sm.LOOP_ITERATION, q)
    assert int((d.exact & d.written).sum()) > lay.V * 8                        # the duplicates are really there
    for form, kw in (('listed', dict(listed=(0, lay.V))), ('ranged', dict(var_range=(0, lay.V)))):
        out, uq, rows = smp.call(sm.LOOP_SEED, sm.LOOP_ITERATION, **kw)
        check_particles(out, d, 'persistent loop, %s' % form)
        check_mask(uq, out, lay, 64, rows, form)
        assert int((uq == 0).sum()) > lay.V * 8


# ---- d. pair halves --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', sm.PAIR_N)
def test_every_pairing_of_variable_classes_in_both_halves(api, n):
    """three continuous domains, two discrete ones and observed variables, every ordered pair of them as the two halves of a
    wavefront (range from an even and from an odd variable; the list and the list less its first record for the continuous
    ones): each half takes its own domain and proposal, discrete rows are the states with mask lane < np, observed rows have no
    particles and a zero mask, entries beyond np and rows outside the range or list keep the sentinel"""
    lay, q, _ = sm.pair_case()
    smp = Sampler(api, lay, n, q)
    V, nrec = lay.V, int(lay.cont.sum())
    path = 'table' if n <= 64 else 'series'
    calls = [('whole', {})]
    if n <= 64:
        calls += [('from 0', dict(var_range=(0, V))), ('from 1', dict(var_range=(1, V))), ('from 2 to V - 1', dict(var_range=(2, V - 1))),
                  ('listed', dict(listed=(0, nrec))), ('listed from 1', dict(listed=(1, nrec - 1))), ('listed, one less', dict(listed=(0, nrec - 1)))]
    for label, kw in calls:
        out, uq, rows = smp.call(sm.PAIR_SEED, sm.PAIR_ITERATION, **kw)
        d = sm.draw(lay, n, sm.PAIR_SEED, sm.PAIR_ITERATION, q, None, path, rows=rows)
        assert int(d.undecided.sum()) == 0
        check_particles(out, d, 'n = %d, %s' % (n, label), fused=n <= 64)
        check_mask(uq, out, lay, n, rows, label)
    plain, _, _ = smp.call(sm.PAIR_SEED, sm.PAIR_ITERATION, entry='plain')
    check_particles(plain, sm.draw(lay, n, sm.PAIR_SEED, sm.PAIR_ITERATION, q, None, 'series'), 'n = %d, plain' % n, fused=False)


# ---- e. clipping and masks on hand-set proposals ---------------------------------------------------------------------------------
@pytest.mark.parametrize('n', sm.CLIP_N)
def test_clipped_rows_and_their_masks(api, n):
    """rows clipped to lo, to hi, in part, a point proposal, a mean outside the domain, mu = -0.0, a domain ending at -0.0, and
    pairs with duplicates in one half only: clipped entries are the bound bit for bit, the fused path stores no -0.0, the masks
    are the definition; with LHVI_PBP_NO_UNIQ the listed form writes the particles and leaves the mask buffer alone"""
    lay, q, what = sm.clip_case()
    smp = Sampler(api, lay, n, q)
    V = lay.V
    path = 'table' if n <= 64 else 'series'
    calls = [('whole', {})]
    if n <= 64:
        calls += [('from 1', dict(var_range=(1, V))), ('listed', dict(listed=(0, V))), ('listed from 1', dict(listed=(1, V - 1)))]
    for label, kw in calls:
        out, uq, rows = smp.call(sm.CLIP_SEED, sm.CLIP_ITERATION, **kw)
        d = sm.draw(lay, n, sm.CLIP_SEED, sm.CLIP_ITERATION, q, None, path, rows=rows)
        assert int(d.undecided.sum()) == 0
        check_particles(out, d, 'n = %d, %s' % (n, label), fused=n <= 64)
        check_mask(uq, out, lay, n, rows, label)
        first_only = np.array([1] + [0] * (n - 1), dtype=np.uint8)
        for v in rows:
            if what[v] in ('low', 'high'):
                assert (out[v] == (lay.lo[v] if what[v] == 'low' else lay.hi[v])).all() and (uq[v] == first_only).all(), (label, v)
            elif what[v] == 'point':
                assert (out[v] == q[v, 0]).all() and (uq[v] == first_only).all(), (label, v)
            elif what[v] == 'none':
                assert (uq[v] == 1).all() and ((out[v] > lay.lo[v]) & (out[v] < lay.hi[v])).all(), (label, v)
            else:
                at_hi = out[v] == lay.hi[v]
                assert not (out[v] == lay.lo[v]).any() and (n < 33 or 1 < at_hi.sum() < n), (label, v)
                assert (uq[v][at_hi].sum() == min(1, at_hi.sum())) and (uq[v][~at_hi] == 1).all(), (label, v)
    if n <= 64:
        out, uq, rows = smp.call(sm.CLIP_SEED, sm.CLIP_ITERATION, listed=(0, V), flags=api.PBP_NO_UNIQ)
        check_particles(out, sm.draw(lay, n, sm.CLIP_SEED, sm.CLIP_ITERATION, q, None, path), 'n = %d, particles only' % n)
        assert (uq == sm.MASK_SENTINEL).all()


# ---- f. transformed draws, g. the two entry points -------------------------------------------------------------------------------
@pytest.mark.parametrize('n', sm.GENERAL_N)
def test_transformed_draws_and_the_two_entry_points(api, n):
    """general proposals on three domains with 64-bit global ids: |x_dev - x_ref| <= sqrt(var) z_bound + 2 spacing(|mu| + sqrt(var) |z|),
    clipped entries the bound itself, for ``lhvi_pbp_resample_uniq`` and for ``lhvi_pbp_resample``.  For n <= 64 the two take
    different logarithms (table / series) and square roots: they agree to rounding -- within the sum of their bounds -- and not
    to the bit, and they clip the same entries"""
    lay, q, gid = sm.general_case()
    smp = Sampler(api, lay, n, q, gid)
    path = 'table' if n <= 64 else 'series'
    d = sm.draw(lay, n, sm.GENERAL_SEED, sm.GENERAL_ITERATION, q, gid, path)
    ds = sm.draw(lay, n, sm.GENERAL_SEED, sm.GENERAL_ITERATION, q, gid, 'series')
    assert int(d.undecided.sum()) == 0 and int(ds.undecided.sum()) == 0
    fused, uq, rows = smp.call(sm.GENERAL_SEED, sm.GENERAL_ITERATION)
    check_particles(fused, d, 'resample_uniq n = %d' % n, fused=n <= 64)
    check_mask(uq, fused, lay, n, rows, 'general')
    plain, _, _ = smp.call(sm.GENERAL_SEED, sm.GENERAL_ITERATION, entry='plain')
    check_particles(plain, ds, 'resample n = %d' % n, fused=False)
    same = fused == plain
    inner = d.tol > 0
    print('n = %d: %d of %d drawn entries bit-identical between lhvi_pbp_resample and lhvi_pbp_resample_uniq, largest difference %.3g'
          % (n, int(same[inner].sum()), int(inner.sum()), np.abs(fused - plain).max()))
    assert (np.abs(fused - plain) <= d.tol + ds.tol).all() and same[~inner].all()
    if n > 64:
        assert same.all()                   # beyond 64 particles lhvi_pbp_resample_uniq IS lhvi_pbp_resample + lhvi_pbp_uniq
    else:
        assert not same[inner].all()


# ---- h. the fused per-variable kernels -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', list(sm.FUSED_CASES))
def test_fused_kernels_take_gid_seed_and_iteration(api, case):
    """``lhvi_pbp_var_fused`` (n = 16, 32) and ``lhvi_pbp_var_fused64`` (n = 64) with a gid array whose high words are set, a seed
    beyond 2**32 and several sweeps: particles and masks equal the three-kernel path bit for bit, the first sample and the last
    one (iteration = draws - 1, drawn from the proposal the same pass wrote) meet the twin's bound"""
    import torch
    from lhvi import synth
    from lhvi.pbp import EPBP
    from test_gpu_pbp import _init
    n, V, gseed = sm.FUSED_CASES[case]
    gid = sm.fused_gids(V)
    runs, first = [], []
    for fused in (True, False):
        flat = synth.hybrid_mrf_flat(V=V, deg=4, seed=gseed, frac_discrete=0.3, T=32)
        assert flat.V == V
        bp = EPBP(None, n=n, proposal_approximation='simple', sampler='device', seed=sm.FUSED_SEED)
        if n <= 32:
            bp.fused_var_kernel, bp.fused_max_particles = fused, 32
        else:
            bp.fused_var_kernel, bp.fused_max_particles = True, 64 if fused else 32
        bp._setup(None, flat=flat)
        bp.var_gid = api.to_dev(gid)
        _init(api, bp)
        first.append(bp.particles.cpu().numpy().copy())
        for _ in range(4):
            bp.sweep(last=False)
        torch.cuda.synchronize()
        runs.append(bp)
    a, b = runs
    assert a._fused is not None and b._fused is None
    assert sum(a._fused['counts' if n <= 32 else 'counts64']) > 0 and a._draws == 5
    for name in ('q_dev', 'eta', 'particles', 'old_particles', 'uniq', 'v2f', 'f2v'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    fl = a.flat
    doms = [((fl.dom_lo[k], fl.dom_hi[k]) if fl.dom_cont[k] else tuple(fl.dom_val[fl.dom_ptr[k]:fl.dom_ptr[k + 1]])) for k in range(fl.dom_cont.size)]
    lay = sm.Layout(doms, np.where(fl.var_hidden, fl.var_dom, -1 - fl.var_dom.astype(np.int64)), dom_cont=fl.dom_cont.astype(bool))
    assert (lay.np_of(n) == a.np_host).all() and lay.cont.sum() > V // 2
    assert tuple(doms[int(fl.var_dom[np.flatnonzero(lay.cont)[0]])]) == sm.FUSED_DOMAIN
    cont = lay.cont
    q0 = np.tile(sm.FUSED_Q0, (V, 1))
    d0 = sm.draw(lay, n, sm.FUSED_SEED, 0, q0, gid, 'table')
    assert int(d0.undecided.sum()) == 0 and (first[0] == first[1]).all()
    check_particles(np.where(d0.written, first[0], sm.SENTINEL)[cont], sm.Draw(*[f[cont] for f in d0]), case + ', first sample')
    q = a.q_dev.cpu().numpy()
    assert np.isfinite(q[cont]).all() and (q[cont, 1] > 0).all()
    dl = sm.draw(lay, n, sm.FUSED_SEED, a._draws - 1, np.where(cont[:, None], q, 1.0), gid, 'table')
    out = a.particles.cpu().numpy()
    check_particles(np.where(dl.written, out, sm.SENTINEL)[cont], sm.Draw(*[f[cont] for f in dl]), case + ', last sample')
    check_mask(a.uniq.cpu().numpy()[cont], out[cont], sm.Layout([sm.FUSED_DOMAIN], np.zeros(int(cont.sum()), dtype=np.int64)), n,
               np.arange(int(cont.sum())), case)
    assert not (dl.z[cont] == d0.z[cont]).any()                # the iteration did move the stream
