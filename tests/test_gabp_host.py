"""CPU suite: the longdouble twin of the Gaussian sweep (tests/gabp_models.py) against the C oracle and the goldens, the
invariants of ``pull_plan``, and the condition caps of the hand-built inputs that the GPU tests (test_gpu_gabp_kernels.py) use."""
import numpy as np
import pytest

import gabp_models as gm
import modelio
from lhvi.flat import flatten
from lhvi.gabp import pull_plan
from oracle import oracle
from test_oracle_golden import API, load

MODELS = ['rows', 'layout64', 'layout256', 'lifted_counts', 'alias', 'closed_forms', 'dominant']


model, covered, oracle_marginals, oracle_pull = gm.model, gm.covered, gm.oracle_marginals, gm.oracle_pull


@pytest.mark.parametrize('name', MODELS)
def test_twin_matches_the_c_oracle_on_hand_built_messages(name):
    """v -> f, f -> v and marginals of the twin against oracle/c/gabp_oracle.c, within ``bound``, on messages of every class"""
    flat = model(name)
    f2v = gm.dominant()[1] if name == 'dominant' else gm.messages(flat, np.random.default_rng(1))
    v2f0 = np.full((flat.E, 2), 7.0)                               # (observed rows and alias edges must not keep this)
    ov2f, of2v = oracle.gabp_half_sweeps(flat, f2v, v2f0)
    tw = gm.v2f(flat, f2v)
    gm.compare(name + ' v2f: oracle against twin', ov2f, tw, covered(flat))
    assert (ov2f[~covered(flat)] == 7.0).all()
    obs_edge = ~np.isnan(flat.var_value)[flat.edge_var] & covered(flat)
    assert np.isnan(ov2f[obs_edge]).all() and np.isnan(tw.array()[obs_edge]).all()
    gm.compare_f2v(name + ' f2v: oracle against twin', of2v, gm.f2v(flat, ov2f, f2v))
    gm.compare(name + ' marginals: oracle against twin', oracle_marginals(flat, f2v), gm.marginals(flat, f2v))


def test_twin_closed_forms_on_every_class_of_partner_message():
    flat, v2f_in = gm.closed_forms()
    f2v0 = np.full((flat.E, 2), 7.0)
    of2v = gm.oracle_f2v(flat, v2f_in, f2v0)
    gm.compare_f2v('closed forms: oracle against twin', of2v, gm.f2v(flat, v2f_in, f2v0))
    hidden = np.isnan(flat.var_value)[flat.edge_var]
    # every kind of result is there: None, +inf, -0.0 from an infinite partner variance, negative, NaN from a `None` partner
    got = of2v[hidden]
    assert np.isnan(got[:, 1]).any() and np.isposinf(got[:, 1]).any() and (got[:, 1] < 0).any() and (got[:, 0] == 0).any()


@pytest.mark.parametrize('name', MODELS)
def test_twin_pull_matches_the_oracle_halves_and_keeps_the_condition_cap(name):
    flat = model(name)
    vprev = gm.dominant()[2] if name == 'dominant' else gm.slot_messages(flat, np.random.default_rng(2))
    tw = gm.pull(flat, vprev, 0)
    gm.compare(name + ' pull: oracle halves against twin', oracle_pull(flat, vprev), tw)
    hidden = np.isnan(flat.var_value)[np.repeat(np.arange(flat.V), np.diff(flat.var_ptr))]
    cond = tw.cond()
    if name == 'dominant':
        slots = gm.dominant()[3]
        assert (np.abs(tw.P[hidden]) > 0).all()
        assert np.allclose(cond[slots], 1e9, rtol=1e-3)
        rest = np.ones(cond.size, dtype=bool)
        rest[slots] = False
        assert cond[rest & hidden].max() <= 1e3                   # (the other slots see the dominant entry in both sums)
    else:
        assert (np.abs(tw.P[hidden]) > 0).all() and cond[hidden].max() <= gm.COND_CAP, cond[hidden].max()
    # the first sweep: (0, 1) everywhere
    tw1 = gm.pull(flat, None, 1)
    f2v = np.zeros((flat.E, 2))
    f2v[:, 1] = 1.0
    ref = gm.v2f(flat, f2v)
    assert np.array_equal(tw1.array(), ref.array()[flat.var_edge], equal_nan=True)


@pytest.mark.parametrize('name', MODELS)
def test_hand_built_messages_keep_the_condition_cap_and_hold_every_class(name):
    """no message is left out of a comparison: every leave-one-out sum of every hidden row has |P| > 0 and
    sum |p c| / |P| <= 1e6; ``dominant()`` has the condition it states"""
    flat = model(name)
    hidden_edge = np.isnan(flat.var_value)[flat.edge_var] & covered(flat)
    if name == 'dominant':
        _, f2v, _, slots = gm.dominant()
        cond = gm.v2f(flat, f2v).cond()
        e = flat.var_edge[slots]
        assert np.allclose(cond[e], 1e9, rtol=1e-6)
        rest = hidden_edge.copy()
        rest[e] = False
        assert cond[rest].max() <= 1e3                            # (the other slots see the dominant entry in both sums)
        return
    f2v = gm.messages(flat, np.random.default_rng(1))
    tw = gm.v2f(flat, f2v)
    assert (np.abs(tw.P[hidden_edge]) > 0).all()
    assert tw.cond()[hidden_edge].max() <= gm.COND_CAP
    mg = gm.marginals(flat, f2v)
    hv = np.isnan(flat.var_value) & (np.diff(flat.var_ptr) > 0)
    assert (np.abs(mg.P[hv]) > 0).all() and mg.cond()[hv].max() <= gm.COND_CAP
    if name in ('rows', 'layout64', 'layout256', 'lifted_counts'):
        # every row class has every class of message at every special position
        deg = np.diff(flat.var_ptr)
        slot = f2v[flat.var_edge]
        kind = np.where(np.isnan(slot[:, 1]), 1, np.where(np.isinf(slot[:, 1]), 2, np.where(slot[:, 1] < 0, 3, np.where(slot[:, 0] == 0, 4, 0))))
        for lo_n, hi_n in ((5, gm.ROW_DIRECT), (gm.ROW_DIRECT + 1, gm.HUB), (gm.HUB + 1, 1 << 20)):
            seen = set()
            for v in np.flatnonzero((deg >= lo_n) & (deg <= hi_n)):
                for i, x in enumerate(gm.special_positions(int(deg[v]))):
                    seen.add((i if hi_n > gm.ROW_DIRECT else min(i, 1), int(kind[flat.var_ptr[v] + x])))
            n_pos = 5 if hi_n > gm.ROW_DIRECT else 2              # (short rows: the first and the last entry)
            assert seen >= {(i, c) for i in range(n_pos) for c in range(5)}, (lo_n, sorted(seen))


@pytest.mark.parametrize('name', ['rows', 'layout64', 'layout256', 'lifted_counts'])
def test_pull_inputs_put_every_contribution_class_at_the_special_positions(name):
    """in the pull form the `None`, infinite and negative variances come out of the closed forms of the potentials: every class of
    contribution sits at special positions of hidden rows of every row class, and (in the models that keep the rows' order) each special position (first, last, ends of a
    middle chunk, last chunk's remainder) of the chunked and the hub rows sees a `None`, an infinite and a negative variance"""
    flat = model(name)
    cls = gm.pull_contribution_classes(flat, gm.slot_messages(flat, np.random.default_rng(2)))
    deg = np.diff(flat.var_ptr)
    hid = np.isnan(flat.var_value)
    for lo_n, hi_n in ((4, gm.ROW_DIRECT), (gm.ROW_DIRECT + 1, gm.HUB), (gm.HUB + 1, 1 << 20)):
        seen = set()
        for v in np.flatnonzero(hid & (deg >= lo_n) & (deg <= hi_n)):
            for i, x in enumerate(gm.special_positions(int(deg[v]))):
                seen.add((i, int(cls[flat.var_ptr[v] + x])))
        print(name, lo_n, sorted(seen))
        assert {c for _, c in seen} >= {0, 1, 2, 3}
        if lo_n > gm.ROW_DIRECT and not name.startswith('layout'):
            # (six hub rows: the remainder position of the 577-row is its last entry, so that position sees five rows only)
            n_pos = 5 if hi_n <= gm.HUB else 4
            assert seen >= {(i, c) for i in range(n_pos) for c in (1, 2, 3)}, (lo_n, sorted(seen))


@pytest.mark.parametrize('name', ['gauss_g1_chain', 'gauss_g2_kalman', 'gauss_g3_rgm0'])
def test_twin_matches_the_goldens_after_their_recorded_sweeps(golden_dir, name):
    rec = load(golden_dir, name)
    g, rvs, factors = modelio.load_model(rec['model'], API)
    flat = flatten(g)
    for k, want in rec['sweeps'].items():
        f2v, v2f, mv = oracle.gabp_run(flat, int(k))
        # the reference's own messages as input where it recorded them (hidden edges), the oracle's elsewhere
        hidden_edge = flat.var_hidden[flat.edge_var]
        f2v_in = f2v.copy()
        f2v_in[hidden_edge] = np.asarray(want['f2v'], dtype=float)[hidden_edge]
        gm.compare('%s %s sweeps v2f: golden against twin' % (name, k), np.asarray(want['v2f'], dtype=float), gm.v2f(flat, f2v_in),
                   covered(flat))
        gm.compare('%s %s sweeps marginals: golden against twin' % (name, k), np.asarray(want['mu_var'], dtype=float),
                   gm.marginals(flat, f2v_in))
        if int(k) >= 2:
            # ... and the f -> v half from the v -> f messages of the sweep before
            _, v2f_before, _ = oracle.gabp_run(flat, int(k) - 1)
            gm.compare_f2v('%s %s sweeps f2v: oracle against twin' % (name, k), f2v, gm.f2v(flat, v2f_before, f2v))


# ---- pull_plan ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['rows', 'layout64', 'layout256', 'lifted_counts'])
def test_pull_plan_invariants(name, monkeypatch):
    flat = model(name)
    window = 256 if name == 'layout256' else 64
    monkeypatch.setenv('LHVI_GABP_WINDOW', str(window))
    plan = pull_plan(flat)
    nnz = int(flat.var_edge.size)
    deg = np.diff(flat.var_ptr).astype(np.int64)
    svar = np.repeat(np.arange(flat.V), deg)
    within = np.arange(nnz) - flat.var_ptr[svar]
    hub = deg[svar] > gm.HUB
    assert hub.any() and (deg == gm.HUB).any()
    seg = plan['seg'].astype(np.int64)
    # every non-hub slot in exactly one segment, no hub slot in any
    cover = np.zeros(nnz + 1, dtype=np.int64)
    np.add.at(cover, seg[:, 0], 1)
    np.add.at(cover, seg[:, 1], -1)
    cover = np.cumsum(cover)[:nnz]
    assert (cover[~hub] == 1).all() and (cover[hub] == 0).all()
    # no row is cut: segments begin and end on row boundaries
    bounds = set(flat.var_ptr.tolist())
    assert all(int(a) in bounds and int(b) in bounds and a < b for a, b in seg)
    # rows are grouped by the window their first slot lies in
    for a, b in seg:
        starts = flat.var_ptr[svar[a:b]]
        assert (starts // window == a // window).all()
    length = seg[:, 1] - seg[:, 0]
    assert length.max() <= 768
    if name.startswith('layout'):
        assert length.max() == window - 1 + 512, length.max()
        # ... and what the layout promises the array kernel (blocks of 256 slots)
        start512 = int(flat.var_ptr[np.flatnonzero((deg == 512) & np.isnan(flat.var_value))[0]])
        assert start512 % 256 != 0 and start512 % window == window - 1 and np.isnan(flat.var_value[svar[start512 - 1]])
        hub_rows = np.flatnonzero((deg > gm.HUB) & np.isnan(flat.var_value))
        assert any(flat.var_ptr[v + 1] % 256 == 0 and flat.var_ptr[v] % 256 != 0 for v in hub_rows)
        assert any(flat.var_ptr[v] % 256 == 0 for v in hub_rows)
        last = flat.V - 1
        assert gm.ROW_DIRECT < deg[last] <= gm.HUB and np.isnan(flat.var_value[last]) and flat.var_ptr[last + 1] == nnz and nnz % 256 != 0
    # the record: 10 / 10 / 1 / 1 bits
    z = plan['rec'][:, 2].astype(np.int64)
    assert np.array_equal(z & 1023, np.where(hub, 0, within))
    assert np.array_equal((z >> 10) & 1023, np.where(hub, 0, deg[svar]))
    assert np.array_equal((z >> 20) & 1, np.isnan(flat.var_value[svar]).astype(np.int64))
    assert np.array_equal((z >> 21) & 1, hub.astype(np.int64))
    assert (z >> 22 == 0).all() and (((z >> 10) & 1023) == 512).any()
    # partner slot / -1 - variable of an observed partner; 4 * potential + position code
    ve = flat.var_edge.astype(np.int64)
    f = flat.edge_fac[ve]
    base = flat.fac_ptr[f].astype(np.int64)
    arity = flat.fac_ptr[f + 1] - base
    es = gm.edge_slot(flat)
    for k in range(nnz):
        if arity[k] == 2:
            pe = base[k] + (1 - (ve[k] - base[k]))
            pv = int(flat.edge_var[pe])
            want = es[flat.edge_canon[pe]] if np.isnan(flat.var_value[pv]) else -1 - pv
            assert plan['pslot'][k] == want == plan['rec'][k, 0]
            code = 1 + (ve[k] - base[k])
        else:
            code = 0 if arity[k] == 1 else 3
        assert plan['info'][k] == 4 * flat.fac_pot[f[k]] + code == plan['rec'][k, 1]
    if flat.lifted:
        assert np.array_equal(plan['count'], flat.edge_count[ve]) and (plan['count'] != 1).any()
    else:
        assert plan['count'] is None
    # the potential words: eleven parameters and the kind
    for i in range(flat.pot_kind.size):
        par = flat.pot_param[flat.pot_off[i]:flat.pot_off[i + 1]][:11]
        assert np.array_equal(plan['pot_words'][i, :par.size], par) and plan['pot_words'][i, 11] == flat.pot_kind[i]


def test_pull_plan_window_switch(monkeypatch):
    """64-slot windows below 2^17 slots, 256 above; the environment's value is clamped to [1, 256]"""
    from lhvi import synth
    monkeypatch.delenv('LHVI_GABP_WINDOW', raising=False)
    small = gm.layout(64)
    assert small.var_edge.size < (1 << 17)
    seg = pull_plan(small)['seg']
    assert (seg[:, 1] - seg[:, 0]).max() == 63 + 512
    big = synth.random_gaussian_mrf(V=30000, deg=4, seed=5)
    assert big.var_edge.size >= (1 << 17)
    seg = pull_plan(big)['seg'].astype(np.int64)
    first_window = seg[:, 0] // 256
    assert np.unique(first_window).size == seg.shape[0]           # one segment per 256-slot window
    assert (seg[:, 1] - seg[:, 0]).max() > 64 + 4 * 2
    monkeypatch.setenv('LHVI_GABP_WINDOW', '4096')
    seg = pull_plan(gm.layout(256))['seg']
    assert (seg[:, 1] - seg[:, 0]).max() == 767


def test_models_are_what_they_say():
    flat = gm.rows()
    deg = np.diff(flat.var_ptr)
    hid = np.isnan(flat.var_value)
    assert sorted(deg[flat.centres][hid[flat.centres]].tolist()) == sorted(gm.ROW_LENGTHS)
    assert sorted(deg[flat.centres][~hid[flat.centres]].tolist()) == sorted(gm.ROW_LENGTHS)
    leaves = np.ones(flat.V, dtype=bool)
    leaves[flat.centres] = False
    assert 0.05 < (~hid[leaves]).mean() < 0.2 and deg[leaves].max() <= 3
    assert flat.var_edge.size < 40000
    lf = gm.lifted_counts()
    own1 = lf.edge_count[lf.var_edge] == 1
    svar = np.repeat(np.arange(lf.V), deg)
    assert set(np.unique(lf.edge_count).tolist()) == {1.0, 2.0, 3.0, 7.0, 90.0}
    assert all(own1[svar == c].any() for c in lf.centres)
    g, lifted, rvc, fc = gm.alias_chain()
    assert lifted.lifted and lifted.V < g.V and (lifted.edge_canon != np.arange(lifted.E)).any()
    for n in (32, 33):
        assert gm.potentials_graph(n).pot_kind.size == n
