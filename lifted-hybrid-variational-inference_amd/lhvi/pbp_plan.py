"""Which variable and which edge of a particle sweep goes to which kernel, and the records those kernels read: pure functions of
their arguments -- no environment, same arguments give the same bytes.  The record layouts are those of ``include/lhvi.h``
(``lhvi_pbp_t``).  The variable side (``var_side_plan``) works on the graph's host arrays; ``lhvi/pbp.py::_setup`` uploads what it
returns in one copy.  The factor side (``f_side_plan``, ``f2v_split``, ``pair_records``) works on tensors, on the device they
live on -- the device in a sweep, the CPU in a test -- and takes the two device calls that describe edges as callables; its lists
travel as one record (``F2vLists``), as the variable side's do (``VarLists``, with its ``V2fLists`` and ``FusedLists``)."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import _abi

V2F_CLASSES = ('wide', 'narrow', 'hub', 'mid16', 'mid32')

# everything var_side_plan depends on besides the graph (_ParticleSweep._plan_options).  v2f_records: the wide list travels as records
# (LHVI_PBP_V2F_RECORDS), not as a plain list; fused_records16: sixteen words per fused record (LHVI_PBP_FUSED_RECORDS16), not eight
PlanOptions = namedtuple('PlanOptions', 'sampler_on_device listed_proposal listed_resample sliced_proposal prop_slice packed_v2f '
                                        'v2f_records fused fused_max_particles fused_records16')

class V2fLists(namedtuple('V2fLists', 'wide n_wide narrow n_narrow hub n_hub mid16 n_mid16 mid32 n_mid32', defaults=(None, 0) * 5)):
    """the v -> f half's five lists (``lhvi_pbp_t.v2f_wide / v2f_narrow / v2f_hub / v2f_mid16 / v2f_mid32``), each with its count;
    host arrays in a plan, device tensors once uploaded (``on``).  ``V2fLists()`` is no lists: variables by range."""

    def install(self, s):
        for name in V2F_CLASSES:
            setattr(s, 'v2f_' + name, _abi.ptr(getattr(self, name)))
            setattr(s, 'n_v2f_' + name, getattr(self, 'n_' + name))

    def named(self, prefix):
        return {prefix + name: getattr(self, name) for name in V2F_CLASSES}

    def on(self, dev, prefix):
        return self._replace(**{name: dev[prefix + name] for name in V2F_CLASSES})


class FusedLists(namedtuple('FusedLists', 'counts counts64 desc desc64 v2f_rest prop_desc_rest n_prop_rest resample_rest n_resample_rest')):
    """the fused per-variable kernels' records (``lhvi_pbp_var_fused``: `counts` variables of the 16 / 32a / 32b sub-classes in
    `desc`; ``lhvi_pbp_var_fused64``: `counts64` of 64a / 64b in `desc64`, None without any) and what is left for the three kernels"""

    def __getitem__(self, key):         # F['counts'] reads as F.counts, as on the dict this record replaced
        return getattr(self, key) if isinstance(key, str) else tuple.__getitem__(self, key)

    def named(self):
        return {'fused_desc': self.desc, 'fused64_desc': self.desc64, 'prop_desc_rest': self.prop_desc_rest,
                'resample_rest': self.resample_rest, **self.v2f_rest.named('v2f_rest_')}

    def on(self, dev):
        return self._replace(desc=dev['fused_desc'], desc64=dev.get('fused64_desc'), prop_desc_rest=dev['prop_desc_rest'],
                             resample_rest=dev['resample_rest'], v2f_rest=self.v2f_rest.on(dev, 'v2f_rest_'))


class VarLists(namedtuple('VarLists', 'np_dev resample_vars n_resample_vars static_idx prop_desc n_prop_desc prop_hub n_prop_hub prop_partial '
                                      'v2f fused')):
    """the variable side's lists on the device (``VarSidePlan.on``): particles per variable (``lhvi_pbp_t.np``), the sampler's records
    with their count (None without a hidden continuous variable), `static_idx`: the rows no listed draw writes (None without any),
    the proposal kernel's records, its hub rows with the scratch rows of their slices (``prop_partial``; None without hubs), the
    ``V2fLists`` (None: variables by range) and the ``FusedLists`` (None: no fused pass)."""

    def named(self):
        """the lists under the names a sweep object holds them by"""
        return dict(np_dev=self.np_dev, resample_vars=self.resample_vars, n_prop_desc=self.n_prop_desc, prop_hub=self.prop_hub,
                    n_prop_hub=self.n_prop_hub, v2f_lists=self.v2f, _fused=self.fused)

    def install(self, s, proposal_records=True):
        """every variable through its lists; `proposal_records` off: the proposal kernel walks the graph arrays"""
        s.np = _abi.ptr(self.np_dev)
        if self.v2f is not None:
            self.v2f.install(s)
        if proposal_records and self.prop_desc is not None:
            s.prop_desc, s.n_prop_desc = _abi.ptr(self.prop_desc), self.n_prop_desc
            if self.prop_hub is not None:
                s.prop_hub, s.n_prop_hub, s.prop_partial = _abi.ptr(self.prop_hub), self.n_prop_hub, _abi.ptr(self.prop_partial)

    def install_range(self, s, lo, hi):
        """the variables [lo, hi) by range (0, 0: all of them): no list of any kernel"""
        s.np = _abi.ptr(self.np_dev)
        s.prop_desc, s.n_prop_desc = None, 0
        s.prop_hub, s.n_prop_hub, s.prop_partial = None, 0, None
        s.resample_vars, s.n_resample_vars = None, 0
        V2fLists().install(s)
        s.var_lo, s.var_hi = int(lo), int(hi)

    def install_sampler(self, s):
        """the device sampler draws for its listed variables only"""
        s.resample_vars, s.n_resample_vars = _abi.ptr(self.resample_vars), self.n_resample_vars

    def install_rest(self, s, kernel):
        """what the fused pass leaves to one of the three kernels, in the place of its full list (`s`: installed); `kernel`: 'v2f',
        'proposal' or 'sampler'.  One at a time: each launch of a sweep sees the lists it has always seen."""
        F = self.fused
        if kernel == 'v2f':
            F.v2f_rest.install(s)
        elif kernel == 'proposal':
            s.prop_desc, s.n_prop_desc = _abi.ptr(F.prop_desc_rest), F.n_prop_rest
        else:
            s.resample_vars, s.n_resample_vars = _abi.ptr(F.resample_rest), F.n_resample_rest


class VarSidePlan(namedtuple('VarSidePlan', 'host flags np_host T n_prop_desc n_prop_hub n_prop_partial v2f fused')):
    """host: name -> host array (or None), what goes to _abi.upload;  flags: to OR into lhvi_pbp_t.flags;  n_prop_partial: rows of
    lhvi_pbp_t.prop_partial;  v2f: V2fLists, or None (the v -> f half addresses the variables by range);  fused: FusedLists or None"""

    def on(self, dev, prop_partial):
        """the lists a sweep holds: `dev` is `host` once uploaded, `prop_partial` the [n_prop_partial, 2] scratch rows (None without)"""
        rr = dev['resample_vars']
        return VarLists(np_dev=dev['np_dev'], resample_vars=rr, n_resample_vars=0 if rr is None else int(rr.shape[0]),
                        static_idx=dev['_static_idx'], prop_desc=dev['prop_desc'], n_prop_desc=self.n_prop_desc,
                        prop_hub=dev.get('prop_hub'), n_prop_hub=self.n_prop_hub, prop_partial=prop_partial,
                        v2f=self.v2f.on(dev, 'v2f_') if self.v2f is not None else None,
                        fused=self.fused.on(dev) if self.fused is not None else None)


def first_edges(flat, vs, k, clamp):
    """[len(vs), k]: the first `k` entries of the ``var_edge`` rows of the variables `vs`.  Beyond a row's end: its last edge
    (`clamp`; the proposal and v -> f records) or zero (the fused records)."""
    out = np.zeros((vs.size, k), dtype=np.int32)
    if flat.var_edge.size == 0:
        return out
    deg = np.diff(flat.var_ptr)[vs][:, None]
    base = flat.var_ptr[vs].astype(np.int64)[:, None]
    j = np.arange(k)[None, :]
    if clamp:
        return flat.var_edge[np.minimum(base + np.minimum(j, np.maximum(deg - 1, 0)), flat.var_edge.size - 1)].astype(np.int32)
    has = deg > j
    out[has] = flat.var_edge[(base + j)[has]]
    return out


def _double_words(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int32).reshape(-1, 2)


def _or_zero_row(a):
    """an empty list keeps a non-null pointer: one zero row"""
    return np.ascontiguousarray(a) if a.shape[0] else np.zeros((1,) + a.shape[1:], dtype=a.dtype)


def v2f_records(flat, np_host, vs):
    """``lhvi_pbp_t.v2f_wide`` as records (LHVI_PBP_V2F_RECORDS, include/lhvi.h): variable, incident edges, particles, domain and
    the first four incident edges in row order, so that the kernel's row loads hang on one scalar load"""
    rec = np.zeros((vs.size, 8), dtype=np.int32)
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3] = vs, np.diff(flat.var_ptr)[vs], np_host[vs], flat.var_dom[vs]
    rec[:, 4:] = first_edges(flat, vs, 4, clamp=True)
    return _or_zero_row(rec)


def v2f_split(flat, np_host, vs, records):
    """the v -> f half's split of the variables `vs` (include/lhvi.h, lhvi_pbp_t.v2f_wide / v2f_narrow): at most four particles;
    more than 64 incident edges and at most 64 particles; of the others those with at most 16 / 32 particles; the rest"""
    npv, deg = np_host[vs], np.diff(flat.var_ptr)[vs]
    narrow = npv <= 4
    hub = ~narrow & (deg > 64) & (npv <= 64)
    mid16 = ~narrow & ~hub & (npv <= 16)
    mid32 = ~narrow & ~hub & ~mid16 & (npv <= 32)
    fields = {}
    for name, m in (('wide', ~narrow & ~hub & ~mid16 & ~mid32), ('narrow', narrow), ('hub', hub), ('mid16', mid16), ('mid32', mid32)):
        fields[name] = v2f_records(flat, np_host, vs[m]) if name == 'wide' and records else _or_zero_row(vs[m].astype(np.int32))
        fields['n_' + name] = int(m.sum())
    return V2fLists(**fields)


def var_side_plan(flat, n, *, owned, opts):
    """The per-variable work lists of a sweep with `n` particles on `flat`.
    `owned` (owner-computes shards): the lists of the v -> f half and of the proposal update hold the variables below this index
    only (the rank's own; the sampler's list keeps all of them: ghosts are drawn here too)."""
    sizes = np.diff(flat.dom_ptr)
    cont = flat.dom_cont.astype(bool)
    T = int(sizes[cont].max()) if cont.any() else 0
    nst = flat.var_nstates
    deg = np.diff(flat.var_ptr)
    if (flat.var_hidden & ~flat.var_cont & (nst > n)).any():
        raise _abi.LhviError('a discrete variable has more states than particle slots n=%d' % n)
    if (flat.var_hidden & flat.var_cont & (deg == 0)).any():
        # the reference fails in gaussian_product (`0 ** -1`, EPBP:30-41) on the first proposal update of such a variable
        raise ZeroDivisionError('a hidden continuous variable has no incident factor: its proposal is an empty product')
    np_host = np.where(flat.var_hidden, np.where(flat.var_cont, n, nst), 0).astype(np.int32)
    host = {'np_dev': np_host}
    # records of the hidden continuous variables for the proposal kernel (include/lhvi.h, lhvi_pbp_t.prop_desc)
    pv_all = np.flatnonzero(flat.var_hidden & flat.var_cont)
    pv = pv_all if owned is None else pv_all[pv_all < owned]
    pdeg, pdom = deg[pv], flat.var_dom[pv]
    pT = sizes[pdom]
    pd = np.zeros((pv.size, 8), dtype=np.int32)
    pd[:, 0], pd[:, 1], pd[:, 2], pd[:, 3] = pv, pdeg, flat.dom_ptr[pdom], pT
    pd[:, 4:] = first_edges(flat, pv, 4, clamp=True)
    # the device sampler's list (include/lhvi.h, lhvi_pbp_t.resample_vars); the other rows are filled once, by the first draw
    rdom = flat.var_dom[pv_all]
    rr = np.zeros((pv_all.size, 8), dtype=np.int32)
    rr[:, 0], rr[:, 1] = pv_all, np_host[pv_all]
    rr[:, 2:4], rr[:, 4:6] = _double_words(flat.dom_lo[rdom]), _double_words(flat.dom_hi[rdom])
    host['resample_vars'] = rr if pv_all.size else None
    static = np.flatnonzero(~(flat.var_hidden & flat.var_cont))
    host['_static_idx'] = static.astype(np.int64) if static.size else None
    # rows longer than prop_slice entries go in as slices of that length, a wavefront each, ahead of the ordinary records
    n_prop_hub = n_prop_partial = 0
    hubs = np.flatnonzero(pdeg > opts.prop_slice) if opts.sliced_proposal else np.zeros(0, dtype=np.int64)
    if hubs.size:
        L = int(opts.prop_slice)
        nsl = (pdeg[hubs] + L - 1) // L
        first = np.concatenate([[0], np.cumsum(nsl)[:-1]])
        owner = np.repeat(np.arange(hubs.size), nsl)
        within = np.arange(int(nsl.sum())) - first[owner]
        sl = np.zeros((owner.size, 8), dtype=np.int32)
        sl[:, 0], sl[:, 2], sl[:, 3] = pd[hubs[owner], 0], pd[hubs[owner], 2], pd[hubs[owner], 3]
        sl[:, 1] = -np.minimum(L, pdeg[hubs][owner] - within * L)
        sl[:, 4], sl[:, 5] = within * L, np.arange(owner.size)
        ph = np.zeros((hubs.size, 4), dtype=np.int32)
        ph[:, 0], ph[:, 1], ph[:, 2] = pv[hubs], first, nsl
        pd = np.concatenate([sl, np.delete(pd, hubs, axis=0)])
        host['prop_hub'], n_prop_hub, n_prop_partial = ph, int(hubs.size), int(owner.size)
    host['prop_desc'] = np.ascontiguousarray(pd) if pv.size else None
    # the v -> f half's lists; all variables in the wide class: by range, no lists
    hidden_v = np.flatnonzero(flat.var_hidden)
    if owned is not None:
        hidden_v = hidden_v[hidden_v < owned]
    flags, v2f, fused = 0, None, None
    if opts.packed_v2f and hidden_v.size:
        v2f = v2f_split(flat, np_host, hidden_v, opts.v2f_records)
        if v2f.n_wide == hidden_v.size:
            v2f = None
    if v2f is not None:
        host.update(v2f.named('v2f_'))
        flags |= _abi.PBP_V2F_RECORDS if opts.v2f_records else 0
    # ---- the fused per-variable kernel's records (lhvi_pbp_var_fused) and what is left for the three kernels
    fz = (pdeg <= min(64, opts.prop_slice)) & (pT <= 64) & (n <= min(64, opts.fused_max_particles))
    if opts.fused and owned is None and opts.sampler_on_device and opts.listed_proposal and opts.listed_resample \
            and v2f is not None and fz.any():
        k16 = fz & (n <= 16) & (pT <= 32)
        k32a = fz & (n <= 32) & ~k16 & (pT <= 32)
        k32b = fz & (n <= 32) & ~k16 & ~k32a
        # 32 < n <= 64: one variable per wavefront (lhvi_pbp_var_fused64), a list of its own, always in the sixteen-word layout
        k64a = fz & (n > 32) & (pT <= 32)
        k64b = fz & (n > 32) & ~k64a
        # sixteen words per variable (LHVI_PBP_FUSED_RECORDS16): the eight of include/lhvi.h, then np, var_ptr[v] and the first six
        # incident edges -- the kernel's row loads then hang on one load behind the record (fused_records16 off: eight words)
        fd64 = np.zeros((pv.size, 16), dtype=np.int32)
        fd64[:, 0], fd64[:, 1], fd64[:, 2], fd64[:, 3] = pv, pdeg, flat.dom_ptr[pdom], pT
        fd64[:, 4:6], fd64[:, 6:8] = _double_words(flat.dom_lo[pdom]), _double_words(flat.dom_hi[pdom])
        fd64[:, 8], fd64[:, 9] = np_host[pv], flat.var_ptr[pv]
        fd64[:, 10:] = first_edges(flat, pv, 6, clamp=False)
        fd = fd64 if opts.fused_records16 else fd64[:, :8]
        flags |= _abi.PBP_FUSED_RECORDS16 if opts.fused_records16 else 0
        fused_var = np.zeros(flat.V, dtype=bool)
        fused_var[pv[fz]] = True
        # the rest: proposal records (slices of hub rows sit at the head of pd and are never fused), sampler records, v -> f lists
        keep, rkeep = ~fused_var[pd[:, 0]], ~fused_var[rr[:, 0]]
        fused = FusedLists(counts=(int(k16.sum()), int(k32a.sum()), int(k32b.sum())), counts64=(int(k64a.sum()), int(k64b.sum())),
                           desc=_or_zero_row(np.concatenate([fd[k16], fd[k32a], fd[k32b]])),
                           desc64=np.ascontiguousarray(np.concatenate([fd64[k64a], fd64[k64b]])) if k64a.any() or k64b.any() else None,
                           v2f_rest=v2f_split(flat, np_host, hidden_v[~fused_var[hidden_v]], opts.v2f_records),
                           prop_desc_rest=_or_zero_row(pd[keep]), n_prop_rest=int(keep.sum()),
                           resample_rest=_or_zero_row(rr[rkeep]), n_resample_rest=int(rkeep.sum()))
        host.update({k: a for k, a in fused.named().items() if a is not None})
    return VarSidePlan(host=host, flags=flags, np_host=np_host, T=T, n_prop_desc=int(pd.shape[0]), n_prop_hub=n_prop_hub,
                       n_prop_partial=n_prop_partial, v2f=v2f, fused=fused)


# masks over the described edges: the lists are heavy & ~(small16 | small32), small16, small32, light, rest (heavy: the heavy CLASS)
F2vSplit = namedtuple('F2vSplit', 'heavy small16 small32 light rest heavy_terms heavy_grid_terms')


def f2v_split(words, small_f2v, long_grid_min_edges):
    """Which kernel serves which described edge: `words` is the [k, 32] int32 view of ``lhvi_pbp_describe``'s descriptors (a
    tensor, on any device); words 4 = class, 6 = potential kind, 7 = nj, 8 = np, 9 = T, 14 = light type, 15 = uniform grid."""
    base = (words[:, 4] == 1) & (words[:, 6] != 4)
    # edges with few particles on both sides go four / two to a wavefront, whatever their number of integral points
    # (include/lhvi.h, small16_desc)
    small16 = small32 = base.new_zeros(base.shape)
    if small_f2v:
        small16 = base & (words[:, 7] <= 16) & (words[:, 8] <= 16)
        small32 = base & ~small16 & (words[:, 7] <= 32) & (words[:, 8] <= 32)
    small = small16 | small32
    # (a uniform grid of up to 128 integral points is tabulated by the recurrence, whatever np + T; otherwise two rounds of 64 points)
    on_recurrence = (words[:, 15] == 1) & (words[:, 7] >= 24) & (words[:, 9] <= 128) & (words[:, 8] <= 128)
    two_rounds = words[:, 8] + words[:, 9] <= 128
    if int((on_recurrence & ~two_rounds & ~small).sum().item()) < long_grid_min_edges:
        on_recurrence = two_rounds          # (a short list would only add a launch to a launch-bound sweep)
    heavy = (base & (words[:, 7] <= 64) & (two_rounds | on_recurrence)) | small
    # (output point, partner particle) terms of the heavy kernel: sum over its edges of (np + T) * nj
    hw = words[heavy].long()
    heavy_terms = int(((hw[:, 8] + hw[:, 9]) * hw[:, 7]).sum().item())
    # of those, the terms at the integral points of edges served by the grid recurrence (word 15: uniform grid;
    # at least 24 partner particles, T <= 128; the kernel's range guard is data dependent and assumed to pass)
    # (the few-particle kernel takes the recurrence for every edge with a uniform grid, whatever its particle count)
    on_grid = (hw[:, 15] == 1) & (hw[:, 9] <= 128) & ((hw[:, 7] >= 24) | small[heavy])
    heavy_grid_terms = int((hw[:, 9] * hw[:, 7])[on_grid].sum().item())
    light = ~heavy & (words[:, 14] != 0)          # word 14: set by lhvi_pbp_describe for the light kernel's edges
    return F2vSplit(heavy, small16, small32, light, ~heavy & ~light, heavy_terms, heavy_grid_terms)


def pair_records(light_words, E, key=None):
    """``lhvi_pbp_t.pair_desc``: one record per HybridQuadratic(1 discrete, 1 continuous) factor from the per-edge light
    descriptors (`light_words`: [k, 128] uint8, or its int32 / float64 view; words 0 e, 1 target, 2 partner, 3 partner's canonical
    edge, 7 nj, 8 np, 9 T, 10 grid base, 12-13 partner value, 14 type, 16-27 coefficients), on the descriptors' device.  A type-1
    entry (continuous target) is joined with the type-2 entry (discrete target) of the same factor when there is one; what is left
    of either type becomes a one-sided record.  `E`: the graph's edges; `key`: 0 / 1 per edge, or None.  Returns the records
    ([n1 + n2, 128] uint8: type-1 rows, then the leftover type-2 rows; stable-sorted by `key`) and the number of those with key 0."""
    import torch
    light = light_words.view(torch.uint8).view(-1, 128)
    dev = light.device
    w = light.view(torch.int32).view(-1, 32).long()
    dd = light.view(torch.float64).view(-1, 16)
    i1, i2 = torch.nonzero(w[:, 14] == 1).flatten(), torch.nonzero(w[:, 14] == 2).flatten()
    w1, w2, d1, d2 = w[i1], w[i2], dd[i1], dd[i2]
    lookup = torch.full((max(E, 1),), -1, dtype=torch.int64, device=dev)
    lookup[w2[:, 0]] = torch.arange(i2.numel(), device=dev)
    j = torch.where(torch.isnan(d1[:, 6]), lookup[w1[:, 3]], torch.full_like(w1[:, 3], -1))      # partner hidden: its own entry
    taken = torch.zeros(i2.numel(), dtype=torch.bool, device=dev)
    taken[j[j >= 0]] = True
    rest = torch.nonzero(~taken).flatten()
    n1, n2 = int(i1.numel()), int(rest.numel())
    out = torch.zeros(n1 + n2, 128, dtype=torch.uint8, device=dev)
    ow, od = out.view(torch.int32).view(-1, 32), out.view(torch.float64).view(-1, 16)
    nan = float('nan')
    if n1:
        jj = j.clamp_min(0)
        has = j >= 0
        ow[:n1, 0] = w1[:, 0].int()
        ow[:n1, 1] = torch.where(has, w2[jj, 0], torch.full_like(jj, -1)).int() if i2.numel() else -1
        ow[:n1, 2], ow[:n1, 3] = w1[:, 1].int(), w1[:, 2].int()
        ow[:n1, 4], ow[:n1, 5], ow[:n1, 6], ow[:n1, 7] = w1[:, 8].int(), w1[:, 9].int(), w1[:, 10].int(), w1[:, 7].int()
        od[:n1, 4], od[:n1, 5] = nan, d1[:, 6]
        od[:n1, 6:12] = d1[:, 8:14]
        ow[:n1, 24] = w1[:, 3].int()
        ow[:n1, 25] = (torch.where(has, w2[jj, 3], torch.zeros_like(jj)).int() if i2.numel() else 0)
    if n2:
        r2, rd = w2[rest], d2[rest]
        ow[n1:, 0], ow[n1:, 1] = -1, r2[:, 0].int()
        ow[n1:, 2], ow[n1:, 3] = r2[:, 2].int(), r2[:, 1].int()
        ow[n1:, 4], ow[n1:, 7] = r2[:, 7].int(), r2[:, 8].int()
        od[n1:, 4], od[n1:, 5] = rd[:, 6], nan
        od[n1:, 6:12] = rd[:, 8:14]
        ow[n1:, 25] = r2[:, 3].int()
    first = 0
    if key is not None and n1 + n2:      # sharded runs: records of factors that touch no boundary variable first
        # (a record's key: that of its edges -- both belong to one factor, and a factor's edges share their key)
        edge = torch.where(ow[:, 0] >= 0, ow[:, 0], ow[:, 1]).long()
        order = torch.sort(key[edge], stable=True).indices
        out = out[order].contiguous()
        first = int((key[edge] == 0).sum().item())
    return out, first


F2V_LISTS = ('heavy', 'small16', 'small32', 'light', 'pair', 'fast', 'generic', 'cq')
_F2V_DESC_BYTES = {'heavy': 128, 'small16': 128, 'small32': 128, 'light': 128, 'pair': 128, 'cq': 256}      # per record (include/lhvi.h)


class F2vLists(namedtuple('F2vLists', 'fast_edges fast_desc generic_edges cq_edges cq_desc n_cq heavy_desc n_heavy small16_desc n_small16 '
                                      'small32_desc n_small32 light_desc n_light pair_desc n_pair part_counts generic_pts_log2 '
                                      'n_heavy_class heavy_terms heavy_grid_terms cq_terms pad')):
    """the f -> v half's eight lists (F2V_LISTS): descriptors with their counts (``lhvi_pbp_t.heavy_desc / small16_desc /
    small32_desc / light_desc / pair_desc / cq_desc``; None without any, `pair_desc` also when the light edges are served one by one),
    the edge lists ``fast_edges`` (with ``fast_desc``) and ``generic_edges``, and `cq_edges`, the edges `cq_desc` describes.
    `part_counts`: per list the length of its interior prefix (key 0).  `pad`: one word for the pointer of an empty edge list -- to
    ``lhvi_pbp_f2v`` a null edge list is every edge of the graph."""

    @classmethod
    def empty(cls, pad):
        """no list at all (what a state of the v -> f half alone holds); `pad`: one int32 zero on the state's device"""
        fields = dict.fromkeys(cls._fields, 0)
        fields.update({name: None for name in cls._fields if name.endswith('_desc')})
        fields.update(fast_edges=pad[:0], generic_edges=pad[:0], cq_edges=pad[:0], pad=pad, part_counts=dict.fromkeys(F2V_LISTS, 0),
                      generic_pts_log2=6)
        return cls(**fields)

    n_fast = property(lambda self: int(self.fast_edges.numel()))
    n_generic = property(lambda self: int(self.generic_edges.numel()))
    # entries of the lists, and of their interior prefixes, without the light list's (OwnerRunner.interior_fraction)
    n_items = property(lambda self: sum(getattr(self, 'n_' + name) for name in F2V_LISTS if name != 'light'))
    n_interior = property(lambda self: sum(first for name, first in self.part_counts.items() if name != 'light'))

    def named(self):
        """the lists under the names a sweep object holds them by"""
        named = dict(self._asdict(), _fast_list=self.fast_edges if self.n_fast else self.pad,
                     _generic_list=self.generic_edges if self.n_generic else self.pad)
        del named['pad']
        return named

    def install(self, s):
        s.fast_edges, s.n_fast = _abi.ptr(self.fast_edges if self.n_fast else self.pad), self.n_fast
        s.generic_edges, s.n_generic = _abi.ptr(self.generic_edges if self.n_generic else self.pad), self.n_generic
        s.generic_pts_log2 = int(self.generic_pts_log2)
        s.fast_desc = _abi.ptr(self.fast_desc)
        s.heavy_desc, s.n_heavy = _abi.ptr(self.heavy_desc), int(self.n_heavy)
        s.light_desc, s.n_light = _abi.ptr(self.light_desc), int(self.n_light)
        if self.n_small16:
            s.small16_desc, s.n_small16 = _abi.ptr(self.small16_desc), int(self.n_small16)
        if self.n_small32:
            s.small32_desc, s.n_small32 = _abi.ptr(self.small32_desc), int(self.n_small32)
        if self.pair_desc is not None:
            s.pair_desc, s.n_pair = _abi.ptr(self.pair_desc), int(self.n_pair)
        s.cq_desc, s.n_cq = _abi.ptr(self.cq_desc), int(self.n_cq)

    def install_part(self, s, part):
        """restrict the lists of `s` (installed) to their interior prefix (part 0) or their boundary suffix (part 1)"""
        def cut(name):
            first = self.part_counts[name]
            return (0, first) if part == 0 else (first, getattr(self, 'n_' + name) - first)
        for name, stride in _F2V_DESC_BYTES.items():
            off, cnt = cut(name)
            setattr(s, name + '_desc', getattr(self, name + '_desc').data_ptr() + off * stride if cnt else None)
            setattr(s, 'n_' + name, cnt)
        off, cnt = cut('fast')
        if cnt:
            s.fast_edges, s.fast_desc = self.fast_edges.data_ptr() + 4 * off, self.fast_desc.data_ptr() + off * _abi.PBP_DESC_BYTES
        s.n_fast = cnt                       # 0 with a non-null list pointer = nothing to do
        off, cnt = cut('generic')
        if cnt:
            s.generic_edges = self.generic_edges.data_ptr() + 4 * off
        s.n_generic = cnt
        return s


def f_side_plan(cls, flat, np_host, *, describe, describe_cq, key=None, skip=None, paired_light=True, small_f2v=True,
                long_grid_min_edges=1 << 16):
    """The static work lists of the f -> v half sweep: which kernel serves which edge.
    `cls`: ``lhvi_pbp_classify``'s class per edge ([E] uint8 tensor; the lists live on its device).  `describe`, `describe_cq`:
    edges (int32 tensor) -> their descriptors (uint8 tensor; ``lhvi_pbp_describe``: 128 bytes per edge, ``lhvi_pbp_describe_cq``: 256).
    `key` (sharded runs): 0 / 1 per edge (tensor); every list is ordered key-0 edges first and `part_counts` gives the length of that
    first part.  `skip` (owner-computes shards): boolean per edge (tensor); a marked edge enters no list."""
    import torch
    if skip is not None:
        cls = torch.where(skip, torch.zeros_like(cls), cls)
    L = F2vLists.empty(torch.zeros(1, dtype=torch.int32, device=cls.device))._asdict()
    fast = torch.nonzero((cls == 1) | (cls == 2)).flatten().to(torch.int32)
    generic = torch.nonzero(cls == 3).flatten().to(torch.int32)
    cq = torch.nonzero(cls == 4).flatten().to(torch.int32)
    if key is not None:
        fast, generic, cq = (e[torch.sort(key[e.long()], stable=True).indices].contiguous() for e in (fast, generic, cq))

    def first_part(edges):      # entries of an (ordered) edge list with key 0
        return int((key[edges.long()] == 0).sum().item()) if key is not None and edges.numel() else 0
    first = L['part_counts']
    first.update(generic=first_part(generic), cq=first_part(cq))
    L.update(fast_edges=fast, generic_edges=generic, cq_edges=cq)
    # lanes per generic edge: smallest power of two covering its output points (particles + integral points)
    ge = generic.cpu().numpy()
    tv = flat.edge_var[ge]
    pts = np_host[tv] + np.where(flat.var_cont[tv], flat.var_nstates[tv], 0) if ge.size else np.zeros(0, dtype=int)
    L['generic_pts_log2'] = int(min(6, max(0, int(np.ceil(np.log2(max(int(pts.max()), 1)))) if ge.size else 6)))
    ncq = int(cq.numel())
    if ncq:
        # two-partner edges of conditionally quadratic factors (include/lhvi.h, lhvi_pbp_describe_cq)
        L['cq_desc'], L['n_cq'] = describe_cq(cq), ncq
        cw = L['cq_desc'].view(torch.int32).view(ncq, 2 * _abi.PBP_DESC_BYTES // 4).to(torch.int64)
        # (output point, partner particle, state) terms: type 1: (np + T) * ny * S;  type 2: S * nx * ny
        L['cq_terms'] = int(torch.where(cw[:, 2] == 1, (cw[:, 4] + cw[:, 5]) * cw[:, 9] * cw[:, 3],
                                        cw[:, 3] * cw[:, 12] * cw[:, 9]).sum().item())
    nf = int(fast.numel())
    if nf:
        # split off the edges the specialised kernels serve (f2v_split)
        rows = describe(fast).view(nf, _abi.PBP_DESC_BYTES)
        sp = f2v_split(rows.view(torch.int32), small_f2v, long_grid_min_edges)
        small = sp.small16 | sp.small32
        L.update(heavy_terms=sp.heavy_terms, heavy_grid_terms=sp.heavy_grid_terms, n_heavy_class=int(sp.heavy.sum().item()))
        # (sharded runs: every list is ordered interior part first -- `fast` is -- and split at these counts)
        for name, mask in (('small16', sp.small16), ('small32', sp.small32), ('heavy', sp.heavy & ~small), ('light', sp.light)):
            L[name + '_desc'] = rows[mask].contiguous()
            L['n_' + name], first[name] = int(L[name + '_desc'].shape[0]), first_part(fast[mask])
        L['fast_desc'], L['fast_edges'] = rows[sp.rest].contiguous(), fast[sp.rest].contiguous()
        first['fast'] = first_part(L['fast_edges'])
        if paired_light and L['n_light']:
            L['pair_desc'], first['pair'] = pair_records(L['light_desc'], flat.E, key)
            L['n_pair'] = int(L['pair_desc'].shape[0])
    return F2vLists(**L)


