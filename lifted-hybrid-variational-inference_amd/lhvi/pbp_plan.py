"""Which variable (and which described edge) of a particle sweep goes to which kernel, and the records those kernels read:
pure host functions of the graph arrays -- no device, no environment, same arguments give the same bytes.  The record layouts are
those of ``include/lhvi.h`` (``lhvi_pbp_t``); ``lhvi/pbp.py::_setup`` uploads what ``var_side_plan`` returns in one copy."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import _abi

V2F_CLASSES = ('wide', 'narrow', 'hub', 'mid16', 'mid32')

# everything var_side_plan depends on besides the graph (_ParticleSweep._plan_options).  v2f_records: the wide list travels as records
# (LHVI_PBP_V2F_RECORDS), not as a plain list; fused_records16: sixteen words per fused record (LHVI_PBP_FUSED_RECORDS16), not eight
PlanOptions = namedtuple('PlanOptions', 'sampler_on_device listed_proposal listed_resample sliced_proposal prop_slice packed_v2f '
                                        'v2f_records fused fused_max_particles fused_records16')

# host: name -> host array (or None), what goes to _abi.upload;  flags: to OR into lhvi_pbp_t.flags;  n_prop_partial: rows of
# lhvi_pbp_t.prop_partial;  v2f: V2fLists, or None (the v -> f half addresses the variables by range);  fused: FusedLists or None
VarSidePlan = namedtuple('VarSidePlan', 'host flags np_host T n_prop_desc n_prop_hub n_prop_partial v2f fused')


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
