"""CPU test of ``gibbs.place``: the lanes of a chain and the place of the reduced tables that the plain, the annealed and the
tempered sampler's runners share (docs/kernels_gibbs.md, "Lanes"), restated by brute force over the library's
``lhvi_gibbs_lds_bytes`` / ``lhvi_ais_lds_bytes`` / ``lhvi_pt_lds_bytes`` (plain host functions) and compared on a grid of
shapes, with no device asked for."""
import itertools

import pytest

from lhvi import _abi, gibbs

LIMIT, BLOCK = 64 * 1024, 256
POW2 = (1, 2, 4, 8, 16, 32, 64)
ND, MAX_STATES = 3, 4
NCS, TABLE_DOUBLES, TABLES = (0, 1, 2, 8, 33, 64), (0, 630, 9000), (None, 'lds', 'global')
LANES, REPLICAS = (None, 1, 4, 64, 3, 128), (1, 2, 8, 64, 256, 257)


def sizes(fn, Nc, td, R):
    """{(lanes, tables in LDS): the bytes of a workgroup}"""
    rest = () if R is None else (R,)
    return {(l, t): int(fn(Nc, ND, MAX_STATES + (td if t else 0), *rest, l)) for l in POW2 for t in (False, True)}


def restated(size, Nc, tables, lanes, R):
    """('ok', lanes, in_lds) or ('error', text) from the written rules"""
    if R is not None and R > BLOCK:
        return 'error', '%d replicas exceed the %d threads of a workgroup' % (R, BLOCK)
    if lanes is None:
        first = min(l for l in POW2 if l >= 4 and 2 * l >= min(Nc, 64))
        if R is None:       # doubled while the workgroup is too large, sized with the tables in LDS only when they are forced there
            lanes = next((l for l in POW2 if l >= first and size[l, tables == 'lds'] <= LIMIT), 64)
        else:               # halved while the replicas exceed a workgroup, never grown
            lanes = next((l for l in POW2[::-1] if l <= first and R * l <= BLOCK), 1)
    if lanes not in POW2:
        return 'error', 'lanes must be a power of two up to 64'
    if R is not None and R * lanes > BLOCK:
        return 'error', '%d replicas of %d lanes exceed the %d threads of a workgroup' % (R, lanes, BLOCK)
    in_lds = size[lanes, True] <= LIMIT if tables is None else tables == 'lds'
    if size[lanes, in_lds] > LIMIT:
        what = '%d chains' % (64 // lanes) if R is None else '%d replicas' % R
        return 'error', 'a workgroup of %s needs %d bytes of LDS, more than %d' % (what, size[lanes, in_lds], LIMIT)
    return 'ok', lanes, in_lds


def test_place_equals_the_written_rules_without_a_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError('place asked for a device')
    l = _abi.lib()                  # (loading the library imports torch; nothing after this may)
    monkeypatch.setattr(_abi, 'require_gpu', no_device)
    monkeypatch.setattr(_abi, '_torch', no_device)
    kinds = [(l.lhvi_gibbs_lds_bytes, None), (l.lhvi_ais_lds_bytes, None)] + [(l.lhvi_pt_lds_bytes, R) for R in REPLICAS]
    seen = set()
    for (fn, R), Nc, td in itertools.product(kinds, NCS, TABLE_DOUBLES):
        size = sizes(fn, Nc, td, R)
        for tables, lanes in itertools.product(TABLES, LANES):
            want = restated(size, Nc, tables, lanes, R)
            try:
                got = ('ok',) + gibbs.place(fn, Nc, ND, MAX_STATES, td, lanes, tables, R)
            except ValueError as e:
                got = ('error', str(e))
            assert got == want, (R, Nc, td, tables, lanes)
            seen.add((R is None, want[1].split(' ')[-1] if want[0] == 'error' else want[1:]))
    # the grid reaches every rule: each refusal for both families, tables in both places, lanes grown and shrunk
    assert {(True, '64'), (True, str(LIMIT)), (False, 'workgroup'), (False, '64'), (False, str(LIMIT))} <= seen
    assert {(True, (4, True)), (True, (64, False)), (False, (4, False)), (False, (1, True))} <= seen
