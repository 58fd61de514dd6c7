"""CPU suite: the variational solvers' ``map_mode`` switch and the C entry point of the batched MAP (argument checks only --
the kernel itself is exercised by tests/test_gpu_vi_map.py)."""
import ctypes as C

import numpy as np
import pytest


def _one_rv_graph():
    from lhvi.graph import Domain, F, Graph, RV
    from lhvi.potentials import X2Potential
    d = Domain((-5, 5), continuous=True, integral_points=np.linspace(-5, 5, 8))
    rv = RV(d)
    g = Graph()
    g.rvs, g.factors = [rv], [F(X2Potential(1.0, 2.0), [rv])]
    g.init_nb()
    return g, rv


def test_map_mode_defaults_to_scipy():
    from lhvi import c2fvi, vi
    for cls in (vi.VarInference, vi.LiftedVarInference, c2fvi.VarInference, c2fvi._DeviceStage):
        assert cls.map_mode == 'scipy'


def test_unknown_map_mode_raises():
    from lhvi import c2fvi, vi
    g, rv = _one_rv_graph()
    solver = vi.VarInference(g, 2, 3)
    solver.map_mode = 'newton'
    with pytest.raises(ValueError, match='map_mode'):
        solver.map(rv)
    with pytest.raises(ValueError, match='map_mode'):
        solver.map_rows()
    owner = c2fvi.VarInference(g, 2, 3)
    owner.map_mode = 'Device'
    with pytest.raises(ValueError, match='map_mode'):
        c2fvi._DeviceEngine(owner).stage(None, np.zeros(1))


def test_map_entry_point_checks_its_arguments():
    from lhvi import _abi
    lib = _abi.lib()
    g, p = _abi.GraphStruct(), _abi.ViStruct()
    p.K, p.Dmax = 2, 1
    out = (C.c_double * 1)()
    rows = (C.c_int32 * 1)()
    f = lib.lhvi_vi_map_bfgs
    assert f(None, C.byref(p), 1, rows, 1e-5, 200, out, None, None, None, None) == -1
    assert f(C.byref(g), C.byref(p), -1, rows, 1e-5, 200, out, None, None, None, None) == -1
    assert f(C.byref(g), C.byref(p), 1, rows, float('nan'), 200, out, None, None, None, None) == -1
    assert f(C.byref(g), C.byref(p), 1, rows, 1e-5, -1, out, None, None, None, None) == -1
    assert f(C.byref(g), C.byref(p), 1, None, 1e-5, 200, out, None, None, None, None) == -1     # (null arrays)
    assert f(C.byref(g), C.byref(p), 0, None, 1e-5, 200, None, None, None, None, None) == 0      # nothing to do
    p.K = 129
    assert lib.lhvi_strerror(f(C.byref(g), C.byref(p), 1, rows, 1e-5, 200, out, None, None, None, None)) == b'unsupported configuration'
