"""The heavy f2v kernel's resource report, read from the built library (nothing is built here).

Measured on this commit: vgpr 70, sgpr 94, no spills, no private segment (parent: 71 / 94, 35 + 2 spills, 12 bytes)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location('kernel_resources', os.path.join(ROOT, 'scripts', 'kernel_resources.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_heavy_kernel_has_no_spills_and_no_scratch():
    kr = _tool()
    if not os.path.exists(kr.DEFAULT_LIB) or not kr.rocm_tool('llvm-readelf') or not kr.rocm_tool('clang-offload-bundler'):
        pytest.skip('liblhvi.so or the ROCm llvm-readelf / clang-offload-bundler is not here')
    heavy = [r for name, r in kr.kernel_resources(kr.DEFAULT_LIB).items() if 'pbp_f2v_heavy_kernel' in name]
    assert len(heavy) == 1
    r = heavy[0]
    print(r)
    assert r['vgpr'] <= 72                       # 7 waves per SIMD
    assert r['vgpr_spill'] == 0
    assert r['scratch'] == 0
    assert r['sgpr_spill'] == 0
