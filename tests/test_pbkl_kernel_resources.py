"""The particle-belief KL kernel's resource report, read from the built library (nothing is built here).

Measured on this commit: vgpr 256, sgpr 106, 108 spilled scalars, 4 spilled vector registers, 512 bytes of private segment
(the per-argument arrays of ``f2v_point_generic`` and the spills), 20024 bytes of LDS.  docs/kernels_pbkl.md states the
occupancy the kernel is laid out for: 8 waves per CU (2 per SIMD), set by its LDS; the bounds below are that occupancy's.
Nothing is asserted about the instructions."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location('kernel_resources', os.path.join(ROOT, 'scripts', 'kernel_resources.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_pbp_kl_kernel_exists_once_and_fits_eight_waves_per_cu():
    kr = _tool()
    if not os.path.exists(kr.DEFAULT_LIB) or not kr.rocm_tool('llvm-readelf') or not kr.rocm_tool('clang-offload-bundler'):
        pytest.skip('liblhvi.so or the ROCm llvm-readelf / clang-offload-bundler is not here')
    found = [r for name, r in kr.kernel_resources(kr.DEFAULT_LIB).items() if 'pbp_kl_kernel' in name]
    assert len(found) == 1
    r = found[0]
    print(r)
    assert r['vgpr'] <= 256                      # 2 waves per SIMD: 512 / 2
    assert r['lds'] <= 160 * 1024 // 8           # 8 workgroups of one wave per CU
