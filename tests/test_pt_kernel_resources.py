"""The tempered sampler's kernel in the compiler's resource report, read from the built library (nothing is built here).

Measured on this commit: vgpr 160, sgpr 106, no spills of either kind, no private segment; LDS is dynamic
(lhvi_pt_lds_bytes).  docs/kernels_pt.md says how the kernel is written so that it spills no scalar register."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location('kernel_resources', os.path.join(ROOT, 'scripts', 'kernel_resources.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_ladder_kernel_has_no_spills_and_no_scratch():
    kr = _tool()
    if not os.path.exists(kr.DEFAULT_LIB) or not kr.rocm_tool('llvm-readelf') or not kr.rocm_tool('clang-offload-bundler'):
        pytest.skip('liblhvi.so or the ROCm llvm-readelf / clang-offload-bundler is not here')
    found = [r for name, r in kr.kernel_resources(kr.DEFAULT_LIB).items() if 'pt_ladder_kernel' in name]
    assert len(found) == 1
    r = found[0]
    print(r)
    assert r['scratch'] == 0
    assert r['vgpr_spill'] == 0
    assert r['sgpr_spill'] == 0
    assert r['vgpr'] <= 256                      # a workgroup of four wavefronts, one per SIMD, with room for a second
