"""The flat-graph Gibbs sampler's update kernels in the compiler's resource report, read from the built library (nothing is
built here).

Measured on this commit (vgpr / sgpr): fgibbs_colour_kernel<false> 110 / 89, <true> 128 / 106; fgibbs_hub_kernel<false> 100 / 90,
<true> 122 / 106; no spills of either kind, no private segment.  docs/kernels_fgibbs.md says how the kernels are written so that
they keep the argument array in registers and spill no scalar register."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location('kernel_resources', os.path.join(ROOT, 'scripts', 'kernel_resources.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_update_kernels_have_no_spills_and_no_scratch():
    kr = _tool()
    if not os.path.exists(kr.DEFAULT_LIB) or not kr.rocm_tool('llvm-readelf') or not kr.rocm_tool('clang-offload-bundler'):
        pytest.skip('liblhvi.so or the ROCm llvm-readelf / clang-offload-bundler is not here')
    found = {name: r for name, r in kr.kernel_resources(kr.DEFAULT_LIB).items()
             if 'fgibbs_colour_kernel' in name or 'fgibbs_hub_kernel' in name}
    assert len(found) == 4                       # each with and without the formula interpreter
    for name, r in found.items():
        print(name, r)
        assert r['scratch'] == 0, name
        assert r['vgpr_spill'] == 0, name
        assert r['sgpr_spill'] == 0, name
        assert r['vgpr'] <= 128, name            # four wavefronts a SIMD
        assert r['lds'] <= 32 * 1024, name
