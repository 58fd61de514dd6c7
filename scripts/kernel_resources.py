#!/usr/bin/env python3
"""Per-kernel register, spill, scratch and LDS figures of the built library or of an assembly file.

    python3 scripts/kernel_resources.py                     # lifted-hybrid-variational-inference_amd/csrc/liblhvi.so
    python3 scripts/kernel_resources.py path/to/pbp.s       # hipcc -S --cuda-device-only output
    python3 scripts/kernel_resources.py --match heavy       # only kernels whose name contains the word

The figures are the compiler's own: the `amdhsa.kernels` metadata of the gfx950 code object (read with the ROCm
`llvm-readelf --notes` after `clang-offload-bundler` has taken the code object out of the library), or the same metadata
block at the end of an assembly file.  Resource numbers only -- no instruction is looked at.
"""
import argparse
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_LIB = os.path.join(ROOT, 'lifted-hybrid-variational-inference_amd', 'csrc', 'liblhvi.so')
FIELDS = (('vgpr', '.vgpr_count'), ('sgpr', '.sgpr_count'), ('sgpr_spill', '.sgpr_spill_count'), ('vgpr_spill', '.vgpr_spill_count'),
          ('scratch', '.private_segment_fixed_size'), ('lds', '.group_segment_fixed_size'), ('kernarg', '.kernarg_segment_size'))


def rocm_tool(name):
    for pat in ('/opt/rocm/llvm/bin/', '/opt/rocm/lib/llvm/bin/', '/opt/rocm*/llvm/bin/', '/opt/rocm*/lib/llvm/bin/'):
        for d in sorted(glob.glob(pat)):
            if os.access(os.path.join(d, name), os.X_OK):
                return os.path.join(d, name)
    return None


def parse_metadata(text):
    """the `amdhsa.kernels` list of a metadata note (YAML as llvm-readelf or the assembler prints it) -> {name: {field: int}}"""
    kernels, cur = {}, None
    for line in text.split('\n'):
        m = re.match(r'\s*(-\s+)?(\.[a-z_]+):\s*(\S.*)?$', line)
        if not m:
            continue
        indent = len(line) - len(line.lstrip())
        new_item, key, val = m.group(1), m.group(2), (m.group(3) or '').strip().strip("'\"")
        if new_item and indent <= 2:
            cur = {}
        if cur is None or indent > 4:           # (the entries of .args sit deeper)
            continue
        if key == '.name':
            kernels[val] = cur
        for short, field in FIELDS:
            if key == field and val.isdigit():
                cur[short] = int(val)
    return {k: v for k, v in kernels.items() if 'vgpr' in v}


def metadata_of_library(path):
    bundler, readelf = rocm_tool('clang-offload-bundler'), rocm_tool('llvm-readelf')
    if not bundler or not readelf:
        raise RuntimeError('the ROCm clang-offload-bundler / llvm-readelf were not found')
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, 'fatbin')
        objcopy = rocm_tool('llvm-objcopy')
        subprocess.check_call([objcopy, '--dump-section', '.hip_fatbin=' + fat, path, os.path.join(tmp, 'unused')])
        # one bundle per translation unit, back to back
        with open(fat, 'rb') as f:
            blob = f.read()
        magic = b'__CLANG_OFFLOAD_BUNDLE__'
        starts = [m.start() for m in re.finditer(magic, blob)]
        out = []
        for i, at in enumerate(starts):
            part = os.path.join(tmp, 'bundle%d' % i)
            with open(part, 'wb') as f:
                f.write(blob[at:starts[i + 1] if i + 1 < len(starts) else len(blob)])
            listing = subprocess.check_output([bundler, '--list', '--type=o', '--input=' + part]).decode().split()
            for j, t in enumerate(t for t in listing if 'amdgcn' in t):
                co = os.path.join(tmp, 'co%d_%d' % (i, j))
                subprocess.check_call([bundler, '--unbundle', '--type=o', '--input=' + part, '--targets=' + t, '--output=' + co])
                out.append(subprocess.check_output([readelf, '--notes', co]).decode())
        return '\n'.join(out)


def kernel_resources(path=DEFAULT_LIB):
    if path.endswith('.s'):
        with open(path) as f:
            text = f.read()
        at = text.find('amdhsa.kernels:')
        return parse_metadata(text[at:] if at >= 0 else '')
    return parse_metadata(metadata_of_library(path))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('path', nargs='?', default=DEFAULT_LIB)
    ap.add_argument('--match', default='', help='only kernels whose (mangled) name contains this')
    a = ap.parse_args()
    res = kernel_resources(a.path)
    if not res:
        sys.exit('no kernel metadata in %s' % a.path)
    print('%-72s %5s %5s %7s %7s %8s %7s %8s' % ('kernel', 'vgpr', 'sgpr', 's-spill', 'v-spill', 'scratch', 'lds', 'kernarg'))
    for name in sorted(res):
        if a.match in name:
            r = res[name]
            print('%-72s %5d %5d %7d %7d %8d %7d %8d' % (name[:72], r.get('vgpr', -1), r.get('sgpr', -1), r.get('sgpr_spill', -1),
                                                        r.get('vgpr_spill', -1), r.get('scratch', -1), r.get('lds', -1), r.get('kernarg', -1)))


if __name__ == '__main__':
    main()
