#!/bin/bash
# Build the host twin of csrc/pt.hip into a stand-alone program with AddressSanitizer and UBSan on the HOST code and run it on
# the CPU over the flat models of rand_3_2, wide_states, pure_disc, no_disc and two_wells (no device is touched; sanitizers never run on the
# GPU or on code loaded into python).  Python only writes the models' arrays to a text file; the program under the sanitizers
# reads that file.
set -euo pipefail
here="$(cd "$(dirname "$0")" && pwd)"
out="${TMPDIR:-/tmp}/pt_host_sanitize"
PYTHONPATH="$here/../lifted-hybrid-variational-inference_amd:$here/../tests" "${PYTHON:-python3}" - "$out.models" <<'PY'
import sys
import pt_models as gmod
with open(sys.argv[1], 'w') as fh:
    for name in ('rand_3_2', 'wide_states', 'pure_disc', 'no_disc', 'two_wells'):
        gm = gmod.build(name)['gm']
        ex = gm.ex
        fh.write('%s %d %d %d %d %d %d %d\n' % (name, ex.Nd, ex.Nc, ex.n_quad, ex.n_tab, gm.n_hyb, gm.table_doubles, gm.max_states))
        for a in (ex.dstates, ex.quad_ptr, ex.quad_desc, ex.tab_ptr, ex.tab_desc, gm.dstate_off, gm.vt_ptr, gm.vt_fac, gm.vh_ptr,
                  gm.vh_fac, gm.hyb_quad, gm.hyb_off):
            fh.write('%d %s\n' % (a.size, ' '.join(str(int(v)) for v in a)))
        for a in (ex.quad_par, ex.tab_par):
            fh.write('%d %s\n' % (a.size, ' '.join(float(v).hex() for v in a)))
PY
"${HIPCC:-/opt/rocm/bin/hipcc}" -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
    -Xarch_host -fno-sanitize-recover=undefined "$here/pt_host_sanitize.hip" -o "$out"
"$out" "$out.models"
