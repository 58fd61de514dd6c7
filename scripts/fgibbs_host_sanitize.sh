#!/bin/bash
# Build the host twin of csrc/fgibbs.hip into a stand-alone program with AddressSanitizer and UBSan on the HOST code and run it on
# the CPU over the models of tests/fgibbs_models.py (no device is touched; sanitizers never run on the GPU or on code loaded into
# python).  Python only writes the models' arrays to a text file; the program under the sanitizers reads that file.
set -euo pipefail
here="$(cd "$(dirname "$0")" && pwd)"
out="${TMPDIR:-/tmp}/fgibbs_host_sanitize"
PYTHONPATH="$here/../lifted-hybrid-variational-inference_amd:$here/../tests" "${PYTHON:-python3}" - "$out.models" <<'PY'
import sys
import numpy as np
import fgibbs_models as fm
from lhvi import _abi, fgibbs
with open(sys.argv[1], 'w') as fh:
    for name in fm.DET_MODELS:
        m = fm.build(name)
        s = fgibbs.FlatGibbs(m.g)
        fl = s.flat
        off, par, interpreted = _abi.device_potentials(fl)
        col_ptr, col_var, hub_ptr, hub_var = fgibbs.work_lists(fl, s.colour, s.n_colours, 64)
        keep_row = np.where(s.hidden, np.cumsum(s.hidden) - 1, -1)
        fh.write('%s %d %d %d %d %d %d %d %d %d\n' % (name, fl.V, fl.F, fl.E, fl.dom_cont.size, fl.pot_kind.size, interpreted, s.n_colours,
                                                      fm.MAX_SHRINK[name], s.n_states))
        for a in (fl.fac_ptr, fl.edge_var, fl.edge_fac, fl.var_ptr, fl.var_edge, fl.fac_pot, fl.var_dom, fl.dom_cont, fl.dom_ptr,
                  fl.pot_kind, off, col_ptr, col_var, hub_ptr, hub_var, s.cnt_off, keep_row):
            fh.write('%d %s\n' % (a.size, ' '.join(str(int(v)) for v in a)))
        init = np.zeros(0) if m.init is None else np.tile(m.init, 3)
        for a in (fl.var_value, fl.dom_lo, fl.dom_hi, fl.dom_val, par, init):
            fh.write('%d %s\n' % (a.size, ' '.join(float(v).hex() for v in a)))
PY
"${HIPCC:-/opt/rocm/bin/hipcc}" -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
    -Xarch_host -fno-sanitize-recover=undefined "$here/fgibbs_host_sanitize.hip" -o "$out"
"$out" "$out.models"
