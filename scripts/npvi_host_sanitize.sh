#!/bin/bash
# Build the host twins of csrc/npvi.hip and csrc/oneshot.hip into two stand-alone programs with AddressSanitizer and UBSan on the
# HOST code and run them on the CPU over models of tests/npvi_models.py and tests/oneshot_models.py (no device is touched;
# sanitizers never run on the GPU or on code loaded into python).  Python only writes the models' arrays to a text file; the
# programs under the sanitizers read that file and print a checksum of every output.  CSRC=<another csrc directory> builds the
# programs from another version of the sources with the same entry points, to compare the printed lines.
set -euo pipefail
here="$(cd "$(dirname "$0")" && pwd)"
csrc="${CSRC:-$here/../lifted-hybrid-variational-inference_amd/csrc}"
out="${TMPDIR:-/tmp}/npvi_host_sanitize"
PYTHONPATH="$here/../lifted-hybrid-variational-inference_amd:$here/../tests" "${PYTHON:-python3}" - "$out" <<'PY'
import sys
import numpy as np
import npvi_models as nm
import oneshot_models as om
from lhvi import _abi
from lhvi.npvi import NPVI
from lhvi.oneshot import OneShot
COMMON = [('gaussian_chain5', lambda: nm.gaussian_chain(5), 1, 3), ('hybrid', nm.hybrid_graph, 3, 3), ('interpreted', nm.interpreted_graph, 2, 3),
          ('hybrid_counts', lambda: nm.hybrid_graph(seed=5), 2, 3)]         # with sharing counts; the others pass NULL
ONESHOT = [('isolated', om.isolated_graph, 3, 3), ('leaves_only', om.leaves_only_graph, 2, 3)]
for cls, stem, models in ((NPVI, 'npvi', COMMON), (OneShot, 'oneshot', COMMON + ONESHOT)):
    with open('%s.%s.models' % (sys.argv[1], stem), 'w') as fh:
        for name, make, K, T in models:
            s = cls(make(), K, T, seed=3)
            if name == 'hybrid_counts':
                rng = np.random.RandomState(7)
                s = cls(make(), K, T, seed=3, var_count=rng.randint(2, 5, size=s.flat.V).astype(float),
                        fac_count=rng.randint(1, 4, size=s.flat.F).astype(float))
            fl, h = s.flat, s._h
            off, par, interpreted = _abi.device_potentials(fl)
            lb = np.log(s.Var_bds)
            fh.write('%s %d %d %d %d %d %d %d %d %d %d %d %s %s\n' % (name, fl.V, fl.F, fl.E, fl.dom_cont.size, fl.pot_kind.size, interpreted, K, T,
                                                                     s.Dmax, s.max_slots, s.max_arity, float(lb[0]).hex(), float(lb[1]).hex()))
            for a in (fl.fac_ptr, fl.edge_var, fl.edge_fac, fl.var_ptr, fl.var_edge, fl.fac_pot, fl.var_dom, fl.dom_cont, fl.dom_ptr,
                      fl.pot_kind, off, s._edge_axis[:fl.E]):
                fh.write('%d %s\n' % (a.size, ' '.join(str(int(v)) for v in np.ravel(a))))
            none = np.zeros(0)
            for a in (fl.var_value, fl.dom_lo, fl.dom_hi, fl.dom_val, par, s.quad_x, s.quad_w, s._mu_lo, s._mu_hi,
                      none if s.var_count is None else s.var_count, none if s.fac_count is None else s.fac_count,
                      getattr(s, 'var_coef', none), h['tau'], h['theta_c'], h['rho'], h['w'], h['eta_c'], h['eta_d']):
                fh.write('%d %s\n' % (a.size, ' '.join(float(v).hex() for v in np.ravel(a))))
PY
flags=(-O1 -g -std=c++17 --offload-arch=gfx950 -I "$csrc" -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined)
"${HIPCC:-/opt/rocm/bin/hipcc}" "${flags[@]}" "$here/npvi_host_sanitize.hip" -o "$out.npvi"
"${HIPCC:-/opt/rocm/bin/hipcc}" "${flags[@]}" -DLHVI_SANITIZE_ONESHOT "$here/npvi_host_sanitize.hip" "$csrc/npvi.hip" -o "$out.oneshot"
"$out.npvi" "$out.npvi.models"
"$out.oneshot" "$out.oneshot.models"
