#!/bin/bash
# Build the host twins of csrc/hg_energy.hip into a stand-alone program with AddressSanitizer and UBSan on the HOST code and run it
# on the CPU (no device is touched; sanitizers never run on the GPU or on code loaded into python).
set -euo pipefail
here="$(cd "$(dirname "$0")" && pwd)"
out="${TMPDIR:-/tmp}/hg_energy_host_sanitize"
"${HIPCC:-/opt/rocm/bin/hipcc}" -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
    -Xarch_host -fno-sanitize-recover=undefined "$here/hg_energy_host_sanitize.hip" -o "$out"
"$out"
