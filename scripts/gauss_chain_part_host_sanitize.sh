#!/bin/bash
# Build the host twin of the partitioned chain solve (csrc/gauss_chain_part.hip, csrc/gauss_chain.hip) into a stand-alone program
# with AddressSanitizer and UBSan on the HOST code and run it on the CPU (no device is touched; sanitizers never run on the GPU or
# on code loaded into python).  The twin runs the device's lines with one lane, so an index out of a workspace slot shows here.
set -euo pipefail
here="$(cd "$(dirname "$0")" && pwd)"
csrc="$here/../lifted-hybrid-variational-inference_amd/csrc"
out="${TMPDIR:-/tmp}/gauss_chain_part_host_sanitize"
"${HIPCC:-/opt/rocm/bin/hipcc}" -O1 -g -std=c++17 --offload-arch=gfx950 -Wno-unused-function -Xarch_host -fsanitize=address,undefined \
    -Xarch_host -fno-sanitize-recover=undefined "$here/gauss_chain_part_host_sanitize.hip" "$csrc/gauss_chain.hip" \
    "$csrc/gauss_chain_part.hip" "$csrc/abi.hip" -o "$out"
"$out"
