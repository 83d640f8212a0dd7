#!/bin/bash
# Re-compiles only the two pair-engine units (seconds) and re-links against the existing build/mpe_lib.o: for iterating on
# mpe_pairexp.h.  A full build is ./build.sh; the flags are those of __graft_entry__.py (build_library).
set -e
cd "$(dirname "$0")/.."
python -c 'import sys, __graft_entry__ as g; g.build_library(extra=sys.argv[1:], report=True, only=g.HIP_SOURCES[1:])' "$@"
cp multi_party_ecdsa_amd/libmpecdsa_hip.so build/libmpecdsa_hip.so
grep -h -A12 "Function Name: .*pair_modexp_kernel" build/resource_usage_mpe_pair2048.txt build/resource_usage_mpe_pair1024.txt | grep -E "Function Name|VGPRs:|ScratchSize|VGPRs Spill" | sed 's/remark: [^ ]* *//; s/\[-Rpass.*//'
