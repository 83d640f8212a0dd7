#!/bin/bash
# Builds libmpecdsa_hip.so (gfx950) in-tree: three translation units compiled in parallel, then linked.  The units and the flags are
# those of __graft_entry__.py (build_library).
# Usage: ./build.sh [extra hipcc flags]     (resource usage of every kernel -> build/resource_usage.txt)
set -e
cd "$(dirname "$0")"
python -c 'import sys, __graft_entry__ as g; g.build_library(extra=sys.argv[1:], report=True)' "$@" || { echo "BUILD FAILED"; exit 1; }
cp multi_party_ecdsa_amd/libmpecdsa_hip.so build/libmpecdsa_hip.so
grep -E "Function Name|VGPRs:|Occupancy|VGPRs Spill" build/resource_usage.txt | sed 's/remark: [^ ]* *//' | paste - - - - | sed 's/\[-Rpass-analysis=kernel-resource-usage\]//g' | awk '{print $3, $5, $6, $9, $10, $13,$14,$15}'
