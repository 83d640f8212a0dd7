#!/bin/bash
# Builds libmpecdsa_hip.so (gfx950) in-tree: three translation units compiled in parallel, then linked.  The units and the flags are
# those of __graft_entry__.py (build_library).
# Usage: ./build.sh [extra hipcc flags]     (resource usage of every kernel -> build/resource_usage.txt)
set -e
cd "$(dirname "$0")"
python -c 'import sys, __graft_entry__ as g; g.build_library(extra=sys.argv[1:], report=True)' "$@" || { echo "BUILD FAILED"; exit 1; }
cp multi_party_ecdsa_amd/libmpecdsa_hip.so build/libmpecdsa_hip.so
# one line per kernel: registers, scratch bytes per lane, waves per SIMD and what was spilled
sed 's/remark: [^ ]* *//; s/ *\[-Rpass-analysis=kernel-resource-usage\]//' build/resource_usage.txt | awk '
  /^Function Name:/ { name = $3 }  /^TotalSGPRs:/ { sgpr = $2 }  /^VGPRs:/ { vgpr = $2 }  /^ScratchSize/ { scratch = $3 }
  /^Occupancy/ { occ = $3 }  /^SGPRs Spill:/ { sspill = $3 }
  /^VGPRs Spill:/ { print name, "VGPRs:", vgpr, "SGPRs:", sgpr, "scratch:", scratch, "occupancy:", occ, "spills(SGPR/VGPR):", sspill "/" $3 }'
