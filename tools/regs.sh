#!/bin/bash
# register use of the quad kernel's main variants for (segments per quad, waves per SIMD) pairs, one line per kernel:
# VGPRs, scratch, occupancy, spilled SGPRs (each one a v_writelane / v_readlane pair where it is live) and spilled VGPRs.
#   tools/regs.sh "2 4" "3 4"          EXTRA="-DGCRE_IE_TIMING" tools/regs.sh "2 4"
cd "$(dirname "$0")/../geneticscre_amd/csrc"
for v in "$@"; do set -- $v; echo "QSEGS=$1 QWAVES=$2:"
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -DGCRE_IEQ_ONLY -DGCRE_QSEGS=$1 -DGCRE_QWAVES=$2 $EXTRA -Rpass-analysis=kernel-resource-usage -c gcre_ieq.hip -o /tmp/ieq.o 2>&1 |
    grep -E "error|warning:|Function Name|  VGPRs:|ScratchSize|SGPRs Spill|VGPRs Spill|Occupancy" | sed 's/.*remark: *//; s/ *\[-Rpass.*//; s/Function Name: /\n/' | c++filt | tr '\n' '|' |
    sed 's/||/\n  /g; s/|/  /g; s/void gcre:://g; s/(gcre::IeArgs)//g; s/ \[bytes\/lane\]//g; s/ \[waves\/SIMD\]//g'; echo; done
