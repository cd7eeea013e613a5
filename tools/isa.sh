#!/bin/bash
# tools/isa.sh OUT.s [DEFS] — device assembly of $SRC (default step_merged.hip, the merged kernels'
# plain builds; SRC=step_merged_mom.hip: their moments builds; SRC=chunk_lists.hip, refill.hip,
# trace.hip, step.hip, shade.hip, ... for the other units), gfx950, for tools/isa_count.py and
# tools/isa_diff.py
cd "$(dirname "$0")/../xraytracer_amd/csrc"
/opt/rocm/bin/hipcc -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -I../../include -I. --offload-arch=gfx950 \
    --cuda-device-only -S $2 ${SRC:-step_merged.hip} -o "$1"
