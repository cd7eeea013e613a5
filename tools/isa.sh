#!/bin/bash
# tools/isa.sh OUT.s [DEFS] — device assembly of $SRC (default step_tri.hip, the merged kernels;
# SRC=step.hip, shade.hip, ... for the other units), gfx950, for tools/isa_count.py
cd "$(dirname "$0")/../xraytracer_amd/csrc"
/opt/rocm/bin/hipcc -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -I../../include -I. --offload-arch=gfx950 \
    --cuda-device-only -S $2 ${SRC:-step_tri.hip} -o "$1"
