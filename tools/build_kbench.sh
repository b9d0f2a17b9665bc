#!/bin/bash
# Builds the developer micro-benchmarks (plain and with in-kernel stamps) next to their source.
set -e
cd "$(dirname "$0")/.."
F="--offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize -I3dahv_amd/csrc -Iinclude -Itools"
timeout 900 hipcc $F tools/kbench.cpp -o tools/kbench
timeout 900 hipcc $F -DAHV_STAMPS tools/kbench.cpp -o tools/kbench_stamps
# what the PRESENCE of the exact (non-finite) path costs finite inputs
timeout 900 hipcc $F -DAHV_DIAG_NO_EXACT tools/kbench.cpp -o tools/kbench_noexact
timeout 900 hipcc $F tools/kbench_bwd.cpp -o tools/kbench_bwd
# forward_2d3d from a replayed hipGraph with per-launch marginal costs (tools/gpu_run.sh encoder)
timeout 900 hipcc --offload-arch=gfx950 -O3 -std=c++17 -DAHV_ENC_PROBE -I3dahv_amd/csrc -Iinclude tools/kbench_enc.cpp -o tools/kbench_enc.bin
