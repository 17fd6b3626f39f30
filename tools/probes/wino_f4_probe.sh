#!/bin/bash
# F(4x4,3x3) GEMM timing probe (see wino_f4_probe.py).   build: here;   run: on the GPU box
set -eu
cd "$(dirname "$0")/../.."
if [ "$1" = build ]; then
  bash tools/probes/probe_lib.sh f4probe "-DGIF_WINO_F4_PROBE" conv_winograd
else
  echo "== today: F(2x2,3x3), fused output transform + epilogue"; python tools/probes/wino_f4_probe.py
  cp gif_amd/libgif_hip.so /tmp/keep.so; cp gif_amd/libgif_hip_f4probe.so gif_amd/libgif_hip.so
  echo "== probe: 36 position GEMMs over a quarter of the rows, M planes stored (timing only)"; python tools/probes/wino_f4_probe.py --f4
  cp /tmp/keep.so gif_amd/libgif_hip.so
fi
