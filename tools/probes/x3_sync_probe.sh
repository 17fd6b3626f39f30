#!/bin/bash
# Probe build of the library with cycle counters around the mid-stage sync of the bf16x3 direct kernel (-DGIF_X3_TIMING_PROBE).
#   here:            bash tools/probes/x3_sync_probe.sh build      -> gif_amd/libgif_hip_syncprobe.so
#   on the GPU box:  bash tools/probes/x3_sync_probe.sh run        (swaps the library in for the run, restores it)
set -eu
cd "$(dirname "$0")/../.."
if [ "$1" = build ]; then
  bash tools/probes/probe_lib.sh syncprobe "-DGIF_X3_TIMING_PROBE" conv_igemm
else
  cp gif_amd/libgif_hip.so /tmp/keep.so; cp gif_amd/libgif_hip_syncprobe.so gif_amd/libgif_hip.so
  python tools/probes/x3_sync_probe.py || true
  cp /tmp/keep.so gif_amd/libgif_hip.so
fi
