#!/bin/bash
# Timing probe (round 6): the f16x2 weight gradient with the three dx taps of a kernel row formed from ONE staged pair of tiles
# (-DGIF_WGRAD_KX3_PROBE: results are wrong, instruction and traffic counts are those of such a kernel up to the shifted conversion).
#   here:            bash tools/probes/wgrad_kx3_probe.sh build      -> gif_amd/libgif_hip_wgkx3.so
#   on the GPU box:  bash tools/probes/wgrad_kx3_probe.sh run
set -eu
cd "$(dirname "$0")/../.."
if [ "$1" = build ]; then
  bash tools/probes/probe_lib.sh wgkx3 "-DGIF_WGRAD_KX3_PROBE" conv_wgrad
else
  cp gif_amd/libgif_hip.so /tmp/keep.so
  echo "== normal library"; python tools/probes/wgrad_buf_probe.py child
  cp gif_amd/libgif_hip_wgkx3.so gif_amd/libgif_hip.so
  echo "== three taps per staged stage (timing only, wrong results)"; python tools/probes/wgrad_buf_probe.py child
  cp /tmp/keep.so gif_amd/libgif_hip.so
  echo "== normal library, again"; python tools/probes/wgrad_buf_probe.py child
fi
