#!/bin/bash
# Timing probe (round 6): the direct f16x2 / bf16x3 kernels with the activation tile staged only for the FIRST kx tap of every kernel row
# (-DGIF_KXSHARE_PROBE: results are wrong) — the DMA issue / LDS-write saving of a "row + halo staged once, three shifted reads" K loop for
# stride-1 3x3 layers, before anybody builds it.
#   here:            bash tools/probes/kxshare_probe.sh build      -> gif_amd/libgif_hip_kxshare.so
#   on the GPU box:  bash tools/probes/kxshare_probe.sh run
set -eu
cd "$(dirname "$0")/../.."
if [ "$1" = build ]; then
  bash tools/probes/probe_lib.sh kxshare "-DGIF_KXSHARE_PROBE" conv_igemm
else
  echo "== normal library"; python tools/probes/kxshare_probe.py
  cp gif_amd/libgif_hip.so /tmp/keep.so; cp gif_amd/libgif_hip_kxshare.so gif_amd/libgif_hip.so
  echo "== activation tile staged once per kernel row (timing only, wrong results)"; python tools/probes/kxshare_probe.py
  cp /tmp/keep.so gif_amd/libgif_hip.so
  echo "== normal library, again"; python tools/probes/kxshare_probe.py
fi
