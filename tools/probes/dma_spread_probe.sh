#!/bin/bash
# Timing + correctness probe (round 6): the bf16x3 / f16x2 direct kernels with the stage's LDS-DMA pieces issued one at a time BETWEEN the MFMAs
# of the step's first k-group (-DGIF_DMA_SPREAD) instead of back to back ahead of them.  Tap-grid launches only (the probe build does not handle
# the tap-dense order).
#   here:            bash tools/probes/dma_spread_probe.sh build      -> gif_amd/libgif_hip_spread.so
#   on the GPU box:  bash tools/probes/dma_spread_probe.sh run
set -eu
cd "$(dirname "$0")/../.."
if [ "$1" = build ]; then
  bash tools/probes/probe_lib.sh spread "-DGIF_DMA_SPREAD" conv_igemm
else
  echo "== normal library"; python tools/probes/kxshare_probe.py
  cp gif_amd/libgif_hip.so /tmp/keep.so; cp gif_amd/libgif_hip_spread.so gif_amd/libgif_hip.so
  echo "== DMA pieces spread between the MFMAs of the first k-group"; python tools/probes/kxshare_probe.py
  python -m pytest tests/test_gpu_f16x2.py -x -q -k "not_less_accurate or epilogue_and_determinism or adversarial_operands or rescale_path" 2>&1 | tail -3
  cp /tmp/keep.so gif_amd/libgif_hip.so
  echo "== normal library, again"; python tools/probes/kxshare_probe.py
fi
