#!/bin/bash
# Builds a probe library next to the production one (no GPU needed):
#   bash tools/probes/probe_lib.sh NAME "FLAGS" SOURCE...      -> gif_amd/libgif_hip_NAME.so
# The timing probes and ablation kernels are not in gif_amd/csrc any more: they live in three patch files here.  This script copies
# gif_amd/csrc to gif_amd/csrc/_probe/src, puts them back (wgrad_h2v3.patch, ablation_knobs.patch, probe_blocks.patch, in this order:
# each is the reverse of the change that took its code out), compiles the named SOURCEs (conv_igemm, conv_wgrad, conv_winograd) of
# that copy with FLAGS (e.g. "-DGIF_KXSHARE_PROBE"; "" for the run-time ablation knobs GIF_HALO_DBG / GIF_WINO_DBG / GIF_H2_WGRAD_V3)
# and links them with the production objects of every other source.  Probe libraries compute WRONG results by design.
set -eu
cd "$(dirname "$0")/../.."
NAME=$1; FLAGS=$2; shift 2
make -s -j8 -C gif_amd/csrc ARCH=gfx950
S=gif_amd/csrc/_probe/src
rm -rf $S; mkdir -p $S; cp gif_amd/csrc/*.hip gif_amd/csrc/*.h $S/
for p in wgrad_h2v3 ablation_knobs probe_blocks; do patch -s -p3 -d $S < tools/probes/$p.patch; done
cd gif_amd/csrc
OBJS=$(ls _build/*.o); NEW=
for f in "$@"; do
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -I../../include -Wno-unused-function -Wno-unused-value $FLAGS -c _probe/src/$f.hip -o _probe/${f}_$NAME.o &
  OBJS=$(echo "$OBJS" | grep -v "^_build/$f.o$"); NEW="$NEW _probe/${f}_$NAME.o"
done; wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../libgif_hip_$NAME.so $OBJS $NEW
