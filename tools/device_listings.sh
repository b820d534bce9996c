#!/bin/bash
# Check that a host-side change left the device code alone: write the gfx950 listing of every device translation unit into OUTDIR
# (the Makefile's flags + --cuda-device-only -S), plus kernels.txt, the sorted kernel symbols of all of them.
# usage: tools/device_listings.sh OUTDIR [CSRC]      run it on the parent and on the change, then tools/diff_listings.py the two directories
set -e
OUT=$(mkdir -p "$1" && cd "$1" && pwd)
CS=$(cd "${2:-$(dirname "$0")/../visual-odometry-rs_amd/csrc}" && pwd)
cd "$CS"
FLAGS=$(make -s -f Makefile -f - print-flags <<< 'print-flags: ; @echo $(FLAGS)')
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
PIDS=
listing() { $HIPCC $FLAGS --cuda-device-only -S "$@" & PIDS="$PIDS $!"; }
listing kernels.hip -o "$OUT/kernels.s"
listing -DVORS_FUSED=0 lm_kernels.hip -o "$OUT/lm_kernels.s"
listing -DVORS_FUSED=1 lm_kernels.hip -o "$OUT/lm_kernels_fused.s"
if [ -f product_kernels.hip ]; then listing product_kernels.hip -o "$OUT/product_kernels.s"; fi   # (absent in parents older than the split of lm_kernels.hip)
listing lm_reference.hip -o "$OUT/lm_reference.s"
listing dso_kernels.hip -o "$OUT/dso_kernels.s"
if [ -f render_kernels.hip ]; then listing render_kernels.hip -o "$OUT/render_kernels.s"; fi   # (absent in parents older than the renderer)
if [ -f normal_kernels.hip ]; then listing normal_kernels.hip -o "$OUT/normal_kernels.s"; fi   # (absent in parents older than the normals)
if [ -f icp_kernels.hip ]; then listing icp_kernels.hip -o "$OUT/icp_kernels.s"; fi   # (absent in parents older than the ICP)
if [ -f map_icp_kernels.hip ]; then listing map_icp_kernels.hip -o "$OUT/map_icp_kernels.s"; fi   # (absent in parents older than the map ICP stage)
if [ -f frontend_kernels.hip ]; then listing frontend_kernels.hip -o "$OUT/frontend_kernels.s"; fi   # (absent in parents older than the sensor front end)
if [ -f pose_graph_kernels.hip ]; then listing pose_graph_kernels.hip -o "$OUT/pose_graph_kernels.s"; fi   # (absent in parents older than the pose graph)
for p in $PIDS; do wait $p; done
grep -h '^\s*\.amdhsa_kernel ' "$OUT"/*.s | sort > "$OUT/kernels.txt"
echo "$(wc -l < "$OUT/kernels.txt") kernels, listings in $OUT"
