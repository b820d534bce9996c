#!/bin/bash
# Development aid (GPU): alternating A/B of bench.py between a parent build of the library and this build, and the dumps check.
#   tools/batch_halves_ab.sh series PARENT_LIB LOG RUNS [bench.py arguments]   RUNS x (parent, this build), one line per run appended to LOG
#   tools/batch_halves_ab.sh dumps  PARENT_LIB LOG [bench.py arguments]        bench.py --dump-outputs of both builds compared byte for byte
# PARENT_LIB is libvors_hip.so built from the parent commit (selected with VORS_HIP_LIB). NEW_ENV="VAR=value ..." is set for this build's
# runs only (e.g. NEW_ENV=VORS_BATCH_HALVES=1 forces the two-halves plan at sizes below its default threshold).
# Every GPU step runs under a time limit of its own and the script stops at the first step that fails.
set -o pipefail
what=$1; parent=$2; log=$3; shift 3
line='import sys, json; d = json.loads(sys.stdin.readlines()[-1]); print(sys.argv[1], d["ms_per_step"], d["value"], d["stages_ms"])'
if [ "$what" = series ]; then
  runs=$1; shift
  echo "# bench.py $* ; this build's runs with: ${NEW_ENV:-(nothing set)}" >> "$log"
  for i in $(seq "$runs"); do
    VORS_HIP_LIB=$parent timeout -k 10 150 python bench.py "$@" 2>/dev/null | python -c "$line" parent | tee -a "$log" || exit $?
    env $NEW_ENV timeout -k 10 150 python bench.py "$@" 2>/dev/null | python -c "$line" "new   " | tee -a "$log" || exit $?
  done
else
  d=$(mktemp -d)
  env $NEW_ENV timeout -k 10 150 python bench.py "$@" --steps 3 --warmup 1 --dump-outputs "$d/new" > /dev/null 2>&1 || exit $?
  VORS_HIP_LIB=$parent timeout -k 10 150 python bench.py "$@" --steps 3 --warmup 1 --dump-outputs "$d/parent" > /dev/null 2>&1 || exit $?
  for f in "$d"/new/*.npy; do cmp "$f" "$d/parent/$(basename "$f")" || { echo "bench.py $*: $(basename "$f") DIFFERS" | tee -a "$log"; exit 3; }; done
  echo "bench.py $* (this build with: ${NEW_ENV:-nothing set}): $(ls "$d/new" | wc -l) arrays byte-identical to the parent's" | tee -a "$log"
  rm -r "$d"
fi
