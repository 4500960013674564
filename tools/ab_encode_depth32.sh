#!/bin/bash
# The A/B of DESIGN.md section 4.29 on one GPU box: flacenc_hip_encode_streams at 16 bits on the 2 048-stream library,
# another build of this repository (its parent, built in PARENT_DIR) and this one alternately, one process each:
#   tools/ab_encode_depth32.sh <out-file> <rounds> <PARENT_DIR>       (paths relative to the repo root)
# Two runs of the parent per round give its own spread, the margin the comparison is read against.  Every run has its
# own time limit and the first run that fails ends the script: nothing more is started on a GPU that has just faulted or
# hung.  The raw lines go to <out-file>; tools/time_encode_depth32.py says what they hold.
set -u -o pipefail
OUT=$1; ROUNDS=$2; PARENT=$3
mkdir -p "$(dirname "$OUT")"
: > "$OUT"
for r in $(seq 1 "$ROUNDS"); do
  for tree in "$PARENT" . "$PARENT"; do
    timeout -k 10 150 python tools/time_encode_depth32.py --unchanged --tree "$tree" 2>&1 | grep '^AB ' | tee -a "$OUT" \
      || { echo "ab_encode_depth32.sh: $tree failed in round $r" | tee -a "$OUT"; exit 1; }
  done
done
