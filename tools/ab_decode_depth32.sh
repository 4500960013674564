#!/bin/bash
# The A/B of DESIGN.md section 4.28 on one GPU box: another build of this repository (its parent, built in PARENT_DIR)
# and this one alternately, one process each, then this one with the 16-bit and 32-bit mid/side batches:
#   tools/ab_decode_depth32.sh <out-file> <rounds> <PARENT_DIR>       (paths relative to the repo root)
# Every run has its own time limit and the first run that fails ends the script: nothing more is started on a GPU that
# has just faulted or hung.  The raw lines go to <out-file>; tools/time_decode_depth32.py says what they hold.
set -u -o pipefail
OUT=$1; ROUNDS=$2; PARENT=$3
mkdir -p "$(dirname "$OUT")"
: > "$OUT"
for r in $(seq 1 "$ROUNDS"); do
  for tree in "$PARENT" .; do
    timeout -k 10 150 python tools/time_decode_depth32.py --tree "$tree" 2>&1 | grep '^AB ' | tee -a "$OUT" \
      || { echo "ab_decode_depth32.sh: $tree failed in round $r" | tee -a "$OUT"; exit 1; }
  done
done
timeout -k 10 300 python tools/time_decode_depth32.py --deep --reps 7 --out "${OUT%.*}_deep.json" 2>&1 | grep '^AB ' | tee -a "$OUT" \
  || { echo "ab_decode_depth32.sh: the deep run failed" | tee -a "$OUT"; exit 1; }
