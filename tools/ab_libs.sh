#!/bin/bash
# Process-alternating A/B of whole libraries on the default training step (run on the GPU box from the repo root; works on the
# box's copy of the tree): tools/ab_libs.sh tools/libqst_base.so tools/libqst_x.so ...   -> ms per step per library and round
# ROUNDS (3), STEPS (50), WARMUP (10) from the environment; naming one library twice gives the spread within a build.
# Every run has its own time limit, and the first one that fails ends the script (the library in place is put back).
# A library that lacks an entry point this tree's bindings declare does not load here: measure such a build from a checkout of
# its own commit (profiles/r07_ab_wgrad_phase.txt, section 2, alternated the parent's tree with this one in the same way).
set -e
P=quadruplet-sentence-transformer_amd/libqst.so
ROUNDS=${ROUNDS:-3}; STEPS=${STEPS:-50}; WARMUP=${WARMUP:-10}
cp $P /tmp/libqst_keep.so
trap 'cp /tmp/libqst_keep.so $P' EXIT
set -o pipefail
for r in $(seq 1 $ROUNDS); do
  for L in "$@"; do
    cp $L $P
    timeout -k 10 240 python bench.py --no-extras --no-cpu-baseline --steps $STEPS --warmup $WARMUP 2>/dev/null | python -c "import sys,json; b=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('round $r', '$L', b['ms_per_step'], b['value'], flush=True)"
  done
done
