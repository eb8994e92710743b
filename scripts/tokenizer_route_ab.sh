#!/bin/bash
# Same-box A/B of the headline step over the encoder's route switches (MUSE_POOL_FUSE, MUSE_CONV_IN_NCHW), profiler off, alternating:
#   scripts/tokenizer_route_ab.sh <out-file> [pairs, default 6] [parent-tree]
# One line per bench.py run.  With a parent tree (a built checkout of the parent commit) its bench.py runs first, in the middle and last.
# Every run under its own timeout; the first failing run ends the script.
set -o pipefail
R=$PWD; F=${1:?out file}; N=${2:-6}; P=$3; : > "$F"
run() {  # label dir env...
  local label=$1 dir=$2; shift 2
  ( cd "$dir" && env "$@" timeout -k 10 400 python bench.py --gpus 1 --steps 30 --warmup 5 2> /dev/null ) | grep '^{' | python -c "
import sys, json
d = json.loads(sys.stdin.readline())
print('%-12s %8.2f img/s  %7.3f ms/step' % ('$label', d['value'], d['ms_per_step']))" | tee -a "$F"
}
[ -z "$P" ] || run parent "$P" MUSE_AB=parent || exit 1
for i in $(seq 1 "$N"); do
  run new_off "$R" MUSE_POOL_FUSE=0 MUSE_CONV_IN_NCHW=0 && run new_on "$R" MUSE_POOL_FUSE=1 MUSE_CONV_IN_NCHW=1 || exit 1
  if [ -n "$P" ] && [ "$i" = $((N / 2)) ]; then run parent "$P" MUSE_AB=parent || exit 1; fi
done
[ -z "$P" ] || run parent "$P" MUSE_AB=parent
