#!/bin/bash
# DESIGN.md section 6.21, the headline: the plain `python bench.py --gpus 1 --steps 20 --warmup 5` (C2) of a built checkout of
# the parent commit and of this tree, alternating, three runs each on one box; then C3 and C5 once each, alternating;
# bench_ab.py folds the lines into bench_ab.json.  Every run under its own time limit; the first one that fails ends the script.
#   profiles/first_hit/bench_ab.sh PARENT_TREE [OUT_DIR]      PARENT_TREE: a built checkout of the parent commit
set -o pipefail
PARENT=${1:?a built checkout of the parent commit}
PARENT=$(cd "$PARENT" && pwd)
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
OUT=${2:-$ROOT/profiles/first_hit}
mkdir -p "$OUT"
OUT=$(cd "$OUT" && pwd)
for i in 1 2 3; do
  (cd "$PARENT" && timeout -k 10 300 python bench.py --gpus 1 --steps 20 --warmup 5 | tail -1 > "$OUT/bench_parent_$i.json") || exit 1
  (cd "$ROOT" && timeout -k 10 300 python bench.py --gpus 1 --steps 20 --warmup 5 | tail -1 > "$OUT/bench_new_$i.json") || exit 1
done
for c in c3 c5; do
  (cd "$PARENT" && timeout -k 10 300 python bench.py --gpus 1 --steps 20 --warmup 5 --config $c --no-cpu-baseline --no-per-call | tail -1 > "$OUT/bench_parent_$c.json") || exit 1
  (cd "$ROOT" && timeout -k 10 300 python bench.py --gpus 1 --steps 20 --warmup 5 --config $c --no-cpu-baseline --no-per-call | tail -1 > "$OUT/bench_new_$c.json") || exit 1
done
python "$ROOT/profiles/first_hit/bench_ab.py" "$OUT"
