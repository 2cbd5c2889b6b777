#!/bin/bash
# DESIGN.md section 6.22, "cost to sessions without the flag": `python bench.py` (C2) of the parent commit and of this one,
# alternating, three runs each on one box; then profiles/environment/bench_ab.py (section 6.16's rule, the same one) folds the
# six lines into bench_ab.json.  Every run under its own time limit; the first one that fails ends the script.
#   profiles/bump/bench_ab.sh PARENT_TREE [OUT_DIR]      PARENT_TREE: a built checkout of the parent commit
set -o pipefail
PARENT=${1:?a built checkout of the parent commit}
PARENT=$(cd "$PARENT" && pwd)
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
OUT=${2:-$ROOT/profiles/bump}
mkdir -p "$OUT"
OUT=$(cd "$OUT" && pwd)
for i in 1 2 3; do
  (cd "$PARENT" && timeout -k 10 300 python bench.py --gpus 1 --steps 20 --warmup 5 | tail -1 > "$OUT/bench_parent_$i.json") || exit 1
  (cd "$ROOT" && timeout -k 10 300 python bench.py --gpus 1 --steps 20 --warmup 5 | tail -1 > "$OUT/bench_new_$i.json") || exit 1
done
python "$ROOT/profiles/environment/bench_ab.py" "$OUT"
