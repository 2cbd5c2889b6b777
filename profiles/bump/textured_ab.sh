#!/bin/bash
# DESIGN.md section 6.22, "textured sessions with no bump map": profiles/bump/measure.py's textured step on a built checkout of the
# parent commit and on this tree, alternating, three runs each on one box; textured_ab.py folds the six lines into textured_ab.json
# (section 6.16's rule on ms per step).  Every run under its own time limit; the first one that fails ends the script.
#   profiles/bump/textured_ab.sh PARENT_TREE [OUT_DIR]
set -o pipefail
PARENT=${1:?a built checkout of the parent commit}
PARENT=$(cd "$PARENT" && pwd)
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
OUT=${2:-$ROOT/profiles/bump}
mkdir -p "$OUT"
OUT=$(cd "$OUT" && pwd)
for i in 1 2 3; do
  timeout -k 10 120 python "$ROOT/profiles/bump/measure.py" textured "$PARENT" | tail -1 > "$OUT/textured_parent_$i.json" || exit 1
  timeout -k 10 120 python "$ROOT/profiles/bump/measure.py" textured "$ROOT" | tail -1 > "$OUT/textured_new_$i.json" || exit 1
done
python "$ROOT/profiles/bump/textured_ab.py" "$OUT"
