#!/bin/bash
# DESIGN.md section 6.25, the headline: the plain `python bench.py --gpus 1 --steps 20 --warmup 5` (C2) with the parent commit's
# library (through PTMI355_LIB: the Python side and bench.py are the same in both trees) and with this tree's, alternating, five
# runs each on one box; the image of both (--digest --dump-outputs) for C2, C3 and C5; C3 and C5 timed once each, alternating;
# bench_ab.py folds the lines into bench_ab.json.  Every run under its own time limit; the first one that fails ends the script.
#   profiles/first_state/bench_ab.sh PARENT_LIB [OUT_DIR]      PARENT_LIB: libptmi355.so built from the parent commit
set -o pipefail
PARENT_LIB=$(readlink -f "${1:?libptmi355.so of the parent commit}")
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
OUT=${2:-$ROOT/profiles/first_state}
mkdir -p "$OUT"; OUT=$(cd "$OUT" && pwd)
RAW=$OUT/raw; mkdir -p "$RAW"
cd "$ROOT"
for i in 1 2 3 4 5; do
  PTMI355_LIB=$PARENT_LIB timeout -k 10 300 python bench.py --gpus 1 --steps 20 --warmup 5 | tail -1 > "$RAW/bench_parent_$i.json" || exit 1
  timeout -k 10 300 python bench.py --gpus 1 --steps 20 --warmup 5 | tail -1 > "$RAW/bench_new_$i.json" || exit 1
done
QUIET="--no-cpu-baseline --no-per-call --no-roofline"
for c in c2 c3 c5; do
  PTMI355_LIB=$PARENT_LIB timeout -k 10 300 python bench.py --gpus 1 --steps 20 --warmup 5 --config $c --digest --dump-outputs "$RAW/out_parent_$c" $QUIET | tail -1 > "$RAW/digest_parent_$c.json" || exit 1
  timeout -k 10 300 python bench.py --gpus 1 --steps 20 --warmup 5 --config $c --digest --dump-outputs "$RAW/out_new_$c" $QUIET | tail -1 > "$RAW/digest_new_$c.json" || exit 1
done
python "$ROOT/profiles/first_state/bench_ab.py" "$RAW" "$OUT/bench_ab.json"
