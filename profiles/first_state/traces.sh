#!/bin/bash
# DESIGN.md section 6.25, the kernel traces: rocprofv3 --kernel-trace --stats of bench.py (C2), serial (PTMI355_OVERLAP=0: one
# call at a time, a launch's time is its own), with the parent commit's library and with this tree's, folded by trace_summary.py.
# Every run under its own time limit; the first one that fails ends the script.
#   profiles/first_state/traces.sh PARENT_LIB [OUT_DIR]      PARENT_LIB: libptmi355.so built from the parent commit
set -o pipefail
PARENT_LIB=$(readlink -f "${1:?libptmi355.so of the parent commit}")
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
OUT=${2:-$ROOT/profiles/first_state}
mkdir -p "$OUT"; OUT=$(cd "$OUT" && pwd)
TMP=$(mktemp -d)
ARGS="--no-roofline --no-per-call --no-cpu-baseline --no-sustained"
run() {   # name, library ("" = this tree's)
  ( cd "$ROOT" && if [ -n "$2" ]; then export PTMI355_LIB=$2; fi; export PTMI355_OVERLAP=0
    timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$TMP/$1" -o t -- python bench.py $ARGS > "$TMP/$1.log" 2>&1 ) || { tail -5 "$TMP/$1.log"; return 1; }
  python "$ROOT/profiles/first_state/trace_summary.py" "$(find "$TMP/$1" -name 't_kernel_trace.csv' | head -1)" > "$OUT/trace_$1.txt"
}
run before_parent_serial "$PARENT_LIB" || exit 1
run after_serial "" || exit 1
rm -rf "$TMP"
