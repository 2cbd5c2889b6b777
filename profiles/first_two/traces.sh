#!/bin/bash
# DESIGN.md section 6.23, the kernel traces: rocprofv3 --kernel-trace --stats of bench.py (C2) with the parent commit's library
# and with this tree's, serial (PTMI355_OVERLAP=0) and overlapped, folded by trace_summary.py.  Every run under its own time
# limit; the first one that fails ends the script.
#   profiles/first_two/traces.sh PARENT_LIB [OUT_DIR]      PARENT_LIB: libptmi355.so built from the parent commit
set -o pipefail
PARENT_LIB=$(readlink -f "${1:?libptmi355.so of the parent commit}")
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
OUT=${2:-$ROOT/profiles/first_two}
mkdir -p "$OUT"; OUT=$(cd "$OUT" && pwd)
TMP=$(mktemp -d)
ARGS="--no-roofline --no-per-call --no-cpu-baseline --no-sustained"
run() {   # name, overlap, library ("" = this tree's)
  ( cd "$ROOT" && if [ -n "$3" ]; then export PTMI355_LIB=$3; fi; if [ "$2" = 0 ]; then export PTMI355_OVERLAP=0; fi
    timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$TMP/$1" -o t -- python bench.py $ARGS > "$TMP/$1.log" 2>&1 ) || { tail -5 "$TMP/$1.log"; return 1; }
  python "$ROOT/profiles/first_two/trace_summary.py" "$(find "$TMP/$1" -name 't_kernel_trace.csv' | head -1)" > "$OUT/trace_$1.txt"
}
run before_parent_serial 0 "$PARENT_LIB" || exit 1
run after_serial 0 "" || exit 1
run before_parent_overlapped 1 "$PARENT_LIB" || exit 1
run after_overlapped 1 "" || exit 1
rm -rf "$TMP"
