#!/bin/bash
# DESIGN.md section 6.26, "sessions without normals lose nothing": `python bench.py` (C2) and `python bench.py --config c4 --flags
# compact,bvh` of the parent commit and of this one, alternating, three runs each on one box; profiles/environment/bench_ab.py
# (section 6.16's rule) folds each set of six lines, and the two results go into one bench_ab.json.  Every run under its own time
# limit; the first one that fails ends the script.
#   profiles/smooth/bench_ab.sh PARENT_TREE [OUT_DIR]      PARENT_TREE: a built checkout of the parent commit
set -o pipefail
PARENT=${1:?a built checkout of the parent commit}
PARENT=$(cd "$PARENT" && pwd)
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
OUT=${2:-$ROOT/profiles/smooth}
mkdir -p "$OUT/c2" "$OUT/c4"
OUT=$(cd "$OUT" && pwd)
for i in 1 2 3; do
  (cd "$PARENT" && timeout -k 10 200 python bench.py --gpus 1 --steps 20 --warmup 5 | tail -1 > "$OUT/c2/bench_parent_$i.json") || exit 1
  (cd "$ROOT" && timeout -k 10 200 python bench.py --gpus 1 --steps 20 --warmup 5 | tail -1 > "$OUT/c2/bench_new_$i.json") || exit 1
done
for i in 1 2 3; do
  (cd "$PARENT" && timeout -k 10 200 python bench.py --gpus 1 --steps 20 --warmup 5 --config c4 --flags compact,bvh | tail -1 > "$OUT/c4/bench_parent_$i.json") || exit 1
  (cd "$ROOT" && timeout -k 10 200 python bench.py --gpus 1 --steps 20 --warmup 5 --config c4 --flags compact,bvh | tail -1 > "$OUT/c4/bench_new_$i.json") || exit 1
done
python "$ROOT/profiles/environment/bench_ab.py" "$OUT/c2" > /dev/null; c2=$?
python "$ROOT/profiles/environment/bench_ab.py" "$OUT/c4" > /dev/null; c4=$?
python - "$OUT" <<'EOF'
import json, os, sys
d = sys.argv[1]
out = {"c2": json.load(open(os.path.join(d, "c2", "bench_ab.json"))), "c4 compact,bvh": json.load(open(os.path.join(d, "c4", "bench_ab.json")))}
out["c4 compact,bvh"]["cmd"] += " --config c4 --flags compact,bvh"
out["accepted"] = all(v["accepted"] for v in out.values())
json.dump(out, open(os.path.join(d, "bench_ab.json"), "w"), indent=1)
print(json.dumps({k: (v if k == "accepted" else {f: v[f] for f in ("parent", "new", "new_over_parent", "rule", "accepted")}) for k, v in out.items()}, indent=1))
EOF
[ $c2 -eq 0 ] && [ $c4 -eq 0 ]
