#!/bin/bash
# DESIGN.md section 6.20, "no cost when off": profiles/denoise/measure.py of the parent commit and of this one, alternating,
# three runs each on one box (the switched-off five-level times must lie within the parent's own spread), then `python bench.py`
# (C2) the same way, folded by profiles/environment/bench_ab.py (section 6.16's rule).  Every run under its own time limit; the
# first one that fails ends the script.
#   profiles/denoise/ab_switch_off.sh PARENT_TREE OUT_DIR      PARENT_TREE: a built checkout of the parent commit
set -o pipefail
PARENT=${1:?a built checkout of the parent commit}
PARENT=$(cd "$PARENT" && pwd)
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
OUT=${2:?a directory for the runs}
mkdir -p "$OUT"
OUT=$(cd "$OUT" && pwd)
for i in 1 2 3; do
  (cd "$PARENT" && timeout -k 10 200 python profiles/denoise/measure.py --out "$OUT/denoise_parent_$i.json" > /dev/null) || exit 1
  (cd "$ROOT" && timeout -k 10 200 python profiles/denoise/measure.py --out "$OUT/denoise_new_$i.json" > /dev/null) || exit 1
done
python - "$OUT" <<'PY' || exit 1
import json, sys
out = sys.argv[1]
res = {}
for who in ("parent", "new"):
    runs = [json.load(open("%s/denoise_%s_%d.json" % (out, who, i))) for i in (1, 2, 3)]
    for k, name in enumerate(("800x800", "3840x2160")):
        res.setdefault(name, {})[who + "_five_levels_ms"] = [r["frames"][k]["filter_ms_sum_of_medians"] for r in runs]
        res[name][who + "_k_gbuffer_ms"] = [r["frames"][k]["k_gbuffer_ms"]["median"] for r in runs]
for name, r in res.items():
    p, n = r["parent_five_levels_ms"], r["new_five_levels_ms"]
    r["parent_spread_ms"] = max(p) - min(p)
    r["new_within_parent_range"] = min(p) <= sorted(n)[1] <= max(p)
json.dump(res, open(out + "/ab_switch_off.json", "w"), indent=1)
print(json.dumps(res))
PY
for i in 1 2 3; do
  (cd "$PARENT" && timeout -k 10 300 python bench.py --gpus 1 --steps 20 --warmup 5 | tail -1 > "$OUT/bench_parent_$i.json") || exit 1
  (cd "$ROOT" && timeout -k 10 300 python bench.py --gpus 1 --steps 20 --warmup 5 | tail -1 > "$OUT/bench_new_$i.json") || exit 1
done
python "$ROOT/profiles/environment/bench_ab.py" "$OUT"
