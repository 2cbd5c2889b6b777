"""Folds the six bench.py lines of profiles/environment/bench_ab.sh into bench_ab.json and applies DESIGN.md section 6.16's rule:
this commit's median lies inside the parent's own min-max spread -- or, when the parent's three runs agree to better than 1 %,
within 1 % of the parent's median.
    python profiles/environment/bench_ab.py DIR"""
import json
import os
import statistics
import sys


def sustained_ghz(line):
    """the box's sustained shader clock as bench.py's line reports it (any object that carries `ghz`), or None"""
    found = []

    def walk(o):
        if isinstance(o, dict):
            for k, v in o.items():
                if k in ("shader_clock_ghz", "measured_clock_ghz") and isinstance(v, (int, float)):
                    found.append(float(v))
                walk(v)
        elif isinstance(o, list):
            for v in o:
                walk(v)
    walk(line)
    return found[0] if found else None


def main(d):
    runs = {}
    for who in ("parent", "new"):
        runs[who] = [json.load(open(os.path.join(d, "bench_%s_%d.json" % (who, i)))) for i in (1, 2, 3)]
    pv = [r["value"] for r in runs["parent"]]
    nv = [r["value"] for r in runs["new"]]
    pm, nm = statistics.median(pv), statistics.median(nv)
    tight = (max(pv) - min(pv)) / pm < 0.01
    ok = nm >= pm * 0.99 if tight else nm >= min(pv)
    out = {"cmd": "python bench.py --gpus 1 --steps 20 --warmup 5", "unit": runs["new"][0].get("unit"), "order": "parent, new, alternating",
           "parent": pv, "new": nv, "parent_median": pm, "new_median": nm, "new_over_parent": nm / pm,
           "parent_spread": (max(pv) - min(pv)) / pm, "rule": "within 1 % of the parent's median" if tight else "inside the parent's min-max spread",
           "accepted": bool(ok), "sustained_ghz": {"parent": [sustained_ghz(r) for r in runs["parent"]], "new": [sustained_ghz(r) for r in runs["new"]]}}
    with open(os.path.join(d, "bench_ab.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
