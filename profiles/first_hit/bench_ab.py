"""Folds the bench.py lines of profiles/first_hit/bench_ab.sh into bench_ab.json.  The headline is accepted when every run of
this tree is above every run of the parent (the gain exceeds the spread, the two sets do not overlap); config.per_call, which
runs the one-launch plan this change does not touch, has to stay inside the parent's own min-max spread (DESIGN.md section
6.16's rule).  C3 and C5 are recorded, one run each.
    python profiles/first_hit/bench_ab.py DIR"""
import json
import os
import statistics
import sys


def per_call(line):
    pc = line.get("config", {}).get("per_call")
    return pc.get("mrays_per_s") if isinstance(pc, dict) else None


def main(d):
    load = lambda name: json.load(open(os.path.join(d, name)))
    runs = {who: [load("bench_%s_%d.json" % (who, i)) for i in (1, 2, 3)] for who in ("parent", "new")}
    pv = [r["value"] for r in runs["parent"]]
    nv = [r["value"] for r in runs["new"]]
    pm, nm = statistics.median(pv), statistics.median(nv)
    ppc = [per_call(r) for r in runs["parent"]]
    npc = [per_call(r) for r in runs["new"]]
    pc_ok = None
    if all(v is not None for v in ppc + npc):
        pc_ok = bool(statistics.median(npc) >= min(ppc))
    out = {"cmd": "python bench.py --gpus 1 --steps 20 --warmup 5", "unit": runs["new"][0].get("unit"), "order": "parent, new, alternating",
           "parent": pv, "new": nv, "parent_median": pm, "new_median": nm, "new_over_parent": nm / pm,
           "parent_spread": (max(pv) - min(pv)) / pm, "margin_over_parent_max": (min(nv) - max(pv)) / pm,
           "rule": "every run of this tree above every run of the parent", "accepted": bool(min(nv) > max(pv)),
           "ms_per_step": {"parent": [r["ms_per_step"] for r in runs["parent"]], "new": [r["ms_per_step"] for r in runs["new"]]},
           "rays_per_step_equal": len({r["config"].get("rays_per_step") for r in runs["parent"] + runs["new"]}) == 1,
           "per_call_mrays_per_s": {"parent": ppc, "new": npc, "rule": "this tree's median not below the parent's minimum", "accepted": pc_ok}}
    for c in ("c3", "c5"):
        try:
            p, n = load("bench_parent_%s.json" % c), load("bench_new_%s.json" % c)
            out[c] = {"parent": p["value"], "new": n["value"], "new_over_parent": n["value"] / p["value"],
                      "ms_per_step": [p["ms_per_step"], n["ms_per_step"]], "workload": n["config"].get("workload")}
        except OSError:
            pass
    with open(os.path.join(d, "bench_ab.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))
    return 0 if out["accepted"] else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
