"""Folds the bench.py lines of profiles/first_two/bench_ab.sh into bench_ab.json.  Compared on ms_per_step: the headline is
accepted when every run of this tree is faster than every run of the parent AND the margin over the parent's fastest run is
larger than the parent's own min-max spread; rays_per_step must be identical and both trees must dump the same image.npy.
config.per_call (the one-launch plan, untouched) is reported against the parent's spread.  C3 and C5: one run each.
    python profiles/first_two/bench_ab.py RAW_DIR OUT.json"""
import hashlib
import json
import os
import statistics
import sys


def per_call(line):
    pc = line.get("config", {}).get("per_call")
    return pc.get("mrays_per_s") if isinstance(pc, dict) else None


def md5_of(path):
    try:
        return hashlib.md5(open(path, "rb").read()).hexdigest()
    except OSError:
        return None


def main(d, dest):
    load = lambda name: json.load(open(os.path.join(d, name)))
    runs = {who: [load("bench_%s_%d.json" % (who, i)) for i in (1, 2, 3)] for who in ("parent", "new")}
    pm = [r["ms_per_step"] for r in runs["parent"]]
    nm = [r["ms_per_step"] for r in runs["new"]]
    spread = max(pm) - min(pm)
    margin = min(pm) - max(nm)
    ppc = [per_call(r) for r in runs["parent"]]
    npc = [per_call(r) for r in runs["new"]]
    img = {who: md5_of(os.path.join(d, "out_%s" % who, "image.npy")) for who in ("parent", "new")}
    out = {"cmd": "python bench.py --gpus 1 --steps 20 --warmup 5", "order": "parent, new, alternating",
           "ms_per_step": {"parent": pm, "new": nm}, "parent_median": statistics.median(pm), "new_median": statistics.median(nm),
           "new_over_parent": statistics.median(nm) / statistics.median(pm),
           "parent_spread_ms": spread, "margin_over_parent_fastest_ms": margin,
           "rule": "every run of this tree faster than every run of the parent, by more than the parent's own spread",
           "accepted": bool(margin > 0 and margin > spread),
           "value_mrays_per_s": {"parent": [r["value"] for r in runs["parent"]], "new": [r["value"] for r in runs["new"]]},
           "rays_per_step_equal": len({r["config"].get("rays_per_step") for r in runs["parent"] + runs["new"]}) == 1,
           "image_npy_md5": img, "image_equal": bool(img["parent"] is not None and img["parent"] == img["new"]),
           "per_call_mrays_per_s": {"parent": ppc, "new": npc}}
    try:
        out["image_md5"] = {who: load("digest_%s.json" % who).get("image_md5") for who in ("parent", "new")}
    except OSError:
        pass
    for c in ("c3", "c5"):
        try:
            p, n = load("bench_parent_%s.json" % c), load("bench_new_%s.json" % c)
            out[c] = {"ms_per_step": [p["ms_per_step"], n["ms_per_step"]], "new_over_parent": n["ms_per_step"] / p["ms_per_step"],
                      "value_mrays_per_s": [p["value"], n["value"]], "workload": n["config"].get("workload")}
        except OSError:
            pass
    with open(dest, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))
    return 0 if out["accepted"] and out["rays_per_step_equal"] and out["image_equal"] else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
