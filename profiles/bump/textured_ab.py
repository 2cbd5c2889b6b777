"""Folds the six lines of profiles/bump/textured_ab.sh into textured_ab.json and applies DESIGN.md section 6.16's rule to the time
per step (smaller is better): this tree's median is no worse than the parent's slowest run -- or, when the parent's three runs agree
to better than 1 %, within 1 % of the parent's median.
    python profiles/bump/textured_ab.py DIR"""
import json
import os
import statistics
import sys


def main(d):
    runs = {who: [json.load(open(os.path.join(d, "textured_%s_%d.json" % (who, i)))) for i in (1, 2, 3)] for who in ("parent", "new")}
    pv = [r["ms_per_step"] for r in runs["parent"]]
    nv = [r["ms_per_step"] for r in runs["new"]]
    pm, nm = statistics.median(pv), statistics.median(nv)
    tight = (max(pv) - min(pv)) / pm < 0.01
    ok = nm <= pm * 1.01 if tight else nm <= max(pv)
    same_image = len({r["mean_of_image"] for r in runs["parent"] + runs["new"]}) == 1
    out = {"cmd": "python profiles/bump/measure.py textured TREE", "unit": "ms per step of 64 iterations, 800x800 cornell_textured, PT_TEXTURES, three textures, no bump map",
           "order": "parent, new, alternating", "parent": pv, "new": nv, "parent_median": pm, "new_median": nm, "new_over_parent": nm / pm,
           "parent_spread": (max(pv) - min(pv)) / pm, "rule": "within 1 % of the parent's median" if tight else "no slower than the parent's slowest run",
           "accepted": bool(ok), "same_image": same_image}
    with open(os.path.join(d, "textured_ab.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
