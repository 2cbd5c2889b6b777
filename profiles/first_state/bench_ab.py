"""Folds the bench.py lines of profiles/first_state/bench_ab.sh into bench_ab.json.  Compared on ms_per_step: the change counts
as a gain only when every run of this tree is faster than the parent's fastest run; the margin is stated as a multiple of the
parent's own min-max spread.  rays_per_step must be identical, and for C2, C3 and C5 both trees must dump the same image.npy.
C3 and C5: the one timed pair each is the pair of digest runs.
    python profiles/first_state/bench_ab.py RAW_DIR OUT.json"""
import glob
import hashlib
import json
import os
import statistics
import sys


def md5_of(path):
    try:
        return hashlib.md5(open(path, "rb").read()).hexdigest()
    except OSError:
        return None


def main(d, dest):
    load = lambda name: json.load(open(os.path.join(d, name)))
    count = len(glob.glob(os.path.join(d, "bench_parent_[0-9]*.json")))
    runs = {who: [load("bench_%s_%d.json" % (who, i)) for i in range(1, count + 1)] for who in ("parent", "new")}
    pm = [r["ms_per_step"] for r in runs["parent"]]
    nm = [r["ms_per_step"] for r in runs["new"]]
    spread = max(pm) - min(pm)
    margin = min(pm) - max(nm)
    out = {"cmd": "python bench.py --gpus 1 --steps 20 --warmup 5", "order": "parent, new, alternating",
           "ms_per_step": {"parent": pm, "new": nm}, "parent_median": statistics.median(pm), "new_median": statistics.median(nm),
           "new_over_parent": statistics.median(nm) / statistics.median(pm),
           "parent_spread_ms": spread, "parent_spread_share": spread / statistics.median(pm),
           "margin_over_parent_fastest_ms": margin, "margin_in_parent_spreads": (margin / spread) if spread > 0 else None,
           "rule": "a gain only if every run of this tree is faster than the parent's fastest run",
           "gain": bool(margin > 0),
           "value_mrays_per_s": {"parent": [r["value"] for r in runs["parent"]], "new": [r["value"] for r in runs["new"]]},
           "rays_per_step_equal": len({r["config"].get("rays_per_step") for r in runs["parent"] + runs["new"]}) == 1}
    same = True
    for c in ("c2", "c3", "c5"):
        try:
            p, n = load("digest_parent_%s.json" % c), load("digest_new_%s.json" % c)
        except OSError:
            continue
        # (a frame past bench.py's dump limit -- C5 -- is dumped as a fixed sample of its pixels: image_sample.npy; image_md5
        # covers the whole frame either way)
        img = {who: md5_of(os.path.join(d, "out_%s_%s" % (who, c), "image.npy")) or md5_of(os.path.join(d, "out_%s_%s" % (who, c), "image_sample.npy"))
               for who in ("parent", "new")}
        out[c] = {"ms_per_step": [p["ms_per_step"], n["ms_per_step"]], "new_over_parent": n["ms_per_step"] / p["ms_per_step"],
                  "image_md5": [p.get("image_md5"), n.get("image_md5")], "image_npy_md5": img,
                  "image_equal": bool(img["parent"] is not None and img["parent"] == img["new"] and p.get("image_md5") == n.get("image_md5")),
                  "rays_per_step": [p["config"].get("rays_per_step"), n["config"].get("rays_per_step")],
                  "workload": n["config"].get("workload")}
        same = same and out[c]["image_equal"] and out[c]["rays_per_step"][0] == out[c]["rays_per_step"][1]
    out["results_unchanged"] = bool(same and out["rays_per_step_equal"])
    with open(dest, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))
    return 0 if out["results_unchanged"] else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
