"""DESIGN.md section 6.22, "resource usage of every kernel": fold two logs of
    hipcc <the library's flags> -Rpass-analysis=kernel-resource-usage ... csrc/ptmi355.hip 2> LOG
(the parent commit's and this tree's; cross-compiling is enough) into one row per kernel and hold the two conditions:
every kernel that is not an SH_TEX form of k_bounce keeps its SGPRs, VGPRs, AGPRs, scratch, spills, LDS and occupancy to the last
register, and no SH_TEX form loses a wave per SIMD.  Prints the SH_TEX rows of both trees side by side and writes the summary.
    python profiles/bump/kernel_regs.py PARENT_LOG NEW_LOG [OUT.json]     (default: profiles/bump/kernel_regs.json)"""
import json, os, re, sys

FIELDS = (("TotalSGPRs", "sgpr"), ("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("ScratchSize [bytes/lane]", "scratch"),
          ("Occupancy [waves/SIMD]", "waves"), ("SGPRs Spill", "sspill"), ("VGPRs Spill", "vspill"), ("LDS Size [bytes/block]", "lds"))


def parse(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        for label, key in FIELDS:
            m = re.search(r"remark:\s+" + re.escape(label) + r": (\d+)", line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return out


def is_tex(name):
    """k_bounce<MODE, COMPACT, MESH, SLDS, GEN, SORT, OWN, SH> with SH & SH_TEX (8): the last template argument, Li<SH>E"""
    m = re.search(r"8k_bounceILi\d+ELb\dELi\d+ELb\dELb\dELb\dELb\dELi(\d+)EEE", name)
    return bool(m) and (int(m.group(1)) & 8) != 0


def main():
    parent, new = parse(sys.argv[1]), parse(sys.argv[2])
    out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "kernel_regs.json")
    added = sorted(set(new) - set(parent))
    removed = sorted(set(parent) - set(new))
    changed = [k for k in sorted(set(new) & set(parent)) if not is_tex(k) and new[k] != parent[k]]
    tex = [k for k in sorted(new) if is_tex(k)]
    lost = [k for k in tex if k in parent and new[k]["waves"] < parent[k]["waves"]]
    print("# SH_TEX forms of k_bounce: parent | this tree   (vgpr sgpr scratch sspill vspill waves/SIMD)")
    for k in tex:
        a, b = parent.get(k), new[k]
        row = lambda r: "%3d %3d %4d %3d %3d %d" % (r["vgpr"], r["sgpr"], r["scratch"], r["sspill"], r["vspill"], r["waves"]) if r else "-"
        print("%s  %s | %s" % (re.search(r"8k_bounceI(\w+?)EEE", k).group(1), row(a), row(b)))
    summary = {"kernels_parent": len(parent), "kernels_new": len(new), "added": added, "removed": removed,
               "other_kernels_changed": changed, "tex_forms": len(tex), "tex_forms_that_lost_a_wave": lost,
               "tex_scratch_parent_max": max(parent[k]["scratch"] for k in tex if k in parent),
               "tex_scratch_new_max": max(new[k]["scratch"] for k in tex),
               "tex_forms_whose_scratch_grew": sum(1 for k in tex if k in parent and new[k]["scratch"] > parent[k]["scratch"]),
               "tex_rows": {k: {"parent": parent.get(k), "new": new[k]} for k in tex}}
    json.dump(summary, open(out, "w"), indent=1)
    print("kernels: %d -> %d; added %s; removed %s" % (len(parent), len(new), added, removed))
    print("kernels outside the SH_TEX forms whose resources changed: %d %s" % (len(changed), changed[:5]))
    print("SH_TEX forms: %d, that lost a wave per SIMD: %d" % (len(tex), len(lost)))
    return 1 if changed or lost or removed else 0


if __name__ == "__main__":
    sys.exit(main())
