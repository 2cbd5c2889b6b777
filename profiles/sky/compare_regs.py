"""Compare two builds' -Rpass-analysis=kernel-resource-usage remarks, kernel by kernel:
    hipcc <the flags of build.py> -Rpass-analysis=kernel-resource-usage ... csrc/ptmi355.hip 2> before.log   (the parent commit)
    hipcc ...                                                                                 2> after.log    (this commit)
    python profiles/sky/compare_regs.py before.log after.log > profiles/sky/kernel_regs.txt
Prints the kernels only one build has, every kernel whose SGPRs, VGPRs, scratch, occupancy or LDS differ, and a summary of the
k_bounce instantiations with and without SH_DIRECT (the last template argument's bit 2)."""
import re
import subprocess
import sys

FIELDS = ("TotalSGPRs", "VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")


def parse(path):
    out, name = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\S+) \[-Rpass", line)
        if m and name and m.group(1) in FIELDS:
            out[name][m.group(1)] = m.group(2)
    return out


def is_direct(name):
    """A k_bounce instantiation whose last template argument (SH) has bit 2 (SH_DIRECT)."""
    m = re.search(r"k_bounceILi\d+ELb[01]ELi\d+ELb[01]ELb[01]ELb[01]ELb[01]ELi(\d+)E", name)
    return bool(m) and (int(m.group(1)) & 4) != 0


def demangle(names):
    try:
        p = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, p.stdout.split("\n")))
    except Exception:
        return {n: n for n in names}


def main():
    before, after = parse(sys.argv[1]), parse(sys.argv[2])
    print("%d kernels before, %d after" % (len(before), len(after)))
    gone, new = sorted(set(before) - set(after)), sorted(set(after) - set(before))
    names = demangle(gone + new + [n for n in before if n in after and before[n] != after[n]])
    for n in gone:
        print("only before: %s" % names[n])
    for n in new:
        print("only after:  %s %s" % (names[n], " / ".join(after[n].get(f, "?") for f in FIELDS)))
    same = {True: 0, False: 0}
    changed = {True: [], False: []}
    for n in before:
        if n not in after:
            continue
        d = is_direct(n)
        if before[n] == after[n]:
            same[d] += 1
        else:
            changed[d].append(n)
    print("without SH_DIRECT: %d kernels keep SGPRs / VGPRs / scratch / occupancy / LDS, %d change" % (same[False], len(changed[False])))
    for n in changed[False]:
        print("  CHANGED %s: %s -> %s" % (names[n], " / ".join(before[n].get(f, "?") for f in FIELDS), " / ".join(after[n].get(f, "?") for f in FIELDS)))
    print("k_bounce with SH_DIRECT: %d unchanged, %d change (SGPRs / VGPRs / scratch bytes per lane / waves per SIMD / LDS)" % (same[True], len(changed[True])))
    for n in changed[True]:
        print("  %s: %s -> %s" % (names[n], " / ".join(before[n].get(f, "?") for f in FIELDS), " / ".join(after[n].get(f, "?") for f in FIELDS)))


if __name__ == "__main__":
    main()
