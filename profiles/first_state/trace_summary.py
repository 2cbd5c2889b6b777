"""per-kernel and per-bounce launch times (us) of a rocprofv3 kernel trace csv -- profiles/first_two/trace_summary.py with the
first-state form counted as the launch of bounces 0 and 1 too (k_bounce<MODE_FIRST2 = 3, ...> or k_bounce<MODE_STATE2 = 4, ...>):
it is printed as "bounces 0+1" and the launch behind it counts as bounce 2.
    python profiles/first_state/trace_summary.py TRACE.csv"""
import csv
import re
import statistics as st
import sys
from collections import defaultdict

rows = list(csv.DictReader(open(sys.argv[1])))
by = defaultdict(list)
for r in rows:
    by[r["Kernel_Name"]].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
print("%8s %10s %10s %10s %10s  name" % ("calls", "median", "mean", "min", "max"))
for k, v in sorted(by.items(), key=lambda kv: -sum(kv[1])):
    print("%8d %10.1f %10.1f %10.1f %10.1f  %s" % (len(v), st.median(v), st.mean(v), min(v), max(v), k))
qkey = "Queue_Id" if "Queue_Id" in rows[0] else None
skey = "Stream_Id" if "Stream_Id" in rows[0] else qkey
per = defaultdict(list)
pos = {}
for r in sorted(rows, key=lambda r: int(r["Start_Timestamp"])):
    n = r["Kernel_Name"]
    if "k_bounce" not in n:
        continue
    m = re.search(r"k_bounce<([^>]*)>", n)
    args = [a.strip() for a in m.group(1).split(",")] if m else []
    mode = re.sub(r"\(.*?\)", "", args[0]) if args else ""
    first = len(args) >= 5 and (args[4] in ("true", "1") or mode == "2")
    two = first and mode in ("3", "4")
    s = r.get(skey, "0")
    us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    if two:
        per["0+1"].append(us)
        pos[s] = 1
        continue
    pos[s] = 0 if first else pos.get(s, 0) + 1
    per[pos[s]].append(us)
print("\nk_bounce by position in the batch (per %s)" % skey)
for p in sorted(per, key=lambda p: (0.5 if p == "0+1" else p)):
    v = per[p]
    print("bounce%s %s: calls %d median %.1f mean %.1f min %.1f max %.1f" % ("s" if p == "0+1" else "", p, len(v), st.median(v), st.mean(v), min(v), max(v)))
