"""Per-build table of the plan steps gs_debug_options.plan_timing prints (stderr of a run, lines "plan <step> <ms> ms"): python scripts/plan_phase_table.py FILE
(records made before the steps had names hold "plan phase <number>: <ms> ms" lines, which the library no longer prints and this script no longer reads)"""
import re, sys
runs, cur = [], []
for line in open(sys.argv[1]):
    m = re.match(r"plan (.+?)\s+([\d.]+) ms$", line)
    if m:
        if m.group(1) == "index" and cur: runs.append(cur); cur = []
        cur.append((m.group(1).replace(" ", "_"), float(m.group(2))))
if cur: runs.append(cur)
for i, r in enumerate(runs): print("plan build %d:" % i, " ".join("%s=%.1f" % kv for kv in r), " total %.1f" % sum(v for _, v in r))
