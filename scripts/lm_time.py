"""Times a Levenberg-Marquardt trial against a plain Gauss-Newton iteration: the same graph, the same starting estimates (a fresh
handle per run, one plain iteration to warm it), `its` iterations of gs_optimize and `its` iterations of gs_optimize_lm with default parameters — a run without
rejections (asserted), so trials == iterations.  Time = gs_stats.ms_total: HIP events on the handle's stream around the whole
call, divided by the iterations; the median of the interleaved rounds.  Both calls carry their host round trips between chunks
(gs_optimize: 1 + 9 iterations; gs_optimize_lm: chunks of up to 8 trials) and gs_optimize its closing chi2 pass, so the difference
is what a caller pays per iteration, not a kernel sum; the split into damp / scale / chi2 / step comes from a kernel trace of its own
(--trace-run: one gs_optimize_lm call and nothing else to time, for `rocprofv3 --kernel-trace --stats -- python scripts/lm_time.py --trace-run ...`).

Sizes: the reference's lap (240 poses / 200 cones), cfg3 (10k / 2k), cfg4 (100k / 10k).
The JSON lines go to stdout and to --out (default profiles/lm_time.jsonl, rewritten by every run); --table prints the DESIGN section 14
table from that file and, for the split columns, from the kernel statistics of the trace runs (--stats SIZE=FILE ..., the
*_kernel_stats.csv rocprofv3 writes; the committed ones: profiles/lm_kernel_stats_<size>.csv) — no GPU needed for --table.
Usage: python scripts/lm_time.py [--its 10] [--rounds 5] [--sizes 240x200,10000x2000,100000x10000] [--out FILE] [--trace-run]
       python scripts/lm_time.py --table [--out FILE] [--stats 240x200=profiles/lm_kernel_stats_240x200.csv ...]"""
import argparse
import importlib
import json
import os
import sys

import csv

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
NAMES = {(240, 200): "lap 240 / 200", (10000, 2000): "cfg3 10k / 2k", (100000, 10000): "cfg4 100k / 10k"}


def kernel_means(path):
    """kernel name (without arguments) -> mean duration in us, from a rocprofv3 kernel statistics file"""
    out = {}
    for r in csv.DictReader(open(path)):
        out[r["Name"].split("(")[0].replace("void ", "").replace("gs::", "")] = float(r["AverageNs"]) / 1e3
    return out


def table(out, stats):
    print("| graph | GN iteration | LM trial | difference | damp | scale | chi2 pass (gather + reduce) | step | kernel sum |")
    print("|---|---|---|---|---|---|---|---|---|")
    for line in open(out):
        r = json.loads(line); size = "%dx%d" % (r["N"], r["M"])
        row = "| %s | %.1f | %.1f | %.1f |" % (NAMES.get((r["N"], r["M"]), size), r["us_per_gn_iteration"], r["us_per_lm_trial"], r["us_difference"])
        if size in stats:
            k = kernel_means(stats[size])
            d, s, st, red = k["k_lm_damp"], k["k_lm_scale"], k["k_lm_step"], k["k_reduce_chi2"]
            ga = [v for n, v in k.items() if n.startswith("k_linearize_pose_gather<false")][0]
            row += " %.1f | %.1f | %.1f + %.1f | %.1f | %.1f |" % (d, s, ga, red, st, d + s + ga + red + st)
        else:
            row += " | | | | |"
        print(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--its", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="240x200,10000x2000,100000x10000")
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lm_time.jsonl"))
    ap.add_argument("--table", action="store_true")
    ap.add_argument("--stats", nargs="*", default=[])
    a = ap.parse_args()
    if a.table:
        table(a.out, dict(v.split("=", 1) for v in a.stats))
        return
    pkg = importlib.import_module("opendlv-logic-cfsd18-sensation-slam_amd")
    lines = []
    for size in a.sizes.split(","):
        N, M = (int(v) for v in size.split("x"))
        t = pkg.track.generate(N, M)
        fe = pkg.Graph(device=0)
        g = pkg.track.bench_graph(t, fe); fe.close()

        def handle():
            G = pkg.Graph(device=0); G.load_bench_graph(g); return G
        if a.trace_run:
            G = handle(); G.optimize_lm(a.its); G.close()
            continue
        runs = {"gn": [], "lm": []}
        rejected = 0
        for r in range(a.rounds + 1):                                 # interleaved; round 0 warms both paths (structure phase, first launches) and is dropped
            for which in ("gn", "lm"):
                G = handle(); G.optimize(1)                         # a handle of its own per run (the same start, bit for bit), warmed by one plain iteration
                if which == "gn":
                    done, st = G.optimize(a.its)
                else:
                    done, st, info = G.optimize_lm(a.its); rejected += info["rejected"]
                assert done == a.its
                if r > 0:
                    runs[which].append(1e3 * st.ms_total / a.its)
                G.close()
        assert rejected == 0
        gn, lm = float(np.median(runs["gn"])), float(np.median(runs["lm"]))
        lines.append(json.dumps(dict(N=N, M=M, iterations=a.its, rounds=a.rounds, us_per_gn_iteration=gn, us_per_lm_trial=lm, us_difference=lm - gn,
                                     gn_runs=runs["gn"], lm_runs=runs["lm"])))
        print(lines[-1], flush=True)
    if lines:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
