"""Times Gauss-Newton iterations by phase (gs_time_iterations: HIP events on the handle's stream, estimates restored afterwards) with
no robust kernel, Huber on the observation edges and Huber on both edge kinds — same handle, same estimates, the setting changed
between the measurements (it costs no structure phase).  delta per kind = the median of sqrt(s) of that kind at those estimates
(gs_get_edge_chi2), so that half of the edges take the sqrt + divide branch.  Sizes: the reference's lap (240 poses / 200 cones),
cfg3 (10k / 2k) and cfg4 (100k / 10k), each after two plain iterations; the median of the repeats of every phase.

What to look at: ms_linearize / ms_linearize_kernel — the model says zero extra bytes and a sqrt + divide per edge for the ROBUST
instance of k_linearize_ell; the other phases run the same kernels on different numbers.
Usage: python scripts/robust_time.py [--reps 20] [--rounds 5] [--sizes 240x200,10000x2000,100000x10000]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
pkg = importlib.import_module("opendlv-logic-cfsd18-sensation-slam_amd")

PHASES = ("ms_linearize", "ms_linearize_kernel", "ms_factor", "ms_backsolve", "ms_update", "ms_total")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="240x200,10000x2000,100000x10000")
    a = ap.parse_args()
    for size in a.sizes.split(","):
        N, M = (int(v) for v in size.split("x"))
        t = pkg.track.generate(N, M)
        fe = pkg.Graph(device=0)
        g = pkg.track.bench_graph(t, fe); fe.close()
        G = pkg.Graph(device=0); G.load_bench_graph(g); G.optimize(2)
        dpp = float(np.median(np.sqrt(G.edge_chi2("odometry")[0]))); dpl = float(np.median(np.sqrt(G.edge_chi2("observation")[0])))
        settings = {"none": (("none", 1.0), ("none", 1.0)), "huber-observation": (("none", 1.0), ("huber", dpl)),
                    "huber-both": (("huber", dpp), ("huber", dpl))}
        runs = {k: [] for k in settings}
        for _ in range(a.rounds):                                  # interleaved, so that drift of the box lands on all three alike
            for name, (kpp, kpl) in settings.items():
                G.set_robust_kernel("odometry", *kpp); G.set_robust_kernel("observation", *kpl)
                runs[name].append(G.time_iterations(a.reps).as_dict())
        for name, (kpp, kpl) in settings.items():
            G.set_robust_kernel("odometry", *kpp); G.set_robust_kernel("observation", *kpl)
            w = G.edge_chi2("observation")[1]
            med = {k: float(np.median([r[k] for r in runs[name]])) for k in PHASES}
            print(json.dumps(dict(N=N, M=M, kernels=name, delta_odometry=kpp[1], delta_observation=kpl[1],
                                  observation_edges_down_weighted=float((w < 1).mean()), reps=a.reps, rounds=a.rounds, **med)), flush=True)
        G.close()


if __name__ == "__main__":
    main()
