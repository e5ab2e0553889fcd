"""Times gs_compute_marginals by phase (HIP events on the handle's stream): linearise + factor (the iteration's kernels, with the
pivots captured), the selected inversion (k_selinv_panel / k_selinv_big, one launch per level and form from the root) and the extraction of the blocks
(k_sigma_gather + one device -> host copy).  Sizes: the reference's lap (240 poses / 200 cones), cfg3 (10k / 2k) and cfg4
(100k / 10k), each after optimize(10); warmup calls, then the median of the repeats.

The selinv phase's model: it reads every front's L panel (npiv columns of f rows) and its parent's Sigma rows (nbnd^2 / 2), and
writes its own image (f (f + 1) / 2); flops 2 npiv f^2 (the column products).  Bytes / time against the 8 TB/s of HBM.
Usage: python scripts/marginals_time.py [--warmup 3] [--reps 10] [--sizes 240x200,10000x2000,100000x10000]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
pkg = importlib.import_module("opendlv-logic-cfsd18-sensation-slam_amd")
from plan_exec import Plan  # noqa: E402

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", default="240x200,10000x2000,100000x10000")
    a = ap.parse_args()
    for size in a.sizes.split(","):
        N, M = (int(v) for v in size.split("x"))
        t = pkg.track.generate(N, M)
        fe = pkg.Graph(device=0)
        g = pkg.track.bench_graph(t, fe); fe.close()
        G = pkg.Graph(device=0); G.load_bench_graph(g); G.optimize(10)
        for _ in range(a.warmup):
            G.compute_marginals()
        runs = [G.compute_marginals() for _ in range(a.reps)]
        P = Plan(G.plan_export())
        npiv, nb = P.npiv.astype(np.int64), P.nbnd.astype(np.int64); f = npiv + nb
        bytes_ = 8 * int((npiv * f).sum() + (nb * (nb + 1) // 2).sum() + (f * (f + 1) // 2).sum() + P.n_scalar)
        flops = int((2 * npiv * f * f).sum())
        med = {k: float(np.median([r[k] for r in runs])) for k in ("ms_linearize_factor", "ms_selinv", "ms_extract", "ms_total")}
        sel_s = med["ms_selinv"] * 1e-3
        print(json.dumps(dict(N=N, M=M, n_fronts=runs[0]["n_fronts"], n_levels=runs[0]["n_levels"], max_front=int(f.max()),
                              sigma_bytes=runs[0]["sigma_bytes"], selinv_model_bytes=bytes_, selinv_model_flops=flops,
                              selinv_hbm_fraction=bytes_ / sel_s / HBM_PEAK if sel_s > 0 else None,
                              selinv_gflops=flops / sel_s * 1e-9 if sel_s > 0 else None, reps=a.reps, **med)), flush=True)
        G.close()


if __name__ == "__main__":
    main()
