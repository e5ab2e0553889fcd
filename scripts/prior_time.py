"""Cost of the prior pass per iteration: gs_time_iterations with and without priors on the SAME handle, XY priors on all
poses, at lap size, cfg3 and cfg4; median of 5 interleaved rounds.  Usage: python scripts/prior_time.py [out.jsonl]
(default profiles/prior_time.jsonl).  prior_pass_us = the difference of the linearise phase (event to event: linearise + tail + priors)."""
import importlib, json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("opendlv-logic-cfsd18-sensation-slam_amd")
out = open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "prior_time.jsonl"), "w")
for name, (N, M) in (("lap", (1000, 200)), ("cfg3", pkg.track.CONFIGS["cfg3"]), ("cfg4", pkg.track.CONFIGS["cfg4"])):
    t = pkg.track.generate(N, M)
    fe = pkg.Graph(device=0); g = pkg.track.bench_graph(t, fe); fe.close()
    G = pkg.Graph(device=0); G.load_bench_graph(g); G.initialize_optimization()
    ids = np.arange(N); z = np.asarray(g["pose_est"])[:, :2].copy(); W = np.tile(np.eye(2).reshape(1, 4), (N, 1))
    rounds = {"without": [], "with": []}
    for r in range(5):
        G.clear_priors(); s = G.time_iterations(20); rounds["without"].append((s.ms_total, s.ms_linearize))
        G.add_pose_xy_priors(ids, z, W); s = G.time_iterations(20); rounds["with"].append((s.ms_total, s.ms_linearize))
    med = {k: np.median(np.array(v), axis=0).tolist() for k, v in rounds.items()}
    rec = dict(graph=name, poses=N, cones=M, priors=N, reps=20, rounds=5, ms_total_without=med["without"][0], ms_total_with=med["with"][0],
               ms_linearize_phase_without=med["without"][1], ms_linearize_phase_with=med["with"][1],
               prior_pass_us=1e3 * (med["with"][1] - med["without"][1]), all_rounds=rounds)
    print(json.dumps(rec)); out.write(json.dumps(rec) + "\n"); out.flush()
    G.close()
