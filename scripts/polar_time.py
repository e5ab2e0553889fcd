"""Cost of the polar pass per iteration: gs_time_iterations on the same graph with all observation edges Cartesian against all
of them range-bearing, at lap size, cfg3 and cfg4; median of 5 interleaved rounds of 20 iterations.
Usage: python scripts/polar_time.py [out.jsonl] [graph ...]   (default profiles/polar_time.jsonl; graphs lap cfg3 cfg4)
polar_pass_us = the difference of the linearise phase (event to event: linearise + tail + priors + polar); the fused kernel's own time
(ms_linearize_kernel, the yardstick) comes from the all-Cartesian handle.  Record layout measured: vertex-sorted structure-of-arrays
planes (lane v reads record pv_start[v] + i: neighbouring lanes are a run length apart); bytes per edge counted below."""
import importlib, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("opendlv-logic-cfsd18-sensation-slam_amd")
args = sys.argv[1:]
out = open(args[0] if args else os.path.join(ROOT, "profiles", "polar_time.jsonl"), "w")
graphs = dict(lap=(1000, 200), cfg3=pkg.track.CONFIGS["cfg3"], cfg4=pkg.track.CONFIGS["cfg4"])
# per edge and pass: pose side 5 doubles + 2 ints of the record, 2 + 2 doubles of the landmark / the pose's cos, sin (gathered), 6 doubles of
# H_pl stored; landmark side the record again through the second index (5 doubles + 2 ints), the pose's 3 + 2 doubles (gathered); the
# diagonal blocks and right-hand sides (9 + 9 doubles per pose, 5 + 5 per landmark, read-modify-write) are per vertex
BYTES_PER_EDGE = (5 * 8 + 2 * 4 + 4 * 8 + 6 * 8) + (4 + 5 * 8 + 2 * 4 + 5 * 8)
for name in (args[1:] or ["lap", "cfg3", "cfg4"]):
    N, M = graphs[name]
    t = pkg.track.generate(N, M)
    fe = pkg.Graph(device=0); g = pkg.track.bench_graph(t, fe); fe.close()
    z = np.asarray(g["pl_z"], dtype=np.float64).reshape(-1, 2); W = np.asarray(g["pl_info"], dtype=np.float64).reshape(-1, 2, 2); E = len(z)
    r = np.hypot(z[:, 0], z[:, 1]); zp = np.stack([r, np.arctan2(z[:, 1], z[:, 0])], 1)
    Om = np.zeros((E, 4)); Om[:, 0] = W[:, 0, 0]; Om[:, 1] = Om[:, 2] = W[:, 0, 1] * r; Om[:, 3] = W[:, 1, 1] * r * r
    C = pkg.Graph(device=0); C.load_bench_graph(g); C.initialize_optimization()
    P = pkg.Graph(device=0)
    P.add_poses(np.arange(N), g["pose_est"]); P.add_landmarks(np.arange(M), g["lm_est"]); P.add_odometry_edges(g["pp_i"], g["pp_j"], g["pp_z"], g["pp_info"])
    P.add_range_bearing_edges(g["pl_p"], g["pl_l"], zp, Om)
    for i in g["fixed_poses"]: P.set_fixed_pose(int(i))
    for l in g["fixed_landmarks"]: P.set_fixed_landmark(int(l))
    P.initialize_optimization()
    rounds = {"cartesian": [], "polar": []}
    for _ in range(5):
        s = C.time_iterations(20); rounds["cartesian"].append((s.ms_total, s.ms_linearize, s.ms_linearize_kernel))
        s = P.time_iterations(20); rounds["polar"].append((s.ms_total, s.ms_linearize, s.ms_linearize_kernel))
    med = {k: np.median(np.array(v), axis=0).tolist() for k, v in rounds.items()}
    pass_us = 1e3 * (med["polar"][1] - med["cartesian"][1])
    rec = dict(graph=name, poses=N, cones=M, observation_edges=E, polar_edges=P.num_polar_edges(), reps=20, rounds=5, layout="vertex-sorted SoA planes",
               ms_total_cartesian=med["cartesian"][0], ms_total_polar=med["polar"][0],
               ms_linearize_phase_cartesian=med["cartesian"][1], ms_linearize_phase_polar=med["polar"][1],
               fused_kernel_us_cartesian=1e3 * med["cartesian"][2], fused_kernel_us_on_carriers=1e3 * med["polar"][2],
               polar_pass_us=pass_us, polar_pass_ns_per_edge=1e3 * pass_us / E, fused_kernel_ns_per_edge=1e6 * med["cartesian"][2] / E,
               polar_bytes_per_edge=BYTES_PER_EDGE, polar_gb_per_s=BYTES_PER_EDGE * E / (pass_us * 1e3) if pass_us > 0 else None, all_rounds=rounds)
    print(json.dumps(rec)); out.write(json.dumps(rec) + "\n"); out.flush()
    C.close(); P.close()
