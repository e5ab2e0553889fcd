"""The covariance-gated resident association next to the Euclidean one, in ONE session on one handle: both timing hooks back to back
(gs_debug_time_associate_resident, gs_debug_time_associate_nn_resident: HIP events on the query dispatch, mean of `reps` launches) at a
config of the track generator (default cfg4: 100k poses x 8 cones in view = 800k observations against 10k cones).  The cones carry random
covariances with eigenvalues 0.01 .. 0.5 m^2, the poses a small random covariance; default gs_nn_params.  Prints one JSON line."""
import importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
pkg = importlib.import_module("opendlv-logic-cfsd18-sensation-slam_amd")
name = sys.argv[1] if len(sys.argv) > 1 else "cfg4"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
N, M = pkg.track.CONFIGS[name]
t = pkg.track.generate(N, M); fe = pkg.Graph(); g = pkg.track.bench_graph(t, fe); fe.close()
DA = pkg.binding.DeviceArray
K = t["K"]; obs = np.ascontiguousarray(t["obs"].reshape(-1, 4)); po_ = np.repeat(np.arange(N, dtype=np.int32), K); n = len(obs)
mxy, mty = np.ascontiguousarray(g["lm_est"]), g["lm_type"].astype(np.int32)
rng = np.random.default_rng(1)
a = rng.uniform(0, np.pi, M); l1 = rng.uniform(0.01, 0.5, M); l2 = rng.uniform(0.01, 0.5, M); c, s = np.cos(a), np.sin(a); off = (l1 - l2) * c * s
cov = np.stack([l1 * c * c + l2 * s * s, off, off, l1 * s * s + l2 * c * c], axis=1)
pc = np.tile(np.diag([0.04, 0.04, 1e-3]).reshape(9), (N, 1))
G = pkg.Graph(); G.map_append(mxy, mty); G.map_set_cov(0, cov)
d_p, d_po, d_ob, d_pc = DA(t["odom_poses"]), DA(po_), DA(obs), DA(pc)
d_i, d_d, d_s, d_e = DA(nbytes=4 * n), DA(nbytes=8 * n), DA(nbytes=8 * n), DA(nbytes=4 * n)
out = dict(config=name, observations=int(n), map_cones=int(M), reps=reps)
for rnd in range(2):                                            # twice, in the same order: the second pair shows how far one run moves
    out["euclid_1.2m_ms_%d" % rnd] = G.time_associate_resident(d_p, N, d_po, d_ob, n, 1.2, d_e, reps)
    out["euclid_3.0m_ms_%d" % rnd] = G.time_associate_resident(d_p, N, d_po, d_ob, n, 3.0, d_e, reps)
    out["nn_no_pose_cov_index_only_ms_%d" % rnd] = G.time_associate_nn_resident(d_p, N, d_po, d_ob, n, d_i, reps)
    out["nn_ms_%d" % rnd] = G.time_associate_nn_resident(d_p, N, d_po, d_ob, n, d_i, reps, d_d, d_s, d_pc)
idx = d_i.to_host(np.int32, n); sec = d_s.to_host(np.float64, n); eu = d_e.to_host(np.int32, n)
out["nn_matched_fraction"] = float((idx >= 0).mean()); out["euclid_3.0m_matched_fraction"] = float((eu >= 0).mean())
out["nn_with_runner_up_fraction"] = float(np.isfinite(sec).mean()); out["nn_differs_from_euclid_3.0m_fraction"] = float((idx != eu).mean())
out["note"] = ("HIP start / stop events on the query dispatch; the Euclidean figure is k_pose_trig + k_associate_grid_dev (first match in map order), the NN figure "
               "k_assoc_nn_grid (sincos per observation, every candidate of the nine buckets evaluated, three outputs)")
for x in (d_p, d_po, d_ob, d_pc, d_i, d_d, d_s, d_e):
    x.free()
G.close()
print(json.dumps(out))
