"""The one-to-one resident association next to the nearest-cone one, in ONE session on one handle: both timing hooks alternate
(gs_debug_time_associate_nn_resident, gs_debug_time_assign_nn_resident: HIP events on the dispatch, mean of `reps` launches, two passes) at a
config of the track generator (default cfg4: 100k poses x 8 cones in view = 800k observations in 100k frames of 8, against 10k cones; random
cone covariances with eigenvalues 0.01 .. 0.5 m^2, a small pose covariance, default gs_nn_params).  Both calls write index and d2 and read the
pose covariances; the NN call also writes the runner-up.

The track has no contests, so a second, DENSER synthetic workload follows: the first half of the poses, every observation seen twice (a second
return with 0.5 % range and 0.2 degree azimuth noise: frames of 16, the same number of observations), against the map plus one jittered copy
of every cone (0.3 m sigma, same type).  Two returns of one cone contest it; the loser takes the copy or nothing.

Per workload: the two times and their ratio, the distribution of the kernel's rounds per frame (a round takes one pair, so a frame's rounds are
its matched observations), and the share of DISPLACED observations (the one-to-one index differs from the nearest-cone index).  One JSON line."""
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
K = t["K"]; rng = np.random.default_rng(1)


def covs(m):
    a = rng.uniform(0, np.pi, m); l1 = rng.uniform(0.01, 0.5, m); l2 = rng.uniform(0.01, 0.5, m); c, s = np.cos(a), np.sin(a); off = (l1 - l2) * c * s
    return np.stack([l1 * c * c + l2 * s * s, off, off, l1 * s * s + l2 * c * c], axis=1)


def measure(tag, poses, obs, per_frame, mxy, mty, out):
    P = len(poses); n = len(obs); assert n == P * per_frame
    po_ = np.repeat(np.arange(P, dtype=np.int32), per_frame); fs = (np.arange(P + 1, dtype=np.int64) * per_frame).astype(np.int32)
    pc = np.tile(np.diag([0.04, 0.04, 1e-3]).reshape(9), (P, 1))
    G = pkg.Graph(); G.map_append(mxy, mty); G.map_set_cov(0, covs(len(mty)))
    d_p, d_po, d_ob, d_pc, d_fs = DA(poses), DA(po_), DA(np.ascontiguousarray(obs)), DA(pc), DA(fs)
    d_i, d_d, d_s, d_ai, d_ad = DA(nbytes=4 * n), DA(nbytes=8 * n), DA(nbytes=8 * n), DA(nbytes=4 * n), DA(nbytes=8 * n)
    r = dict(observations=int(n), frames=int(P), frame_size=int(per_frame), map_cones=int(len(mty)))
    for rnd in range(2):                                        # alternating, twice: the second pair shows how far one run moves
        r["nn_ms_%d" % rnd] = G.time_associate_nn_resident(d_p, P, d_po, d_ob, n, d_i, reps, d_d, d_s, d_pc)
        r["assign_ms_%d" % rnd] = G.time_assign_nn_resident(d_p, P, d_po, d_ob, n, P, d_fs, d_ai, reps, d_ad, d_pc)
        r["ratio_%d" % rnd] = r["assign_ms_%d" % rnd] / r["nn_ms_%d" % rnd]
    nn = d_i.to_host(np.int32, n); nd = d_d.to_host(np.float64, n); ai = d_ai.to_host(np.int32, n); ad = d_ad.to_host(np.float64, n)
    rounds = (ai.reshape(P, per_frame) >= 0).sum(axis=1)
    r["rounds_per_frame_histogram"] = {int(k): int(v) for k, v in zip(*np.unique(rounds, return_counts=True))}
    r["nn_matched_fraction"] = float((nn >= 0).mean()); r["assign_matched_fraction"] = float((ai >= 0).mean())
    r["displaced_fraction"] = float((ai != nn).mean()); r["displaced_to_none_fraction"] = float(((ai != nn) & (ai < 0)).mean())
    srt = np.sort(np.where(nn.reshape(P, per_frame) >= 0, nn.reshape(P, per_frame), -1 - np.arange(per_frame)), axis=1)
    r["nn_frames_with_a_cone_taken_twice_fraction"] = float((srt[:, 1:] == srt[:, :-1]).any(axis=1).mean())
    srt = np.sort(np.where(ai.reshape(P, per_frame) >= 0, ai.reshape(P, per_frame), -1 - np.arange(per_frame)), axis=1)
    r["assign_frames_with_a_cone_taken_twice"] = int((srt[:, 1:] == srt[:, :-1]).any(axis=1).sum())
    same = ai == nn
    r["undisplaced_d2_bits_equal"] = bool(np.array_equal(ad[same].view(np.int64), nd[same].view(np.int64)))
    for x in (d_p, d_po, d_ob, d_pc, d_fs, d_i, d_d, d_s, d_ai, d_ad):
        x.free()
    G.close()
    out[tag] = r


out = dict(config=name, reps=reps)
obs = np.ascontiguousarray(t["obs"].reshape(-1, 4)); mxy, mty = np.ascontiguousarray(g["lm_est"]), g["lm_type"].astype(np.int32)
measure("track", t["odom_poses"], obs, K, mxy, mty, out)
H = N // 2; o = t["obs"][:H].reshape(H, K, 4); o2 = o.copy()
o2[:, :, 2] *= 1.0 + rng.normal(size=(H, K)) * 0.005; o2[:, :, 0] += rng.normal(size=(H, K)) * 0.2
dense_obs = np.concatenate([o, o2], axis=1).reshape(-1, 4)
dense_xy = np.concatenate([mxy, mxy + rng.normal(size=mxy.shape) * 0.3]); dense_ty = np.concatenate([mty, mty])
measure("dense", np.ascontiguousarray(t["odom_poses"][:H]), dense_obs, 2 * K, dense_xy, dense_ty, out)
out["note"] = ("HIP start / stop events on the dispatch; nn = k_assoc_nn_grid (a thread per observation), assign = k_assign_nn<grid> (frames of 8 run eight to a wave, "
               "frames of 16 four to a wave; one pair is taken per round)")
print(json.dumps(out))
