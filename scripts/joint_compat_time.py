"""The joint compatibility test next to the minimum-cost association whose result it takes, in ONE session on one handle: both timing hooks
alternate (gs_debug_time_assign_opt_resident, gs_debug_time_joint_compat_resident: HIP events from the first dispatch of a call to its last,
mean of `reps` launches, two passes) on the two workloads of scripts/assign_opt_time.py — the track of a config of the generator (default
cfg4: 800k observations in 100k frames of 8 against 10k cones) and the denser synthetic one (the first half of the poses, every observation
seen twice: frames of 16, against the map and a jittered copy) — with the same covariances and default parameters.  The joint test is fed
gs_assign_opt_resident's index and writes the pruned index and the whole per-frame record.

Per workload: the two times and their ratio, the share of frames that left after one round (n_dropped == 0), the share of pairs dropped and
untestable, and the mean |delta|.  One JSON line."""
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
    d_oi, d_od, d_on, d_ji = DA(nbytes=4 * n), DA(nbytes=8 * n), DA(nbytes=4 * n), DA(nbytes=4 * n)
    d_j, d_k, d_d, d_u, d_dl = DA(nbytes=8 * P), DA(nbytes=4 * P), DA(nbytes=4 * P), DA(nbytes=4 * P), DA(nbytes=24 * P)
    r = dict(observations=int(n), frames=int(P), frame_size=int(per_frame), map_cones=int(len(mty)))
    for rnd in range(2):                                        # alternating, twice: the second pair shows how far one run moves
        r["opt_ms_%d" % rnd] = G.time_assign_opt_resident(d_p, P, d_po, d_ob, n, P, d_fs, d_oi, reps, d_od, d_on, d_pc)
        r["jc_ms_%d" % rnd] = G.time_joint_compat_resident(d_p, P, d_po, d_ob, n, P, d_fs, d_oi, d_ji, reps, d_j, d_k, d_d, d_u, d_dl, d_pc)
        r["ratio_%d" % rnd] = r["jc_ms_%d" % rnd] / r["opt_ms_%d" % rnd]
    G.synchronize()
    oi = d_oi.to_host(np.int32, n); ji = d_ji.to_host(np.int32, n); J = d_j.to_host(np.float64, P)
    nk, nd, nu = d_k.to_host(np.int32, P), d_d.to_host(np.int32, P), d_u.to_host(np.int32, P); dl = d_dl.to_host(np.float64, 3 * P).reshape(P, 3)
    named = int((oi >= 0).sum())
    r["one_round_frames_fraction"] = float((nd == 0).mean()); r["pairs"] = named
    r["pairs_dropped_fraction"] = float(nd.sum() / max(named, 1)); r["pairs_untestable_fraction"] = float(nu.sum() / max(named, 1))
    r["counts_add_up"] = bool(np.array_equal((nk + nd + nu), (oi >= 0).reshape(P, per_frame).sum(axis=1)) and np.array_equal(nk, (ji >= 0).reshape(P, per_frame).sum(axis=1)))
    r["kept_is_subset"] = bool(((ji == oi) | (ji == -1)).all())
    r["most_dropped_in_a_frame"] = int(nd.max()); r["mean_joint_d2"] = float(J.mean()); r["mean_abs_delta"] = [float(x) for x in np.abs(dl).mean(axis=0)]
    for x in (d_p, d_po, d_ob, d_pc, d_fs, d_oi, d_od, d_on, d_ji, d_j, d_k, d_d, d_u, d_dl):
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
out["note"] = ("HIP start / stop events on the dispatches; opt = k_assign_opt<grid> + k_assign_opt_big<grid>, jc = k_joint_compat (frames of 8 eight to a wave, "
               "frames of 16 four to a wave) + k_joint_compat_big over groups of 64 frames, which finds no frame above 64 observations here")
print(json.dumps(out))
