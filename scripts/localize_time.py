"""Frame localisation next to the joint compatibility test whose pruned index it takes, in ONE session on one handle: the timing hooks alternate
(gs_debug_time_joint_compat_resident, gs_debug_time_localize_resident at max_iterations 1 and 5: HIP events from the first dispatch of a call
to its last, mean of `reps` launches, two passes) on the two workloads of scripts/joint_compat_time.py — the track of a config of the generator
(default cfg4: 800k observations in 100k frames of 8 against 10k cones) and the denser synthetic one (frames of 16 against the map and a
jittered copy) — with the same covariances and default parameters.  The hypothesis is gs_assign_opt_resident's index pruned by the joint test.

Per workload: the three times and the ratios to the joint test, the share of frames per iteration count and per status at max_iterations 5, the
mean chi2 per pair and the mean |pose - prior|.  One JSON line."""
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
    d_oi, d_ji, d_od, d_on = DA(nbytes=4 * n), DA(nbytes=4 * n), DA(nbytes=8 * n), DA(nbytes=4 * n)
    d_j, d_k, d_d, d_u, d_dl = DA(nbytes=8 * P), DA(nbytes=4 * P), DA(nbytes=4 * P), DA(nbytes=4 * P), DA(nbytes=24 * P)
    d_x, d_c, d_chi, d_np, d_it, d_st = DA(nbytes=24 * P), DA(nbytes=72 * P), DA(nbytes=8 * P), DA(nbytes=4 * P), DA(nbytes=4 * P), DA(nbytes=4 * P)
    G.time_assign_opt_resident(d_p, P, d_po, d_ob, n, P, d_fs, d_oi, 1, d_od, d_on, d_pc)
    one, five = pkg.binding.loc_params(max_iterations=1), pkg.binding.loc_params()
    r = dict(observations=int(n), frames=int(P), frame_size=int(per_frame), map_cones=int(len(mty)))
    for rnd in range(2):                                        # alternating, twice: the second pass shows how far one run moves
        r["jc_ms_%d" % rnd] = G.time_joint_compat_resident(d_p, P, d_po, d_ob, n, P, d_fs, d_oi, d_ji, reps, d_j, d_k, d_d, d_u, d_dl, d_pc)
        r["loc1_ms_%d" % rnd] = G.time_localize_resident(d_p, P, d_po, d_ob, n, P, d_fs, d_ji, reps, d_x, d_c, d_chi, d_np, d_it, d_st, d_pc, None, one)
        r["loc5_ms_%d" % rnd] = G.time_localize_resident(d_p, P, d_po, d_ob, n, P, d_fs, d_ji, reps, d_x, d_c, d_chi, d_np, d_it, d_st, d_pc, None, five)
        r["loc1_over_jc_%d" % rnd] = r["loc1_ms_%d" % rnd] / r["jc_ms_%d" % rnd]; r["loc5_over_jc_%d" % rnd] = r["loc5_ms_%d" % rnd] / r["jc_ms_%d" % rnd]
    G.synchronize()
    x = d_x.to_host(np.float64, 3 * P).reshape(P, 3); chi = d_chi.to_host(np.float64, P); npairs = d_np.to_host(np.int32, P)
    it = d_it.to_host(np.int32, P); st = d_st.to_host(np.int32, P); cv = d_c.to_host(np.float64, 9 * P).reshape(P, 9)
    ok = st <= 1
    r["frames_per_iteration_count"] = (np.bincount(it, minlength=6) / P).tolist(); r["frames_per_status"] = (np.bincount(st, minlength=5) / P).tolist()
    r["pairs"] = int(npairs.sum()); r["mean_chi2_per_pair"] = float(chi[ok].sum() / max(npairs[ok].sum(), 1))
    dx = x[ok] - poses[ok]; dx[:, 2] = (dx[:, 2] + np.pi) % (2 * np.pi) - np.pi
    r["mean_abs_pose_minus_prior"] = [float(v) for v in np.abs(dx).mean(axis=0)]
    r["mean_posterior_variances"] = [float(v) for v in cv[ok][:, [0, 4, 8]].mean(axis=0)]
    for a in (d_p, d_po, d_ob, d_pc, d_fs, d_oi, d_ji, d_od, d_on, d_j, d_k, d_d, d_u, d_dl, d_x, d_c, d_chi, d_np, d_it, d_st):
        a.free()
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
out["note"] = ("HIP start / stop events on the dispatches; jc = k_joint_compat + k_joint_compat_big, loc = k_localize (frames of 8 eight to a wave, frames of 16 "
               "four to a wave) + k_localize_big over groups of 64 frames, which finds no frame above 64 observations here")
print(json.dumps(out))
