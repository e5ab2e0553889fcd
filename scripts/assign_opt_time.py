"""The minimum-cost resident association next to the greedy one-to-one one, in ONE session on one handle: both timing hooks alternate
(gs_debug_time_assign_nn_resident, gs_debug_time_assign_opt_resident: HIP events on the dispatch — for the minimum-cost call from its first
dispatch to its last — mean of `reps` launches, two passes) on the two workloads of scripts/assign_nn_time.py: the track of a config of the
generator (default cfg4: 100k poses x 8 cones in view = 800k observations in 100k frames of 8, against 10k cones; random cone covariances with
eigenvalues 0.01 .. 0.5 m^2, a small pose covariance, default gs_nn_params), which has no contests, and the DENSER synthetic one: the first half
of the poses, every observation seen twice (a second return with 0.5 % range and 0.2 degree azimuth noise: frames of 16), against the map plus
one jittered copy of every cone (0.3 m sigma, same type).  Both calls write index and d2 and read the pose covariances; the minimum-cost call
also writes n_admissible.

Per workload: the two times and their ratio, the share of frames that took the kernel's shortcut (their first candidates are distinct: the
frames where gs_associate_nn_resident takes no cone twice), the share of observations whose cone differs from the greedy's, the exact total
gain of both over all frames, the frames where the minimum-cost gain is below the greedy's (none are expected where no n_admissible exceeds 8),
and the largest n_admissible.  One JSON line."""
import importlib, json, os, sys
from fractions import Fraction
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
    d_i, d_d, d_s, d_gi, d_gd, d_oi, d_od, d_on = (DA(nbytes=4 * n), DA(nbytes=8 * n), DA(nbytes=8 * n), DA(nbytes=4 * n), DA(nbytes=8 * n), DA(nbytes=4 * n),
                                                   DA(nbytes=8 * n), DA(nbytes=4 * n))
    r = dict(observations=int(n), frames=int(P), frame_size=int(per_frame), map_cones=int(len(mty)))
    for rnd in range(2):                                        # alternating, twice: the second pair shows how far one run moves
        r["greedy_ms_%d" % rnd] = G.time_assign_nn_resident(d_p, P, d_po, d_ob, n, P, d_fs, d_gi, reps, d_gd, d_pc)
        r["opt_ms_%d" % rnd] = G.time_assign_opt_resident(d_p, P, d_po, d_ob, n, P, d_fs, d_oi, reps, d_od, d_on, d_pc)
        r["ratio_%d" % rnd] = r["opt_ms_%d" % rnd] / r["greedy_ms_%d" % rnd]
    G.associate_nn_resident(d_p, P, d_po, d_ob, n, d_i, d_d, d_s, d_pc); G.synchronize()
    nn = d_i.to_host(np.int32, n).reshape(P, per_frame); gi = d_gi.to_host(np.int32, n); gd = d_gd.to_host(np.float64, n)
    oi = d_oi.to_host(np.int32, n); od = d_od.to_host(np.float64, n); on = d_on.to_host(np.int32, n)
    srt = np.sort(np.where(nn >= 0, nn, -1 - np.arange(per_frame)), axis=1)
    r["shortcut_frames_fraction"] = float(1.0 - (srt[:, 1:] == srt[:, :-1]).any(axis=1).mean())
    r["differs_from_greedy_fraction"] = float((oi != gi).mean()); r["frames_differing_from_greedy_fraction"] = float((oi != gi).reshape(P, per_frame).any(axis=1).mean())
    r["greedy_matched_fraction"] = float((gi >= 0).mean()); r["opt_matched_fraction"] = float((oi >= 0).mean())
    srt = np.sort(np.where(oi.reshape(P, per_frame) >= 0, oi.reshape(P, per_frame), -1 - np.arange(per_frame)), axis=1)
    r["opt_frames_with_a_cone_taken_twice"] = int((srt[:, 1:] == srt[:, :-1]).any(axis=1).sum())
    gate = G_GATE; fg = np.where(gi >= 0, gate - gd, 0.0).reshape(P, per_frame); fo = np.where(oi >= 0, gate - od, 0.0).reshape(P, per_frame)
    lower = np.flatnonzero(fo.sum(axis=1) < fg.sum(axis=1) - 1e-9)          # candidates in fp64; decided exactly below
    exact = lambda f, idx, d2: sum((Fraction(gate) - Fraction(float(d)) for j, d in zip(idx[f * per_frame:(f + 1) * per_frame], d2[f * per_frame:(f + 1) * per_frame]) if j >= 0), Fraction(0))
    r["frames_with_gain_below_greedy"] = int(sum(exact(f, oi, od) < exact(f, gi, gd) for f in lower))
    r["total_gain_greedy"] = float(fg.sum()); r["total_gain_opt"] = float(fo.sum())
    r["max_n_admissible"] = int(on.max()); r["observations_cut_fraction"] = float((on > 8).mean())
    same = oi == gi
    r["same_cone_d2_bits_equal"] = bool(np.array_equal(od[same].view(np.int64), gd[same].view(np.int64)))
    for x in (d_p, d_po, d_ob, d_pc, d_fs, d_i, d_d, d_s, d_gi, d_gd, d_oi, d_od, d_on):
        x.free()
    G.close()
    out[tag] = r


G_GATE = pkg.binding.nn_params().gate_chi2
out = dict(config=name, reps=reps)
obs = np.ascontiguousarray(t["obs"].reshape(-1, 4)); mxy, mty = np.ascontiguousarray(g["lm_est"]), g["lm_type"].astype(np.int32)
measure("track", t["odom_poses"], obs, K, mxy, mty, out)
H = N // 2; o = t["obs"][:H].reshape(H, K, 4); o2 = o.copy()
o2[:, :, 2] *= 1.0 + rng.normal(size=(H, K)) * 0.005; o2[:, :, 0] += rng.normal(size=(H, K)) * 0.2
dense_obs = np.concatenate([o, o2], axis=1).reshape(-1, 4)
dense_xy = np.concatenate([mxy, mxy + rng.normal(size=mxy.shape) * 0.3]); dense_ty = np.concatenate([mty, mty])
measure("dense", np.ascontiguousarray(t["odom_poses"][:H]), dense_obs, 2 * K, dense_xy, dense_ty, out)
out["note"] = ("HIP start / stop events on the dispatch; greedy = k_assign_nn<grid>, opt = k_assign_opt<grid> (frames of 8 run eight to a wave, frames of 16 four "
               "to a wave) followed by k_assign_opt_big<grid> over groups of 64 frames, which finds no frame above 64 observations here")
print(json.dumps(out))
