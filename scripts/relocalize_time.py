"""Relocalisation on the synthetic track of a config of the generator (default cfg4: 10 000 cones), frames of 16 observations (the
generator's own, obs_per_pose = 16) taken at 64 poses spread over the lap, against the true cone map, NO pose given: the time of the search
alone and of the search plus the runner-up's pass, for ONE frame and for the batch of 64, through gs_debug_time_relocalize_resident (HIP
events from the first dispatch of a call to its last, mean of `reps` launches; the four measurements alternate, two passes, in one session on
one handle; the grid is built before).  Also: the seeds that existed, the statuses, the share of frames whose second_count equals count, and
the distance of the found pose from the generator's true pose.
Two workloads: "regular", the generator's own observations against its own cones — a stadium of cones EXACTLY 5 m apart, so every frame fits
every place along it and the runner-up equals the winner by construction; and "jittered", the same cones moved by up to 0.3 m (seeded) and the
same frames' observations recomputed exactly from the true poses (the inverse of the A0 formula), which is what a surveyed track looks like.
One JSON line."""
import importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
pkg = importlib.import_module("opendlv-logic-cfsd18-sensation-slam_amd")
name = sys.argv[1] if len(sys.argv) > 1 else "cfg4"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
N, M = pkg.track.CONFIGS[name]
K, F = 16, 64
t = pkg.track.generate(N, M, K)
DA = pkg.binding.DeviceArray
at = np.linspace(0, N - 1, F + 2).astype(int)[1:-1]                            # 64 poses, none at the lap's ends
truth = t["truth_poses"][at]; seen = t["obs_cone"][at]
fs = (np.arange(F + 1) * K).astype(np.int32)
LIDAR = float(pkg.binding.default_config().lidar_to_cog); D2R = 0.017453292522222


def exact_obs(cones):
    """the frames' observations of `cones` from the true poses: az = atan2(y, x - lidar) in the A0 formula's degrees, zenith 0"""
    out = np.zeros((F, K, 4))
    for f in range(F):
        x, y, th = truth[f]; d = cones[seen[f]] - np.array([x, y]); c, s = np.cos(th), np.sin(th)
        zx, zy = d[:, 0] * c + d[:, 1] * s - LIDAR, -d[:, 0] * s + d[:, 1] * c
        out[f] = np.stack([np.arctan2(zy, zx) / D2R, np.zeros(K), np.hypot(zx, zy), t["cone_type"][seen[f]].astype(np.float64)], axis=1)
    return np.ascontiguousarray(out.reshape(-1, 4))


def measure(tag, cones, obs, out):
  global G, d_ob, d_fs, d_fs1
  G = pkg.Graph(); G.map_append(cones, t["cone_type"])
  d_ob, d_fs, d_fs1 = DA(obs), DA(fs), DA(fs[:2])
  _measure(out.setdefault(tag, {}))


def _measure(out):
  global G
  d_pose, d_sp, d_cost, d_ns = DA(nbytes=24 * F), DA(nbytes=24 * F), DA(nbytes=8 * F), DA(nbytes=8 * F)
  d_seed, d_cnt, d_sc, d_st, d_idx, d_e2 = DA(nbytes=16 * F), DA(nbytes=4 * F), DA(nbytes=4 * F), DA(nbytes=4 * F), DA(nbytes=4 * F * K), DA(nbytes=8 * F * K)

  def time(n_frames, second):
      return G.time_relocalize_resident(d_ob, n_frames * K, n_frames, d_fs1 if n_frames == 1 else d_fs, reps, d_pose, d_cnt, d_cost, d_seed,
                                        d_sc if second else None, d_sp if second else None, d_ns, d_st, d_idx, d_e2)

  for rnd in range(2):                                                            # alternating, twice: the second pass shows how far one run moves
      out["one_frame_search_ms_%d" % rnd] = time(1, False); out["one_frame_search_and_second_ms_%d" % rnd] = time(1, True)
      out["batch64_search_ms_%d" % rnd] = time(F, False); out["batch64_search_and_second_ms_%d" % rnd] = time(F, True)
  G.synchronize()
  pose = d_pose.to_host(np.float64, 3 * F).reshape(F, 3); cnt = d_cnt.to_host(np.int32, F); sc = d_sc.to_host(np.int32, F); st = d_st.to_host(np.int32, F)
  ns = d_ns.to_host(np.int64, F); idx = d_idx.to_host(np.int32, F * K).reshape(F, K)
  out["n_seeds_min_mean_max"] = [int(ns.min()), float(ns.mean()), int(ns.max())]
  out["frames_per_status"] = np.bincount(st, minlength=5).tolist()
  out["count_min_mean_max"] = [int(cnt.min()), float(cnt.mean()), int(cnt.max())]
  out["second_count_min_mean_max"] = [int(sc.min()), float(sc.mean()), int(sc.max())]
  out["share_second_equals_count"] = float((sc == cnt).mean())
  err = np.hypot(pose[:, 0] - truth[:, 0], pose[:, 1] - truth[:, 1])
  dth = np.abs((pose[:, 2] - truth[:, 2] + np.pi) % (2 * np.pi) - np.pi)
  out["frames_within_half_a_metre_of_the_truth"] = int((err < 0.5).sum())
  out["median_position_error_m"] = float(np.median(err)); out["median_heading_error_rad"] = float(np.median(dth))
  out["matches_equal_to_the_generator_s"] = float((idx == seen).mean())
  out["note"] = ("HIP start / stop events on the dispatches: k_reloc_seed + k_reloc_pick, twice with the runner-up; the score walks the hashed grid (cell edge "
                 "from inlier_radius); default gs_reloc_params")
  for a in (d_ob, d_fs, d_fs1, d_pose, d_sp, d_cost, d_ns, d_seed, d_cnt, d_sc, d_st, d_idx, d_e2):
      a.free()
  G.close()


out = dict(config=name, reps=reps, map_cones=int(M), frame_size=K, frames=F)
measure("regular", t["cone_xy"], np.ascontiguousarray(t["obs"][at].reshape(-1, 4)), out)
jit = t["cone_xy"] + np.random.default_rng(27).uniform(-0.3, 0.3, t["cone_xy"].shape)
measure("jittered", jit, exact_obs(jit), out)
print(json.dumps(out))
