"""Frame following next to what the library offered before it, in ONE session on one handle: a run of `steps` frames of 16 observations along
the generator's track for 1, 2, 8 and 64 hypotheses (the true start and poses scattered 0.1 m / 0.01 rad around it, merge_xy = 0 so that
every one of them works through the whole run), against the true cones of a config's map (default cfg4: 10 000 cones; cfg2: the reference's
lap size, 200 cones).

    follow_ms      gs_debug_time_follow_resident: HIP events from the run's first dispatch to its last, mean of `reps` runs
    host_loop_ms   the same work as a host loop of gs_frame_frontend_localize per hypothesis and step with the prediction in numpy on the host
                   (wall clock, mean of 3 runs): one wait and one PCIe round trip per call
Two alternating passes; the second shows how far one run moves.  Also the per-step dispatch count (from the launchers' rule for frames of 16)
and, per hypothesis count, how many hypotheses still track at the end and the best one's distance from the true end pose.  One JSON line."""
import importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
pkg = importlib.import_module("opendlv-logic-cfsd18-sensation-slam_amd")
b = pkg.binding
name = sys.argv[1] if len(sys.argv) > 1 else "cfg4"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 32
N, M = pkg.track.CONFIGS[name]
N = min(N, 2000)                                                   # the lap's first poses are all the run needs; the map is the config's
t = pkg.track.generate(N, M, 16)
DA = b.DeviceArray; rng = np.random.default_rng(1)
path = t["truth_poses"][10:10 + steps]; frames = np.ascontiguousarray(t["obs"][10:10 + steps].reshape(-1, 4))
fs = (np.arange(steps + 1) * 16).astype(np.int32)


def between(p0, p1):
    c, s = np.cos(p0[2]), np.sin(p0[2]); d = p1[:2] - p0[:2]
    return np.array([c * d[0] + s * d[1], -s * d[0] + c * d[1], (p1[2] - p0[2] + np.pi) % (2 * np.pi) - np.pi])


motion = np.array([between(path[i], path[i + 1]) for i in range(steps - 1)]); qu = np.tile(np.diag([0.05 ** 2, 0.05 ** 2, 0.01 ** 2]).reshape(9), (steps - 1, 1))
cov0 = np.diag([0.1 ** 2, 0.1 ** 2, 0.02 ** 2]).reshape(9)
prm, jc, loc, fp = b.nn_params(), b.jc_params(), b.loc_params(), b.follow_params(merge_xy=0.0)
G = pkg.Graph(); G.map_append(t["cone_xy"], t["cone_type"])


def predict(x, P, u, Q):
    c, s = np.cos(x[2]), np.sin(x[2]); p, q = c * u[0] - s * u[1], s * u[0] + c * u[1]
    F = np.array([[1, 0, -q], [0, 1, p], [0, 0, 1.0]]); W = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    return np.array([x[0] + p, x[1] + q, (x[2] + u[2] + np.pi) % (2 * np.pi) - np.pi]), F @ P @ F.T + W @ Q @ W.T


def host_loop(poses):
    """what a caller did before: per step and hypothesis one gs_frame_frontend_localize, the motion model on the host"""
    X = [p.copy() for p in poses]; P = [cov0.reshape(3, 3).copy() for _ in poses]; gate = np.array(jc.gate[:])
    for i in range(steps):
        ob = frames[16 * i:16 * i + 16]
        for h in range(len(X)):
            if i:
                X[h], P[h] = predict(X[h], P[h], motion[i - 1], qu[i - 1].reshape(3, 3))
            r = G.frame_frontend_localize(X[h], ob, P[h].reshape(9), prm, jc, loc)[6]
            if r["status"][0] <= 1 and r["n_pairs"][0] >= 3 and r["chi2"][0] <= gate[r["n_pairs"][0]]:
                X[h], P[h] = r["pose"][0].copy(), r["cov"][0].reshape(3, 3).copy()
    return X


out = dict(config=name, map_cones=int(M), steps=steps, frame_size=16, reps=reps, runs={})
d_ob, d_fs, d_mo, d_qu = DA(frames), DA(fs), DA(motion), DA(qu)
for rnd in range(2):
    for nh in (1, 2, 8, 64):
        poses = path[0] + np.concatenate([np.zeros((1, 3)), rng.normal(size=(nh - 1, 3)) * [0.1, 0.1, 0.01]]); covs = np.tile(cov0, (nh, 1))
        d_p, d_c = DA(poses), DA(covs); d_st, d_b = DA(nbytes=136 * nh), DA(nbytes=8)
        ms = G.time_follow_resident(d_p, nh, d_ob, len(frames), steps, d_fs, 16, reps, d_mo, d_c, d_qu, None, None, d_st, d_b, prm, jc, loc, fp)
        G.synchronize()
        st = d_st.to_host(np.uint8, 136 * nh).view(b.FOLLOW_STATE); b2 = d_b.to_host(np.int32, 2)
        host_loop(poses)                                               # warm
        t0 = time.perf_counter()
        for _ in range(3):
            X = host_loop(poses)
        host_ms = (time.perf_counter() - t0) / 3 * 1e3
        r = out["runs"].setdefault(str(nh), {})
        r["follow_ms_%d" % rnd] = ms; r["host_loop_ms_%d" % rnd] = host_ms; r["follow_us_per_step_%d" % rnd] = ms * 1e3 / steps
        r["tracking_at_end"] = int(b2[1]); r["best"] = int(b2[0])
        r["best_end_error_m"] = float(np.hypot(*(st["pose"][b2[0], :2] - path[-1, :2]))) if b2[0] >= 0 else None
        r["host_loop_end_error_m"] = float(np.hypot(*(X[0][:2] - path[-1, :2])))
        for a in (d_p, d_c, d_st, d_b):
            a.free()
out["dispatches_per_step"] = 8
out["note"] = ("per step: k_follow_stage, k_assign_opt + k_assign_opt_big, k_joint_compat + k_joint_compat_big, k_localize + k_localize_big, k_follow_update "
               "(frames of 16: the chain's small kernels, their big ones behind them find no frame above 64); one k_follow_init per run")
print(json.dumps(out))
G.close()
