"""Cone candidates next to what the library offered before them, in ONE session on one handle: a run of `steps` frames of 16 observations along
the generator's track (cfg4's cones, nothing explained: every observation goes to the candidates), starting from a table with 0, 64 and 1024
live candidates (the true cones nearest the start, confirmed, 0.2 m sigma).

    cand_ms        gs_debug_time_cand_resident: HIP events from the run's first dispatch to its last, mean of `reps` runs
    host_loop_ms   the same work as the parent commit offers it: per step one gs_assign_opt_batch against the table as a map, then the fusion,
                   the misses, the confirmation and the spawning in numpy on the host (wall clock, mean of 3 runs): one wait, one upload of the
                   table and one PCIe round trip per step
Two alternating passes; the second shows how far one run moves.  Also the counters of the run's last step.  One JSON line.
`--resident-only`: just the resident runs (for a rocprofv3 --kernel-trace run of them alone)."""
import importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
pkg = importlib.import_module("opendlv-logic-cfsd18-sensation-slam_amd")
b = pkg.binding
args = [a for a in sys.argv[1:] if not a.startswith("--")]; resident_only = "--resident-only" in sys.argv
reps = int(args[0]) if len(args) > 0 else 20
steps = int(args[1]) if len(args) > 1 else 32
t = pkg.track.generate(2000, 10000, 16)
DA = b.DeviceArray
path = np.ascontiguousarray(t["truth_poses"][10:10 + steps]); frames = np.ascontiguousarray(t["obs"][10:10 + steps].reshape(-1, 4))
fs = (np.arange(steps + 1) * 16).astype(np.int32)
prm, cp = b.nn_params(), b.cand_params()
G = pkg.Graph()
Z = G.polar_to_xy(frames[:, 0], frames[:, 1], frames[:, 2])               # the CoG-frame XY of every observation, once (not part of the timed loop)


def table_of(n_live):
    rec = np.zeros(n_live, dtype=b.CAND)
    near = np.argsort(np.hypot(*(t["cone_xy"] - path[0, :2]).T))[:n_live]
    rec["xy"] = t["cone_xy"][near]; rec["cov"] = [0.04, 0.0, 0.0, 0.04]; rec["type"] = t["cone_type"][near]; rec["id"] = np.arange(n_live)
    rec["state"] = 2; rec["hits"] = 3; rec["confirm_step"] = 0
    return rec


def host_loop(rec):
    """what a caller did before: the association on the device per step, everything else of the rule in numpy"""
    tab = np.zeros(b.CAND_MAX, dtype=b.CAND); tab["xy"] = np.nan; tab["id"] = -1; tab[:len(rec)] = rec; next_id = len(rec); v2 = cp.view_range ** 2
    for i in range(steps):
        ob = frames[16 * i:16 * i + 16]; pose = path[i]
        idx, _, na = G.assign_opt(pose[None], np.zeros(16, dtype=np.int32), ob, [0, 16], np.ascontiguousarray(tab["xy"]), np.ascontiguousarray(tab["type"]),
                                  np.ascontiguousarray(tab["cov"]), None, prm)
        zz = Z[16 * i:16 * i + 16]; c, s = np.cos(pose[2]), np.sin(pose[2])
        w = np.stack([zz[:, 0] * c - zz[:, 1] * s, zz[:, 0] * s + zz[:, 1] * c], axis=1); g = w + pose[:2]; r2 = (zz ** 2).sum(1)
        k = prm.sigma_range ** 2 / r2; sb2 = prm.sigma_bearing ** 2; sx2 = prm.sigma_xy ** 2
        A = np.stack([k * w[:, 0] ** 2 + sb2 * w[:, 1] ** 2 + sx2, (k - sb2) * w[:, 0] * w[:, 1], k * w[:, 1] ** 2 + sb2 * w[:, 0] ** 2 + sx2], axis=1)
        live = tab["state"] != 0; was_free = np.flatnonzero(~live); hit = np.zeros(b.CAND_MAX, dtype=bool)
        for o in np.flatnonzero(idx >= 0):
            sl = idx[o]; C = tab["cov"][sl].reshape(2, 2); Am = np.array([[A[o, 0], A[o, 1]], [A[o, 1], A[o, 2]]]); K = C @ np.linalg.inv(C + Am)
            tab["xy"][sl] = tab["xy"][sl] + K @ (g[o] - tab["xy"][sl]); tab["cov"][sl] = (K @ Am).reshape(4); hit[sl] = True
        tab["hits"][hit] += 1; tab["misses"][hit] = 0; tab["last_step"][hit] = i
        e = tab["xy"] - pose[:2]; dx = c * e[:, 0] + s * e[:, 1]; dy = c * e[:, 1] - s * e[:, 0]; rr = dx * dx + dy * dy
        with np.errstate(invalid="ignore"):
            vis = live & ~hit & (rr < v2) & (dx >= cp.view_cos * np.sqrt(rr))
        tab["misses"][vis] += 1
        gone = vis & (tab["state"] == 1) & (tab["misses"] >= cp.max_misses)
        tab["state"][gone] = 0; tab["xy"][gone] = np.nan; tab["cov"][gone] = 0
        conf = (tab["state"] == 1) & (tab["hits"] >= cp.confirm_hits); tab["state"][conf] = 2; tab["confirm_step"][conf] = i
        sp = np.flatnonzero((idx < 0) & (na == 0) & (ob[:, 2] < cp.spawn_range))[:len(was_free)]
        for r, o in enumerate(sp):
            sl = was_free[r]; tab["xy"][sl] = g[o]; tab["cov"][sl] = [A[o, 0], A[o, 1], A[o, 1], A[o, 2]]; tab["type"][sl] = int(ob[o, 3]); tab["id"][sl] = next_id + r
            tab["state"][sl] = 1; tab["hits"][sl] = 1; tab["misses"][sl] = 0; tab["first_step"][sl] = tab["last_step"][sl] = i
        next_id += len(sp)
    return tab


out = dict(steps=steps, frame_size=16, reps=reps, runs={})
d_ob, d_fs, d_po = DA(frames), DA(fs), DA(path)
for rnd in range(2):
    for n_live in (0, 64, 1024):
        rec = table_of(n_live)
        d_rec = DA(rec.view(np.uint8)) if n_live else None; d_steps = DA(nbytes=48 * steps); d_meta = DA(nbytes=16)
        ms = G.time_cand_resident(d_ob, len(frames), steps, d_fs, 16, d_po, reps, None, None, n_live, d_rec, d_steps, None, None, None, d_meta, prm, cp)
        G.synchronize()
        st = d_steps.to_host(np.uint8, 48 * steps).view(b.CAND_STEP); meta = d_meta.to_host(np.int32, 4)
        r = out["runs"].setdefault(str(n_live), {})
        r["cand_ms_%d" % rnd] = ms; r["cand_us_per_step_%d" % rnd] = ms * 1e3 / steps
        r["last_step"] = {k: int(st[-1][k]) for k in ("n_fused", "n_spawned", "n_contested", "n_missed", "n_retired", "n_confirmed", "n_live")}
        r["next_id"] = int(meta[0])
        if not resident_only:
            host_loop(rec)                                                 # warm
            t0 = time.perf_counter()
            for _ in range(3):
                tab = host_loop(rec)
            r["host_loop_ms_%d" % rnd] = (time.perf_counter() - t0) / 3 * 1e3
            r["host_loop_live_at_end"] = int((tab["state"] != 0).sum())
        for a in (d_rec, d_steps, d_meta):
            if a is not None:
                a.free()
out["dispatches_per_step"] = 4
out["note"] = ("per step: k_cand_stage, k_assign_opt + k_assign_opt_big (frames of 16: the small kernel, the big one behind it finds no frame above 64), "
               "k_cand_update; one k_cand_init per run")
print(json.dumps(out))
G.close()
