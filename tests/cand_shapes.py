"""Scenes of the cone candidates (TEST-ONLY): the smallest shapes at which k_cand_stage / k_cand_update can still go wrong, and the truth scene.

A scene is a dict: records (the table to load, None: empty), poses [n_steps, 3], pose_covs [n_steps, 9] or None, frames (a list of [k, 4]
observations), in_idx (a list of [k] int32, or None: nothing is explained), obs / frame_start (the frames in one array), params (gs_nn_params
fields), cand (gs_cand_params fields), lidar.  Observations are built from global cone positions through the inverse of the A0 formula
(relocalize_shapes.obs_of_xy), so a cone seen twice from one pose gives the same bits twice.

Every position is placed with margin: cones of one frame are at least 4 m apart (above max_distance = 3: uncontested) unless the scene is about
contention; slots that a visibility test decides lie at least a centimetre from the view's range and cone — cand_ref rejects a scene that
does not keep its bands clear, and test_cand_cpu asserts that none is rejected.

THE TRUTH SCENE: relocalize_shapes.track() from its pose 7 on in quarter steps (about 1.4 m a frame), 25 frames.  The cones with an even index
are in the map (their observations are explained), the odd ones are to be discovered.  The sensor sees every cone with r < 14 m inside the
cone dx > 0.4 r of the CoG frame — wider than the candidates' view (12 m, cos 0.5), so that a candidate that counts as visible is one the
sensor does report.  Noise: range N(0, sigma_range), bearing N(0, sigma_bearing) at the CoG, then N(0, sigma_xy) per axis; zero Sigma_p; seed
fixed.  gate_chi2 is the 99.9 % point of chi-square with 2 degrees of freedom (13.8155...): with the 95 % gate one sighting in twenty would
fail its own candidate's gate and spawn a twin, which merging (not done) would have to clean up.  Three one-off false detections on the centre
line 8 m ahead.  spawn_range 67 m: no cone is anywhere near it."""
import functools

import numpy as np

import cand_ref as cr
import relocalize_shapes as rs

LIDAR = rs.LIDAR
PI = 3.14159265358979323846
POSE0 = np.array([3.0, -2.0, 0.7])
COV_DIAG = np.diag([0.04, 0.03, 0.0004]).reshape(9)
COV_FULL = np.array([0.04, 0.005, 0.001, 0.005, 0.03, -0.002, 0.001, -0.002, 0.0004])
GATE_999 = 13.815510557964274


def to_body(pose, xy):
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2); c, s = np.cos(pose[2]), np.sin(pose[2]); d = xy - pose[:2]
    return np.stack([d[:, 0] * c + d[:, 1] * s, -d[:, 0] * s + d[:, 1] * c], axis=1)


def see(pose, xy, ty):
    """the observations of global cones xy from pose (exact to rounding)"""
    return rs.obs_of_xy(to_body(pose, xy), ty)


def ahead(pose, z):
    """global positions of CoG-frame points z"""
    return rs.rot(pose, np.asarray(z, dtype=np.float64).reshape(-1, 2))


def grid_z(k, spacing=4.0, x0=4.0):
    """k CoG-frame points ahead of the car, `spacing` apart: rows of 16 across"""
    i = np.arange(k)
    return np.stack([x0 + spacing * (i // 16), spacing * ((i % 16) - 7.5)], axis=1)


def far_records(n, state=cr.CONFIRMED, first_id=0, skip=()):
    """n records on a grid 1 km away (seen by nobody, visible to nobody); the slots in `skip` are free"""
    rec = np.empty(n, dtype=cr.CAND)
    for s in range(n):
        rec[s] = cr.free_record() if s in skip else cr.record((1000.0 + 4.0 * (s % 32), 1000.0 + 4.0 * (s // 32)), type=1 + s % 2, id=first_id + s, state=state,
                                                              hits=3, confirm_step=0 if state == cr.CONFIRMED else -1)
    return rec


def pack(name, poses, frames, records=None, in_idx=None, pose_covs=None, params=None, cand=None):
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3); frames = [np.ascontiguousarray(f, dtype=np.float64).reshape(-1, 4) for f in frames]
    assert len(poses) == len(frames)
    obs = np.concatenate(frames) if frames else np.zeros((0, 4)); fs = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int32)
    ii = None if in_idx is None else [np.ascontiguousarray(a, dtype=np.int32) for a in in_idx]
    pc = None if pose_covs is None else np.ascontiguousarray(pose_covs, dtype=np.float64).reshape(-1, 9)
    assert pc is None or len(pc) == len(poses)
    return dict(name=name, poses=poses, frames=frames, obs=np.ascontiguousarray(obs), frame_start=fs, in_idx=ii,
                in_idx_all=None if ii is None else (np.concatenate(ii) if ii else np.zeros(0, dtype=np.int32)), pose_covs=pc,
                records=None if records is None else np.ascontiguousarray(records, dtype=cr.CAND), params=dict(params or {}),
                cand=cr.params_of(**dict(cand or {})), lidar=LIDAR)


def _sized(k):
    """a frame of k observations that all spawn, the same frame again (all fuse), an empty frame (the near ones are missed), the frame again"""
    xy = ahead(POSE0, grid_z(k)); ty = 1 + np.arange(k) % 3; f = see(POSE0, xy, ty)
    return pack("k%d" % k, [POSE0] * 4, [f, f, np.zeros((0, 4)), f], cand=dict(view_range=20.0))


def _steps(n):
    """runs of n steps over eight cones, two of which drop out after the first sighting"""
    xy = ahead(POSE0, grid_z(8)); ty = np.full(8, 2); f = see(POSE0, xy, ty)
    return pack("steps%d" % n, [POSE0] * n, [f if t % 4 != 1 else f[2:] for t in range(n)], cand=dict(view_range=40.0, view_cos=0.0))


def _wave_boundary():
    """66 observations of which only 63 and 64 are unexplained: two spawners in two waves"""
    xy = ahead(POSE0, grid_z(66)); f = see(POSE0, xy, np.full(66, 1)); ii = np.arange(66, dtype=np.int32); ii[63] = ii[64] = -1
    return pack("spawn_63_64", [POSE0] * 2, [f, f], in_idx=[ii, ii])


def _live(n_live, k=3):
    """a loaded table with n_live live slots and k spawners: above the free slots the rest is dropped"""
    free = () if n_live >= 1024 else (500,) if n_live == 1023 else ()
    rec = far_records(1024 if n_live >= 1023 else n_live, skip=free)
    f = see(POSE0, ahead(POSE0, grid_z(k)), np.full(k, 1))
    return pack("live%d" % n_live, [POSE0] * 2, [f, f], records=rec)


def _free_slots():
    """free slots only at 255, 256 and 1023 — across a thread, a wave and the table's end — and four spawners"""
    f = see(POSE0, ahead(POSE0, grid_z(4)), np.full(4, 2))
    return pack("free_255_256_1023", [POSE0] * 2, [f, f], records=far_records(1024, state=cr.TENTATIVE, skip=(255, 256, 1023)))


def _all_explained():
    f = see(POSE0, ahead(POSE0, grid_z(5)), np.full(5, 1))
    near = cr.record(ahead(POSE0, [[5.0, 0.5]])[0], id=4, misses=1)
    return pack("all_explained", [POSE0] * 2, [f, f], records=[near], in_idx=[np.arange(5), np.arange(5)])


def _retire_spawn():
    """slot 0 is one miss from retirement and visible; the spawner of the same step must take slot 1, the next step's slot 0"""
    doomed = cr.record(ahead(POSE0, [[6.0, 1.0]])[0], id=9, misses=2, last_step=4)
    f0 = see(POSE0, ahead(POSE0, [[9.0, -3.0]]), [1]); f1 = see(POSE0, ahead(POSE0, [[9.0, -3.0], [5.0, 5.0]]), [1, 2])
    return pack("retire_spawn", [POSE0] * 2, [f0, f1], records=[doomed])


def _confirm1():
    f = see(POSE0, ahead(POSE0, grid_z(3)), [1, 2, 1])
    return pack("confirm1", [POSE0] * 2, [f, f[:1]], cand=dict(confirm_hits=1))


def _all_round():
    """view_cos -1: the slots behind and abeam of the car are visible too (and one exactly behind: dx = -r)"""
    z = [[-5.0, 0.0], [0.0, 4.0], [-3.0, -3.0], [6.0, 0.0], [-20.0, 0.0]]
    rec = [cr.record(p, id=i) for i, p in enumerate(ahead(np.array([0.0, 0.0, 0.0]), z))]
    return pack("all_round", [[0.0, 0.0, 0.0]] * 3, [np.zeros((0, 4))] * 3, records=rec, cand=dict(view_cos=-1.0, max_misses=2))


def _cov(kind):
    pc = {"none": None, "diag": [COV_DIAG] * 3, "full": [COV_FULL] * 3}[kind]
    xy = ahead(POSE0, grid_z(6)); f = see(POSE0, xy, np.full(6, 1)); f2 = see(POSE0, xy + [0.05, -0.04], np.full(6, 1))
    return pack("cov_" + kind, [POSE0] * 3, [f, f2, f], pose_covs=pc)


def _nan_pose():
    f = see(POSE0, ahead(POSE0, grid_z(3)), [1, 1, 1])
    return pack("nan_pose", [POSE0, [np.nan, 0.0, 0.0], [0.0, 0.0, np.nan], POSE0], [f] * 4, cand=dict(view_range=30.0))


def _nan_obs():
    f = see(POSE0, ahead(POSE0, grid_z(5)), np.full(5, 1)); g = f.copy(); g[1, 0] = np.nan; g[2, 2] = np.nan; g[3, 0] = 0.0
    return pack("nan_obs", [POSE0] * 2, [g, f])


def _nan_record():
    """a loaded record with NaN xy is live, seen by nobody and visible to nobody: it stays as it is"""
    rec = [cr.record((np.nan, 1.0), id=0), cr.record(ahead(POSE0, [[6.0, 0.5]])[0], id=1), cr.record((np.nan, np.nan), id=2, state=cr.CONFIRMED, confirm_step=0)]
    f = see(POSE0, ahead(POSE0, [[6.0, 0.5], [10.0, 4.0]]), [1, 1])
    return pack("nan_record", [POSE0] * 2, [f, f[1:]], records=rec)


def _heading(sign):
    pose = np.array([2.0, 1.0, sign * PI]); xy = ahead(pose, grid_z(4)); f = see(pose, xy, np.full(4, 2))
    return pack("heading_%s_pi" % ("plus" if sign > 0 else "minus"), [pose] * 3, [f, f[:2], f], cand=dict(view_range=30.0))


def _contested():
    """two observations 0.4 m apart on either side of one candidate: one fuses, the other neither fuses nor spawns"""
    c = ahead(POSE0, [[8.0, 0.0]])[0]; rec = [cr.record(c, cov=(0.09, 0.0, 0.0, 0.09), id=3)]
    f = see(POSE0, ahead(POSE0, [[8.0, 0.15], [8.0, -0.25], [12.0, 6.0]]), [1, 1, 1])
    return pack("contested", [POSE0], [f], records=rec)


def _far():
    """beyond spawn_range (10 m at the lidar): counted far, nothing spawns; at 9 m one does"""
    f = see(POSE0, ahead(POSE0, [[10.0, 1.0], [14.0, 3.0], [30.0, -8.0]]), [1, 1, 1])
    return pack("far", [POSE0], [f], cand=dict(spawn_range=10.0))


def _type_mismatch():
    """an observation of another type on top of a candidate spawns beside it"""
    c = ahead(POSE0, [[7.0, 1.0]])[0]
    f = see(POSE0, [c, c], [2, 1])
    return pack("type_mismatch", [POSE0] * 2, [f[:1], f], records=[cr.record(c, type=1, id=0)])


@functools.lru_cache(maxsize=None)
def truth_world():
    xy, ty, cl = rs.track(); n = len(cl)
    poses = []
    for q in range(25):
        a, f = 7 + q // 4, (q % 4) / 4.0; p0, p1 = cl[a % n], cl[(a + 1) % n]
        dth = (p1[2] - p0[2] + PI) % (2 * PI) - PI
        poses.append([p0[0] + f * (p1[0] - p0[0]), p0[1] + f * (p1[1] - p0[1]), p0[2] + f * dth])
    return xy, ty, np.array(poses)


def _truth():
    xy, ty, poses = truth_world(); rng = np.random.default_rng(11); prm = dict(cr.nr.DEFAULTS); prm["gate_chi2"] = GATE_999
    mapped = np.arange(len(xy)) % 2 == 0; map_index = np.cumsum(mapped) - 1
    frames, in_idx, seen, false_at = [], [], [], {3: 0, 9: 1, 15: 2}
    for t, pose in enumerate(poses):
        z = to_body(pose, xy); r = np.hypot(z[:, 0], z[:, 1]); vis = np.flatnonzero((r < 14.0) & (z[:, 0] > 0.4 * r))
        rr = r[vis] + rng.normal(0.0, prm["sigma_range"], len(vis)); bb = np.arctan2(z[vis, 1], z[vis, 0]) + rng.normal(0.0, prm["sigma_bearing"], len(vis))
        zn = np.stack([rr * np.cos(bb), rr * np.sin(bb)], axis=1) + rng.normal(0.0, prm["sigma_xy"], (len(vis), 2))
        ob = rs.obs_of_xy(zn, ty[vis]); ii = np.where(mapped[vis], map_index[vis], -1).astype(np.int32); who = list(vis)
        if t in false_at:
            ob = np.concatenate([ob, rs.obs_of_xy([[8.0, 0.3]], [1])]); ii = np.concatenate([ii, [-1]]).astype(np.int32); who.append(-1 - false_at[t])
        frames.append(ob); in_idx.append(ii); seen.append(np.array(who))
    sc = pack("truth", poses, frames, in_idx=in_idx, params=dict(gate_chi2=GATE_999))
    sc.update(truth_xy=xy, truth_ty=ty, mapped=mapped, seen=seen, false_at=false_at)
    return sc


BUILDERS = {
    "k0": lambda: _sized(0), "k1": lambda: _sized(1), "k63": lambda: _sized(63), "k64": lambda: _sized(64), "k65": lambda: _sized(65), "k256": lambda: _sized(256),
    "steps1": lambda: _steps(1), "steps2": lambda: _steps(2), "steps3": lambda: _steps(3), "steps12": lambda: _steps(12),
    "spawn_63_64": _wave_boundary, "live1": lambda: _live(1), "live1023": lambda: _live(1023), "live1024": lambda: _live(1024),
    "free_255_256_1023": _free_slots, "all_explained": _all_explained, "retire_spawn": _retire_spawn, "confirm1": _confirm1, "all_round": _all_round,
    "cov_none": lambda: _cov("none"), "cov_diag": lambda: _cov("diag"), "cov_full": lambda: _cov("full"),
    "nan_pose": _nan_pose, "nan_obs": _nan_obs, "nan_record": _nan_record, "heading_plus_pi": lambda: _heading(1.0), "heading_minus_pi": lambda: _heading(-1.0),
    "contested": _contested, "far": _far, "type_mismatch": _type_mismatch, "truth": _truth,
}
NAMES = tuple(BUILDERS)


@functools.lru_cache(maxsize=None)
def scene(name):
    return BUILDERS[name]()


def nn_params_of(sc):
    p = dict(cr.nr.DEFAULTS); p.update(sc["params"])
    return p
