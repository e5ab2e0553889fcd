"""The purpose-made scenes of the frame following tests (TEST-ONLY): the smallest runs at which the new code can go wrong.

The world is relocalize_shapes.track(): 120 cones on two boundaries of a closed centre line whose 60 poses lie about 5 m apart — one cone spacing.
A car drives along those poses: frame t is seen from poses[at + t] as exact observations (relocalize_shapes.view), record t - 1 is the exact
motion between the two poses in the body frame of the earlier one.  Observations of type 7 ("junk") match no cone: they pad a frame to the sizes
at which the chain's kernels change path (64 / 65, 256) without contesting anything, and make frames that every hypothesis misses.

A scene is a dict: poses [h,3], covs [h,9] or None, frames (a list of [k,4] arrays), obs / frame_start (the same, concatenated), motion
[steps-1,3], motion_cov [steps-1,9] or None, map_xy, map_ty, map_cov (None), params (gs_nn_params fields), loc (gs_loc_params fields), follow
(gs_follow_params fields), lidar, name, and expect: {key: value} of what the scene is there for (checked by both test files where they can)."""
import functools

import numpy as np

import relocalize_shapes as rs

LIDAR = rs.LIDAR
PI = 3.14159265358979323846
AT = 7
COV0 = np.diag([0.1 ** 2, 0.1 ** 2, 0.02 ** 2]).reshape(9)
QU_DIAG = np.diag([0.05 ** 2, 0.05 ** 2, 0.01 ** 2]).reshape(9)
QU_FULL = np.array([2.5e-3, 4e-4, 1e-4, 4e-4, 2.5e-3, -2e-4, 1e-4, -2e-4, 1e-4])
JUNK = 7.0


def motion_between(p0, p1):
    """the odometry measurement from pose p0 to pose p1: the displacement in p0's body frame, the heading difference into [-pi, pi)"""
    c, s = np.cos(p0[2]), np.sin(p0[2]); d = p1[:2] - p0[:2]
    dth = (p1[2] - p0[2] + np.pi) % (2.0 * np.pi) - np.pi
    return np.array([c * d[0] + s * d[1], -s * d[0] + c * d[1], dth])


def junk(k, rng):
    """k observations of a type no cone has"""
    z = np.stack([rng.uniform(4.0, 30.0, k), rng.uniform(-15.0, 15.0, k)], axis=1)
    return rs.obs_of_xy(z, np.full(k, JUNK))


def frame_at(pose, k, rng, real=8):
    """a frame of k observations from `pose`: up to `real` exact views of the nearest cones ahead, the rest junk, shuffled"""
    xy, ty, _ = rs.track(); r = min(real, k)
    ob = rs.view(xy, ty, pose, r, rng)[0] if r else np.zeros((0, 4))
    ob = np.concatenate([ob, junk(k - len(ob), rng)]) if k > len(ob) else ob
    return np.ascontiguousarray(ob[rng.permutation(len(ob))])


def pack(name, poses, covs, frames, motion, motion_cov=None, params=None, loc=None, follow=None, expect=None, map_xy=None):
    xy, ty, _ = rs.track()
    frames = [np.ascontiguousarray(f, dtype=np.float64).reshape(-1, 4) for f in frames]
    fs = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int32)
    obs = np.concatenate(frames) if frames else np.zeros((0, 4))
    ns = len(frames)
    return dict(name=name, poses=np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3), covs=None if covs is None else np.ascontiguousarray(covs, dtype=np.float64).reshape(-1, 9),
                frames=frames, obs=np.ascontiguousarray(obs), frame_start=fs,
                motion=np.ascontiguousarray(motion, dtype=np.float64).reshape(-1, 3)[:max(ns - 1, 0)],
                motion_cov=None if motion_cov is None else np.ascontiguousarray(motion_cov, dtype=np.float64).reshape(-1, 9)[:max(ns - 1, 0)],
                map_xy=np.ascontiguousarray(xy if map_xy is None else map_xy), map_ty=np.ascontiguousarray(ty), map_cov=None,
                params=dict(params or {}), loc=dict(loc or {}), follow=dict(follow or {}), lidar=LIDAR, expect=dict(expect or {}))


def drive(name, n_hyp, sizes, seed=3, spread=0.5, covs="default", qu="diag", moving=True, hyp_poses=None, real=8, **kw):
    """the car over len(sizes) frames of the given sizes; hypothesis 0 is the true start, the others are scattered around it (or hyp_poses)"""
    _, _, cl = rs.track(); rng = np.random.default_rng(seed); ns = len(sizes)
    path = [cl[AT + (t if moving else 0)] for t in range(ns)]
    frames = [frame_at(path[t], sizes[t], rng, real) for t in range(ns)]
    motion = np.array([motion_between(path[t], path[t + 1]) for t in range(ns - 1)]).reshape(-1, 3)
    if hyp_poses is None:
        off = np.concatenate([np.zeros((1, 3)), np.stack([rng.normal(0, spread, n_hyp - 1), rng.normal(0, spread, n_hyp - 1), rng.normal(0, 0.03, n_hyp - 1)], axis=1)])
        hyp_poses = path[0] + off
    nh = len(hyp_poses)
    cv = None if covs is None else np.tile(COV0, (nh, 1)) if isinstance(covs, str) else covs
    mq = None if qu is None else np.tile(QU_DIAG if qu == "diag" else QU_FULL, (max(ns - 1, 1), 1))
    return pack(name, hyp_poses, cv, frames, motion, mq, **kw)


def _start():
    return np.array(rs.track()[2][AT])


def _wrap():
    p = _start(); rng = np.random.default_rng(11)
    poses = np.array([[p[0], p[1], 3.1], [p[0] + 5.0, p[1], PI], [p[0] + 10.0, p[1], -PI], [p[0] + 15.0, p[1], -3.1]])
    frames = [junk(3, rng), junk(2, rng), junk(2, rng)]
    motion = np.array([[0.5, 0.0, 0.1], [0.0, 0.25, -0.2]])
    return pack("wrap", poses, np.tile(COV0, (4, 1)), frames, motion, np.tile(QU_DIAG, (2, 1)), follow=dict(max_misses=9))


def _row3():
    p = _start(); c, s = np.cos(p[2]), np.sin(p[2])
    poses = np.array([p, p + [0.3 * c, 0.3 * s, 0.0], p + [0.6 * c, 0.6 * s, 0.0]])
    return pack("row3", poses, None, [np.zeros((0, 4))], np.zeros((0, 3)), expect=dict(state=[0, 2, 0], duplicate_of=[-1, 0, -1]))


def _lost_frozen():
    """a standing car at the true pose: three frames of junk lose it at step max_misses - 1; the real frames after it find it frozen"""
    p = _start(); rng = np.random.default_rng(5)
    frames = [junk(6, rng), junk(1, rng), junk(9, rng), frame_at(p, 8, rng), frame_at(p, 8, rng)]
    return pack("lost_frozen", [p], [COV0], frames, np.zeros((4, 3)), np.tile(QU_DIAG, (4, 1)), expect=dict(state=[1], state_step=[2], frames_hit=[0]))


def _miss_hit():
    p = _start(); rng = np.random.default_rng(6)
    frames = [frame_at(p, 8, rng), junk(5, rng), frame_at(p, 8, rng)]
    return pack("miss_hit", [p], [COV0], frames, np.zeros((2, 3)), np.tile(QU_DIAG, (2, 1)), expect=dict(state=[0], misses=[0], frames_hit=[2], frames_missed=[1]))


def _nan_pose():
    s = drive("nan_pose", 3, [8, 8], seed=8)
    s["poses"][1, 0] = np.nan; s["expect"] = dict(state=[0, 1, None])
    s["follow"] = dict(max_misses=2)
    return s


def _nan_obs():
    s = drive("nan_obs", 2, [8, 8], seed=9)
    s["obs"][2, 0] = 0.0; s["frames"][0][2, 0] = 0.0                              # azimuth 0: a NaN query
    return s


def _nan_cone():
    s = drive("nan_cone", 2, [8, 8], seed=10)
    xy = s["map_xy"].copy(); d = np.hypot(*(xy - s["poses"][0, :2]).T); xy[np.argsort(d)[1], 0] = np.nan
    s["map_xy"] = xy
    return s


def _truth():
    """12 steps along the track; the true start, the pose one cone spacing further along, a pose 30 m away towards the track's inside"""
    _, _, cl = rs.track(); p = cl[AT]; to_centre = -p[:2] / np.hypot(*p[:2])
    poses = np.array([p, cl[AT + 1], [p[0] + 30.0 * to_centre[0], p[1] + 30.0 * to_centre[1], p[2]]])
    return drive("truth", 3, [10] * 12, seed=21, hyp_poses=poses, real=10, expect=dict(best=0))


BUILDERS = {
    "h1_s1": lambda: drive("h1_s1", 1, [8]),
    "h2_s2": lambda: drive("h2_s2", 2, [8, 5]),
    "h63_s3": lambda: drive("h63_s3", 63, [8, 3, 9]),
    "h64_s12": lambda: drive("h64_s12", 64, [8, 5, 0, 12, 1, 7, 8, 2, 9, 4, 8, 6], spread=0.8),
    "empty_alone": lambda: drive("empty_alone", 2, [0]),
    "sizes": lambda: drive("sizes", 2, [1, 64, 0, 65, 256, 7], seed=4),
    "same_pose": lambda: drive("same_pose", 2, [8, 8], hyp_poses=np.array([_start(), _start()]), expect=dict(state=[0, 2], duplicate_of=[-1, 0], state_step=[-1, 0])),
    "row3": _row3,
    "lost_frozen": _lost_frozen,
    "miss_hit": _miss_hit,
    "wrap": _wrap,
    "qu_null": lambda: drive("qu_null", 3, [8, 8, 8], qu=None, seed=12),
    "qu_full": lambda: drive("qu_full", 3, [8, 8, 8], qu="full", seed=13),
    "cov_null": lambda: drive("cov_null", 3, [8, 8, 8], covs=None, seed=14),
    "nan_pose": _nan_pose,
    "nan_obs": _nan_obs,
    "nan_cone": _nan_cone,
    "min_pairs_high": lambda: drive("min_pairs_high", 2, [8, 8, 8], seed=15, follow=dict(min_pairs=50), expect=dict(state=[1, 1], frames_hit=[0, 0])),
    "one_iter": lambda: drive("one_iter", 2, [8, 8], seed=16, spread=0.05, loc=dict(max_iterations=1), follow=dict(merge_xy=0.0)),
    "truth": _truth,
}
NAMES = tuple(BUILDERS)


@functools.lru_cache(maxsize=None)
def scene(name):
    return BUILDERS[name]()
