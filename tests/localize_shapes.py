"""The purpose-made scenes of the frame localisation tests (TEST-ONLY).  One pose, 8 observations at about 10 m, 8 cones with a type each and zero
covariance, sigma_range = sigma_bearing = 0 and sigma_xy = 1, so that D = I; the prior heading is 0 (w = z bit for bit).  Cone i sits where
observation i falls from the TRUE pose, which differs from the prior by the scene's error; the hypothesis is index[i] = i unless stated.

    shift        prior (0, 0, 0), Sigma_p = diag(1, 1, 0), three pairs, the cones at z + (-1/2, 0): linear in t, d = 3 s / 4 = -3/8 after the
                 first solve and the second moves nothing: status 0, iterations 2.  With cones placed from the DEVICE's z every number is
                 exact in binary (z_x > 1/2, so z_x - 1/2 and z_x - 3/8 are representable): d, pose, cov = diag(1/4, 1/4, 0) and chi2 = 3/16 are asserted
                 as bits by the GPU test
    rotation     the true heading is 0.1 rad, Sigma_p = diag(2^-6, 2^-6, 1): one linear step leaves about r dtheta^2 / 2 = 5 cm per cone; the
                 default five iterations converge.  rotation_one (max_iterations 1) and rotation_limit (max_iterations 2) stop early with status 1
    wide         Sigma_p = 2^20 I, a small error in all three: the Woodbury form under a prior that says next to nothing
    singular     Sigma_p = diag(1, 0, 0), the error along x alone
    nocov        no pose covariance: no solve, chi2 = a at the prior
    none         every index -1: status 2
    one, two     one and two pairs: M alone is rank-deficient, the prior carries the rest
    nonfinite    cone 3 has a NaN position: that pair never counts
    nanquery     observation 2 has azimuth 0 (a NaN query): that pair never counts"""
import functools

import numpy as np

import assoc_exec as ax

LIDAR = 1.5
ZERO = np.zeros((1, 3))
POSE = np.array([[3.0, -2.0, 0.0]])
OBS = np.array([[35.0, 1.0, 8.0, 1.0], [50.0, -2.0, 11.5, 2.0], [-77.7, 0.0, 9.3, 3.0], [-9.25, 2.0, 12.0, 4.0],
                [20.5, 0.0, 11.0, 5.0], [33.0, 1.0, 10.25, 6.0], [-61.0, -1.0, 8.5, 7.0], [-70.0, 0.5, 9.75, 8.0]])
for _a in (ZERO, POSE, OBS):
    _a.setflags(write=False)
DIAG = lambda a, b, c: np.diag([a, b, c]).reshape(1, 9)
ALL = np.arange(8, dtype=np.int32)


def only(*keep):
    h = np.full(8, -1, dtype=np.int32); h[list(keep)] = list(keep)
    return h


# name: (prior pose, true pose - prior, Sigma_p, hypothesis, gs_loc_params fields, (status, iterations) or None where the reference decides)
SCENES = {
    "shift": (ZERO, (-0.5, 0.0, 0.0), DIAG(1.0, 1.0, 0.0), only(0, 1, 2), {}, (0, 2)),
    "rotation": (POSE, (0.0, 0.0, 0.1), DIAG(2.0 ** -6, 2.0 ** -6, 1.0), ALL, {}, None),
    "rotation_one": (POSE, (0.0, 0.0, 0.1), DIAG(2.0 ** -6, 2.0 ** -6, 1.0), ALL, dict(max_iterations=1), (1, 1)),
    "rotation_limit": (POSE, (0.0, 0.0, 0.1), DIAG(2.0 ** -6, 2.0 ** -6, 1.0), ALL, dict(max_iterations=2), (1, 2)),
    "wide": (POSE, (0.0625, -0.03125, 0.005), 2.0 ** 20 * np.eye(3).reshape(1, 9), ALL, {}, None),
    "singular": (POSE, (0.5, 0.0, 0.0), DIAG(1.0, 0.0, 0.0), ALL, {}, None),
    "nocov": (POSE, (0.25, 0.125, 0.0), None, ALL, {}, (0, 0)),
    "none": (POSE, (0.25, 0.0, 0.0), DIAG(1.0, 1.0, 2.0 ** -6), np.full(8, -1, dtype=np.int32), {}, (2, 0)),
    "one": (POSE, (0.0625, -0.03125, 0.0025), DIAG(1.0, 1.0, 2.0 ** -6), only(4), {}, None),
    "two": (POSE, (0.0625, -0.03125, 0.0025), DIAG(1.0, 1.0, 2.0 ** -6), only(1, 6), {}, None),
    "nonfinite": (POSE, (0.0625, -0.03125, 0.0025), DIAG(1.0, 1.0, 2.0 ** -6), ALL, {}, None),
    "nanquery": (POSE, (0.0625, -0.03125, 0.0025), DIAG(1.0, 1.0, 2.0 ** -6), ALL, {}, None),
}
NAMES = tuple(SCENES)
PARAMS = dict(sigma_range=0.0, sigma_bearing=0.0, sigma_xy=1.0, gate_chi2=1e9, max_distance=100.0)


def scene(name, z=None):
    """a case dict in assoc_nn_shapes' layout plus hyp, frame_start, loc (gs_loc_params fields) and expect.  z: the CoG-frame XY of OBS to place
    the cones from (the device's own, for the exact-bits scene); None: assoc_exec's"""
    return _scene(name) if z is None else _build(name, np.asarray(z, dtype=np.float64))


@functools.lru_cache(maxsize=None)
def _scene(name):
    return _build(name, ax.cone_to_global(ZERO, np.zeros(8, dtype=np.int32), OBS, LIDAR))


def _build(name, z):
    prior, err, pc, hyp, loc, expect = SCENES[name]
    obs = OBS
    if name == "nanquery":
        obs = OBS.copy(); obs[2, 0] = 0.0
    if name == "shift":                                                       # exactly z + (s, 0): nothing else is rounded
        xy = z + np.array([err[0], err[1]])
    else:
        th = prior[0, 2] + err[2]; c, s = np.cos(th), np.sin(th)
        xy = np.stack([z[:, 0] * c - z[:, 1] * s, z[:, 0] * s + z[:, 1] * c], axis=1) + (prior[0, :2] + np.array(err[:2]))
    if name == "nonfinite":
        xy[3, 0] = np.nan
    c = dict(lidar=LIDAR, poses=prior, pose_of=np.zeros(8, dtype=np.int32), obs=obs, map_xy=np.ascontiguousarray(xy), map_ty=np.arange(1, 9, dtype=np.int32),
             map_cov=None, pose_cov=pc, params=dict(PARAMS), hyp=hyp, frame_start=np.array([0, 8], dtype=np.int32), loc=dict(loc), expect=expect,
             name=name, truth=prior[0] + np.array(err))
    return c
