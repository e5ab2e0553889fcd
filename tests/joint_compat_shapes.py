"""The purpose-made scenes of the joint compatibility tests (TEST-ONLY).  One pose at heading 0, 8 observations, 8 cones with zero covariance,
cone i placed at observation i's global XY plus a chosen residual nu_i, the hypothesis index[i] = i; sigma_range = sigma_bearing = 0, so that
D = sigma_xy^2 I, and Sigma_p = diag(1, 1, 2^-6).  With heading 0 w = z bit for bit, so the device's whole computation is reproducible in numpy
fp64 from its own z and g (test_gpu_joint_compat.py does that); here the scenes are fixed numbers the exact reference decides.

Two REGIMES, because the gate decides what a residual of 1 m means:
    "s1"    sigma_xy = 1 and the table of confidence 2^-6.  Against 1 m of noise an alternating 1 m residual is unremarkable: J = 7.9 with 16
            degrees of freedom, far below the 95 % quantile 26.3 — at 0.95 nothing would be dropped, rightly.  The low confidence makes the
            gate bite (gate[8] = 6.4) while every number stays as stated: 1 m shifts, sigma_xy = 1.
    "s4"    sigma_xy = 2^-2 and the default table (0.95): the same residuals against 0.25 m of noise.  Still powers of two throughout.
Scenes (residuals in metres, x then y):
    common       all (1, 0): a pose error explains it; nothing is dropped and delta_x is close to the shift
    alternating  (+1, 0), (-1, 0), ...: every pair passes the per-pair gate of gs_associate_nn_batch WITH Sigma_p, the joint test drops pairs
    outlier      (1, 0) except pair 5 at (0, 16): that pair is dropped in one round
    outliers2    (1, 0) except pair 2 at (0, 16) and pair 6 at (0, -9): dropped in two rounds, the larger first
    hopeless     (+-(6 + i), 0) alternating: no subset passes, everything is dropped
    nocov        no pose covariance, residuals (0.25 (1 + i / 8), 0): nothing is dropped and J is the fixed-order sum of the pairs' d2"""
import functools

import numpy as np

import assoc_exec as ax

LIDAR = 1.5
POSE = np.array([[3.0, -2.0, 0.0]])
# (the azimuths' signs go + + - -, not + - + -: an alternating x residual that followed the side of the car would be a rotation, which Sigma_p explains)
# Every observation has a type of its own and cone i has observation i's: whatever the residuals, the only matching an assignment can find is
# index[i] = i, so that gs_frame_frontend_jc (which makes its own hypothesis) tests the same one as the other two calls.
OBS = np.array([[35.0, 1.0, 8.0, 1.0], [50.0, -2.0, 14.5, 2.0], [-77.7, 0.0, 3.3, 3.0], [-9.25, 2.0, 21.0, 4.0],
                [20.5, 0.0, 11.0, 5.0], [33.0, 1.0, 17.25, 6.0], [-61.0, -1.0, 6.5, 7.0], [-70.0, 0.5, 9.75, 8.0]])
POSE_COV = np.diag([1.0, 1.0, 2.0 ** -6]).reshape(1, 9)
REGIMES = {"s1": dict(sigma_xy=1.0, confidence=2.0 ** -6), "s4": dict(sigma_xy=0.25, confidence=0.95)}
SHIFT = np.tile([1.0, 0.0], (8, 1))
RESIDUALS = {
    "common": SHIFT,
    "alternating": SHIFT * np.where(np.arange(8) % 2 == 0, 1.0, -1.0)[:, None],
    "outlier": np.array([[0.0, 16.0] if i == 5 else [1.0, 0.0] for i in range(8)]),
    "outliers2": np.array([[0.0, 16.0] if i == 2 else [0.0, -9.0] if i == 6 else [1.0, 0.0] for i in range(8)]),
    "hopeless": np.array([[(6.0 + i) * (1.0 if i % 2 == 0 else -1.0), 0.0] for i in range(8)]),
    "nocov": np.array([[0.25 * (1.0 + i / 8.0), 0.0] for i in range(8)]),
}
for _a in (POSE, OBS, POSE_COV):
    _a.setflags(write=False)
NAMES = tuple((s, r) for s in RESIDUALS for r in REGIMES)


@functools.lru_cache(maxsize=None)
def scene(name, regime):
    """a case dict in assoc_nn_shapes' layout plus hyp, frame_start and confidence"""
    g = ax.cone_to_global(POSE, np.zeros(8, dtype=np.int32), OBS, LIDAR)
    reg = REGIMES[regime]
    c = dict(lidar=LIDAR, poses=POSE, pose_of=np.zeros(8, dtype=np.int32), obs=OBS, map_xy=np.ascontiguousarray(g + RESIDUALS[name]),
             map_ty=np.arange(1, 9, dtype=np.int32), map_cov=None, pose_cov=None if name == "nocov" else POSE_COV,
             params=dict(sigma_range=0.0, sigma_bearing=0.0, sigma_xy=reg["sigma_xy"], gate_chi2=5.991464547107979, max_distance=3.0),
             hyp=np.arange(8, dtype=np.int32), frame_start=np.array([0, 8], dtype=np.int32), confidence=reg["confidence"], name=name, regime=regime)
    for a in ("map_xy", "map_ty", "hyp", "frame_start"):
        c[a].setflags(write=False)
    return c


# what each scene is for: (kept positions, positions in the order they leave); None = not prescribed, the reference decides
EXPECT = {
    "common": (list(range(8)), []),
    "alternating": None,
    "outlier": ([0, 1, 2, 3, 4, 6, 7], [5]),
    "outliers2": ([0, 1, 3, 4, 5, 7], [2, 6]),
    "hopeless": ([], None),
    "nocov": (list(range(8)), []),
}
