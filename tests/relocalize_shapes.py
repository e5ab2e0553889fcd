"""The purpose-made scenes of the relocalisation tests (TEST-ONLY).  A scene is a dict: obs [n, 4] (collector layout), frame_start, map_xy, map_ty,
params (gs_reloc_params fields that differ from the defaults), slice (gs_debug_relocalize: the cones p a workgroup enumerates, 0 = the
launcher's choice), status (per frame, what the scene was made for; None = the reference's) and truth: per frame None or (pose, index) — the
pose the frame was synthesised from and the cone every observation then falls on exactly (-1: a spurious one).

Where a scene needs EXACT geometry its cones are placed from z, the CoG-frame XY of its observations: scene(name, zfun) takes the function
obs -> z (the device's own gs_polar_to_xy_batch on the GPU, assoc_exec's numpy A0 otherwise), so that "the cone sits where the observation
falls" holds for the bits the device works with.

    small_frames   frames of 0 and 1 observations and one of 2 whose baseline is below min_baseline: status 2 each
    two_on_two     a frame of 2 on a map of 2 same-type cones: two seeds (p, q) and (q, p), count 2: status 1; the runner-up is the flipped pose
    track8         a closed track of 120 cones (two boundaries, 0.3 m jitter), a frame of 8 of which 2 are spurious: status 0
    twelve, thirteen   frames of 12 and 13 at seed_obs 12
    equal_r2       observations 1 and 2 are mirror images (equal r2 bit for bit), seed_obs 2 cuts between them: the lower index is the seed
    map1023, map1024, map1025, map2049   the track plus far cones up to that size (2049: scored through the grid as the calls choose)
    frame64, frame65, frame256           frames of that many observations on a field of as many cones
    line<N>        N equally spaced same-type cones on a line, a frame of 2 three spacings apart: 2 (N - 3) equal-length seeds; the whole map
                   in ONE workgroup (slice = N), so that a wave's rings of 128 (drained at 64) see the fills ring_fill() lists
    line300s       the same 300 cones in slices of 16: 19 records a frame
    square         four same-type cones on a square of 3 m: forty seeds, eight poses of count 4, costs equal to rounding; second_count == count
    twins          the square with every cone AND every observation doubled: seeds whose keys tie exactly in (count, cost) and differ only in
                   (u, v, p, q) — the order the key is strict in
    heading_pi, heading_minus   the truth's heading is exactly pi (s = +0, c = -1: cones at t - z) and -3.1
    nan_cone       a cone of the frame has a NaN position;  nan_query: an observation has azimuth 0 (NaN z)
    hundred        100 frames of 5 .. 9 observations along the track, two spurious each"""
import functools

import numpy as np

import assoc_exec as ax

LIDAR = 1.5
R2D = 1.0 / ax.K_D2R


def default_z(obs):
    obs = np.asarray(obs, dtype=np.float64).reshape(-1, 4)
    return ax.polar_to_xy(obs[:, 0], obs[:, 1], obs[:, 2], LIDAR)


def obs_of_xy(xy, ty):
    """collector observations (zenith 0) whose CoG-frame XY is xy to within rounding: the inverse of the A0 formula"""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    xl = xy[:, 0] - LIDAR
    return np.stack([np.arctan2(xy[:, 1], xl) * R2D, np.zeros(len(xy)), np.hypot(xl, xy[:, 1]), np.asarray(ty, dtype=np.float64)], axis=1)


def rot(pose, z):
    c, s = np.cos(pose[2]), np.sin(pose[2])
    return np.stack([z[:, 0] * c - z[:, 1] * s + pose[0], z[:, 0] * s + z[:, 1] * c + pose[1]], axis=1)


@functools.lru_cache(maxsize=None)
def track():
    """120 cones: 60 left (type 1) and 60 right (type 2) of a closed centre line, 0.3 m jitter; also the centre line's poses"""
    rng = np.random.default_rng(27)
    a = np.linspace(0.0, 2.0 * np.pi, 60, endpoint=False)
    cx, cy = 55.0 * np.cos(a) + 9.0 * np.cos(3 * a), 35.0 * np.sin(a) + 6.0 * np.sin(2 * a)
    dx, dy = np.gradient(cx), np.gradient(cy); nrm = np.hypot(dx, dy); nx, ny = -dy / nrm, dx / nrm
    left = np.stack([cx + 1.8 * nx, cy + 1.8 * ny], axis=1); right = np.stack([cx - 1.8 * nx, cy - 1.8 * ny], axis=1)
    xy = np.concatenate([left, right]) + rng.uniform(-0.3, 0.3, (120, 2))
    ty = np.concatenate([np.full(60, 1), np.full(60, 2)]).astype(np.int32)
    poses = np.stack([cx, cy, np.arctan2(dy, dx)], axis=1)
    xy.setflags(write=False); ty.setflags(write=False); poses.setflags(write=False)
    return xy, ty, poses


def view(xy, ty, pose, k, rng, spurious=0):
    """the k nearest cones ahead of `pose` as exact observations (in a shuffled order), then `spurious` more that fall on nothing: (obs, index)"""
    c, s = np.cos(pose[2]), np.sin(pose[2]); d = xy - pose[:2]
    z = np.stack([d[:, 0] * c + d[:, 1] * s, -d[:, 0] * s + d[:, 1] * c], axis=1)
    ahead = np.nonzero(z[:, 0] > LIDAR + 1.0)[0]
    near = ahead[np.argsort((z[ahead] ** 2).sum(1))[:k]]; near = near[rng.permutation(len(near))]
    ob = obs_of_xy(z[near], ty[near]); idx = list(near)
    for _ in range(spurious):
        while True:
            zs = np.array([rng.uniform(4.0, 14.0), rng.uniform(-7.0, 7.0)]); g = rot(pose, zs[None])[0]
            if np.hypot(*(xy - g).T).min() > 1.5:
                break
        ob = np.concatenate([ob, obs_of_xy(zs[None], [rng.integers(1, 3)])]); idx.append(-1)
    return ob, np.array(idx, dtype=np.int32)


def _one(obs, map_xy, map_ty, truth=None, status=None, params=None, slice_=0):
    obs = np.ascontiguousarray(obs, dtype=np.float64).reshape(-1, 4)
    return dict(obs=obs, frame_start=np.array([0, len(obs)], dtype=np.int32), map_xy=np.ascontiguousarray(map_xy, dtype=np.float64).reshape(-1, 2),
                map_ty=np.ascontiguousarray(map_ty, dtype=np.int32), params=dict(params or {}), slice=slice_, status=[status], truth=[truth])


def _track_frame(k, spurious, at=7, seed=5, extra=0, params=None):
    xy, ty, poses = track(); rng = np.random.default_rng(seed)
    pose = poses[at] + np.array([0.4, -0.3, 0.05])
    ob, idx = view(xy, ty, pose, k, rng, spurious)
    if extra:                                                                    # far cones: they lengthen the enumeration, no frame sees them
        far = np.stack([rng.uniform(200.0, 900.0, extra), rng.uniform(-400.0, 400.0, extra)], axis=1)
        xy = np.concatenate([xy, far]); ty = np.concatenate([ty, rng.integers(1, 3, extra).astype(np.int32)])
    return _one(ob, xy, ty, (pose, idx), 0, params)


OBS2 = np.array([[25.0, 0.0, 6.0, 1.0], [-40.0, 1.0, 9.0, 1.0]])
SQUARE = np.array([[4.0, 1.5], [7.0, 1.5], [7.0, -1.5], [4.0, -1.5]])           # the corners in the CoG frame: sides of 3 m
POSE = np.array([3.0, -2.0, 0.7])


def _field(k, zfun, seed):
    """k observations scattered ahead, a cone of one of four types under each, seen from POSE"""
    rng = np.random.default_rng(seed); side = np.sqrt(40.0 * k); zs = np.zeros((0, 2))
    while len(zs) < k:                                                           # 40 m2 a cone, no two within 1.2 m
        z1 = np.array([rng.uniform(3.0, 3.0 + side), rng.uniform(-0.5 * side, 0.5 * side)])
        if len(zs) == 0 or np.hypot(*(zs - z1).T).min() > 1.2:
            zs = np.concatenate([zs, z1[None]])
    t = rng.integers(1, 5, k)
    ob = obs_of_xy(zs, t)
    return _one(ob, rot(POSE, zfun(ob)), t, (POSE, np.arange(k, dtype=np.int32)), 0)


def _line(n, zfun, slice_):
    z = zfun(OBS2); d = (z[1] - z[0]) / 3.0                                     # three spacings between the two observations
    pose0 = z[0] - 5 * d if n > 8 else z[0]                                      # observation 0 falls on cone 5 (cone 0 on the short lines)
    xy = pose0[None, :] + np.arange(n)[:, None] * d[None, :]
    return _one(OBS2, xy, np.ones(n, dtype=np.int32), truth=None, status=1 if n >= 4 else 2, slice_=slice_)      # (every pose along the line fits: no truth to hold)


LINES = (3, 4, 5, 35, 36, 65, 67, 97, 98, 131, 300)


def ring_fill(n, k=3, slice_=None):
    """the candidates |p - q| == k a wave of the seed kernel meets, per (slice, wave): lane q of wave w holds the cones q = 256 m + 64 w + lane"""
    slice_ = n if not slice_ else slice_
    out = []
    for p0 in range(0, n, slice_):
        for w in range(4):
            out.append(sum(1 for p in range(p0, min(n, p0 + slice_)) for q in (p - k, p + k) if 0 <= q < n and (q % 256) // 64 == w))
    return out


def _small_frames(zfun):
    xy, ty, poses = track()
    ob = np.array([[30.0, 0.0, 7.0, 1.0], [10.0, 0.0, 5.0, 1.0], [12.0, 0.0, 5.5, 2.0]])       # the last two lie 0.55 m apart
    c = _one(ob, xy[:6], ty[:6]); c["frame_start"] = np.array([0, 0, 1, 3], dtype=np.int32); c["status"] = [2, 2, 2]; c["truth"] = [None] * 3
    return c


def _two_on_two(zfun):
    return _one(OBS2, rot(POSE, zfun(OBS2)), [1, 1], None, 1)                 # (the pose and its flip fit equally well: no truth to hold)


def _equal_r2(zfun):
    # r2: observation 0 the smallest, 1 and 2 equal (mirror images), 3 and 4 farther; seed_obs 2 takes 0 and 1.  Cones under 0, 1, 3, 4 and
    # NOT under 2: were 2 the seed instead of 1 the pair (0, 2) would find no cone pair of its length
    ob = np.array([[5.0, 0.0, 4.0, 1.0], [35.0, 0.0, 8.0, 1.0], [-35.0, 0.0, 8.0, 1.0], [20.0, 0.0, 11.0, 1.0], [-15.0, 0.0, 12.0, 1.0]])
    g = rot(POSE, zfun(ob))
    return _one(ob, g[[0, 1, 3, 4]], [1, 1, 1, 1], (POSE, np.array([0, 1, -1, 2, 3], dtype=np.int32)), 0, dict(seed_obs=2))


def _square(zfun, twins=False):
    ob = obs_of_xy(SQUARE, [1, 1, 1, 1]); g = rot(POSE, zfun(ob)); idx = np.arange(4, dtype=np.int32)
    if twins:
        ob = np.repeat(ob, 2, axis=0); g = np.repeat(g, 2, axis=0); idx = np.repeat(2 * idx, 2)        # the lowest of two equal cones
    return _one(ob, g, np.ones(len(g), dtype=np.int32), (POSE, idx), 0)


def _heading(zfun, exact_pi):
    ob = _track_frame(8, 0)["obs"]; z = zfun(ob)
    if exact_pi:
        t = np.array([12.0, -7.0]); g = t[None, :] - z; pose = np.array([t[0], t[1], np.pi])           # R(pi) z = -z exactly
    else:
        pose = np.array([12.0, -7.0, -3.1]); g = rot(pose, z)
    return _one(ob, g, ob[:, 3].astype(np.int32), (pose, np.arange(8, dtype=np.int32)), 0)


def _nan_cone(zfun):
    c = _track_frame(8, 0); xy = c["map_xy"].copy(); hit = int(c["truth"][0][1][2]); xy[hit] = np.nan
    idx = c["truth"][0][1].copy(); idx[2] = -1
    c["map_xy"] = xy; c["truth"] = [(c["truth"][0][0], idx)]
    return c


def _nan_query(zfun):
    c = _track_frame(8, 0); ob = c["obs"].copy(); ob[3, 0] = 0.0
    idx = c["truth"][0][1].copy(); idx[3] = -1
    c["obs"] = ob; c["truth"] = [(c["truth"][0][0], idx)]
    return c


def _hundred(zfun):
    xy, ty, poses = track(); rng = np.random.default_rng(100)
    obs, fs, truth = [], [0], []
    for f in range(100):
        pose = poses[rng.integers(0, 60)] + np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.uniform(-0.1, 0.1)])
        ob, idx = view(xy, ty, pose, int(rng.integers(5, 10)), rng, 2)
        obs.append(ob); fs.append(fs[-1] + len(ob)); truth.append((pose, idx))
    c = _one(np.concatenate(obs), xy, ty)
    c["frame_start"] = np.array(fs, dtype=np.int32); c["truth"] = truth; c["status"] = [None] * 100
    return c


BUILDERS = {
    "small_frames": _small_frames,
    "two_on_two": _two_on_two,
    "track8": lambda zfun: _track_frame(6, 2),
    "twelve": lambda zfun: _track_frame(10, 2, at=21, seed=12),
    "thirteen": lambda zfun: _track_frame(11, 2, at=33, seed=13),
    "equal_r2": _equal_r2,
    "map1023": lambda zfun: _track_frame(6, 2, extra=1023 - 120),
    "map1024": lambda zfun: _track_frame(6, 2, extra=1024 - 120),
    "map1025": lambda zfun: _track_frame(6, 2, extra=1025 - 120),
    "map2049": lambda zfun: _track_frame(6, 2, extra=2049 - 120),
    "frame64": lambda zfun: _field(64, zfun, 64),
    "frame65": lambda zfun: _field(65, zfun, 65),
    "frame256": lambda zfun: _field(256, zfun, 256),
    "line300s": lambda zfun: _line(300, zfun, 16),
    "square": _square,
    "twins": lambda zfun: _square(zfun, twins=True),
    "heading_pi": lambda zfun: _heading(zfun, True),
    "heading_minus": lambda zfun: _heading(zfun, False),
    "nan_cone": _nan_cone,
    "nan_query": _nan_query,
    "hundred": _hundred,
}
for _n in LINES:
    BUILDERS["line%d" % _n] = (lambda n: lambda zfun: _line(n, zfun, n))(_n)
NAMES = tuple(BUILDERS)


def scene(name, zfun=None):
    c = BUILDERS[name](default_z if zfun is None else zfun)
    c["name"] = name
    return c
