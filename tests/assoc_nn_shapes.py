"""The cases of the covariance-gated association tests (TEST-ONLY): small scenes — at most 600 queries and 2304 cones — that between them reach
every place the kernels of gs_assoc_nn.hip can go wrong; test_assoc_nn_cpu.py holds the census that proves what each one reaches.

A case is a dict: lidar, poses [P, 3], pose_of [n], obs [n, 4] (az, zen, dist, type), map_xy [m, 2], map_ty [m], map_cov [m, 4] or None,
pose_cov [P, 9] or None, params (the gs_nn_params fields that differ from the defaults), family, tie (built to tie), notes.  Observations are
drawn first (|az| <= 80 degrees: far from the abeam branch point of A0) and cones are then placed RELATIVE TO the observations' global XY, so
what a query sees is there by construction whatever the pose.  Map sizes sit on the edges of the kernels' paths: the LDS tile of 1024
(1023 / 1024 / 1025), the grid switch of the batch call (2047 / 2048), the 256-thread workgroup (255 / 256 / 257 queries), the frame kernel's
wave (k = 1, 64, 65)."""
import functools

import numpy as np

import assoc_exec as ax
import assoc_nn_ref as nr

LIDAR = 1.5
FAR = 1.0e5


def spd(rng, k, lo=0.01, hi=0.5):
    """k symmetric positive definite 2x2 blocks with eigenvalues in [lo, hi], bitwise symmetric"""
    a = rng.uniform(0, np.pi, k); l1 = rng.uniform(lo, hi, k); l2 = rng.uniform(lo, hi, k)
    c, s = np.cos(a), np.sin(a); off = (l1 - l2) * c * s
    return np.stack([l1 * c * c + l2 * s * s, off, off, l1 * s * s + l2 * c * c], axis=1)


def pose_covs(rng, k):
    out = np.zeros((k, 9))
    for p in range(k):
        A = rng.normal(size=(3, 3)) * np.array([0.2, 0.2, 0.03]); S = A.T @ A
        out[p] = ((S + S.T) / 2).reshape(9)
    return out


def _obs(rng, n, dist=(3.0, 25.0)):
    az = rng.uniform(2.0, 80.0, n) * rng.choice([-1.0, 1.0], n)
    return np.stack([az, rng.uniform(-3, 3, n), rng.uniform(dist[0], dist[1], n), rng.integers(1, 5, n).astype(np.float64)], axis=1)


def scene(seed, n, n_map, n_poses=2, spread=40.0, attach=0.7, with_pose_cov=True, params=None, centre=(0.0, 0.0), obs=None):
    """poses within 15 m of `centre`, n observations, n_map cones uniform within `spread` with random covariances; `attach` of the queries get a
    cone of their own 0.6 m (sigma) from their global XY, nine in ten of the query's type"""
    rng = np.random.default_rng(seed)
    poses = np.concatenate([np.asarray(centre) + rng.uniform(-15, 15, (n_poses, 2)), rng.uniform(-3, 3, (n_poses, 1))], axis=1)
    ob = _obs(rng, n) if obs is None else np.asarray(obs, dtype=np.float64)
    n = len(ob)
    pose_of = rng.integers(0, n_poses, n).astype(np.int32)
    g = ax.cone_to_global(poses, pose_of, ob, LIDAR)
    mxy = np.asarray(centre) + rng.uniform(-spread, spread, (n_map, 2)); mty = rng.integers(1, 5, n_map).astype(np.int32)
    if n_map:
        own = rng.permutation(n_map)[:n]
        for i, j in enumerate(own):
            if rng.uniform() < attach and np.isfinite(g[i]).all():
                mxy[j] = g[i] + rng.normal(size=2) * 0.6
                mty[j] = int(ob[i, 3]) if rng.uniform() < 0.9 else int(ob[i, 3]) % 4 + 1
    return dict(lidar=LIDAR, poses=poses, pose_of=pose_of, obs=ob, map_xy=mxy, map_ty=mty, map_cov=spd(rng, n_map),
                pose_cov=pose_covs(rng, n_poses) if with_pose_cov else None, params=dict(params or {}), gxy=g, family="shape", tie=False, notes={})


def plant(c, j, i, offset, cov=None, dty=0):
    """cone j becomes a cone of query i's type + dty at query i's global XY + offset (metres), with covariance cov (4 numbers) if given"""
    c["map_xy"][j] = c["gxy"][i] + np.asarray(offset, dtype=np.float64); c["map_ty"][j] = int(c["obs"][i, 3]) + dty
    if cov is not None:
        c["map_cov"][j] = cov


def _own_types(c, k):
    """queries 0 .. k-1 get types of their own (7, 12, ...), which no random cone has: what they match is planted"""
    c["obs"][:k, 3] = 7 + 5 * np.arange(k)


# ---- grid placement (the cell edge is max_distance (1 + 1e-9), assoc_exec.inv_cell_of)
def _grid_border():
    """cones exactly on cell borders (x or y a multiple of the cell edge as the device computes it, and the fp64 neighbour of that), inside the gate or not"""
    c = scene(24, 120, 0, centre=(-7.0, 5.0)); md = 3.0
    rng = np.random.default_rng(24); cell = 1.0 / ax.inv_cell_of(md)
    xy, ty = [], []
    for i in range(len(c["obs"])):
        g = c["gxy"][i]; k = np.round(g / cell)
        for mode in range(3):
            r = md * (0.3 if rng.uniform() < 0.5 else 0.9); p = g.copy(); a = mode % 2
            p[a] = k[a] * cell
            if mode == 2:
                p[a] = np.nextafter(p[a], rng.choice([-np.inf, np.inf]))
            if abs(p[a] - g[a]) < r:
                p[1 - a] = g[1 - a] + rng.choice([-1.0, 1.0]) * np.sqrt(r * r - (p[a] - g[a]) ** 2)
            xy.append(p); ty.append(int(c["obs"][i, 3]))
    order = rng.permutation(len(xy))
    c["map_xy"] = np.array(xy)[order]; c["map_ty"] = np.array(ty, dtype=np.int32)[order]; c["map_cov"] = spd(rng, len(xy))
    return c


def _grid_diag():
    """every query has ONE cone of its own type, in the diagonally adjacent cell past its nearest cell corner"""
    c = scene(25, 80, 300, centre=(-40.0, -30.0)); cell = 1.0 / ax.inv_cell_of(3.0)
    _own_types(c, 80)
    for i in range(80):
        g = c["gxy"][i]; f = g / cell - np.floor(g / cell); s = np.where(f >= 0.5, 1.0, -1.0)
        corner = (np.floor(g / cell) + (s > 0)) * cell
        c["map_xy"][3 * i] = corner + s * 0.01 * cell; c["map_ty"][3 * i] = int(c["obs"][i, 3])
    c["notes"]["expect_cone"] = {i: 3 * i for i in range(80)}              # the only cone of the query's type: that one or none
    return c


def _grid_crowd():
    c = scene(26, 50, 800); rng = np.random.default_rng(26)
    _own_types(c, 1)
    for j in range(100, 600):                                                # 500 cones within 0.3 m of one point, a quarter of them of the query's type
        plant(c, j, 0, rng.uniform(-0.3, 0.3, 2) + (0.4, 0.0), dty=0 if j % 4 == 0 else 1)
    return c


def _grid_collide():
    """far cones of the query's type in cells that hash to the buckets of the query's own nine cells: candidates that fail the Euclidean test"""
    c = scene(27, 40, 600); _own_types(c, 2)
    inv = ax.inv_cell_of(3.0); mask = ax.buckets_of(600) - 1; cell = 1.0 / inv
    a, b = np.meshgrid(np.arange(-400, 400), np.arange(-400, 400), indexing="ij")
    H = ax.grid_bucket(a, b, mask); j = 100
    for i in range(2):
        g = c["gxy"][i]; cx, cy = int(ax.grid_coord(g[0], inv)), int(ax.grid_coord(g[1], inv))
        for k in range(9):
            t = int(ax.grid_bucket(cx + k % 3 - 1, cy + k // 3 - 1, mask))
            hits = np.argwhere((H == t) & ((np.abs(a - cx) > 50) | (np.abs(b - cy) > 50)))
            assert len(hits), "no far cell hashes to the bucket"
            for h in hits[:2]:
                c["map_xy"][j] = ((h[0] - 400) + 0.5) * cell, ((h[1] - 400) + 0.5) * cell; c["map_ty"][j] = int(c["obs"][i, 3]); j += 1
        plant(c, 90 + i, i, (0.5, -0.3))
    c["notes"]["expect"] = {0: 90, 1: 91}; c["notes"]["colliders"] = j - 100
    return c


def nine_buckets(g, n_map, md=3.0):
    """the buckets of the 3 x 3 cells around g, in the kernel's order"""
    inv = ax.inv_cell_of(md); mask = ax.buckets_of(n_map) - 1
    cx, cy = int(ax.grid_coord(g[0], inv)), int(ax.grid_coord(g[1], inv))
    return [int(ax.grid_bucket(cx + k % 3 - 1, cy + k // 3 - 1, mask)) for k in range(9)]


def _grid_twice():
    """TWO of a query's nine cells hash to ONE bucket, and its only cone sits in one of them: a kernel that walks the bucket once per cell
    meets the cone twice and reports it as its own runner-up (second_d2 == d2 where +inf is due).  One pose with heading 0, moved so that the
    queries' global XY land in such cells"""
    n = 6; c = scene(29, n, 500, n_poses=n, attach=0.0); _own_types(c, n)
    c["poses"][:, 2] = 0.0; c["pose_of"] = np.arange(n, dtype=np.int32)
    inv = ax.inv_cell_of(3.0); mask = ax.buckets_of(500) - 1; cell = 1.0 / inv
    a, b = np.meshgrid(np.arange(-300, 300), np.arange(-300, 300), indexing="ij")
    H = [ax.grid_bucket(a + k % 3 - 1, b + k // 3 - 1, mask) for k in range(9)]
    found = []
    for k in range(9):
        for m in range(k):
            for h in np.argwhere(H[k] == H[m])[:2]:
                found.append((h[0] - 300, h[1] - 300, k if k != 4 else m))
    assert len(found) >= n, "no cell with two neighbours in one bucket"
    z = ax.polar_to_xy(c["obs"][:, 0], c["obs"][:, 1], c["obs"][:, 2], LIDAR)
    for i, (cx, cy, k) in enumerate(found[::max(1, len(found) // n)][:n]):
        d = np.array([k % 3 - 1, k // 3 - 1], dtype=np.float64)
        centre = (np.array([cx, cy]) + 0.5) * cell
        c["poses"][i, :2] = centre + 0.4 * cell * d - z[i]
        c["map_xy"][10 + i] = centre + 0.6 * cell * d; c["map_ty"][10 + i] = int(c["obs"][i, 3])
    c["gxy"] = ax.cone_to_global(c["poses"], c["pose_of"], c["obs"], LIDAR)
    c["notes"]["expect_cone"] = {i: 10 + i for i in range(n)}; c["notes"]["alone"] = list(range(n))
    return c


def _nonfinite():
    c = scene(28, 60, 400, n_poses=3); _own_types(c, 1)
    for j, p in {2: (np.nan, 3.0), 3: (np.inf, -8.0), 17: (4.0, -np.inf), 40: (np.nan, np.nan), 41: (-np.inf, np.inf), 399: (1.0, np.nan)}.items():
        c["map_xy"][j] = p; c["map_ty"][j] = int(c["obs"][0, 3])
    plant(c, 300, 0, (0.2, 0.1))
    c["notes"]["expect"] = {0: 300}
    return c


# ---- covariance and type
def _type_mismatch():
    c = scene(31, 20, 100, attach=0.0); _own_types(c, 1)
    plant(c, 5, 0, (0.1, 0.0), dty=1); plant(c, 9, 0, (0.6, 0.2))            # the nearest cone has another type
    c["notes"]["expect"] = {0: 9}
    return c


def _elongated():
    """cone 4 at 0.2 m with a small round covariance, cone 8 at 1.5 m with a covariance elongated towards the query: the Mahalanobis winner is
    NOT the Euclidean nearest (small sigmas, no pose covariance: S is the cone's own covariance to a few per cent)"""
    c = scene(32, 20, 100, attach=0.0, with_pose_cov=False, params=dict(sigma_range=0.05, sigma_bearing=0.001, sigma_xy=0.05)); _own_types(c, 1)
    plant(c, 4, 0, (0.2, 0.0), cov=(0.01, 0.0, 0.0, 0.01)); plant(c, 8, 0, (1.5, 0.0), cov=(4.0, 0.0, 0.0, 0.01))
    c["notes"]["expect"] = {0: 8}; c["notes"]["euclid_nearest"] = {0: 4}
    return c


def _heading():
    """a cone 2.5 m ACROSS the ray of a query at 20 m: far outside the gate for the measurement noise alone, admitted by a heading variance of
    0.05 rad^2 (P adds 0.05 * 400 m^2 across the ray).  notes.without: the same case without pose covariances, where it must be -1"""
    ob = np.array([[30.0, 0.0, 20.0, 7.0], [-20.0, 1.0, 20.0, 12.0]])
    c = scene(33, 2, 50, n_poses=1, attach=0.0, obs=ob)
    c["pose_cov"] = np.array([[1e-4, 0, 0, 0, 1e-4, 0, 0, 0, 0.05]])
    for i in range(2):
        w = c["gxy"][i] - c["poses"][0, :2]; wp = np.array([-w[1], w[0]]) / np.hypot(*w)
        plant(c, 10 + i, i, 2.5 * wp, cov=(0.01, 0.0, 0.0, 0.01))
    c["notes"]["expect"] = {0: 10, 1: 11}; c["notes"]["without_pose_cov"] = {0: -1, 1: -1}
    return c


def _indefinite():
    """all sigmas 0: S is the cone's block alone.  Cone 3 (nearest) has an indefinite symmetric block: skipped; cone 6 a proper one: taken"""
    c = scene(34, 10, 60, attach=0.0, with_pose_cov=False, params=dict(sigma_range=0.0, sigma_bearing=0.0, sigma_xy=0.0)); _own_types(c, 2)
    plant(c, 3, 0, (0.3, 0.0), cov=(1.0, 2.0, 2.0, 1.0)); plant(c, 6, 0, (0.5, 0.0), cov=(0.1, 0.0, 0.0, 0.1))
    plant(c, 7, 1, (0.3, 0.1), cov=(0.0, 1.0, 1.0, 0.0))                     # a zero diagonal (which gs_map_set_cov accepts) around an off-diagonal: det < 0, skipped too
    c["notes"]["expect"] = {0: 6, 1: -1}
    return c


def _all_zero():
    c = scene(35, 10, 60, attach=0.0, with_pose_cov=False, params=dict(sigma_range=0.0, sigma_bearing=0.0, sigma_xy=0.0))
    c["map_cov"] = None
    for i in range(10):
        plant(c, i, i, (0.2, 0.1))
    c["notes"]["expect"] = {i: -1 for i in range(10)}
    return c


def _nan_query():
    c = scene(36, 12, 100, n_poses=1)
    c["obs"][0, 0] = 0.0; c["obs"][5, 0] = -0.0                              # azimuth 0: NaN in the formula
    c["gxy"] = ax.cone_to_global(c["poses"], c["pose_of"], c["obs"], LIDAR)
    c["notes"]["expect"] = {0: -1, 5: -1}
    return c


def _random2048():
    """the random family: 2048 cones over +-40 m, eigenvalues 0.01 .. 0.5, 8 poses with covariances, the default parameters"""
    c = scene(3, 600, 2048, n_poses=8); c["family"] = "random"
    return c


def _with(c, **kw):
    c.update(kw)
    return c


BUILDERS = {
    "map0": lambda: scene(40, 30, 0), "map1_n1": lambda: scene(41, 1, 1, attach=1.0), "map257": lambda: scene(42, 255, 257),
    "map1023": lambda: scene(43, 100, 1023), "map1024": lambda: scene(44, 256, 1024), "map1025": lambda: scene(45, 100, 1025),
    "map2047": lambda: scene(46, 257, 2047), "map2048": lambda: scene(47, 100, 2048), "map2304_nocov": lambda: _with(scene(48, 100, 2304), map_cov=None, pose_cov=None),
    "k1": lambda: scene(51, 1, 300, n_poses=1, attach=1.0), "k64": lambda: scene(52, 64, 300, n_poses=1), "k65": lambda: scene(53, 65, 300, n_poses=1),
    "grid_border": lambda: _with(_grid_border(), family="grid"), "grid_diag": lambda: _with(_grid_diag(), family="grid"),
    "grid_crowd": lambda: _with(_grid_crowd(), family="grid"), "grid_collide": lambda: _with(_grid_collide(), family="grid"),
    "grid_nonfinite": lambda: _with(_nonfinite(), family="grid"), "grid_twice": lambda: _with(_grid_twice(), family="grid"),
    "type_mismatch": lambda: _with(_type_mismatch(), family="cov"), "elongated": lambda: _with(_elongated(), family="cov"),
    "heading": lambda: _with(_heading(), family="cov"), "indefinite": lambda: _with(_indefinite(), family="cov"),
    "all_zero": lambda: _with(_all_zero(), family="cov"), "nan_query": lambda: _with(_nan_query(), family="cov"),
    "random2048": _random2048,
}
NAMES = tuple(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    c = BUILDERS[name]()
    c["map_xy"] = np.ascontiguousarray(c["map_xy"], dtype=np.float64).reshape(-1, 2); c["map_ty"] = np.ascontiguousarray(c["map_ty"], dtype=np.int32)
    if c["map_cov"] is not None:
        c["map_cov"] = np.ascontiguousarray(c["map_cov"], dtype=np.float64).reshape(-1, 4)
    c["name"] = name
    assert len(c["obs"]) <= 600 and len(c["map_xy"]) <= 2304
    for a in ("poses", "obs", "map_xy", "map_ty", "pose_of", "map_cov", "pose_cov"):
        if c[a] is not None:
            c[a].setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference(name):
    """the exact reference of a case, computed once and shared"""
    return nr.make(case(name))


@functools.lru_cache(maxsize=None)
def reference_without_pose_cov(name):
    c = dict(case(name)); c["pose_cov"] = None
    return nr.make(c)


# ---- exact by construction, from a path's OWN reported global XY
EQ_OBS = np.array([[35.0, 1.0, 8.0, 2.0], [-50.0, -2.0, 14.5, 3.0], [77.7, 0.0, 3.3, 1.0], [-9.25, 2.0, 21.0, 4.0]])
EQ_POSE = np.array([[3.0, -2.0, 0.7]])
EQ_SIGMAS = dict(sigma_range=0.0, sigma_bearing=0.0, sigma_xy=1.0)             # S = I exactly: d2 = nu0^2 + nu1^2, one rounding per square


def _offset(gx, a):
    """m = fl(gx + a) and a' = fl(m - gx), the device's nu0 for a cone at m"""
    m = gx + a
    return m, m - gx


def exact_cases(gxy):
    """(kind, i, map_xy, map_ty, map_cov, params, expect_index, expect_d2, expect_second) — a cone of query i's type at g + (a', 0), a = 1 (a power
    of two), zero cone covariance, sigma_xy = 1 and the other sigmas 0, so that S = I and the device's d2 is fl(a'^2) EXACTLY:
      gate     gate_chi2 = d2 gives -1 (the test is <), nextafter(d2) gives the cone
      dist     max_distance = a' gives -1 (sqrt(fl(a'^2)) == a' in fp64), nextafter(a') gives the cone
      tie      cones 1 and 2 at g + (a', 0) and g - (a', 0) with equal covariance: the lower index, and second_d2 == d2
    once in a map of 3 cones, once with the cones behind the first LDS tile (1024, 1025) of 1030"""
    gxy = np.asarray(gxy, dtype=np.float64).reshape(-1, 2)
    for i in range(len(gxy)):
        gx, gy = gxy[i]
        for a in (1.0, 0.5, 2.0, 0.25):
            m1, a1 = _offset(gx, a); m2 = gx - a1
            if m2 - gx == -a1:
                break
        else:
            raise AssertionError("no power of two gives an exact pair of offsets")
        d2 = a1 * a1
        for m, j in ((3, 1), (1030, 1024)):
            xy = np.full((m, 2), FAR) + np.arange(m)[:, None] * 7.0; ty = np.full(m, 9, dtype=np.int32)
            xy[j] = (m1, gy); ty[j] = int(EQ_OBS[i, 3])
            yield "gate", i, xy, ty, None, dict(EQ_SIGMAS, gate_chi2=d2, max_distance=3.0), -1, np.inf, np.inf
            yield "gate", i, xy, ty, None, dict(EQ_SIGMAS, gate_chi2=float(np.nextafter(d2, np.inf)), max_distance=3.0), j, d2, np.inf
            yield "dist", i, xy, ty, None, dict(EQ_SIGMAS, gate_chi2=1e9, max_distance=a1), -1, np.inf, np.inf
            yield "dist", i, xy, ty, None, dict(EQ_SIGMAS, gate_chi2=1e9, max_distance=float(np.nextafter(a1, np.inf))), j, d2, np.inf
            xy2 = xy.copy(); ty2 = ty.copy(); xy2[j + 1] = (m2, gy); ty2[j + 1] = ty[j]
            cov = np.zeros((m, 4)); cov[j] = cov[j + 1] = (0.25, 0.0, 0.0, 0.5)
            dt = ((1.5 * a1) * a1) / (1.25 * 1.5)                               # S = diag(1.25, 1.5), nu = (+-a', 0): the header's formula in fp64, step by step
            yield "tie", i, xy2, ty2, cov, dict(EQ_SIGMAS, gate_chi2=1e9, max_distance=3.0), j, dt, dt
