"""The cases of the front-end tests (TEST-ONLY): small scenes — at most a few thousand observations and cones — that between them reach every
place the front-end kernels can go wrong; test_frontend_exact_cpu.py holds the census that proves what each one reaches.

A case is a dict: lidar, poses [P, 3], pose_of [n], obs [n, 4] (az, zen, dist, type), map_xy [m, 2], map_ty [m], thr, tol, family, random,
notes.  Observations are drawn first; cones are then placed RELATIVE TO the observations' global XY (numpy's, or the exact reference's where a
case needs the band), so a cone is inside or outside the threshold by construction whatever the pose.  `random` cases must hold no query
with a candidate inside +-band of thr (the builder reseeds until the reference says so, and the CPU test asserts it): only constructed cases
reach the band branch of the checker.  Queries 0 .. reserved-1 of a scene carry types of their own (7, 12, 17, ...), which no random cone has: what they match is planted.

Kilometre coordinates: the grid's cell edge is thr (1 + 1e-9), and the 3 x 3 neighbourhood covers the threshold because of that 1e-9 hair.
floor(v / cell) is computed with a relative error of about 2^-52, which eats the hair only beyond about 1e-9 / 2.2e-16 = 4.5e6 cells from the
origin.  Every case stays below that: 25 km at thr = 1.2 is 2.1e4 cells, 60 km 5e4; the thr = 1e-3 case keeps its coordinates below 100 m
(1e5 cells)."""
import functools

import numpy as np

import assoc_exec as ax
import frontend_exact_ref as fx

RESERVED_TYPE = 7
FAR = 1.0e5                                                    # where cones go that must match nothing


def _obs(rng, n, reserved=0, dist=(2.0, 40.0)):
    az = rng.uniform(0.5, 170.0, n) * rng.choice([-1.0, 1.0], n)
    ob = np.stack([az, rng.uniform(-5, 5, n), rng.uniform(dist[0], dist[1], n), rng.integers(1, 5, n).astype(np.float64)], axis=1)
    ob[:reserved, 3] = RESERVED_TYPE + 5 * np.arange(reserved)            # a type of its own per reserved query
    return ob


def _around(rng, g, thr, inside):
    r = thr * (rng.uniform(0.0, 0.9) if inside else rng.uniform(1.1, 2.0)); a = rng.uniform(-np.pi, np.pi)
    return g + r * np.array([np.cos(a), np.sin(a)])


def scene(seed, n, n_map, thr=1.2, centre=(0.0, 0.0), n_poses=2, lidar=1.5, spread=60.0, reserved=0, attach=0.7, obs=None, poses=None, tol=1e-4):
    """poses around `centre`, n observations, n_map cones: `attach` of them around some unreserved query (half inside 0.9 thr, half beyond
    1.1 thr; four in five of the query's type), the rest loners within `spread` of the centre"""
    rng = np.random.default_rng(seed + 1000 * _BUMP)
    if poses is None:
        poses = np.concatenate([np.asarray(centre) + rng.uniform(-20, 20, (n_poses, 2)), rng.uniform(-np.pi, np.pi, (n_poses, 1))], axis=1)
    ob = _obs(rng, n, reserved) if obs is None else np.asarray(obs, dtype=np.float64)
    n = len(ob)
    pose_of = rng.integers(0, len(poses), n).astype(np.int32)
    g = ax.cone_to_global(poses, pose_of, ob, lidar)
    usable = np.flatnonzero(np.isfinite(g).all(axis=1) & (np.arange(n) >= reserved))
    mxy = np.zeros((n_map, 2)); mty = np.zeros(n_map, dtype=np.int32)
    for j in range(n_map):
        if len(usable) and rng.uniform() < attach:
            i = int(rng.choice(usable))
            mxy[j] = _around(rng, g[i], thr, rng.uniform() < 0.5)
            mty[j] = int(ob[i, 3]) if rng.uniform() < 0.8 else int(ob[i, 3]) % 4 + 1
        else:
            mxy[j] = np.asarray(centre) + rng.uniform(-spread, spread, 2); mty[j] = rng.integers(1, 5)
    return dict(lidar=lidar, poses=poses, pose_of=pose_of, obs=ob, map_xy=mxy, map_ty=mty, thr=float(thr), tol=float(tol), gxy=g,
                family="shape", random=True, notes={})


def plant(c, j, i, offset, dty=0, ty=None):
    """cone j becomes a cone of query i's type + dty (or of type ty) at query i's global XY + offset (in units of thr)"""
    c["map_xy"][j] = c["gxy"][i] + c["thr"] * np.asarray(offset, dtype=np.float64); c["map_ty"][j] = int(c["obs"][i, 3]) + dty if ty is None else ty


# ---- A0 inputs
def abeam_inputs(lidar, n_dist, seed, own=False):
    """az = +-acos(-lidar / dist) in degrees, perturbed by relative 0, +-1e-13, +-1e-10, +-1e-7, at n_dist distances in 1.6 .. 60.  With the
    float kPiF and the truncated kDeg2Rad the FORMULA's branch point lies 8.7e-8 rad from there; own: az = (kPiF - acos(lidar / dist)) /
    kDeg2Rad instead, which is abeam as the formula sees it"""
    rng = np.random.default_rng(seed)
    dist = np.sort(rng.uniform(1.6, 60.0, n_dist))
    rows = []
    for d in dist:
        a = (ax.K_PIF - np.arccos(lidar / d)) / ax.K_D2R if own else np.degrees(np.arccos(-lidar / d))
        for p in (0.0, 1e-13, -1e-13, 1e-10, -1e-10, 1e-7, -1e-7):
            for s in (1.0, -1.0):
                rows.append((s * a * (1.0 + p), rng.uniform(-5, 5), d, float(rng.integers(1, 5))))
    return np.array(rows)


def edge_inputs(lidar):
    """az -> 0+- (and exactly +-0: NaN), az = +-180 and next to it, zen = +-90, dist = 0 and tiny, dnew -> 0 (dist next to lidar, |az| next to 180)"""
    tiny = 5e-324
    azs = [0.0, -0.0, tiny, -tiny, 1e-300, -1e-300, 1e-9, -1e-9, 1e-3, -1e-3, 180.0, -180.0, 179.999999, -179.999999, 179.99, -179.99, 90.0, -45.0]
    zens = [0.0, 90.0, -90.0, 89.9999, -3.0]
    dists = [0.0, 1e-12, 0.3, 7.0, 60.0] + ([lidar * (1 + 1e-5), lidar * (1 - 1e-5), lidar * (1 + 1e-3), lidar] if lidar > 0 else [1e-5])
    rows = [(a, z, d, float(1 + (k % 4))) for k, (a, z, d) in enumerate((a, z, d) for a in azs for z in zens for d in dists)]
    rows = [r for r in rows if not (lidar > 0 and r[2] == lidar and abs(r[0]) >= 179.99)]          # dnew far below 1e-5: refused by the reference
    return np.array(rows)


def _a0_case(kind, lidar):
    seed = dict(random=11, abeam=12, edges=13)[kind] + (0 if lidar else 100)
    if kind == "random":
        rng = np.random.default_rng(seed); n = 400
        az = rng.uniform(-170, 170, n); az[az == 0] = 1.0
        ob = np.stack([az, rng.uniform(-5, 5, n), rng.uniform(0.3, 60, n), rng.integers(1, 5, n).astype(np.float64)], axis=1)
    elif kind == "abeam":
        ob = np.concatenate([abeam_inputs(lidar, 300 if lidar else 40, seed), abeam_inputs(lidar, 100 if lidar else 20, seed + 1, own=True)])
    else:
        ob = edge_inputs(lidar)
    c = scene(seed, len(ob), 64, poses=np.array([[3.0, -2.0, 0.7]]), lidar=lidar, obs=ob, attach=0.9)
    c["family"] = "a0_" + kind; c["random"] = kind == "random"
    return c


# ---- A1 shapes
def _tile2():
    c = scene(21, 60, 1300, reserved=4)
    plant(c, 1024, 0, (0.3, 0.0)); plant(c, 1100, 0, (0.1, 0.0))                     # the first cone of the second tile, a nearer one later
    plant(c, 1023, 1, (0.0, 0.5)); plant(c, 1024 + 1, 1, (0.0, 0.1))                 # the last of the first tile before one of the second
    plant(c, 1299, 2, (-0.4, 0.2))                                                   # the last cone alone
    plant(c, 0, 3, (0.9, 0.0)); plant(c, 1026, 3, (0.05, 0.0))                       # the first cone at 0.9 thr, a nearer one in the second tile
    c["notes"]["expect"] = {0: 1024, 1: 1023, 2: 1299, 3: 0}
    return c


def _frame_lanes():
    c = scene(22, 40, 600, reserved=4, n_poses=1)
    plant(c, 200, 0, (0.3, 0.0)); plant(c, 261, 0, (0.1, 0.0))                       # wave 3 in round 0 before thread 5 in round 1
    plant(c, 10, 1, (0.5, 0.0)); plant(c, 266, 1, (0.1, 0.1))                        # one thread: j and j + 256
    plant(c, 300, 2, (0.2, 0.0)); plant(c, 130, 2, (0.6, 0.0))                       # thread 44 of wave 0 in round 1, wave 2 in round 0
    for j in (67, 131, 195, 259):
        plant(c, j, 3, (0.1, 0.2))                                                   # one match in every wave
    c["notes"]["expect"] = {0: 200, 1: 10, 2: 130, 3: 67}
    return c


def _types(tol):
    c = scene(23, 40, 300, reserved=3, tol=tol)
    plant(c, 5, 0, (0.3, 0.0), 1); plant(c, 9, 0, (0.2, 0.0), -1); plant(c, 50, 0, (0.5, 0.0))      # |dt| == 1 before the type itself
    plant(c, 3, 1, (0.1, 0.1), -2); plant(c, 70, 1, (0.4, 0.0))                                                     # a lower type first: the fabs
    plant(c, 8, 2, (0.1, 0.1), 2); plant(c, 90, 2, (0.4, 0.0))                                                     # a higher type first
    one = tol > 1.0
    c["notes"]["expect"] = {0: 5 if one else 50, 1: 70, 2: 90}
    c["notes"]["expect_signed"] = {0: 5 if one else 9, 1: 3, 2: 90}                  # the localizer's test has no fabs: lower types pass
    return c


def _grid_border():
    """cones exactly on cell borders (x, y or both a multiple of the cell edge as the device computes it, and the fp64 neighbours of that)"""
    c = scene(24, 120, 0, reserved=0, centre=(-7.0, 5.0))
    rng = np.random.default_rng(24); cell = 1.0 / ax.inv_cell_of(c["thr"])
    xy, ty = [], []
    for i in range(len(c["obs"])):
        g = c["gxy"][i]; k = np.round(g / cell)
        for mode in range(3):
            inside = rng.uniform() < 0.5; r = c["thr"] * (0.8 if inside else 1.3)
            p = g.copy(); a = mode % 2
            p[a] = k[a] * cell
            if mode == 2:
                p[a] = np.nextafter(p[a], rng.choice([-np.inf, np.inf]))
            p[1 - a] = g[1 - a] + rng.choice([-1.0, 1.0]) * np.sqrt(r * r - (p[a] - g[a]) ** 2)
            xy.append(p); ty.append(int(c["obs"][i, 3]))
    order = rng.permutation(len(xy))
    c["map_xy"] = np.array(xy)[order]; c["map_ty"] = np.array(ty, dtype=np.int32)[order]
    return c


def _grid_diag():
    """every query has ONE cone of its own type, in the diagonally adjacent cell past its nearest cell corner, inside the threshold"""
    c = scene(25, 80, 300, reserved=80, centre=(-40.0, -30.0))
    cell = 1.0 / ax.inv_cell_of(c["thr"])
    c["obs"][:, 3] = RESERVED_TYPE + np.arange(80)                                  # a type per query, none a random cone's
    for i in range(80):
        g = c["gxy"][i]; f = g / cell - np.floor(g / cell); s = np.where(f >= 0.5, 1.0, -1.0)
        corner = (np.floor(g / cell) + (s > 0)) * cell
        c["map_xy"][3 * i] = corner + s * 0.01 * cell; c["map_ty"][3 * i] = int(c["obs"][i, 3])
    return c


def _grid_crowd():
    c = scene(26, 50, 800, reserved=2)
    rng = np.random.default_rng(26)
    for j in range(100, 600):                                                        # 500 cones within 0.1 thr of one point
        plant(c, j, 0, rng.uniform(-0.1, 0.1, 2) + (0.3, 0.0), ty=int(rng.integers(1, 5)))
    plant(c, 431, 0, (0.3, 0.05)); plant(c, 577, 0, (0.25, 0.0)); plant(c, 610, 0, (0.0, 0.0))
    c["notes"]["expect"] = {0: 431}
    return c


def _nonfinite():
    """NaN and infinite map entries (the grid's count and fill skip them: `items` is shorter than the map), and a query of a pose of its own,
    moved so that one of its nine cells hashes to the bucket the first non-finite cone would be counted in"""
    c = scene(27, 60, 400, reserved=1, n_poses=3)
    c["pose_of"][0] = 2; c["pose_of"][1:] = c["pose_of"][1:] % 2; c["poses"][2, 2] = 0.0
    bad = {2: (np.nan, 3.0), 3: (np.inf, -8.0), 17: (4.0, -np.inf), 40: (np.nan, np.nan), 41: (-np.inf, np.inf), 399: (1.0, np.nan)}
    for j, p in bad.items():
        c["map_xy"][j] = p
    inv = ax.inv_cell_of(c["thr"]); mask = ax.buckets_of(400) - 1; cell = 1.0 / inv
    target = int(ax.grid_bucket(ax.grid_coord(np.nan, inv), ax.grid_coord(3.0, inv), mask))
    a, b = np.meshgrid(np.arange(-150, 150), np.arange(-150, 150), indexing="ij")
    hits = np.argwhere(ax.grid_bucket(a, b, mask) == target)
    assert len(hits), "no cell of the search window hashes to the bucket of the non-finite cone"
    ca, cb = (hits[0] - 150).tolist()
    z = ax.polar_to_xy(c["obs"][0, 0], c["obs"][0, 1], c["obs"][0, 2], c["lidar"])
    c["poses"][2, :2] = (ca + 0.5) * cell - z[0], (cb + 0.5) * cell - z[1]
    c["gxy"] = ax.cone_to_global(c["poses"], c["pose_of"], c["obs"], c["lidar"])
    plant(c, 300, 0, (0.2, 0.1))
    c["notes"]["expect"] = {0: 300}; c["notes"]["nonfinite"] = sorted(bad)
    return c


def _near_thr():
    """cones 8 bands inside and 8 bands outside the threshold of the exact global XY (rounding a cone to fp64 moves it by less than one band):
    cone 2 i inside for even i, outside for odd i; cone 2 i + 1 far.  Cones 400 + k, k < 50, sit AT the threshold of query k (inside the band):
    for odd k they are the in-band candidates of the checker — the device may take them or not"""
    c = scene(28, 200, 0, n_poses=3)
    R = fx.Ref(c["obs"], c["poses"], c["pose_of"], c["lidar"])
    rng = np.random.default_rng(28); band = R.band_of(c["thr"])
    xy = np.full((450, 2), FAR); ty = np.ones(450, dtype=np.int32); pairs = []
    for i in range(200):
        a = rng.uniform(-np.pi, np.pi); inside = i % 2 == 0
        r = c["thr"] + (-8.0 if inside else 8.0) * band[i]
        xy[2 * i] = R.g_hi[i] + r * np.array([np.cos(a), np.sin(a)]); ty[2 * i] = int(c["obs"][i, 3])
        xy[2 * i + 1] += (3.0 * i, 0.0)
        pairs.append((i, 2 * i, inside))
        if i < 50:
            a = rng.uniform(-np.pi, np.pi)
            xy[400 + i] = R.g_hi[i] + c["thr"] * np.array([np.cos(a), np.sin(a)]); ty[400 + i] = int(c["obs"][i, 3])
    c["map_xy"] = xy; c["map_ty"] = ty; c["ref"] = R; c["random"] = False; c["family"] = "near_thr"; c["notes"]["pairs"] = pairs
    return c


def _with(c, **kw):
    c.update(kw)
    return c


BUILDERS = {
    "a0_random": lambda: _a0_case("random", 1.5), "a0_random_l0": lambda: _a0_case("random", 0.0),
    "a0_abeam": lambda: _a0_case("abeam", 1.5), "a0_abeam_l0": lambda: _a0_case("abeam", 0.0),
    "a0_edges": lambda: _a0_case("edges", 1.5), "a0_edges_l0": lambda: _a0_case("edges", 0.0),
    "map1_n1": lambda: scene(31, 1, 1, attach=1.0), "map255": lambda: scene(32, 100, 255), "map256": lambda: scene(33, 100, 256),
    "map257": lambda: scene(34, 255, 257), "map1023": lambda: scene(35, 100, 1023), "map1024": lambda: scene(36, 257, 1024),
    "map1025": lambda: scene(37, 100, 1025), "map2047": lambda: scene(38, 100, 2047), "map2048": lambda: scene(39, 513, 2048),
    "map0": lambda: scene(40, 30, 0),
    "k1": lambda: scene(41, 1, 300, n_poses=1, attach=1.0), "k64": lambda: scene(42, 64, 300, n_poses=1), "k65": lambda: scene(43, 65, 300, n_poses=1),
    "tile2": _tile2, "frame_lanes": _frame_lanes, "type_tol1": lambda: _types(1.0), "type_tol1p": lambda: _types(float(np.nextafter(1.0, np.inf))),
    "grid_neg": lambda: _with(scene(51, 150, 500, centre=(-300.0, -200.0)), family="grid"),
    "grid_border": lambda: _with(_grid_border(), family="grid"), "grid_diag": lambda: _with(_grid_diag(), family="grid"),
    "grid_crowd": lambda: _with(_grid_crowd(), family="grid"), "grid_nonfinite": lambda: _with(_nonfinite(), family="grid"),
    "km_spread": lambda: _with(scene(52, 200, 2048, centre=(25.0e3, -25.0e3), spread=30.0e3, attach=0.4), family="km"),
    "km_neg": lambda: _with(scene(53, 150, 300, centre=(-25.0e3, -25.0e3), spread=100.0), family="km"),
    "thr_1e-3": lambda: _with(scene(54, 120, 300, thr=1e-3), family="thr"), "thr_3": lambda: _with(scene(55, 120, 1100, thr=3.0), family="thr"),
    "thr_1e6": lambda: _with(scene(56, 120, 300, thr=1e6), family="thr"),
    "thr_0": lambda: _with(scene(57, 60, 300), thr=0.0, family="thr", random=False), "thr_neg": lambda: _with(scene(57, 60, 300), thr=-1.2, family="thr", random=False),
    "thr_nan": lambda: _with(scene(57, 60, 300), thr=float("nan"), family="thr", random=False),
    "near_thr": _near_thr,
}
NAMES = tuple(BUILDERS)
MAX_RESEED = 4
_BUMP = 0                                                      # added (times 1000) to a scene's seed while its case is being reseeded


@functools.lru_cache(maxsize=None)
def case(name):
    """the case, built once; a random case is rebuilt with another seed until the reference finds no candidate inside +-band of thr"""
    global _BUMP
    for _BUMP in range(MAX_RESEED):
        c = BUILDERS[name]()
        c["map_xy"] = np.ascontiguousarray(c["map_xy"], dtype=np.float64).reshape(-1, 2); c["map_ty"] = np.ascontiguousarray(c["map_ty"], dtype=np.int32)
        if not c["random"]:
            break
        c["ref"] = fx.Ref(c["obs"], c["poses"], c["pose_of"], c["lidar"])
        if not any(c["ref"].admissible(c["map_xy"], c["map_ty"], c["thr"], c["tol"], s, key="case").n_inband for s in (False, True)):
            break
    _BUMP = 0
    c["name"] = name
    for a in ("poses", "obs", "map_xy", "map_ty", "pose_of"):
        c[a].setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference(name):
    """the exact A0 of a case (frontend_exact_ref.Ref); admissible(name) is its A1"""
    c = case(name)
    return c["ref"] if "ref" in c else fx.Ref(c["obs"], c["poses"], c["pose_of"], c["lidar"])


def admissible(name, signed=False):
    c = case(name)
    return reference(name).admissible(c["map_xy"], c["map_ty"], c["thr"], c["tol"], signed, key="case")


# ---- equality at the threshold, built from a path's OWN reported global XY
EQ_OBS = np.array([[35.0, 1.0, 8.0, 2.0], [-120.0, -2.0, 14.5, 3.0], [77.7, 0.0, 3.3, 1.0], [-9.25, 4.0, 41.0, 4.0]])
EQ_POSE = np.zeros((1, 3))                                     # the origin, heading 0: gxy is the A0 output exactly, whichever cos / sin a path uses


def equality_maps(gxy):
    """for every query i and axis: (i, map_xy, map_ty, thr, j) with cone j of query i's type at m = fl(g + a) along that axis, the other
    coordinate equal, thr = m - g in fp64 — the device's sqrt(dx * dx + 0) is then thr exactly.  Once in a map of 2 cones (j = 1), once as
    the first cone of the second tile of 1030 (j = 1024).  No match at thr, a match at nextafter(thr, inf)."""
    gxy = np.asarray(gxy, dtype=np.float64).reshape(-1, 2)
    for i in range(len(gxy)):
        for a in (0, 1):
            for m, j in ((2, 1), (1030, 1024)):
                p = gxy[i].copy(); p[a] = gxy[i, a] + 1.2 * (1.0 + 0.1 * i) * (-1.0) ** i
                thr = abs(p[a] - gxy[i, a])
                xy = np.full((m, 2), FAR) + np.arange(m)[:, None] * 3.0; ty = np.full(m, 9, dtype=np.int32)
                xy[j] = p; ty[j] = int(EQ_OBS[i, 3])
                yield i, xy, ty, float(thr), j
