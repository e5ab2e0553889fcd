"""The smallest graphs that reach each path of the two side passes (TEST-ONLY; deterministic): the prior edges and the polar observation
edges, on graphs of lin_shapes.make (70 poses; the fixed first pose, the fixed landmark 1, the hub, anisotropic information come with it).

A case is dict(g, polar, pri, kernels, off, notes): the graph dict (conftest layout; at a polar edge's index it keeps a Cartesian placeholder
with zero information), a polar set (polar_ref layout), a prior set (prior_ref layout), the robust kernels, the inactive observation edges.
The base graph has at most 3 observations per pose and the special edges go on poses that have none, four at the most, so every case but
`ring` (25 edges on one pose: fused at T = 8 only) and `near_far` (6 on pose 16, the weak wrapped edge among them: fused from T = 2) runs the fused kernel at every forced lane count
T = 1, 2, 4, 8 (R = 3 or 4, 2, 1, 1); each runs once more on the gather kernels.  The special poses are moved where the geometry wants them:
their odometry residuals are metres, which the linearisation does not mind.

Polar cases (CASES[name]["paths"] = forced T 1, 2, 4, 8 and "gather"):
  ring      pose 8 at (2, 0) with heading -0.0 (cos 1, sin -0 on the device): landmarks every 15 degrees around it at radius 3 — integer offsets on
            the four half-axes —, one more on the negative x-axis whose dy is -0 in the device's operation order beside the one at +0
            (atan2(+-0, -x) = +-pi); pose 12 with a generic heading sees the same landmarks
  wrap      z_beta chosen so that beta - z_beta is 6 (in (pi, 2 pi)), -6, +-(pi - 1e-5), +-(pi + 1e-5), 0, and — the extreme two angles of
            [-pi, pi] allow, z_beta being normalised when stored — 2 pi exactly on a bearing-only edge (beta = pi on the negative x-axis,
            z_beta = -pi).  z is independent of where the landmark is now: the landmark "moved after z was taken".  The two landmarks
            that only a bearing sees get a range-bearing edge from pose 16 (a bearing alone leaves H_ll with rank 1, and the case is iterated)
  near_far  ranges 1e-3, 1e-2, 0.1, 1, 20 m from pose 16 (the 20 m one at a bearing of 1e-6: the largest J_d entry is 1e10 times the smallest)
            and the same ranges on ONE landmark from poses 20, 24, 28, 32, 36
  zero      pose 8 at (6, 2, +0) and a landmark exactly there: r == 0 in the device's operation order; a Cartesian edge between the same pair,
            another polar edge on the pose, a polar edge on the landmark from pose 12
  mixed     full Omega, bearing-only, two polar edges and a Cartesian one between one pair, polar edges on the fixed pose, on the fixed
            landmark, between the two fixed vertices, an inactive polar edge
  far       the graph at lin_shapes.FAR (4e4, -3e4) with polar_ref.polar_set
  cauchy, huber   the observation kind's kernel, delta from lin_shapes._clear_delta over the combined s, gross outliers among the polar edges
Every polar case also carries polar_ref.polar_set of its base graph (a third of the edges range-bearing, a seventh bearing-only).

Prior cases (paths T = 1, 8 and "gather"), priors of all three kinds on top of a polar set:
  priors          <= 12 landmark groups per tile (10 landmarks): two priors on one pose and on one cone, priors on the fixed pose and the fixed
                  cone, one landmark prior strong against the observations, theta - z_theta wrapping each way, a pose whose own heading is theta + 2 pi, full 3 x 3 Omega with weak and strong directions
  priors_groups   the t1_groups layout (300 landmarks, > 25 groups in a tile): landmark priors on landmarks of the first tile
  priors_far      the set at the FAR offset
Launch boundary: launch255 / launch257 — 260 poses, one polar edge each on 255 / 257 free poses and 255 / 257 vertices with a prior
(200 poses + 55 / 57 landmarks): one workgroup adds its chi2 itself, two go through k_side_total."""
import numpy as np

import lin_shapes as ls
import polar_ref as plr
import prior_ref as pr

RB, BO = plr.RANGE_BEARING, plr.BEARING


def device_d(px, py, th, lx, ly):
    """d = x_p^-1 . l in the device's operation order (lm_in_pose_frame, gs_edge_dev.hpp), in numpy: signs of zeros included"""
    c, s = np.cos(th), np.sin(th)
    ix = -(c * px + s * py); iy = s * px - c * py
    return (c * lx + s * ly) + ix, (c * ly - s * lx) + iy


class Builder:
    def __init__(self, seed=0, far=False, **kw):
        args = dict(N=70, kmax=3, T=1, seed=seed, far=far); args.update(kw)
        g, _, notes = ls.make(**args)
        self.g = {k: np.array(v, copy=True) for k, v in g.items()}; self.notes = dict(notes)
        self.extra = []                                   # (model, z[2], W[2, 2]) of the edges appended here, model 0: Cartesian
        self.E0 = len(g["pl_p"]); self.inactive = []

    def set_pose(self, q, x):
        self.g["pose_est"][q] = x

    def add_lm(self, xy):
        self.g["lm_est"] = np.vstack([self.g["lm_est"], np.reshape(np.asarray(xy, dtype=np.float64), (1, 2))])
        return len(self.g["lm_est"]) - 1

    def lm_at(self, q, r, beta):
        """a new landmark at range r and bearing beta of pose q (as numpy rounds it)"""
        x, y, th = self.g["pose_est"][q]
        return self.add_lm([x + r * np.cos(th + beta), y + r * np.sin(th + beta)])

    def seen(self, q, l):
        """(r, beta) of landmark l from pose q in the device's operation order"""
        x, y, th = self.g["pose_est"][q]; dx, dy = device_d(x, y, th, *self.g["lm_est"][l])
        return float(np.sqrt(dx * dx + dy * dy)), float(np.arctan2(dy, dx))

    def edge(self, q, l, model, z, W):
        z = (float(z[0]), float(z[1]) if -np.pi <= z[1] < np.pi else float((z[1] + np.pi) % (2 * np.pi) - np.pi))     # as the host would store it
        self.g["pl_p"] = np.append(self.g["pl_p"], np.int32(q)); self.g["pl_l"] = np.append(self.g["pl_l"], np.int32(l))
        W = np.asarray(W, dtype=np.float64).reshape(2, 2)
        self.g["pl_z"] = np.vstack([self.g["pl_z"], np.reshape(z if model == 0 else (0.0, 0.0), (1, 2))])
        self.g["pl_info"] = np.vstack([self.g["pl_info"], (W if model == 0 else np.zeros((2, 2))).reshape(1, 4)])
        if model == BO:
            assert z[0] == 0.0 and W[0, 0] == 0.0 and W[0, 1] == 0.0
        self.extra.append((model, np.asarray(z, dtype=np.float64), W))
        return len(self.g["pl_p"]) - 1

    def rb(self, q, l, dz=(0.01, -0.004), W=((40.0, 3.0), (3.0, 900.0)), z=None):
        r, beta = self.seen(q, l)
        return self.edge(q, l, RB, (r + dz[0], beta + dz[1]) if z is None else z, W)

    def bo(self, q, l, dz=0.003, w=700.0, z=None):
        r, beta = self.seen(q, l)
        return self.edge(q, l, BO, (0.0, beta + dz if z is None else z), ((0.0, 0.0), (0.0, w)))

    def finish(self, base_polar=True, pri=None, kernels=None, **notes):
        g = self.g
        base = plr.polar_set(dict(g, pl_p=g["pl_p"][:self.E0], pl_l=g["pl_l"][:self.E0], pl_z=g["pl_z"][:self.E0], pl_info=g["pl_info"][:self.E0])) if base_polar else plr.empty_set()
        ex = [(self.E0 + t, m, z, W) for t, (m, z, W) in enumerate(self.extra) if m]
        polar = dict(idx=np.concatenate([base["idx"], np.array([e[0] for e in ex], dtype=np.int64)]).astype(np.int64),
                     model=np.concatenate([base["model"], np.array([e[1] for e in ex], dtype=np.int32)]).astype(np.int32),
                     z=np.vstack([base["z"]] + [e[2].reshape(1, 2) for e in ex]), W=np.concatenate([base["W"]] + [e[3].reshape(1, 2, 2) for e in ex]))
        assert np.all(np.diff(polar["idx"]) > 0) and np.all(polar["z"][:, 1] >= -np.pi) and np.all(polar["z"][:, 1] < np.pi) and np.all(polar["z"][:, 0] >= 0)
        self.notes.update(notes); self.notes["first_extra"] = self.E0
        return dict(g=g, polar=polar, pri=pri or dict(pose=[], lm=[]), kernels=kernels, off=list(self.inactive), notes=self.notes)


def _ring():
    b = Builder(seed=11)
    b.set_pose(8, (2.0, 0.0, -0.0)); b.set_pose(12, (4.0, 1.0, 0.7))
    lms = []
    for k in range(24):
        a = np.deg2rad(15.0 * k)
        off = {0: (3.0, 0.0), 6: (0.0, 3.0), 12: (-3.0, -0.0), 18: (0.0, -3.0), 3: (2.0, 2.0), 9: (-2.0, 2.0), 15: (-2.0, -2.0), 21: (2.0, -2.0)}.get(k, (3 * np.cos(a), 3 * np.sin(a)))
        lms.append(b.add_lm((2.0 + off[0], off[1])))                     # k = 12: (-1, -0.0), dy = -0 on the device
    lms.append(b.add_lm((-2.0, 0.0)))                                    # the negative x-axis again, dy = +0
    edges = []
    for q in (8, 12):
        for t, l in enumerate(lms):
            edges.append(b.rb(q, l) if t % 2 == 0 else b.bo(q, l))
    return b.finish(ring_pose=8, second_pose=12, ring_lms=lms, ring_edges=edges)


def _wrap():
    b = Builder(seed=12)
    poses = (8, 12, 16); b.set_pose(8, (6.0, 2.0, 0.0))
    want = []                                              # (pose, beta of the landmark, beta - z_beta wanted, model)
    want += [(8, 3.0, 6.0, RB), (8, -3.0, -6.0, RB), (12, 2.0, np.pi - 1e-5, RB)]
    want += [(12, -2.0, -(np.pi - 1e-5), BO), (12, 2.5, np.pi + 1e-5, RB), (16, -2.5, -(np.pi + 1e-5), RB), (16, 0.4, 0.0, RB)]
    edges = []
    for q, beta, diff, model in want:
        l = b.lm_at(q, 2.5, beta); r, bt = b.seen(q, l)
        zb = bt - diff
        edges.append(b.rb(q, l, z=(r + 0.02, zb)) if model == RB else b.bo(q, l, z=zb))
    l = b.add_lm((3.0, 2.0))                                # pose 8 has heading +0: dx = -3, dy = +0, beta = pi; z_beta = -pi: 2 pi exactly
    edges.append(b.bo(8, l, z=-np.pi))
    b.rb(16, l); b.rb(16, int(b.g["pl_l"][edges[3]]))       # a bearing alone leaves a landmark unobservable (H_ll of rank 1): a range-bearing edge each
    return b.finish(wrap_edges=edges, wrap_poses=poses)


RANGES = (1e-3, 1e-2, 0.1, 1.0, 20.0)


def _near_far():
    b = Builder(seed=13)
    edges = []
    for t, r in enumerate(RANGES):
        l = b.lm_at(16, r, 1e-6 if r == 20.0 else 0.5 + 0.9 * t)
        if t == 0:                                          # the nearest: a strong bearing with a residual of half a radian owns the largest entries of H and b
            edges.append(b.rb(16, l, dz=(1e-5, 0.5), W=((40.0, 3.0), (3.0, 1e4))))
        elif r == 20.0:                                     # the 20 m edges: bearing-only, omega 0.25, a residual of 1e-4 (see test_side_exact_cpu.py's planted bugs)
            edges.append(b.bo(16, l, dz=1e-4, w=0.25))
        else:
            edges.append(b.rb(16, l, dz=(0.01 * r, 1e-3)) if t % 2 == 0 else b.bo(16, l, dz=1e-3))
    cone = b.add_lm((20.0, 3.0))
    for t, (q, r) in enumerate(zip((20, 24, 28, 32, 36), RANGES)):
        a = 0.3 + 1.1 * t
        b.set_pose(q, (20.0 - r * np.cos(a), 3.0 - r * np.sin(a), 0.2 * t - 0.3))
        edges.append(b.bo(q, cone, dz=1e-4, w=0.25) if r == 20.0 else b.rb(q, cone, dz=(0.01 * r, -1e-3)))
    l = b.lm_at(16, 20.0, 3.0)                              # a wrapped bearing (beta - z_beta = 6) of next to no weight, on a landmark of its own
    weak = b.bo(16, l, z=-3.0, w=1e-10)
    return b.finish(nf_pose=16, nf_cone=cone, nf_edges=edges, nf_20m=[edges[4], edges[9]], nf_weak=weak)


def _zero():
    b = Builder(seed=14)
    b.set_pose(8, (6.0, 2.0, 0.0))
    lz = b.add_lm((6.0, 2.0)); l2 = b.add_lm((8.5, 3.25))
    e0 = b.edge(8, lz, RB, (0.5, 0.25), ((40.0, 3.0), (3.0, 900.0)))
    ec = b.edge(8, lz, 0, (0.1, -0.05), ((50.0, 4.0), (4.0, 20.0)))
    e1 = b.rb(8, l2); e2 = b.rb(12, lz)
    return b.finish(zero_edge=e0, zero_pose=8, zero_lm=lz, zero_others=[ec, e1, e2])


def _mixed():
    b = Builder(seed=15)
    F = int(b.g["fixed_landmarks"][0])
    la = b.lm_at(8, 4.0, 0.6); lb = b.lm_at(8, 6.0, -0.9); lc = b.lm_at(12, 3.0, 1.4)
    e = dict(full=b.rb(8, la, W=((35.0, -60.0), (-60.0, 800.0))), bearing=b.bo(8, lb))
    e["pair"] = [b.rb(12, lc), b.bo(12, lc), b.edge(12, lc, 0, (0.2, 2.9), ((60.0, 5.0), (5.0, 9.0)))]
    e["fixed_pose"] = b.rb(0, la); e["fixed_lm"] = b.rb(16, F); e["both_fixed"] = b.bo(0, F)
    e["inactive"] = b.rb(16, la); b.inactive.append(e["inactive"])
    return b.finish(mixed=e)


def _far():
    b = Builder(seed=16, far=True)
    l = b.lm_at(8, 5.0, 0.8); b.rb(8, l); b.bo(12, l)
    return b.finish(far=True)


def _robust(kind):
    b = Builder(seed=17)
    c = b.finish()
    pol = c["polar"]; g = c["g"]
    pol["z"][3::5] += [1.5, 0.4]; pol["z"][pol["model"] == BO, 0] = 0.0; pol["z"][:, 1] = (pol["z"][:, 1] + np.pi) % (2 * np.pi) - np.pi       # gross outliers: a wrong range and bearing
    s = plr.edge_s(plr.carriers(g, pol), pol, g["pose_est"], g["lm_est"])
    delta = ls._clear_delta(s)
    c["kernels"] = {"observation": (kind, delta)}; c["notes"]["robust"] = True
    return c


def _weak_strong(rng):
    A = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    W = A @ np.diag([2e3, 3.0, 2e-3]) @ A.T
    return (W + W.T) / 2


def _priors(layout):
    rng = np.random.default_rng(77)
    if layout == "groups":
        b = Builder(seed=18, kmax=4, n_lms=300, full=True, stride=4)
    elif layout == "far":
        b = Builder(seed=19, far=True, n_lms=10)
    else:
        b = Builder(seed=20, n_lms=10)
    g = b.g; P, L = g["pose_est"], g["lm_est"]
    F = int(g["fixed_landmarks"][0])
    pose, lm = [], []
    def se2(p, zth=None, W=None):
        z = P[p] + rng.normal(0, 0.2, 3) * [1, 1, 0.2]
        if zth is not None:
            z[2] = zth
        pose.append((p, z, ls._spd3(rng, 0.01).reshape(3, 3) if W is None else W, False))
    def xy(p):
        z, W = pr.embed_xy(P[p, :2] + rng.normal(0, 0.2, 2), ls._spd2(rng, 0.05).reshape(2, 2)); pose.append((p, z, W, True))
    def lmp(l):
        lm.append((l, L[l] + rng.normal(0, 0.2, 2), ls._spd2(rng, 0.02).reshape(2, 2)))
    seen = np.bincount(g["pl_l"], minlength=len(L)) > 0
    for p in range(5, 70, 9):
        se2(p)
    for p in range(7, 70, 11):
        xy(p)
    xy(14); se2(14)                                                    # pose 14: an SE2 prior from the loop, then XY and SE2 again
    se2(0)                                                             # the fixed pose
    P[22, 2] = 0.3; se2(22, zth=-3.0)                                  # theta - z_theta = 3.3: wraps down
    P[23, 2] = -0.3; se2(23, zth=3.0)                                  # -3.3: wraps up
    P[30, 2] += 2 * np.pi; se2(30, zth=P[30, 2] - 2 * np.pi + 0.05)                                    # the estimate's own heading outside [-pi, pi)
    se2(31, W=_weak_strong(rng))
    free_l = [l for l in range(len(L)) if l != F and seen[l]]
    for l in free_l[::3 if layout != "groups" else 2][:40]:
        lmp(l)
    lmp(free_l[0]); lmp(F)
    l = free_l[1]; lm.append((l, L[l] + [0.15, -0.2], np.array([[2e4, 3e3], [3e3, 1e4]])))     # a strong one: its share of b_lm shows against the observations' S
    return b.finish(pri=dict(pose=pose, lm=lm), far=layout == "far", layout=layout, wrap_priors=(22, 23), turned_pose=30)


def _launch(count):
    """260 poses; one range-bearing edge each on `count` free poses (to a cone the base graph gives the pose no edge to), priors on 200 poses
    and count - 200 landmarks.  Beyond `count`, up to 257, the pairs are Cartesian edges with zero information: one structure for both counts"""
    b = Builder(seed=21, N=260, kmax=2, n_lms=100)
    g = b.g; rng = np.random.default_rng(257)
    free = np.arange(1, 258); F = int(g["fixed_landmarks"][0])
    for t, q in enumerate(free):
        mine = set(int(l) for l in g["pl_l"][:b.E0][g["pl_p"][:b.E0] == q])
        l = next(l for l in range(2 + t % 50, 100) if l not in mine)
        if t < count:
            b.rb(int(q), l, dz=(0.05, 0.01))
        else:
            b.edge(int(q), l, 0, (0.0, 0.0), np.zeros((2, 2)))
    pose = [(int(p), g["pose_est"][p] + rng.normal(0, 0.1, 3) * [1, 1, 0.2], ls._spd3(rng, 0.01).reshape(3, 3), False) for p in range(1, 201)]
    seen = np.bincount(g["pl_l"], minlength=len(g["lm_est"])) > 0
    free_l = [l for l in range(len(g["lm_est"])) if l != F and seen[l]][:count - 200]
    assert len(free_l) == count - 200
    lm = [(l, g["lm_est"][l] + rng.normal(0, 0.1, 2), ls._spd2(rng, 0.02).reshape(2, 2)) for l in free_l]
    return b.finish(base_polar=False, pri=dict(pose=pose, lm=lm), count=count)


POLAR = ("ring", "wrap", "near_far", "zero", "mixed", "far", "cauchy", "huber")
PRIOR = ("priors", "priors_groups", "priors_far")
LAUNCH = ("launch255", "launch257")
CASES = {n: dict(paths=(1, 2, 4, 8, "gather")) for n in POLAR}
CASES.update({n: dict(paths=(1, 8, "gather")) for n in PRIOR})
CASES.update({n: dict(paths=(0,)) for n in LAUNCH})
_make = dict(ring=_ring, wrap=_wrap, near_far=_near_far, zero=_zero, mixed=_mixed, far=_far, cauchy=lambda: _robust("cauchy"), huber=lambda: _robust("huber"),
             priors=lambda: _priors("few"), priors_groups=lambda: _priors("groups"), priors_far=lambda: _priors("far"),
             launch255=lambda: _launch(255), launch257=lambda: _launch(257))
RUNS = [(n, p) for n, c in CASES.items() for p in c["paths"]]
_built = {}


def case(name):
    """built once per process, never changed by a test"""
    if name not in _built:
        _built[name] = _make[name]()
    return _built[name]


def handle_kw(name, path):
    """keyword arguments of pkg.Graph: the forced lanes (path: T, 0 for the planner's own) or the gather kernels, the robust kernel"""
    c = case(name)
    kw = dict(linearize_gather=1) if path == "gather" else dict(debug=dict(ell_lanes=int(path)))
    for kind, (kname, delta) in (c["kernels"] or {}).items():
        kw["%s_robust_kernel" % kind] = kname; kw["%s_robust_delta" % kind] = delta
    return kw


def load(G, name):
    """the case into a handle: graph with the polar edges in place, priors, inactive edges"""
    c = case(name)
    plr.load(G, c["g"], c["polar"]); pr.add_to(G, c["pri"])
    for k in c["off"]:
        G.set_edge_active("observation", int(k), False)
    return G


def growth_case(N=40, h=3):
    """(base, tail, full, polar set, prior set) for a plan grown by h keyframes: a chain of N poses, pose p seeing the landmarks p and p + 1
    (numbered by first observation, as conftest.split_for_growth wants them) and p - 1.  The tail holds the ring's and the wrap's geometry:
    tail pose N - 3 at an integer position with heading -0.0 sees an old cone on the negative x-axis with dy = -0; tail pose N - 2 has
    bearings that wrap each way and one at 2 pi exactly (beta = pi, z_beta = -pi) on a tail cone; priors on old and tail vertices"""
    from conftest import split_for_growth
    rng = np.random.default_rng(40)
    P = np.stack([1.0 * np.arange(N), 0.3 * np.sin(0.3 * np.arange(N)), 0.2 * np.sin(0.2 * np.arange(N))], axis=1)
    L = np.stack([1.0 * np.arange(N + 1) + 0.4, 1.5 * (-1.0) ** np.arange(N + 1)], axis=1)
    P[N - 3] = (N - 3.0, 0.0, -0.0); L[N - 4] = (N - 3.0 - 44.0, -0.0)             # negative x in the map as well: the -0 of side_shapes' ring
    P[N - 2] = (N - 2.0, 1.0, 0.0); L[N - 1] = (N - 2.0 - 2.0, 1.0)                # dy = +0, dx = -2 from pose N - 2: beta = pi
    pl = [(p, l) for p in range(N) for l in (p, p + 1, p - 1) if l >= 0]
    pl_p = np.array([a for a, _ in pl], dtype=np.int32); pl_l = np.array([b for _, b in pl], dtype=np.int32)
    pp_i = np.arange(N - 1, dtype=np.int32); pp_j = pp_i + 1
    c, s_ = np.cos(P[pp_i, 2]), np.sin(P[pp_i, 2]); d = P[pp_j, :2] - P[pp_i, :2]
    pp_z = np.stack([c * d[:, 0] + s_ * d[:, 1], -s_ * d[:, 0] + c * d[:, 1], P[pp_j, 2] - P[pp_i, 2]], axis=1) + rng.normal(0, 0.01, (N - 1, 3))
    g = dict(pose_est=P, lm_est=L, pp_i=pp_i, pp_j=pp_j, pp_z=pp_z, pp_info=np.stack([ls._spd3(rng, 1.0) for _ in pp_i]),
             pl_p=pl_p, pl_l=pl_l, pl_z=np.zeros((len(pl), 2)), pl_info=np.stack([ls._spd2(rng, 1.0) for _ in pl]),
             fixed_poses=np.array([0], dtype=np.int32), fixed_landmarks=np.array([1], dtype=np.int32))
    dx, dy = device_d(P[pl_p, 0], P[pl_p, 1], P[pl_p, 2], L[pl_l, 0], L[pl_l, 1])
    g["pl_z"] = np.stack([dx, dy], axis=1) + rng.normal(0, 0.02, (len(pl), 2))
    base, tail, full = split_for_growth(g, h)
    model = np.zeros(len(full["pl_p"]), dtype=np.int32); model[1::3] = RB; model[2::7] = BO
    on_tail = np.flatnonzero(full["pl_p"] >= N - h); model[on_tail] = np.where(np.arange(len(on_tail)) % 3 == 2, BO, RB)
    idx = np.flatnonzero(model > 0)
    dx, dy = device_d(*[full["pose_est"][full["pl_p"][idx], k] for k in range(3)], *[full["lm_est"][full["pl_l"][idx], k] for k in range(2)])
    z = np.stack([np.hypot(dx, dy) + 0.01, np.arctan2(dy, dx) + 0.004], axis=1)
    t2 = np.flatnonzero(full["pl_p"][idx] == N - 2)                                 # pose N - 2: beta - z_beta = +-(pi + 0.5), -+(pi + 1e-5), 2 pi
    beta = np.arctan2(dy, dx); seen = list(full["pl_l"][idx][t2])
    ka, kb, k2 = t2[seen.index(N - 2)], t2[seen.index(N - 3)], t2[seen.index(N - 1)]
    assert beta[ka] * beta[kb] < 0 and min(abs(beta[ka]), abs(beta[kb])) > 0.5
    z[ka, 1] = beta[ka] - np.sign(beta[ka]) * (np.pi + 0.5); z[kb, 1] = beta[kb] - np.sign(beta[kb]) * (np.pi + 1e-5)
    assert beta[k2] == np.pi; z[k2, 1] = -np.pi
    z[:, 1] = np.where((z[:, 1] >= -np.pi) & (z[:, 1] < np.pi), z[:, 1], (z[:, 1] + np.pi) % (2 * np.pi) - np.pi)
    z[model[idx] == BO, 0] = 0.0
    W = np.tile(np.array([[40.0, 3.0], [3.0, 900.0]]), (len(idx), 1, 1)); W[model[idx] == BO] = [[0.0, 0.0], [0.0, 700.0]]
    pol = dict(idx=idx.astype(np.int64), model=model[idx], z=z, W=W)
    pose = [(p, full["pose_est"][p] + rng.normal(0, 0.1, 3) * [1, 1, 0.2], ls._spd3(rng, 0.01).reshape(3, 3), False) for p in (5, N - 3, N - 1)]
    z3, W3 = pr.embed_xy(full["pose_est"][N - 2, :2] + 0.1, ls._spd2(rng, 0.05).reshape(2, 2)); pose.append((N - 2, z3, W3, True))
    lm = [(l, full["lm_est"][l] + rng.normal(0, 0.1, 2), ls._spd2(rng, 0.02).reshape(2, 2)) for l in (3, N - 1, N)]
    return base, tail, full, pol, dict(pose=pose, lm=lm)


_exact = {}


def reference(name, cartesian_route=False):
    """the exact reference of a case at its own estimates: computed once, shared by every path and test"""
    import side_exact_ref as sx
    if (name, cartesian_route) not in _exact:
        c = case(name)
        _exact[name, cartesian_route] = sx.exact(c["g"], c["polar"], c["pri"], c["kernels"], c["off"], cartesian_route=cartesian_route)
    return _exact[name, cartesian_route]
