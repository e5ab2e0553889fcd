"""Graphs grown by appended keyframes: what k_linearize_tail, the tail arenas and the two read-modify-write paths into base storage must get
right (TEST-ONLY; deterministic).

The base is a graph of tests/lin_shapes.py (70 poses, anisotropic and weak information, the fixed pose 0, a fixed landmark, a hub) at a forced
lane count T; the tail is written out pose by pose below and cut off again with conftest.split_for_growth, so a handle is grown with
conftest.append_tail exactly as the growth tests grow theirs.  A tail observation edge starts at a tail pose, a tail odometry edge has a
tail pose at one end, a tail cone is free (grow_plan refuses anything else).  CASES maps a name to its recipe; the census
(test_tail_exact_cpu.py) proves per case that the plan absorbed the growth and counts each property named here from the graph and the plan.

  tail_min        one tail pose, its odometry edge, one observation of an old cone
  tail_mixed      6 poses in one step (T = 1: tail_mixed, T = 8: tail_mixed_t8), relative to the first tail pose N:
                    N      chain edge from the last old pose; sees old cone A and the tail cone M
                    N + 1  sees A, M (a tail cone seen by two tail poses) and the old FIXED landmark (H_pl exactly zero, no landmark share)
                    N + 2  a second odometry edge to the old pose 30 (not adjacent: an old pose's H_pp receives a tail share); sees A (an old
                           cone seen by three tail poses: its share sums in edge order) and the old cone B
                    N + 3  no observation
                    N + 4  an odometry edge whose older end is the fixed pose 0; sees the tail cone M + 1 and the old cone C
                    N + 5  the tail pose is the i end of its chain edge; sees B, M + 1 and the landmark every wave tile of the base sees
  tail_two_steps  tail_mixed's graph in two steps of 3 poses: the old cone B is seen in both, the export comes after the second (the tail's
                  CSR lists are rebuilt over the whole tail: step 1's shares must appear once)
  tail_wide       the most tail poses the planner admits on a base of 196 landmarks, each seeing 33 old cones: see below
  tail_far        tail_mixed at the kilometre offset lin_shapes.FAR
  tail_robust     tail_mixed with lin_shapes' Cauchy (observation) and Huber (odometry) kernels, deltas from _clear_delta over the FULL graph's
                  s; gross outliers on a tail observation edge and on a tail odometry edge
  tail_wg         test_gpu_exact's K = 16 track cut to WG_POSES poses (the fewest, in steps of 10, whose grown plan holds a workgroup front
                  that was a wave front before), grown by three keyframes one at a time

tail_wide, what the planner admitted (the census asserts every figure): the base has 196 landmarks, each pose four observations, and a root of
41 scalars; fits() in gs_plan.cpp lets the root hold max(63, root_f0 + 24) = 65, so 8 tail poses and no tail cone.  A ninth pose is refused
with "a front would exceed 159 scalars" (the root's limit reads so in a plan that holds workgroup fronts), and so are 16 poses on every base
tried (lin_shapes bases with roots of 41 .. 201 scalars, the K = 16 track cut to 60 .. 250 poses with roots of 60 .. 80: 48 more scalars
need a root of at most 15).  Reached: 8 tail poses, 262 tail observation edges — the loop e += 256 runs a second round —, 195 touched cones —
the loop j += 192 runs a second round.
"""
import numpy as np

import lin_shapes as ls
import robust_ref as rr
from conftest import split_for_growth

OLD_POSE = 30                  # the old pose the second odometry edge of tail_mixed goes to
A, B, C_ = 5, 9, 14            # old cones of tail_mixed (free, observed by the base)
FIXED_LM, WIDE_LM = 1, 0       # lin_shapes.make: the fixed landmark, the landmark every wave tile sees
WG_POSES = 60


def _truth(p):
    p = np.asarray(p, dtype=np.float64)
    return np.stack([0.8 * p, 2.0 * np.sin(0.11 * p), 0.4 * np.sin(0.07 * p + 0.3)], axis=-1)        # lin_shapes.make's trajectory, continued


def _rel_pl(P, L):
    c, s = np.cos(P[2]), np.sin(P[2]); d = L - P[:2]
    return np.array([c * d[0] + s * d[1], -s * d[0] + c * d[1]])


def _rel_pp(xi, xj):
    c, s = np.cos(xi[2]), np.sin(xi[2]); d = xj[:2] - xi[:2]
    return np.array([c * d[0] + s * d[1], -s * d[0] + c * d[1], xj[2] - xi[2]])


def mixed_recipe(N, M, wide):
    """per tail pose: (odometry edges (i, j), observed landmarks); tail cones are M, M + 1"""
    return [([(N - 1, N)], [A, M]),
            ([(N, N + 1)], [A, M, FIXED_LM]),
            ([(N + 1, N + 2), (N + 2, OLD_POSE)], [A, B]),
            ([(N + 2, N + 3)], []),
            ([(N + 3, N + 4), (0, N + 4)], [M + 1, C_]),
            ([(N + 5, N + 4)], [B, M + 1, wide])]


def min_recipe(N, M, wide):
    return [([(N - 1, N)], [A])]


def wide_recipe(n_poses, per_pose, n_new):
    """n_poses tail poses on the chain, each seeing the next per_pose old cones (windows that go round all of them, so that the tail touches
    every free cone) and the first n_new poses a tail cone each, which the next pose sees again"""
    def recipe(N, M, wide):
        out = []
        for t in range(n_poses):
            seen = [l for l in ((t * per_pose + q) % M for q in range(per_pose)) if l != FIXED_LM]
            new = [M + t] if t < n_new else []
            if 0 < t <= n_new:
                new.append(M + t - 1)
            out.append(([(N + t - 1, N + t)], seen + new))
        return out
    return recipe


def grow(base, recipe, seed, far=False, outliers=False):
    """(base, tail, full) in conftest.split_for_growth's form: the base graph with the recipe's poses, cones and edges appended"""
    rng = np.random.default_rng(5000 + seed)
    N, M = len(base["pose_est"]), len(base["lm_est"])
    off = np.array(ls.FAR) if far else np.zeros(2)
    rows = recipe(N, M, WIDE_LM)
    nT = len(rows); new_l = sorted({l for _, obs in rows for l in obs if l >= M})
    assert new_l == list(range(M, M + len(new_l)))
    truth = _truth(np.arange(N + nT))
    lm_true = np.vstack([base["lm_est"] - off, np.zeros((len(new_l), 2))])                      # (an old cone's estimate stands in for its position)
    for l in new_l:
        first = min(t for t, (_, obs) in enumerate(rows) if l in obs)
        lm_true[l] = truth[N + first, :2] + rng.uniform(-6, 6, 2)
    pose_est = truth[N:] + rng.normal(0, 0.03, (nT, 3)) * [1, 1, 0.2]; pose_est[:, :2] += off
    lm_est = lm_true[M:] + rng.normal(0, 0.03, (len(new_l), 2)) + off
    pp, pl = [], []
    for t, (odo, obs) in enumerate(rows):
        for i, j in odo:
            assert max(i, j) == N + t
            pp.append((i, j))
        pl += [(N + t, l) for l in obs]
    pp_z = np.array([_rel_pp(truth[i], truth[j]) for i, j in pp]) + rng.normal(0, 0.01, (len(pp), 3)) * [1, 1, 0.3]
    pl_z = np.array([_rel_pl(truth[p], lm_true[l]) for p, l in pl]).reshape(-1, 2) + rng.normal(0, 0.02, (len(pl), 2))
    pp_info = np.stack([ls._spd3(rng, 1e-3 if k % 5 == 2 else 1.0) for k in range(len(pp))])
    pl_info = np.stack([ls._spd2(rng, 1e-3 if k % 6 == 3 else 1.0) for k in range(len(pl))]) if pl else np.zeros((0, 4))
    if outliers:                                                                                 # wrong cone on a tail edge, slipped odometry on a tail edge
        pl_z[2] += [2.5, -1.5]; pp_z[1] += [0.8, -0.5, 0.1]
    full = dict(base)
    full["pose_est"] = np.vstack([base["pose_est"], pose_est]); full["lm_est"] = np.vstack([base["lm_est"], lm_est])
    cat = lambda k, v, dt=None: np.concatenate([base[k], np.asarray(v, dtype=dt or base[k].dtype).reshape((-1,) + base[k].shape[1:])])
    full["pp_i"] = cat("pp_i", [a for a, _ in pp]); full["pp_j"] = cat("pp_j", [b for _, b in pp]); full["pp_z"] = cat("pp_z", pp_z); full["pp_info"] = cat("pp_info", pp_info)
    full["pl_p"] = cat("pl_p", [a for a, _ in pl]); full["pl_l"] = cat("pl_l", [b for _, b in pl]); full["pl_z"] = cat("pl_z", pl_z); full["pl_info"] = cat("pl_info", pl_info)
    b2, tail, f2 = split_for_growth(full, nT)
    for k in ("pose_est", "lm_est", "pp_i", "pp_j", "pp_z", "pp_info", "pl_p", "pl_l", "pl_z", "pl_info"):
        assert np.array_equal(b2[k], base[k]) and np.array_equal(f2[k], full[k]), k          # the cut gives back what was put together
    return b2, tail, f2


def _case(recipe, T=1, steps=None, **kw):
    d = dict(recipe=recipe, T=T, steps=steps, far=False, robust=False, n_lms=None, full=False, stride=7, kmax=4, seed=0, wg=False); d.update(kw)
    return d


WIDE_POSES, WIDE_PER_POSE, WIDE_NEW, WIDE_LMS = 8, 33, 0, 196

CASES = {
    "tail_min": _case("min", steps=[(0, 1)]),
    "tail_mixed": _case("mixed", steps=[(0, 6)]),
    "tail_mixed_t8": _case("mixed", T=8, steps=[(0, 6)], seed=1),
    "tail_two_steps": _case("mixed", steps=[(0, 3), (3, 6)], seed=2),
    "tail_wide": _case("wide", steps=[(0, WIDE_POSES)], n_lms=WIDE_LMS, full=True, stride=3, seed=3),
    "tail_far": _case("mixed", T=8, steps=[(0, 6)], far=True, seed=4),
    "tail_robust": _case("mixed", steps=[(0, 6)], robust=True, seed=5),
    "tail_wg": _case(None, T=0, steps=[(0, 1), (1, 2), (2, 3)], wg=True),
}
MIXED = ("tail_mixed", "tail_mixed_t8")
_built = {}


def graph(name, pkg=None, frontend=None):
    """(base, tail, full, kernels or None) of a case; built once per process, never changed by a test.  tail_wg needs the package's track
    generator and a front end (the oracle's) the first time"""
    if name not in _built:
        c = CASES[name]
        if c["wg"]:
            t = pkg.track.generate(1000, 200, 16); g = pkg.track.bench_graph(t, frontend)
            base, tail, full = split_for_growth(g, 3, keep=WG_POSES)
            for d in (base, full):                                                               # the cut keeps the lap's cones: only those the stretch sees
                d["fixed_landmarks"] = np.array([l for l in g["fixed_landmarks"] if l < len(d["lm_est"])], dtype=np.int32)
            _built[name] = (base, tail, full, None)
        else:
            g, _, _ = ls.make(N=70, kmax=c["kmax"], T=c["T"], n_lms=c["n_lms"], full=c["full"], stride=c["stride"], seed=c["seed"], far=c["far"], robust=c["robust"])
            recipe = {"min": min_recipe, "mixed": mixed_recipe, "wide": wide_recipe(WIDE_POSES, WIDE_PER_POSE, WIDE_NEW)}[c["recipe"]]
            base, tail, full = grow(g, recipe, c["seed"], far=c["far"], outliers=c["robust"])
            kernels = None
            if c["robust"]:
                s_pp, s_pl = rr.edge_s(full, full["pose_est"], full["lm_est"])
                kernels = {"observation": ("cauchy", ls._clear_delta(s_pl)), "odometry": ("huber", ls._clear_delta(s_pp))}
            _built[name] = (base, tail, full, kernels)
    return _built[name]


def handle_kw(name):
    """keyword arguments of pkg.Graph for the case: the forced lanes (tail_wg: the planner's own), the robust kernels"""
    c = CASES[name]; kernels = _built[name][3] if name in _built else None
    kw = dict(debug=dict(ell_lanes=c["T"])) if c["T"] else {}
    for kind, (kname, delta) in (kernels or {}).items():
        kw["%s_robust_kernel" % kind] = kname; kw["%s_robust_delta" % kind] = delta
    return kw


def tail_edges(name):
    """(indices of the tail's odometry edges, of its observation edges) in the full graph"""
    base, tail, full, _ = _built[name]
    return np.arange(len(base["pp_i"]), len(full["pp_i"])), np.arange(len(base["pl_p"]), len(full["pl_p"]))
