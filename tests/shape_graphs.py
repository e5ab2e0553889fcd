"""Graphs whose multifrontal plans hold chosen front shapes, and the census of the shapes a set of plans reaches (TEST-ONLY).

The fronts of track graphs come out of nested dissection; nobody chooses them.  Dense pose cliques do: k mutually connected free poses
give a root of 2k pivots and a largest front of 3k scalars, and a landmark seen by every pose of the clique adds 2.  Chains hanging
off a clique give boundaries of 3 j scalars, extra landmarks f = 3 a + 2 b of every size from 2 up, and disconnected components (each
with a fixed pose) plans with more than one root.  A front without boundary rows is always a root (plan_exec.check_invariants), so
"several roots" is the only form of that shape.  The forest's cone seen only from a fixed pose is a component of its own, which the
planner amalgamates into a front of another component: the forest's plan has two roots, not three.

CASES is the set tests/test_gpu_exact.py runs and tests/test_exact_cpu.py's census covers (with the bench and random graphs of the
GPU tests): name -> (builder, the factor variants to run).  A planner change that moves a generator off its shape fails that census on
the CPU, before any GPU run.
"""
import numpy as np


def _spd(rng, n, cond=30.0):
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    return (Q * np.geomspace(1.0, cond, n)) @ Q.T


def _graph(rng, n_poses, n_lms, pp, pl, fixed_poses, fixed_lms=()):
    """a bench_graph dict: estimates scattered over a 20 m square, measurements close to consistent, anisotropic information"""
    pp = np.asarray(pp, dtype=np.int32).reshape(-1, 2); pl = np.asarray(pl, dtype=np.int32).reshape(-1, 2)
    P = np.c_[rng.uniform(0, 20, (n_poses, 2)), rng.uniform(-np.pi, np.pi, n_poses)]
    L = rng.uniform(-5, 25, (n_lms, 2))
    info = lambda n, k: np.array([_spd(rng, n).reshape(n * n) for _ in range(k)]).reshape(k, n * n)
    return dict(pose_est=P, lm_est=L, pp_i=pp[:, 0].copy(), pp_j=pp[:, 1].copy(), pp_z=rng.normal(0, 0.3, (len(pp), 3)),
                pp_info=info(3, len(pp)), pl_p=pl[:, 0].copy(), pl_l=pl[:, 1].copy(), pl_z=rng.normal(0, 3, (len(pl), 2)),
                pl_info=info(2, len(pl)),
                fixed_poses=np.asarray(fixed_poses, dtype=np.int32), fixed_landmarks=np.asarray(fixed_lms, dtype=np.int32))


class _Builder:
    """poses / landmarks / edges of one graph, component by component"""

    def __init__(self):
        self.np = 0; self.nl = 0; self.pp = []; self.pl = []; self.fixed = []

    def poses(self, k):
        a = self.np; self.np += k; return list(range(a, a + k))

    def lms(self, k):
        a = self.nl; self.nl += k; return list(range(a, a + k))

    def clique(self, k_free, lms_all=0, fixed=True):
        """k_free mutually connected free poses (+ a fixed one connected to all of them), lms_all landmarks seen by every pose"""
        ps = self.poses(k_free + (1 if fixed else 0))
        if fixed:
            self.fixed.append(ps[0])
        self.pp += [(a, b) for i, a in enumerate(ps) for b in ps[i + 1:]]
        for l in self.lms(lms_all):
            self.pl += [(p, l) for p in ps]
        return ps

    def chain(self, at, k, lms_each=0):
        """k poses in a chain off pose `at` (odometry edges), each seeing lms_each landmarks of its own"""
        ps = self.poses(k)
        prev = at
        for p in ps:
            self.pp.append((prev, p)); prev = p
            for l in self.lms(lms_each):
                self.pl.append((p, l))
        return ps

    def lms_seen_by(self, ps, k):
        for l in self.lms(k):
            self.pl += [(p, l) for p in ps]

    def done(self, seed):
        return _graph(np.random.default_rng(seed), self.np, self.nl, self.pp, self.pl, self.fixed)


def clique(k_free, lms_all=0, seed=0):
    B = _Builder(); B.clique(k_free, lms_all); return B.done(seed)


def clique_with_chains(k_free, chains, lms_all=0, seed=0):
    """chains: (length, landmarks per pose) hanging off consecutive free poses of the clique"""
    B = _Builder(); ps = B.clique(k_free, lms_all)
    for q, (n, m) in enumerate(chains):
        B.chain(ps[1 + q % k_free], n, m)
    return B.done(seed)


def forest(seed=0):
    """three components, each with its fixed pose: a clique with a chain, a clique with landmarks, and a cone seen only from a fixed pose
    (the cone is amalgamated into a front of the first component: two roots)"""
    B = _Builder()
    ps = B.clique(7, 1); B.chain(ps[3], 6, 1)
    B.clique(5, 3)
    f = B.poses(1)[0]; B.fixed.append(f)
    B.pl += [(f, l) for l in B.lms(1)]
    return B.done(seed)


# name -> (builder, factor variants to run).  Front shapes (npiv, nbnd) of the current planner are checked by the census, not assumed.
CASES = {
    "clique21": (lambda: clique(21), (3, 4)),                                      # f = 63: the last wave front
    "clique20_2lm": (lambda: clique(20, 2), (3, 4)),                               # f = 64: the first workgroup front
    "clique21_1lm": (lambda: clique(21, 1), (3, 4)),                               # f = 65
    "clique53": (lambda: clique(53), (3, 4)),                                      # f = 159: the last workgroup front
    "clique53_1lm": (lambda: clique(53, 1), (4,)),                                 # f = 161: variant 4, k_selinv_big
    "clique32": (lambda: clique(32), (3, 4)),                                      # npiv, f - npiv multiples of 16
    "clique16_chains": (lambda: clique_with_chains(16, [(5, 0), (9, 1), (3, 2)], 1), (3, 4)),
    "forest": (forest, (3, 4)),
}


# the other graphs the exact GPU tests run (bench_cases builds them): name -> factor variants to run
BENCH_VARIANTS = {"bench50": (3, 4), "bench1k": (3, 4), "track400_K16": (3,), "track400_K24": (3,), "random80_v4": (4,)}


def bench_cases(pkg, frontend, bench_graphs):
    """name -> (builder, factor variants) for the graphs of BENCH_VARIANTS"""
    from conftest import random_graph

    def track(K):
        return lambda: pkg.track.bench_graph(pkg.track.generate(400, 150, K), frontend)
    build = {"bench50": lambda: bench_graphs(50, 30)[1], "bench1k": lambda: bench_graphs(1000, 200)[1],
             "track400_K16": track(16), "track400_K24": track(24),
             "random80_v4": lambda: random_graph(5, n_poses=80, n_lms=120, obs_per_pose=40, extra_pp=10)}
    return {name: (build[name], v) for name, v in BENCH_VARIANTS.items()}


def front_shapes(P):
    """(npiv, nbnd, is_root) of every front of a plan_exec.Plan"""
    return [(int(a), int(b), int(p) < 0) for a, b, p in zip(P.npiv, P.nbnd, P.parent)]


def form(f):
    return "wave" if f <= 63 else ("workgroup" if f <= 159 else "hbm")


CELLS = (["factor v3 / selinv wave", "factor v3 / selinv workgroup", "factor v4 / selinv wave", "factor v4 / selinv workgroup",
          "factor v4 / selinv hbm", "f == 63", "f == 64", "f == 159", "f in (160, 161)", "npiv % 16 == 0", "npiv % 16 != 0",
          "npiv <= 16", "npiv > 16", "(f - npiv) % 16 == 0, f > npiv", "several roots"])


def census(plans):
    """plans: (name, Plan, variants).  Returns {cell: [names that hit it]}"""
    hit = {c: [] for c in CELLS}
    for name, P, variants in plans:
        sh = front_shapes(P); fmax = max(a + b for a, b, _ in sh)
        cells = set()
        for v in variants:
            if v == 3 and fmax > 159:
                continue                                    # the plan runs variant 4 whatever was asked
            for a, b, _ in sh:
                cells.add("factor v%d / selinv %s" % (v, form(a + b)))
        for a, b, _ in sh:
            f = a + b
            if f in (63, 64, 159):
                cells.add("f == %d" % f)
            if f in (160, 161):
                cells.add("f in (160, 161)")
            cells.add("npiv % 16 == 0" if a % 16 == 0 else "npiv % 16 != 0")
            cells.add("npiv <= 16" if a <= 16 else "npiv > 16")
            if b > 0 and b % 16 == 0:
                cells.add("(f - npiv) % 16 == 0, f > npiv")
        if sum(r for _, _, r in sh) > 1:
            cells.add("several roots")
        for c in cells:
            hit[c].append(name)
    return hit
