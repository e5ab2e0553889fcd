"""GPU tests of the one-to-one association (k_assign_nn of gs_assoc_nn.hip): each frame's cones matched by ascending (d2, observation, cone).

The cases are the 25 of tests/assoc_nn_shapes.py with their observations grouped into frames by pose (test_assign_nn_cpu.py holds the census:
55 frames, 23 of them contested, every one decided by the exact reference).  Every case runs through SIX paths — gs_assign_nn_batch with
assoc_grid 0, 1, -1, gs_assign_nn_resident with the grid and with brute force, gs_frame_frontend_assign frame by frame — which must agree bit
for bit in index and d2, and each is held to the exact reference (assign_nn_ref.FrameRef).  Independently of that reference the result is
rebuilt from THE DEVICE'S OWN d2(i, j): gs_associate_nn_batch (the parent's code, itself held to the exact reference) on a map that holds cone
j alone returns the device's bits of d2(i, j), the sorted greedy walk runs over that matrix in numpy, and index and d2 must be equal bit for
bit with no exclusions.  Scenes with S = I are exact by construction (every d2 reproducible in numpy from the frame path's own global XY): the
3 x 2 trap that separates the rule from the proposer-only shortcut, a displacement cascade, exact ties in both indices, equality with the
gate, and 256 identical observations against 256 cones (256 rounds, every lane slot in use).  Frames of every size run alone and together
(a wave takes up to eight small frames side by side), and the resident call's defences are held against a pre-filled pattern.

Measured on an MI355X: all 55 frames decided and equal to the exact greedy on all six paths; the walk over the device's own distances equal bit
for bit on every case (528 single-cone calls for map2047, the most); the file runs in under five seconds."""
import ctypes as C

import numpy as np
import pytest

import assign_nn_ref as ar
import assoc_exec as ax
import assoc_nn_shapes as ns

pytestmark = pytest.mark.gpu
PATHS = ("batch grid=0", "batch grid=1", "batch grid=-1", "resident grid", "resident brute", "frame")
FILL_I, FILL_D = 12345, 777.0


@pytest.fixture(scope="module")
def G(pkg):
    if pkg.device_count() < 1:
        pytest.fail("no gfx950 device visible: the HIP path cannot run")
    g = pkg.Graph(lidar_to_cog=ns.LIDAR)
    yield g
    g.close()


def bits(a):
    a = np.asarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def same_bits(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def set_map(G, xy, ty, cov=None):
    G.map_clear()
    if len(ty):
        G.map_append(xy, ty)
        if cov is not None:
            G.map_set_cov(0, cov)
    assert G.map_size() == len(ty)


class Dev:
    """poses, pose indices, observations, frame offsets and pose covariances in device memory; the outputs pre-filled with a pattern"""

    def __init__(self, pkg, poses, pose_of, obs, frame_start, pose_cov=None):
        DA = pkg.binding.DeviceArray; f = lambda a, t: DA(np.ascontiguousarray(a, dtype=t))
        self.n = len(obs); self.np = len(poses); self.nf = len(frame_start) - 1
        self.p, self.po, self.ob, self.fs = f(poses, np.float64), f(pose_of, np.int32), f(obs, np.float64), f(frame_start, np.int32)
        self.pc = None if pose_cov is None else f(pose_cov, np.float64)
        self.idx, self.d2 = f(np.full(self.n, FILL_I), np.int32), f(np.full(self.n, FILL_D), np.float64)

    def assign(self, G, params):
        G.assign_nn_resident(self.p, self.np, self.po, self.ob, self.n, self.nf, self.fs, self.idx, self.d2, self.pc, params); G.synchronize()
        return self.idx.to_host(np.int32, self.n), self.d2.to_host(np.float64, self.n)

    def free(self):
        for a in (self.p, self.po, self.ob, self.fs, self.pc, self.idx, self.d2):
            if a is not None:
                a.free()


def six_paths(pkg, G, poses, pose_of, obs, fs, xy, ty, cov, pose_cov, prm):
    """{path: (idx, d2)} in the order of `obs`; every frame of fs must hold one pose's observations (the frame call takes one pose)"""
    out = {}
    for mode in (0, 1, -1):
        G.set_debug(assoc_grid=mode)
        out["batch grid=%d" % mode] = G.assign_nn(poses, pose_of, obs, fs, xy, ty, cov, pose_cov, prm)
    set_map(G, xy, ty, cov)
    d = Dev(pkg, poses, pose_of, obs, fs, pose_cov)
    out["resident grid"] = d.assign(G, prm)
    G.set_debug(assoc_grid=0)
    out["resident brute"] = d.assign(G, prm)
    G.set_debug(assoc_grid=-1)
    d.free()
    n = len(obs); idx = np.full(n, FILL_I, dtype=np.int32); d2 = np.full(n, FILL_D)
    for f in range(len(fs) - 1):
        a, b = int(fs[f]), int(fs[f + 1])
        if b > a:
            p = int(pose_of[a]); assert (np.asarray(pose_of[a:b]) == p).all()
            _, _, idx[a:b], d2[a:b] = G.frame_frontend_assign(poses[p], obs[a:b], None if pose_cov is None else pose_cov[p], prm)
    out["frame"] = (idx, d2)
    assert tuple(out) == PATHS
    return out


def all_agree(res, tag):
    first = res[PATHS[0]]
    for path, r in res.items():
        assert same_bits(first, r), (tag, path, "differs from", PATHS[0], int((r[0] != first[0]).sum()), int((bits(r[1]) != bits(first[1])).sum()))
    return first


@pytest.fixture(scope="module")
def runs(pkg, G):
    """the six paths of a case, framed by pose, computed once and shared: name -> (order, frame_start, framed case arrays, results)"""
    memo = {}
    def get(name):
        if name not in memo:
            c = ns.case(name); order, fs = ar.frames_by_pose(c["pose_of"])
            po = np.ascontiguousarray(c["pose_of"][order]); ob = np.ascontiguousarray(c["obs"][order])
            prm = pkg.binding.nn_params(**c["params"])
            res = six_paths(pkg, G, c["poses"], po, ob, fs, c["map_xy"], c["map_ty"], c["map_cov"], c["pose_cov"], prm)
            G.map_clear()
            memo[name] = (order, fs, po, ob, prm, res)
        return memo[name]
    return get


@pytest.mark.parametrize("name", ns.NAMES)
def test_every_case_on_every_path_against_the_exact_reference(runs, name):
    order, fs, po, ob, prm, res = runs(name); R = ns.reference(name)
    first = all_agree(res, name)
    decided = contested = 0
    for f in range(len(fs) - 1):
        a, b = int(fs[f]), int(fs[f + 1]); F = ar.FrameRef(R, order[a:b])
        for path, r in res.items():
            bad = F.failures(r[0][a:b], r[1][a:b])
            assert not bad, (name, path, "frame %d" % f, bad[0], "%d fail" % len(bad))
        decided += F.decided; contested += F.contested
    print("%-16s frames %d decided %d contested %d matched %d of %d" % (name, len(fs) - 1, decided, contested, int((first[0] >= 0).sum()), len(ob)))
    assert decided == len(fs) - 1                                          # (the census of test_assign_nn_cpu.py: every frame's indices are the exact greedy's)


def device_matrix(G, c, po, ob, prm, cones):
    """D[i, c] = the device's own bits of d2(i, cones[c]), +inf where the pair is not admissible: gs_associate_nn_batch against that cone alone"""
    D = np.full((len(ob), len(cones)), np.inf)
    for col, j in enumerate(cones):
        idx, d2, _ = G.associate_nn(c["poses"], po, ob, c["map_xy"][j:j + 1], c["map_ty"][j:j + 1], None if c["map_cov"] is None else c["map_cov"][j:j + 1], c["pose_cov"], prm)
        assert ((idx == 0) == np.isfinite(d2)).all()
        D[:, col] = d2
    return D


@pytest.mark.parametrize("name", ns.NAMES)
def test_the_greedy_walk_over_the_devices_own_distances(G, runs, name):
    order, fs, po, ob, prm, res = runs(name); R = ns.reference(name); c = ns.case(name)
    first = res[PATHS[0]]
    frames = range(len(fs) - 1) if name != "random2048" else range(2)     # (a few hundred single-cone calls at the most)
    calls = 0
    for f in frames:
        a, b = int(fs[f]), int(fs[f + 1])
        cones = sorted({cd.j for i in order[a:b] for cd in R.cands[int(i)]})
        D = device_matrix(G, c, po[a:b], ob[a:b], prm, cones); calls += len(cones)
        idx, d2 = ar.greedy(D, cones)
        assert np.array_equal(np.array(idx, dtype=np.int32), first[0][a:b]), (name, f, "index")
        assert np.array_equal(bits(np.array(d2, dtype=np.float64)), bits(first[1][a:b])), (name, f, "d2")
    print("%-16s %d single-cone calls" % (name, calls))
    assert calls <= 600                                                    # (a guard on the test's own cost: map2047 needs 528)


@pytest.mark.parametrize("name", ns.NAMES)
def test_uncontested_frames_equal_the_nearest_cone_call(G, runs, name):
    order, fs, po, ob, prm, res = runs(name); c = ns.case(name)
    first = res[PATHS[0]]
    nn = G.associate_nn(c["poses"], po, ob, c["map_xy"], c["map_ty"], c["map_cov"], c["pose_cov"], prm)
    same = dup = 0
    for f in range(len(fs) - 1):
        a, b = int(fs[f]), int(fs[f + 1])
        if ar.has_duplicates(nn[0][a:b]):
            dup += 1
            assert not ar.has_duplicates(first[0][a:b])
            assert not np.array_equal(nn[0][a:b], first[0][a:b])
        else:
            same += 1
            assert same_bits((nn[0][a:b], nn[1][a:b]), (first[0][a:b], first[1][a:b])), (name, f)
    print("%-16s frames equal to gs_associate_nn_batch %d, with a cone taken twice there %d" % (name, same, dup))


# ---- exact by construction: S = I (sigma_xy = 1, the other sigmas 0, no covariances), so d2 = fl(fl(nu0^2) + fl(nu1^2)) in numpy as on the device
def exact_matrix(g, oty, xy, ty, prm):
    """the header's pair formula for S = I, operation by operation, from the device's own global XY"""
    g = np.asarray(g); xy = np.asarray(xy, dtype=np.float64)
    n0 = xy[None, :, 0] - g[:, None, 0]; n1 = xy[None, :, 1] - g[:, None, 1]
    s = n0 * n0 + n1 * n1
    ok = (np.abs(np.asarray(ty, dtype=np.float64)[None, :] - np.asarray(oty)[:, None]) < prm.type_tol) & (np.sqrt(s) < prm.max_distance) & (s < prm.gate_chi2)
    return np.where(ok, s, np.inf)


def run_exact(pkg, G, obs, xy, ty, tag, **kw):
    """the six paths of one frame of `obs` seen from EQ_POSE against (xy, ty); returns (D, expected idx, expected d2, g) after asserting them"""
    obs = np.ascontiguousarray(obs, dtype=np.float64); k = len(obs); xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2); ty = np.asarray(ty, dtype=np.int32)
    prm = pkg.binding.nn_params(**dict(ns.EQ_SIGMAS, **kw))
    set_map(G, xy, ty)
    zn, g, _, _, _ = G.frame_frontend_nn(ns.EQ_POSE[0], obs, None, prm)
    z, g2, _, _ = G.frame_frontend_assign(ns.EQ_POSE[0], obs, None, prm)
    assert same_bits((zn, g), (z, g2)), (tag, "z / g are not gs_frame_frontend_nn's bits")
    D = exact_matrix(g, obs[:, 3], xy, ty, prm)
    idx, d2 = ar.greedy(D)
    res = six_paths(pkg, G, ns.EQ_POSE, np.zeros(k, dtype=np.int32), obs, np.array([0, k], dtype=np.int32), xy, ty, None, None, prm)
    for path, r in res.items():
        assert np.array_equal(r[0], np.array(idx, dtype=np.int32)), (tag, path, r[0].tolist()[:8], idx[:8])
        assert np.array_equal(bits(r[1]), bits(np.array(d2))), (tag, path)
    G.map_clear()
    return D, idx, d2, g


def device_g(G, obs):
    G.map_clear()
    return G.frame_frontend_nn(ns.EQ_POSE[0], np.ascontiguousarray(obs, dtype=np.float64))[1]


def test_exact_the_trap(pkg, G):
    """d2 = [[a, -], [b, c], [-, d]] with a < b < c < d: the greedy gives [0, 1, -1], the proposer-only shortcut [0, -1, 1].  The two '-' come from
    the types (1, 2, 3 against cones of type 1 and 3 with type_tol 1.5)"""
    base = ns.EQ_OBS[0]; obs = np.array([base, base, base]); obs[:, 2] += (0.0, 0.05, 0.10); obs[:, 3] = (1, 2, 3)
    g = device_g(G, obs); u = (g[2] - g[0]) / np.hypot(*(g[2] - g[0]))
    xy = [g[0] - 0.5 * u, g[0] - 1.5 * u]
    D, idx, d2, _ = run_exact(pkg, G, obs, xy, [1, 3], "trap", type_tol=1.5, gate_chi2=100.0)
    assert np.isinf(D[0, 1]) and np.isinf(D[2, 0]) and D[0, 0] < D[1, 0] < D[1, 1] < D[2, 1], D
    assert idx == [0, 1, -1] and ar.mutual_best(D, proposers_only=True)[0] == [0, -1, 1] and ar.mutual_best(D)[0] == idx


def test_exact_a_displacement_cascade_of_five(pkg, G):
    """five observations that all prefer cone 0, then cone 1, ...: observation i is displaced i times"""
    base = ns.EQ_OBS[1]; obs = np.tile(base, (5, 1)); obs[:, 2] += 0.02 * np.arange(5)
    g = device_g(G, obs); u = (g[4] - g[0]) / np.hypot(*(g[4] - g[0]))
    xy = [g[0] - (0.2 + 0.3 * j) * u for j in range(5)]
    D, idx, d2, _ = run_exact(pkg, G, obs, xy, [3] * 5, "cascade", gate_chi2=100.0)
    assert np.isfinite(D).all() and (np.diff(D, axis=1) > 0).all() and (np.diff(D, axis=0) > 0).all(), D
    assert idx == [0, 1, 2, 3, 4]


def test_exact_identical_observations(pkg, G):
    base = ns.EQ_OBS[2]; two = np.array([base, base]); g = device_g(G, two)
    assert np.array_equal(bits(g[0]), bits(g[1]))
    D, idx, d2, _ = run_exact(pkg, G, two, [g[0] + (0.3, 0.1)], [1], "two observations, one cone", gate_chi2=100.0)
    assert idx == [0, -1] and D[0, 0] == D[1, 0]                           # the lower observation wins, the other gets none
    D, idx, d2, _ = run_exact(pkg, G, two, [g[0] + (0.6, 0.1), g[0] + (0.3, 0.1)], [1, 1], "two observations, two cones", gate_chi2=100.0)
    assert idx == [1, 0] and d2[0] < d2[1]


def _tie_offsets(gx):
    for a in (1.0, 0.5, 2.0, 0.25):
        m1, a1 = ns._offset(gx, a); m2 = gx - a1
        if m2 - gx == -a1:
            return m1, m2, a1
    raise AssertionError("no power of two gives an exact pair of offsets")


def test_exact_a_tie_between_two_cones(pkg, G):
    """cones 0 and 1 at g + (a', 0) and g - (a', 0): the lower cone index wins; a second observation nearer to cone 0 takes it, and the first
    moves to cone 1 at the SAME d2"""
    base = ns.EQ_OBS[0]; cand = np.array([base, base, base]); cand[1, 2] += 0.3; cand[2, 2] -= 0.3
    g = device_g(G, cand); m1, m2, a1 = _tie_offsets(g[0, 0]); xy = [(m1, g[0, 1]), (m2, g[0, 1])]
    D, idx, d2, _ = run_exact(pkg, G, cand[:1], xy, [2, 2], "tie", gate_chi2=100.0)
    assert D[0, 0] == D[0, 1] == a1 * a1 and idx == [0]
    second = 1 if (g[1, 0] - m1) ** 2 + (g[1, 1] - g[0, 1]) ** 2 < a1 * a1 else 2
    D, idx, d2, _ = run_exact(pkg, G, cand[[0, second]], xy, [2, 2], "tie, displaced", gate_chi2=100.0)
    assert D[1, 0] < D[0, 0] == D[0, 1] and D[1, 0] < D[1, 1], D
    assert idx == [1, 0] and d2[0] == a1 * a1


def test_exact_a_displaced_observation_at_the_gate(pkg, G):
    """two identical observations, a near cone and one at d2 = a'^2 exactly: the second observation is displaced to it — admissible only when the
    gate is the next fp64 above that d2 (the test is <)"""
    base = ns.EQ_OBS[3]; two = np.array([base, base]); g = device_g(G, two); m1, _, a1 = _tie_offsets(g[0, 0]); d = a1 * a1
    xy = [(g[0, 0] + 0.125, g[0, 1]), (m1, g[0, 1])]
    D, idx, d2, _ = run_exact(pkg, G, two, xy, [4, 4], "gate, equal", gate_chi2=d)
    assert idx == [0, -1] and np.isinf(D[1, 1])
    D, idx, d2, _ = run_exact(pkg, G, two, xy, [4, 4], "gate, next", gate_chi2=float(np.nextafter(d, np.inf)))
    assert idx == [0, 1] and d2[1] == d


def test_exact_256_identical_observations_against_256_cones(pkg, G):
    """256 rounds and every lane slot in use: observation i gets the cone of rank i by distance"""
    obs = np.tile(ns.EQ_OBS[0], (256, 1)); g = device_g(G, obs[:1])
    rng = np.random.default_rng(9); r = 0.05 + 0.01 * rng.permutation(256); th = rng.uniform(0, 2 * np.pi, 256)
    xy = g[0] + np.stack([r * np.cos(th), r * np.sin(th)], axis=1)
    D, idx, d2, _ = run_exact(pkg, G, obs, xy, [2] * 256, "256 x 256", gate_chi2=100.0)
    assert len(np.unique(D[0])) == 256 and np.isfinite(D).all()
    assert idx == np.argsort(D[0]).tolist() and (np.diff(d2) > 0).all()


# ---- frames, defences, the other calls
def crowded(seed, n, n_cones):
    """one pose, n observations of one type and n_cones cones each 0.5 m (sigma) from some observation: more observations than cones, contests everywhere"""
    rng = np.random.default_rng(seed); poses = np.array([[2.0, -1.0, 0.4]]); ob = ns._obs(rng, n); ob[:, 3] = 1.0
    g = ax.cone_to_global(poses, np.zeros(n, dtype=np.int32), ob, ns.LIDAR)
    xy = g[rng.permutation(n)[:n_cones]] + rng.normal(size=(n_cones, 2)) * 0.5
    return poses, ob, xy, np.ones(n_cones, dtype=np.int32), ns.spd(rng, n_cones)


def test_frames_do_not_interact(pkg, G):
    sizes = (0, 1, 2, 63, 64, 65, 128, 255, 256); fs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    poses, base, xy, ty, cov = crowded(11, 256, 128)
    ob = np.concatenate([base[:s] for s in sizes]); po = np.zeros(len(ob), dtype=np.int32); prm = pkg.binding.nn_params()
    res = six_paths(pkg, G, poses, po, ob, fs, xy, ty, cov, None, prm)
    first = all_agree(res, "frames")
    nn = G.associate_nn(poses, po, ob, xy, ty, cov, None, prm)
    taken = []
    for f, s in enumerate(sizes):
        a, b = int(fs[f]), int(fs[f + 1])
        alone = G.assign_nn(poses, po[a:b], ob[a:b], [0, s], xy, ty, cov, None, prm)
        assert same_bits(alone, (first[0][a:b], first[1][a:b])), ("frame of %d" % s)
        assert not ar.has_duplicates(first[0][a:b])
        taken.append(set(first[0][a:b][first[0][a:b] >= 0].tolist()))
    assert taken[-1] & taken[-2], "a cone taken in two frames"
    a, b = int(fs[-2]), int(fs[-1])
    assert ar.has_duplicates(nn[0][a:b]) and (first[0][a:b] != nn[0][a:b]).sum() >= 10, "the frame of 256 is not contested"
    G.map_clear()


def test_small_frames_share_a_wave_with_large_ones(pkg, G):
    """139 frames of mean size 4.5: a wave takes eight consecutive frames, side by side in 8 lanes each where they fit, in 16 / 32 / 64 lanes and
    several passes where one of the eight is larger (16, 33, 256 here).  Every frame must return what it returns alone"""
    sizes = [1] * 60 + [256] + [2] * 40 + [16, 3, 8, 9, 7, 33, 0, 4] + [5] * 30; fs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    assert len(sizes) == 139 and fs[-1] <= 8 * len(sizes)
    poses, base, xy, ty, cov = crowded(13, 256, 128); rng = np.random.default_rng(13)
    starts = [int(rng.integers(0, 257 - s)) for s in sizes]                # every frame a window of the same 256 observations: they share cones
    ob = np.concatenate([base[st:st + s] for st, s in zip(starts, sizes)]); po = np.zeros(len(ob), dtype=np.int32); prm = pkg.binding.nn_params()
    res = six_paths(pkg, G, poses, po, ob, fs, xy, ty, cov, None, prm)
    first = all_agree(res, "mixed frames")
    moved = 0
    for f, s in enumerate(sizes):
        a, b = int(fs[f]), int(fs[f + 1])
        alone = G.assign_nn(poses, po[a:b], ob[a:b], [0, s], xy, ty, cov, None, prm)
        assert same_bits(alone, (first[0][a:b], first[1][a:b])), ("frame %d of %d" % (f, s))
        nn = G.associate_nn(poses, po[a:b], ob[a:b], xy, ty, cov, None, prm) if s else None
        moved += s > 0 and not np.array_equal(nn[0], alone[0])
    assert moved >= 1, "no frame is contested"
    G.map_clear()


def test_resident_defences(pkg, G):
    """a frame of 257 gets -1 / +inf; frames with bounds outside [0, n] or a > b, and uncovered observations, leave the pre-filled outputs untouched;
    the good frames between them return what they return alone"""
    n = 420; poses, base, xy, ty, cov = crowded(12, n, 200); po = np.zeros(n, dtype=np.int32); prm = pkg.binding.nn_params()
    bad = [0, 257, 300, 340, 700, 350, -5, 345]
    for grid, fs, good in ((-1, bad + [400], [(257, 300), (300, 340), (345, 400)]), (0, bad + [400], [(257, 300), (300, 340), (345, 400)]),
                           (-1, bad + list(range(346, 401)), [(257, 300), (300, 340)] + [(i, i + 1) for i in range(345, 400)])):   # (the last: 62 frames, eight to a wave)
        fs = np.array(fs, dtype=np.int32)
        G.set_debug(assoc_grid=grid)
        set_map(G, xy, ty, cov)
        d = Dev(pkg, poses, po, base, fs, None); idx, d2 = d.assign(G, prm)
        assert (idx[:257] == -1).all() and np.isinf(d2[:257]).all()
        written = np.zeros(n, dtype=bool); written[:257] = True
        for a, b in good:
            alone = G.assign_nn(poses, po[a:b], base[a:b], [0, b - a], xy, ty, cov, None, prm)
            assert same_bits(alone, (idx[a:b], d2[a:b])), (grid, a, b)
            assert b - a == 1 or (alone[0] >= 0).any()
            written[a:b] = True
        assert (idx[~written] == FILL_I).all() and (d2[~written] == FILL_D).all() and (~written).sum() == 25
        class Shifted:
            ptr = C.c_void_p(d.ob.ptr.value + 8)
        rc = pkg.binding.lib().gs_assign_nn_resident(G.h, n - 1, d.p.ptr, 1, d.po.ptr, Shifted.ptr, d.nf, d.fs.ptr, None, C.byref(prm), d.idx.ptr, None)
        assert rc == -1
        d.free()
    G.set_debug(assoc_grid=-1); G.map_clear()


def test_the_existing_calls_are_unchanged_by_assign_calls(pkg, G):
    """gs_associate_nn_resident / gs_associate_resident / gs_frame_frontend_nn return the same bits before and after assign calls on the handle
    (which re-key the resident grid on their own max_distance, as the NN calls do)"""
    c = dict(ns.case("map2047")); prm = pkg.binding.nn_params(); order, fs = ar.frames_by_pose(c["pose_of"])
    po = np.ascontiguousarray(c["pose_of"][order]); ob = np.ascontiguousarray(c["obs"][order])
    set_map(G, c["map_xy"], c["map_ty"], c["map_cov"])
    DA = pkg.binding.DeviceArray; n = len(ob)
    d = Dev(pkg, c["poses"], po, ob, fs, c["pose_cov"]); eo = DA(nbytes=4 * n); ni, nd, nsec = DA(nbytes=4 * n), DA(nbytes=8 * n), DA(nbytes=8 * n)
    def existing():
        G.associate_resident(d.p, d.np, d.po, d.ob, n, 1.2, eo)
        G.associate_nn_resident(d.p, d.np, d.po, d.ob, n, ni, nd, nsec, d.pc, prm); G.synchronize()
        fr = G.frame_frontend_nn(c["poses"][0], ob[:int(fs[1])], c["pose_cov"][0], prm)
        return (eo.to_host(np.int32, n), ni.to_host(np.int32, n), nd.to_host(np.float64, n), nsec.to_host(np.float64, n)) + tuple(fr)
    before = existing()
    assert np.array_equal(before[0], G.associate(c["poses"], po, ob, c["map_xy"], c["map_ty"], 1.2)) and (before[0] >= 0).any()
    assert same_bits(before[1:4], G.associate_nn(c["poses"], po, ob, c["map_xy"], c["map_ty"], c["map_cov"], c["pose_cov"], prm))
    a = d.assign(G, prm); assert same_bits(existing(), before)
    b = d.assign(G, pkg.binding.nn_params(max_distance=0.7)); assert same_bits(existing(), before)
    G.frame_frontend_assign(c["poses"][0], ob[:int(fs[1])], c["pose_cov"][0], prm); assert same_bits(existing(), before)
    G.assign_nn(c["poses"], po, ob, fs, c["map_xy"], c["map_ty"], c["map_cov"], c["pose_cov"], prm); assert same_bits(existing(), before)
    assert same_bits(a, d.assign(G, prm)) and (b[0] >= 0).sum() < (a[0] >= 0).sum()
    for x in (d, eo, ni, nd, nsec):
        x.free()
    G.map_clear()
