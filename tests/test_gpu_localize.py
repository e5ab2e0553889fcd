"""GPU tests of frame localisation (k_localize / k_localize_big of gs_assoc_nn.hip): the iterated pose refinement of a frame under its
hypothesis, the posterior covariance and chi2.

THREE paths — gs_localize_batch, gs_localize_resident, gs_frame_frontend_localize frame by frame — and BOTH kernels (gs_debug_localize forces
either) run one device function and must agree bit for bit in pose, covariance, chi2, the counts and the status.  Each frame is held to the exact
reference (localize_ref.Frame): pose, every covariance entry and chi2 within the derived bound B; where the reference is DECIDED (every pair
test sure, every stop comparison with 1000 B to spare) iterations and status are its own; a frame reported converged has an exact Gauss-Newton
step at the RETURNED pose of at most the tolerance plus B, and its covariance is the dense (Sigma_p^-1 + M)^-1 at that pose within B — two
checkers that do not repeat the iteration.  With max_iterations = 1 the step d_f (read through gs_debug_localize's output) is bitwise the delta
of gs_joint_compat_batch.  The shift scene, its cones placed from the device's own z, is exact in binary and asserted as bits.

Measured on an MI355X (the tests print these figures with -s): the 12 purpose-made scenes all decided, counts and status the reference's; the
rotation scene converges in 3 solves and one step stays 4.6 mm and 1.7e-4 rad away; over the file's 68 held frames (43 undecided under the
pessimistic B, 3 more refused by the reference) the largest |device - exact| / B is 0.0114 (grid_twice; 0.0088 on the scenes); the file runs in about
seven seconds."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import assign_nn_ref as ar
import assoc_nn_shapes as ns
import localize_ref as lr
import localize_shapes as ls

pytestmark = pytest.mark.gpu
FILL_I, FILL_D = 12345, 777.0
WORST = {"r": 0.0, "frames": 0, "where": "", "iters": {}, "refused": 0, "undecided": 0}
DEFAULT = dict(max_iterations=5, tol_xy=1e-6, tol_theta=1e-8)


@pytest.fixture(scope="module")
def G(pkg):
    if pkg.device_count() < 1:
        pytest.fail("no gfx950 device visible: the HIP path cannot run")
    g = pkg.Graph(lidar_to_cog=ns.LIDAR)
    yield g
    g.close()
    print("\nlocalisation: %d frames held to the exact reference (%d undecided, %d refused by the reference), iterations %s; largest |device - exact| / B %.3g (%s)" % (
        WORST["frames"], WORST["undecided"], WORST["refused"], dict(sorted(WORST["iters"].items())), WORST["r"], WORST["where"]))


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


def flat(rec):
    """a record as a tuple of arrays: (pose [3 f], cov [9 f], chi2, n_pairs, iterations, status)"""
    return (np.asarray(rec["pose"]).reshape(-1), np.asarray(rec["cov"]).reshape(-1), np.asarray(rec["chi2"]), np.asarray(rec["n_pairs"]),
            np.asarray(rec["iterations"]), np.asarray(rec["status"]))


def frame_of(r, f):
    return r[0][3 * f:3 * f + 3], r[1][9 * f:9 * f + 9], float(r[2][f]), int(r[3][f]), int(r[4][f]), int(r[5][f])


class Dev:
    """a call's inputs in device memory, every output pre-filled with a pattern"""

    def __init__(self, pkg, poses, pose_of, obs, frame_start, hyp, pose_cov=None, n_poses=None):
        DA = pkg.binding.DeviceArray; f = lambda a, t: DA(np.ascontiguousarray(a, dtype=t))
        self.n = len(obs); self.np = len(poses) if n_poses is None else n_poses; self.nf = len(frame_start) - 1
        self.p, self.po, self.ob, self.fs, self.hyp = f(poses, np.float64), f(pose_of, np.int32), f(obs, np.float64), f(frame_start, np.int32), f(hyp, np.int32)
        self.pc = None if pose_cov is None else f(pose_cov, np.float64)
        nf = max(self.nf, 1)
        self.pose = f(np.full(3 * nf, FILL_D), np.float64); self.cov = f(np.full(9 * nf, FILL_D), np.float64); self.chi2 = f(np.full(nf, FILL_D), np.float64)
        self.step = f(np.full(3 * nf, FILL_D), np.float64)
        self.pairs, self.it, self.st = (f(np.full(nf, FILL_I), np.int32) for _ in range(3))

    def run(self, G, prm, loc):
        G.localize_resident(self.p, self.np, self.po, self.ob, self.n, self.nf, self.fs, self.hyp, self.pose, self.cov, self.chi2, self.pairs, self.it, self.st,
                            self.pc, prm, loc); G.synchronize()
        nf = self.nf
        return (self.pose.to_host(np.float64, 3 * nf), self.cov.to_host(np.float64, 9 * nf), self.chi2.to_host(np.float64, nf), self.pairs.to_host(np.int32, nf),
                self.it.to_host(np.int32, nf), self.st.to_host(np.int32, nf))

    def steps(self):
        return self.step.to_host(np.float64, 3 * self.nf)

    def free(self):
        for a in (self.p, self.po, self.ob, self.fs, self.hyp, self.pc, self.pose, self.cov, self.chi2, self.step, self.pairs, self.it, self.st):
            if a is not None:
                a.free()


def paths(pkg, G, poses, po, ob, fs, xy, ty, cov, pose_cov, hyp, prm, loc):
    """{path: flat result}: the batch and the resident call, each on k_localize, on k_localize_big and as the launcher chooses; leaves the map resident"""
    out = {}
    set_map(G, xy, ty, cov)
    d = Dev(pkg, poses, po, ob, fs, hyp, pose_cov)
    for kernel, tag in ((0, "small"), (1, "big"), (-1, "auto")):
        G.debug_localize(kernel)
        out["batch " + tag] = flat(G.localize(poses, po, ob, fs, xy, hyp, cov, pose_cov, prm, loc))
        out["resident " + tag] = d.run(G, prm, loc)
    d.free()
    return out


def all_agree(res, tag):
    first = res["batch auto"]
    for path, r in res.items():
        assert same_bits(first, r), (tag, path, "differs from batch", [int((bits(x) != bits(y)).sum()) for x, y in zip(first, r)])
    cv = first[1].reshape(-1, 3, 3)
    assert same_bits((cv,), (cv.transpose(0, 2, 1),)), (tag, "the covariance is not bitwise symmetric")
    return first


def hold(F, r, f, tag, kw, checkers=True):
    """frame f of the flat result r against the reference; frames the reference refuses to bound (a divisor not surely away from zero) are counted"""
    rec = frame_of(r, f)
    try:
        bad = F.failures(rec, checkers=checkers, **kw)
    except AssertionError as e:
        assert "divisor" in str(e) or "tiny" in str(e), e
        WORST["refused"] += 1
        return None
    assert not bad, (tag, "frame %d" % f, bad[0], "%d fail" % len(bad), rec)
    WORST["frames"] += 1; WORST["undecided"] += not F.res.decided
    WORST["iters"][rec[4]] = WORST["iters"].get(rec[4], 0) + 1
    if F.worst > WORST["r"]:
        WORST["r"] = F.worst; WORST["where"] = str(tag)
    return F.res


def frame_call_agrees(pkg, G, pose, ob, pc, prm, jc, loc, xy, cov):
    """gs_frame_frontend_localize on one frame against the resident map: its first outputs are gs_frame_frontend_jc's bit for bit, its record is the
    batch call's on the pruned index"""
    r = G.frame_frontend_localize(pose, ob, pc, prm, jc, loc); j = G.frame_frontend_jc(pose, ob, pc, prm, jc)
    assert same_bits(r[:5], j[:5]) and same_bits([r[5][k] for k in sorted(r[5])], [j[5][k] for k in sorted(j[5])]), "the frame call's first outputs are not gs_frame_frontend_jc's"
    if len(ob) == 0:
        return r
    own = flat(G.localize([pose], np.zeros(len(ob), dtype=np.int32), ob, [0, len(ob)], xy, r[2], cov, None if pc is None else [pc], prm, loc))
    assert same_bits(flat(r[6]), own), ("the frame call differs from the batch call on its pruned index", flat(r[6]), own)
    return r


# ---- the purpose-made scenes
@pytest.mark.parametrize("name", ls.NAMES)
def test_the_purpose_made_scenes(pkg, G, name):
    c = ls.scene(name); b = pkg.binding; prm = b.nn_params(**c["params"]); loc = b.loc_params(**c["loc"]); kw = dict(DEFAULT, **c["loc"])
    res = paths(pkg, G, c["poses"], c["pose_of"], c["obs"], c["frame_start"], c["map_xy"], c["map_ty"], None, c["pose_cov"], c["hyp"], prm, loc)
    first = all_agree(res, name)
    F = lr.make(c, c["hyp"], c["frame_start"])[0]
    r = hold(F, first, 0, name, kw)
    assert r is not None and r.decided, name
    if c["expect"] is not None:
        assert (first[5][0], first[4][0]) == c["expect"], (name, first[5][0], first[4][0])
    pc = None if c["pose_cov"] is None else c["pose_cov"][0]
    fr = frame_call_agrees(pkg, G, c["poses"][0], c["obs"], pc, prm, b.jc_params(), loc, c["map_xy"], None)
    if np.array_equal(fr[2], c["hyp"]):
        assert same_bits(flat(fr[6]), first), (name, "the frame call differs")
    if name == "none":
        assert same_bits((first[0], first[1]), (c["poses"][0], c["pose_cov"][0])) and first[2][0] == 0.0 and first[3][0] == 0
    if name == "nocov":
        own = G.associate_nn(c["poses"], c["pose_of"], c["obs"], c["map_xy"], c["map_ty"], None, None, prm)
        lanes = [float(x) for x in own[1]] + [0.0] * 56
        for off in (32, 16, 8, 4, 2, 1):
            lanes = [lanes[l] + lanes[l ^ off] for l in range(64)]
        assert np.array_equal(own[0], c["hyp"]) and first[2][0] == lanes[0] and not first[1].any()
    if name in ("nonfinite", "nanquery"):
        assert first[3][0] == 7 and first[5][0] == 0
    print("%-15s status %d iterations %d pairs %d pose (%.12g, %.12g, %.12g) chi2 %.9g largest |device - exact| / B %.3g" % (
        name, first[5][0], first[4][0], first[3][0], *first[0][:3], first[2][0], F.worst))
    G.map_clear()


def test_one_step_stays_far_from_the_converged_pose(pkg, G):
    """the rotation scene: what max_iterations = 1 returns (the joint test's delta applied) is more than 1000 B from the converged pose"""
    c = ls.scene("rotation"); b = pkg.binding; prm = b.nn_params(**c["params"])
    run = lambda **kw: flat(G.localize(c["poses"], c["pose_of"], c["obs"], c["frame_start"], c["map_xy"], c["hyp"], None, c["pose_cov"], prm, b.loc_params(**kw)))
    one, full = run(max_iterations=1), run()
    F = lr.make(c, c["hyp"], c["frame_start"])[0]; r1, r5 = F.run(max_iterations=1), F.run()
    assert full[5][0] == 0 and one[5][0] == 1 and one[4][0] == 1
    for t in range(3):
        assert abs(one[0][t] - full[0][t]) > 1000 * float(2 * (r1.pose[t].e + r5.pose[t].e)), t
    assert abs(one[0][0] - full[0][0]) > 4e-3 and one[2][0] > full[2][0] + 1e-3
    print("rotation: one step (%.9g, %.9g, %.9g) chi2 %.6g; converged in %d: (%.9g, %.9g, %.9g) chi2 %.6g" % (*one[0], one[2][0], full[4][0], *full[0], full[2][0]))


def test_the_shift_scene_is_exact_in_binary(pkg, G):
    """the cones placed from the DEVICE's z at z + (-1/2, 0): every quantity of both solves and of the final pass is exact, so the bits are known"""
    b = pkg.binding; base = ls.scene("shift"); prm = b.nn_params(**base["params"]); loc = b.loc_params()
    set_map(G, base["map_xy"], base["map_ty"])
    z = G.frame_frontend_jc(base["poses"][0], base["obs"], None, prm, b.jc_params())[0]
    c = ls.scene("shift", z)
    for i in (0, 1, 2):                                                      # the precondition, in rationals: z_x - 1/2 and z_x - 3/8 are fp64 numbers
        assert z[i, 0] > 0.5
        for s in (Fraction(1, 2), Fraction(3, 8)):
            assert Fraction(float(z[i, 0] - float(s))) == Fraction(float(z[i, 0])) - s
    res = paths(pkg, G, c["poses"], c["pose_of"], c["obs"], c["frame_start"], c["map_xy"], c["map_ty"], None, c["pose_cov"], c["hyp"], prm, loc)
    first = all_agree(res, "shift, exact")
    assert np.array_equal(first[0], [-0.375, 0.0, 0.0]) and np.array_equal(first[1], [0.25, 0, 0, 0, 0.25, 0, 0, 0, 0]), (first[0], first[1])
    assert first[2][0] == 0.1875 and first[3][0] == 3 and first[4][0] == 2 and first[5][0] == 0
    d = Dev(pkg, c["poses"], c["pose_of"], c["obs"], c["frame_start"], c["hyp"], c["pose_cov"])
    G.debug_localize(-1, d.step); d.run(G, prm, loc); G.debug_localize(-1, None)
    assert np.array_equal(d.steps(), [-0.375, 0.0, 0.0]); d.free()
    G.map_clear()


# ---- max_iterations = 1 is the joint test's delta, bit for bit
def one_step_is_delta(pkg, G, c, po, ob, fs, hyp, prm, tag):
    b = pkg.binding; jc = b.jc_params(); loc = b.loc_params(max_iterations=1)
    pruned, rec = G.joint_compat(c["poses"], po, ob, fs, c["map_xy"], hyp, c["map_cov"], c["pose_cov"], prm, jc)
    set_map(G, c["map_xy"], c["map_ty"], c["map_cov"])
    d = Dev(pkg, c["poses"], po, ob, fs, pruned, c["pose_cov"]); n = 0
    for kernel in (0, 1):
        G.debug_localize(kernel, d.step); r = d.run(G, prm, loc); st = d.steps().reshape(-1, 3)
        for f in range(len(fs) - 1):
            if r[5][f] == 3 or not np.isfinite(rec["delta"][f]).all():
                continue
            assert same_bits((st[f],), (rec["delta"][f],)), (tag, kernel, f, st[f], rec["delta"][f])
            assert r[3][f] <= rec["n_kept"][f] and r[4][f] == (1 if c["pose_cov"] is not None and rec["n_kept"][f] > 0 else 0); n += 1
    G.debug_localize(-1, None); d.free()
    return pruned, n


def test_one_iteration_is_the_joint_delta_on_the_scenes(pkg, G):
    n = 0
    for name in ls.NAMES:
        c = ls.scene(name); prm = pkg.binding.nn_params(**c["params"])
        n += one_step_is_delta(pkg, G, c, c["pose_of"], c["obs"], c["frame_start"], c["hyp"], prm, name)[1]
    assert n >= 2 * (len(ls.NAMES) - 1)
    G.map_clear()


# ---- the 25 inherited cases, framed by pose, with gs_joint_compat_batch's pruned index
@pytest.mark.parametrize("name", ns.NAMES)
def test_inherited_scenes(pkg, G, name):
    c = ns.case(name); order, fs = ar.frames_by_pose(c["pose_of"]); b = pkg.binding
    po = np.ascontiguousarray(c["pose_of"][order]); ob = np.ascontiguousarray(c["obs"][order]); prm = b.nn_params(**c["params"]); loc = b.loc_params(); jc = b.jc_params()
    hyp = G.assign_opt(c["poses"], po, ob, fs, c["map_xy"], c["map_ty"], c["map_cov"], c["pose_cov"], prm)[0]
    pruned, n = one_step_is_delta(pkg, G, c, po, ob, fs, hyp, prm, name)
    res = paths(pkg, G, c["poses"], po, ob, fs, c["map_xy"], c["map_ty"], c["map_cov"], c["pose_cov"], pruned, prm, loc)
    first = all_agree(res, name)
    Fs = lr.make(c, pruned, fs, order, ns.reference(name).R)
    for f, F in enumerate(Fs):
        a, e = int(fs[f]), int(fs[f + 1])
        hold(F, first, f, name, DEFAULT)                                      # with both non-repeating checkers
        if 0 < e - a <= 256:
            p = int(po[a]); pc = None if c["pose_cov"] is None else c["pose_cov"][p]
            fr = frame_call_agrees(pkg, G, c["poses"][p], ob[a:e], pc, prm, jc, loc, c["map_xy"], c["map_cov"])
            if np.array_equal(fr[2], pruned[a:e]):
                assert same_bits(flat(fr[6]), [np.asarray(x) for x in (first[0][3 * f:3 * f + 3], first[1][9 * f:9 * f + 9], first[2][f:f + 1], first[3][f:f + 1],
                                                                      first[4][f:f + 1], first[5][f:f + 1])]), (name, f)
    print("%-16s frames %d status %s iterations %s; so far: %d frames held (%d undecided, %d refused by the reference), iterations %s, worst |device - exact| / B %.3g (%s)" % (
        name, len(fs) - 1, np.bincount(first[5], minlength=4).tolist(), np.bincount(first[4]).tolist(), WORST["frames"], WORST["undecided"], WORST["refused"],
        dict(sorted(WORST["iters"].items())), WORST["r"], WORST["where"]))
    G.map_clear()


# ---- frame sizes, sharing a call
def crowded(seed, n, n_cones):
    """one pose, n observations of one type, n_cones cones each 0.3 m (sigma) from some observation, random covariances, a small pose covariance"""
    import assoc_exec as ax
    rng = np.random.default_rng(seed); poses = np.array([[2.0, -1.0, 0.4]]); ob = ns._obs(rng, n); ob[:, 3] = 1.0
    g = ax.cone_to_global(poses, np.zeros(n, dtype=np.int32), ob, ns.LIDAR)
    xy = g[rng.permutation(n)[:n_cones]] + rng.normal(size=(n_cones, 2)) * 0.3
    return poses, ob, xy, np.ones(n_cones, dtype=np.int32), ns.spd(rng, n_cones, 0.01, 0.05), ns.pose_covs(rng, 1)


SIZES = (0, 1, 2, 3, 63, 64, 65, 255, 256)


@pytest.fixture(scope="module")
def sized(pkg, G):
    """nine frames, each a prefix of the same 256 observations, in one call; the hypothesis of gs_assign_opt_batch"""
    poses, base, xy, ty, cov, pcv = crowded(21, 256, 200); fs = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    ob = np.concatenate([base[:s] for s in SIZES]); po = np.zeros(len(ob), dtype=np.int32); prm = pkg.binding.nn_params()
    hyp = G.assign_opt(poses, po, ob, fs, xy, ty, cov, pcv, prm)[0]
    case = dict(lidar=ns.LIDAR, poses=poses, pose_of=np.zeros(256, dtype=np.int32), obs=base, map_xy=xy, map_cov=cov, pose_cov=pcv, params={})
    return dict(poses=poses, base=base, xy=xy, ty=ty, cov=cov, pcv=pcv, fs=fs, ob=ob, po=po, prm=prm, hyp=hyp, case=case,
                order=np.concatenate([np.arange(s) for s in SIZES]))


def test_frame_sizes_share_a_call(pkg, G, sized):
    """frames of 0 .. 256 in one call and each alone: identical bits — the lanes a frame is given and its neighbours in the wave do not matter"""
    s = sized; loc = pkg.binding.loc_params()
    res = paths(pkg, G, s["poses"], s["po"], s["ob"], s["fs"], s["xy"], s["ty"], s["cov"], s["pcv"], s["hyp"], s["prm"], loc)
    first = all_agree(res, "sizes")
    Fs = lr.make(s["case"], s["hyp"], s["fs"][:8], s["order"])
    for f, k in enumerate(SIZES):
        a, b = int(s["fs"][f]), int(s["fs"][f + 1])
        if k in (1, 2, 3, 65):                                               # the exact reference where it is quick; the rest by the identities below
            hold(Fs[f], first, f, "sizes %d" % k, DEFAULT)
        for kernel in (0, 1):
            G.debug_localize(kernel)
            alone = flat(G.localize(s["poses"], s["po"][a:b], s["ob"][a:b], [0, k], s["xy"], s["hyp"][a:b], s["cov"], s["pcv"], s["prm"], loc))
            assert same_bits(alone, [np.asarray(x).reshape(-1) for x in frame_of(first, f)]), ("frame of %d alone" % k, kernel)
        G.debug_localize(-1)
        fr = frame_call_agrees(pkg, G, s["poses"][0], s["ob"][a:b], s["pcv"][0], s["prm"], pkg.binding.jc_params(), loc, s["xy"], s["cov"])
        if k == 0:                                                           # no launch: the given pose and covariance, status 2
            m = s["pcv"][0].reshape(3, 3); m = np.triu(m) + np.triu(m, 1).T
            assert same_bits(flat(fr[6])[:2], (s["poses"][0], m.reshape(-1))) and fr[6]["status"][0] == 2 and fr[6]["chi2"][0] == 0.0
    assert first[5][0] == 2 and not first[0][:3].any() and (first[3][1:] > 0).all() and (first[5][1:] <= 1).all(), (first[3], first[5])
    print("sizes %s pairs %s iterations %s status %s" % (SIZES, first[3].tolist(), first[4].tolist(), first[5].tolist()))
    G.map_clear()


# ---- the resident call's defences
def test_resident_defences(pkg, G, sized):
    """a frame of 257 and a frame with two poses get status 4 (zeros, chi2 +inf); frames with bounds outside [0, n] or a > b leave the pre-filled
    pattern; an index outside the map (or below -1) never counts; the good frames between them return what they return alone; every output
    may be left out; on both kernels"""
    s = sized; n = 420; b = pkg.binding; loc = b.loc_params()
    ob = np.concatenate([s["base"], s["base"][:n - 256]]); po = np.zeros(n, dtype=np.int32); poses = np.concatenate([s["poses"], s["poses"] + 0.5])
    pcv = np.concatenate([s["pcv"], s["pcv"]])
    set_map(G, s["xy"], s["ty"], s["cov"]); m = len(s["xy"])
    hyp = G.assign_opt(poses, po, ob, [0, 256, n], s["xy"], s["ty"], s["cov"], None, s["prm"])[0]
    po[310] = 1                                                              # the frame [300, 340) names two poses
    hyp[262] = m; hyp[263] = -7; hyp[264] = 2 ** 30                          # outside the map: never count
    head = [0, 257, 300, 340, 700, 350, -5, 345]
    for fs, good in ((head + [400], [(1, (257, 300)), (7, (345, 400))]),
                     (head + list(range(346, 401)), [(1, (257, 300)), (7, (345, 346)), (30, (368, 369)), (61, (399, 400))])):
        fs = np.array(fs, dtype=np.int32); nf = len(fs) - 1
        for kernel in (0, 1, -1):
            G.debug_localize(kernel)
            d = Dev(pkg, poses, po, ob, fs, hyp, pcv); r = d.run(G, s["prm"], loc)
            for f in (0, 2):                                                 # above GS_NN_FRAME_MAX; two poses
                assert r[5][f] == 4 and np.isinf(r[2][f]) and r[3][f] == r[4][f] == 0 and not r[0][3 * f:3 * f + 3].any() and not r[1][9 * f:9 * f + 9].any(), (kernel, f)
            for f in (3, 4, 5, 6):                                           # 340..700, 700..350, 350..-5, -5..345: not frames of this call
                assert r[2][f] == FILL_D and r[3][f] == r[4][f] == r[5][f] == FILL_I and (r[0][3 * f:3 * f + 3] == FILL_D).all() and (r[1][9 * f:9 * f + 9] == FILL_D).all(), (kernel, f)
            for f, (a, e) in good:
                h = hyp[a:e].copy(); h[(h < -1) | (h >= m)] = -1
                alone = flat(G.localize(poses, po[a:e], ob[a:e], [0, e - a], s["xy"], h, s["cov"], pcv, s["prm"], loc))
                assert same_bits(alone, [np.asarray(x).reshape(-1) for x in frame_of(r, f)]), (kernel, f, a, e)
            lib = b.lib()                                                    # every output left out: nothing to write, and no error
            assert lib.gs_localize_resident(G.h, n, d.p.ptr, 2, d.po.ptr, d.ob.ptr, nf, d.fs.ptr, d.pc.ptr, C.byref(s["prm"]), C.byref(loc), d.hyp.ptr,
                                            None, None, None, None, None, None) == 0
            shifted = C.c_void_p(d.ob.ptr.value + 8)
            assert lib.gs_localize_resident(G.h, n - 1, d.p.ptr, 2, d.po.ptr, shifted, nf, d.fs.ptr, None, C.byref(s["prm"]), C.byref(loc), d.hyp.ptr,
                                            None, None, None, None, None, None) == -1
            G.synchronize(); d.free()
    G.debug_localize(-1); G.map_clear()


def test_the_posterior_fed_back_as_the_prior_does_not_move(pkg, G):
    """the wide scene: Sigma_p^-1 = 2^-20 I, so the measurements alone fix the pose and the posterior (pose, cov) as the prior of the same frame is
    already at its maximum: one more solve moves the pose by (Sigma+^-1 + M)^-1 Sigma_p^-1 d_f, below 1e-7 of d_f here — at most the tolerance plus B"""
    c = ls.scene("wide"); b = pkg.binding; prm = b.nn_params(**c["params"])
    a = flat(G.localize(c["poses"], c["pose_of"], c["obs"], c["frame_start"], c["map_xy"], c["hyp"], None, c["pose_cov"], prm, b.loc_params()))
    assert a[5][0] == 0
    again = flat(G.localize([a[0]], c["pose_of"], c["obs"], c["frame_start"], c["map_xy"], c["hyp"], None, [a[1]], prm, b.loc_params(max_iterations=1)))
    r = lr.make(c, c["hyp"], c["frame_start"])[0].run()
    for t, tol in enumerate((1e-6, 1e-6, 1e-8)):
        assert abs(again[0][t] - a[0][t]) <= tol + float(2 * r.pose[t].e), (t, again[0][t] - a[0][t])
    print("fed back: the pose moves by (%.3g, %.3g, %.3g)" % tuple(again[0] - a[0]))


def test_the_existing_calls_are_unchanged_by_localisation_calls(pkg, G):
    c = dict(ns.case("map257")); b = pkg.binding; prm = b.nn_params(); jc = b.jc_params(); order, fs = ar.frames_by_pose(c["pose_of"])
    po = np.ascontiguousarray(c["pose_of"][order]); ob = np.ascontiguousarray(c["obs"][order]); k0 = int(fs[1])
    set_map(G, c["map_xy"], c["map_ty"], c["map_cov"])
    def existing():
        r = G.frame_frontend_jc(c["poses"][0], ob[:k0], c["pose_cov"][0], prm, jc)
        out = tuple(r[:5]) + tuple(r[5][k] for k in sorted(r[5]))
        hyp = G.assign_opt(c["poses"], po, ob, fs, c["map_xy"], c["map_ty"], c["map_cov"], c["pose_cov"], prm)[0]
        return out + tuple(G.joint_compat(c["poses"], po, ob, fs, c["map_xy"], hyp, c["map_cov"], c["pose_cov"], prm, jc)[:1])
    before = existing(); hyp = before[-1]
    G.localize(c["poses"], po, ob, fs, c["map_xy"], hyp, c["map_cov"], c["pose_cov"], prm); assert same_bits(existing(), before)
    G.frame_frontend_localize(c["poses"][0], ob[:k0], c["pose_cov"][0], prm, jc); assert same_bits(existing(), before)
    d = Dev(pkg, c["poses"], po, ob, fs, hyp, c["pose_cov"]); d.run(G, prm, b.loc_params()); d.free(); assert same_bits(existing(), before)
    G.map_clear()
    # one gs_iterate on a handle that has localised equals one on a handle that has not
    t = pkg.track.generate(50, 30); fe = pkg.Graph(device=0); g = pkg.track.bench_graph(t, fe); fe.close(); out = []
    for localise in (False, True):
        H = pkg.Graph(device=0); H.load_bench_graph(g)
        if localise:
            H.localize(c["poses"], po, ob, fs, c["map_xy"], hyp, c["map_cov"], c["pose_cov"], prm)
            H.frame_frontend_localize(c["poses"][0], ob[:k0], c["pose_cov"][0], prm, jc)
        H.initialize_optimization(); H.iterate(); out.append((H.poses(), H.landmarks())); H.close()
    assert same_bits(out[0], out[1])
