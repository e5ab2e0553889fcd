"""GPU tests of the joint compatibility test (k_joint_compat / k_joint_compat_big of gs_assoc_nn.hip): a frame's hypothesis gated as a whole,
pruned by backward elimination, with the pose correction its kept pairs imply.

THREE paths — gs_joint_compat_batch, gs_joint_compat_resident, gs_frame_frontend_jc frame by frame — run one device function and must agree
bit for bit in the pruned index, J, the three counts and delta.  Each is held to the exact reference (joint_compat_ref.FrameRef): every
result must be VALID (kept pairs out of the hypothesis, J of the reported kept set within the derived bound B, J < gate[n_kept], counts
that add up); where the reference is DECIDED (every comparison with 1000 B to spare) the kept set, the counts, J and delta are its own.
The purpose-made scenes (joint_compat_shapes.py: heading 0, sigma_range = sigma_bearing = 0, zero cone covariance, Sigma_p diagonal in powers
of two, in two regimes) are in addition reproduced in numpy fp64 from the device's own z and g, operation by operation in the header's order,
and compared BIT FOR BIT: pair terms, the fixed-order sums, the 3x3 solve, every round of the elimination.  Frame sizes 0 .. 256 share calls;
the 25 cases of assoc_nn_shapes.py are framed by pose with the hypothesis of gs_assign_opt_batch; a frame of 257, bad bounds, a frame with two
poses and an index outside the map go through the resident defences.

Measured on an MI355X (the tests print these figures with -s): the 12 purpose-made scenes all decided, equal to the reference and to the numpy
reproduction bit for bit on all three paths; of the 55 inherited frames 85 pairs dropped, none untestable; over the file's 110 held frames the
largest |J_device - J_exact| / B is 0.056 (grid_twice; 0.0035 on the purpose-made scenes), 57 of them left after one round; the file runs in
under six seconds."""
import ctypes as C

import numpy as np
import pytest

import assign_nn_ref as ar
import assoc_nn_shapes as ns
import joint_compat_ref as jr
import joint_compat_shapes as js

pytestmark = pytest.mark.gpu
FILL_I, FILL_D = 12345, 777.0
WORST = {"r": 0.0, "frames": 0, "one_round": 0}


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


def flat(idx, rec):
    """a result as a tuple of arrays: (index, J, n_kept, n_dropped, n_untestable, delta)"""
    return (np.asarray(idx), np.asarray(rec["joint_d2"]), np.asarray(rec["n_kept"]), np.asarray(rec["n_dropped"]), np.asarray(rec["n_untestable"]),
            np.asarray(rec["delta"]).reshape(-1))


class Dev:
    """a call's inputs in device memory, every output pre-filled with a pattern"""

    def __init__(self, pkg, poses, pose_of, obs, frame_start, hyp, pose_cov=None, n_poses=None):
        DA = pkg.binding.DeviceArray; f = lambda a, t: DA(np.ascontiguousarray(a, dtype=t))
        self.n = len(obs); self.np = len(poses) if n_poses is None else n_poses; self.nf = len(frame_start) - 1
        self.p, self.po, self.ob, self.fs, self.hyp = f(poses, np.float64), f(pose_of, np.int32), f(obs, np.float64), f(frame_start, np.int32), f(hyp, np.int32)
        self.pc = None if pose_cov is None else f(pose_cov, np.float64)
        self.idx = f(np.full(self.n, FILL_I), np.int32); self.j = f(np.full(self.nf, FILL_D), np.float64); self.dl = f(np.full(3 * self.nf, FILL_D), np.float64)
        self.nk, self.nd, self.nu = (f(np.full(self.nf, FILL_I), np.int32) for _ in range(3))

    def run(self, G, prm, jc):
        G.joint_compat_resident(self.p, self.np, self.po, self.ob, self.n, self.nf, self.fs, self.hyp, self.idx, self.j, self.nk, self.nd, self.nu, self.dl,
                                self.pc, prm, jc); G.synchronize()
        return (self.idx.to_host(np.int32, self.n), self.j.to_host(np.float64, self.nf), self.nk.to_host(np.int32, self.nf), self.nd.to_host(np.int32, self.nf),
                self.nu.to_host(np.int32, self.nf), self.dl.to_host(np.float64, 3 * self.nf))

    def free(self):
        for a in (self.p, self.po, self.ob, self.fs, self.hyp, self.pc, self.idx, self.j, self.dl, self.nk, self.nd, self.nu):
            if a is not None:
                a.free()


def paths(pkg, G, poses, po, ob, fs, xy, ty, cov, pose_cov, hyp, prm, jc, frame=True):
    """{path: flat result}.  The frame call makes its own hypothesis (the minimum-cost assignment), so it is run only where `hyp` is that one;
    every frame of fs must hold one pose's observations"""
    out = {"batch": flat(*G.joint_compat(poses, po, ob, fs, xy, hyp, cov, pose_cov, prm, jc))}
    set_map(G, xy, ty, cov)
    d = Dev(pkg, poses, po, ob, fs, hyp, pose_cov); out["resident"] = d.run(G, prm, jc); d.free()
    if frame:
        nf = len(fs) - 1; idx = np.full(len(ob), FILL_I, dtype=np.int32); J = np.zeros(nf); cnt = np.zeros((3, nf), dtype=np.int32); dl = np.zeros((nf, 3))
        for f in range(nf):
            a, b = int(fs[f]), int(fs[f + 1]); p = int(po[a]) if b > a else 0
            r = G.frame_frontend_jc(poses[p], ob[a:b], None if pose_cov is None else pose_cov[p], prm, jc)
            idx[a:b] = r[2]; J[f] = r[5]["joint_d2"][0]; dl[f] = r[5]["delta"][0]
            cnt[0, f], cnt[1, f], cnt[2, f] = r[5]["n_kept"][0], r[5]["n_dropped"][0], r[5]["n_untestable"][0]
        out["frame"] = (idx, J, cnt[0], cnt[1], cnt[2], dl.reshape(-1))
    return out


def all_agree(res, tag):
    first = res["batch"]
    for path, r in res.items():
        assert same_bits(first, r), (tag, path, "differs from batch", [int((bits(x) != bits(y)).sum()) for x, y in zip(first, r)])
    return first


def frame_of(r, fs, f):
    a, b = int(fs[f]), int(fs[f + 1])
    return r[0][a:b], float(r[1][f]), int(r[2][f]), int(r[3][f]), int(r[4][f]), r[5][3 * f:3 * f + 3]


def as_arrays(fr):
    """frame_of's tuple in the layout of a one-frame call's flat result"""
    return (fr[0], np.array([fr[1]]), np.array([fr[2]], dtype=np.int32), np.array([fr[3]], dtype=np.int32), np.array([fr[4]], dtype=np.int32), np.asarray(fr[5]))


def hold(F, r, fs, f, tag):
    bad = F.failures(*frame_of(r, fs, f))
    assert not bad, (tag, "frame %d" % f, bad[0], "%d fail" % len(bad))
    WORST["r"] = max(WORST["r"], F.worst); WORST["frames"] += 1; WORST["one_round"] += int(r[3][f]) == 0


# ---- the rule in numpy fp64, operation by operation (heading 0: w = z; sigma_range = sigma_bearing = 0 and no cone covariance: D = sigma_xy^2 I)
def tree_sum(rows, vals):
    lanes = [0.0] * 64
    for r, v in zip(rows, vals):                                             # rows ascend: a lane adds its own in ascending order, from +0
        lanes[r % 64] = lanes[r % 64] + v
    for off in (32, 16, 8, 4, 2, 1):
        lanes = [lanes[l] + lanes[l ^ off] for l in range(64)]
    return lanes[0]


def solve_fp(S, P):
    if P is None:
        return S[0], [0.0, 0.0, 0.0]
    a, c0, c1, c2, m00, m01, m02, m11, m12, m22 = S; p00, p01, p02, p11, p12, p22 = P
    a00 = 1.0 + ((m00 * p00 + m01 * p01) + m02 * p02); a01 = (m00 * p01 + m01 * p11) + m02 * p12; a02 = (m00 * p02 + m01 * p12) + m02 * p22
    a10 = (m01 * p00 + m11 * p01) + m12 * p02; a11 = 1.0 + ((m01 * p01 + m11 * p11) + m12 * p12); a12 = (m01 * p02 + m11 * p12) + m12 * p22
    a20 = (m02 * p00 + m12 * p01) + m22 * p02; a21 = (m02 * p01 + m12 * p11) + m22 * p12; a22 = 1.0 + ((m02 * p02 + m12 * p12) + m22 * p22)
    k00 = a11 * a22 - a12 * a21; k01 = a12 * a20 - a10 * a22; k02 = a10 * a21 - a11 * a20
    k10 = a02 * a21 - a01 * a22; k11 = a00 * a22 - a02 * a20; k12 = a01 * a20 - a00 * a21
    k20 = a01 * a12 - a02 * a11; k21 = a02 * a10 - a00 * a12; k22 = a00 * a11 - a01 * a10
    det = (a00 * k00 + a01 * k01) + a02 * k02
    x0 = ((k00 * c0 + k10 * c1) + k20 * c2) / det; x1 = ((k01 * c0 + k11 * c1) + k21 * c2) / det; x2 = ((k02 * c0 + k12 * c1) + k22 * c2) / det
    d = [(p00 * x0 + p01 * x1) + p02 * x2, (p01 * x0 + p11 * x1) + p12 * x2, (p02 * x0 + p12 * x1) + p22 * x2]
    return a - ((c0 * d[0] + c1 * d[1]) + c2 * d[2]), d


def emulate(z, g, xy, hyp, sigma_xy, P, gate):
    """(index, J, n_kept, n_dropped, delta, order) of one frame from the device's own z and g"""
    z = np.asarray(z, dtype=np.float64); g = np.asarray(g, dtype=np.float64); T = {}
    sx2 = float(sigma_xy) * float(sigma_xy)
    for r, j in enumerate(hyp):
        if j < 0:
            continue
        n0 = float(xy[j, 0]) - float(g[r, 0]); n1 = float(xy[j, 1]) - float(g[r, 1])
        d00 = 0.0 + sx2; d01 = 0.0 + 0.0; d11 = 0.0 + sx2; det = d00 * d11 - d01 * d01
        ux = -float(z[r, 1]); uy = float(z[r, 0])
        y0 = (d11 * n0 - d01 * n1) / det; y1 = (d00 * n1 - d01 * n0) / det
        e00 = d11 / det; e01 = -(d01 / det); e11 = d00 / det; h0 = e00 * ux + e01 * uy; h1 = e01 * ux + e11 * uy
        T[r] = [(((d11 * n0) * n0 - ((2.0 * d01) * n0) * n1) + (d00 * n1) * n1) / det, y0, y1, ux * y0 + uy * y1, e00, e01, h0, e11, h1, ux * h0 + uy * h1]
    kept = sorted(T); order = []
    while True:
        S = [tree_sum(kept, [T[r][q] for r in kept]) for q in range(10)]; J, d = solve_fp(S, P)
        if not kept or J < gate[len(kept)]:
            break
        best = None
        for r in kept:
            jr_, _ = solve_fp([S[q] - T[r][q] for q in range(10)], P)
            if best is None or jr_ < best[0]:
                best = (jr_, r)
        order.append(best[1]); kept = [r for r in kept if r != best[1]]
    return [int(hyp[r]) if r in kept else -1 for r in range(len(hyp))], J, len(kept), len(order), d, order


@pytest.mark.parametrize("name,regime", js.NAMES)
def test_the_purpose_made_scenes(pkg, G, name, regime):
    c = js.scene(name, regime); b = pkg.binding
    jc = b.jc_params(c["confidence"]); gate = list(jc.gate)
    wide = b.nn_params(**dict(c["params"], gate_chi2=1e9, max_distance=100.0))           # the frame call's assignment must find every pair; the joint test reads the sigmas only
    res = paths(pkg, G, c["poses"], c["pose_of"], c["obs"], c["frame_start"], c["map_xy"], c["map_ty"], None, c["pose_cov"], c["hyp"], wide, jc)
    first = all_agree(res, (name, regime))
    pc = None if c["pose_cov"] is None else c["pose_cov"][0]
    z, g, idx, d2, na, rec = G.frame_frontend_jc(c["poses"][0], c["obs"], pc, wide, jc)
    za, ga, ia, da, naa = G.frame_frontend_assign_opt(c["poses"][0], c["obs"], pc, wide)
    assert same_bits((z, g, d2, na), (za, ga, da, naa)) and np.array_equal(ia, c["hyp"]), "the frame call's assignment is not gs_frame_frontend_assign_opt's"
    # the reference: decided, and what the scene was made for
    F = jr.make(c, c["hyp"], c["frame_start"], gate)[0].eliminate()
    assert F.decided
    for path, r in res.items():
        hold(F, r, c["frame_start"], 0, (name, regime, path))
    exp = js.EXPECT[name]
    if exp is not None:
        assert [a for a in range(8) if first[0][a] >= 0] == exp[0] and (exp[1] is None or F.order == exp[1])
    # numpy, bit for bit
    e_idx, e_J, e_k, e_d, e_dl, e_order = emulate(z, g, c["map_xy"], c["hyp"], c["params"]["sigma_xy"], jr.upper(pc), gate)
    assert same_bits(first, (np.array(e_idx, dtype=np.int32), np.array([e_J]), np.array([e_k], dtype=np.int32), np.array([e_d], dtype=np.int32),
                             np.array([0], dtype=np.int32), np.array(e_dl))), (name, regime, "numpy", e_idx, e_J, e_dl, first)
    assert e_order == F.order
    if name == "alternating":                                                # every pair passes the per-pair gate WITH Sigma_p, at the default gate and distance
        own = G.associate_nn(c["poses"], c["pose_of"], c["obs"], c["map_xy"], c["map_ty"], None, c["pose_cov"], b.nn_params(**c["params"]))
        assert np.array_equal(own[0], c["hyp"]) and (own[1] < 5.991464547107979).all() and first[3][0] >= 2
    if name == "common":
        assert first[3][0] == 0 and 0.8 < first[5][0] < 1.0
    if name == "hopeless":
        assert first[2][0] == 0 and first[3][0] == 8 and first[1][0] == 0.0 and (first[0] == -1).all() and not first[5].any()
    if name == "nocov":                                                      # J is the fixed-order sum of the bits gs_associate_nn_batch returns
        own = G.associate_nn(c["poses"], c["pose_of"], c["obs"], c["map_xy"], c["map_ty"], None, None, wide)
        assert np.array_equal(own[0], c["hyp"]) and first[1][0] == tree_sum(range(8), [float(x) for x in own[1]]) and not first[5].any()
    print("%-12s %s kept %d dropped %d J %.12g |J - exact| / B %.3g" % (name, regime, first[2][0], first[3][0], first[1][0], F.worst))
    G.map_clear()


def test_untestable_pairs(pkg, G):
    """the common scene with an azimuth-0 observation (a NaN query) and a cone whose covariance makes D indefinite, both named by the
    hypothesis: each gets -1 and counts in n_untestable, and the rest of the frame is what it is with those two at -1"""
    c = dict(js.scene("common", "s4")); b = pkg.binding; jc = b.jc_params(); prm = b.nn_params(**c["params"])
    ob = c["obs"].copy(); ob[2, 0] = 0.0; cov = np.zeros((8, 4)); cov[4] = (0.0, 5.0, 5.0, 0.0)
    res = paths(pkg, G, c["poses"], c["pose_of"], ob, c["frame_start"], c["map_xy"], c["map_ty"], cov, c["pose_cov"], c["hyp"], prm, jc, frame=False)
    first = all_agree(res, "untestable")
    assert first[4][0] == 2 and first[0][2] == -1 and first[0][4] == -1 and first[2][0] + first[3][0] == 6
    h = c["hyp"].copy(); h[[2, 4]] = -1
    without = flat(*G.joint_compat(c["poses"], c["pose_of"], ob, c["frame_start"], c["map_xy"], h, cov, c["pose_cov"], prm, jc))
    assert without[4][0] == 0 and same_bits(first[:4] + first[5:], without[:4] + without[5:])
    F = jr.make(dict(c, obs=ob, map_cov=cov), c["hyp"], c["frame_start"], list(jc.gate))[0].eliminate()
    assert F.sure and F.n_untestable == 2 and F.decided
    hold(F, first, c["frame_start"], 0, "untestable")
    G.map_clear()


# ---- frame sizes, sharing calls
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
    ob = np.concatenate([base[:s] for s in SIZES]); po = np.zeros(len(ob), dtype=np.int32); prm = pkg.binding.nn_params(); jc = pkg.binding.jc_params()
    hyp = G.assign_opt(poses, po, ob, fs, xy, ty, cov, pcv, prm)[0]
    case = dict(lidar=ns.LIDAR, poses=poses, pose_of=np.zeros(256, dtype=np.int32), obs=base, map_xy=xy, map_cov=cov, pose_cov=pcv, params={})
    R = jr.fx.Ref(base, poses, case["pose_of"], ns.LIDAR)
    order = np.concatenate([np.arange(s) for s in SIZES])
    return dict(poses=poses, base=base, xy=xy, ty=ty, cov=cov, pcv=pcv, fs=fs, ob=ob, po=po, prm=prm, jc=jc, hyp=hyp, case=case, R=R, order=order, cache={})


def test_frame_sizes_share_a_call(pkg, G, sized):
    s = sized
    res = paths(pkg, G, s["poses"], s["po"], s["ob"], s["fs"], s["xy"], s["ty"], s["cov"], s["pcv"], s["hyp"], s["prm"], s["jc"])
    first = all_agree(res, "sizes")
    Fs = jr.make(s["case"], s["hyp"], s["fs"], list(s["jc"].gate), s["order"], s["R"], s["cache"])
    for f, k in enumerate(SIZES):
        a, b = int(s["fs"][f]), int(s["fs"][f + 1])
        hold(Fs[f], first, s["fs"], f, "sizes")
        alone = flat(*G.joint_compat(s["poses"], s["po"][a:b], s["ob"][a:b], [0, k], s["xy"], s["hyp"][a:b], s["cov"], s["pcv"], s["prm"], s["jc"]))
        assert same_bits(alone, as_arrays(frame_of(first, s["fs"], f))), ("frame of %d alone" % k)
        if first[3][f] == 0 and first[4][f] == 0:                            # pass-through
            assert np.array_equal(first[0][a:b], s["hyp"][a:b]), k
    assert first[2][0] == 0 and first[1][0] == 0.0 and (first[2][1:] > 0).all(), first[2]
    print("sizes %s kept %s dropped %s untestable %s" % (SIZES, first[2].tolist(), first[3].tolist(), first[4].tolist()))
    G.map_clear()


def test_corrupted_hypotheses_in_every_frame_size(pkg, G, sized):
    """three observations of every frame of 3 or more are pointed at cones 40 m and more away: exactly those are dropped, in three rounds, in
    the small kernel and in the large one alike; the batch and the resident call agree (the frame call makes its own hypothesis)"""
    s = sized; hyp = s["hyp"].copy(); far = s["xy"].copy(); ty = s["ty"]; wrong = {}
    far = np.concatenate([far, s["poses"][0, :2] + np.array([[90.0, 40.0], [-70.0, 85.0], [60.0, -95.0]])]); ty = np.concatenate([ty, [1, 1, 1]]).astype(np.int32)
    cov = np.concatenate([s["cov"], s["cov"][:3]])
    for f, k in enumerate(SIZES):
        if k >= 3:
            a = int(s["fs"][f]); pos = [0, k // 2, k - 1]; wrong[f] = pos
            for t, r in enumerate(pos):
                hyp[a + r] = len(s["xy"]) + t
    res = paths(pkg, G, s["poses"], s["po"], s["ob"], s["fs"], far, ty, cov, s["pcv"], hyp, s["prm"], s["jc"], frame=False)
    first = all_agree(res, "corrupted")
    case = dict(s["case"], map_xy=far, map_cov=cov)
    Fs = jr.make(case, hyp, s["fs"], list(s["jc"].gate), s["order"], s["R"], s["cache"])
    for f, k in enumerate(SIZES):
        a, b = int(s["fs"][f]), int(s["fs"][f + 1])
        hold(Fs[f], first, s["fs"], f, "corrupted")
        if f in wrong:
            gone = [r for r in range(k) if hyp[a + r] >= 0 and first[0][a + r] == -1 and r in Fs[f].pairs]
            assert set(wrong[f]) <= set(gone) and first[3][f] >= 3, (k, gone)
            if k <= 65:                                                      # the exact elimination, where it is cheap
                F = Fs[f].eliminate()
                if F.decided:
                    assert F.order[:3] and set(F.order[:3]) == set(wrong[f]), (k, F.order)
                    assert not F.failures(*frame_of(first, s["fs"], f))
    print("corrupted: dropped %s" % first[3].tolist())
    G.map_clear()


# ---- the 25 inherited cases, framed by pose, with the hypothesis of gs_assign_opt_batch
@pytest.mark.parametrize("name", ns.NAMES)
def test_inherited_scenes(pkg, G, name):
    c = ns.case(name); order, fs = ar.frames_by_pose(c["pose_of"]); b = pkg.binding
    po = np.ascontiguousarray(c["pose_of"][order]); ob = np.ascontiguousarray(c["obs"][order]); prm = b.nn_params(**c["params"]); jc = b.jc_params()
    hyp, d2, na = G.assign_opt(c["poses"], po, ob, fs, c["map_xy"], c["map_ty"], c["map_cov"], c["pose_cov"], prm)
    res = paths(pkg, G, c["poses"], po, ob, fs, c["map_xy"], c["map_ty"], c["map_cov"], c["pose_cov"], hyp, prm, jc)
    first = all_agree(res, name)
    Fs = jr.make(c, hyp, fs, list(jc.gate), order, ns.reference(name).R)
    for f, F in enumerate(Fs):
        a, e = int(fs[f]), int(fs[f + 1])
        hold(F, first, fs, f, name)
        if first[3][f] == 0 and first[4][f] == 0:                            # pass-through: the hypothesis unchanged, index for index
            assert np.array_equal(first[0][a:e], hyp[a:e]), (name, f)
        # the frame call: its assignment is gs_frame_frontend_assign_opt's, bit for bit
        if e > a:
            p = int(po[a]); pc = None if c["pose_cov"] is None else c["pose_cov"][p]
            rj = G.frame_frontend_jc(c["poses"][p], ob[a:e], pc, prm, jc); ra = G.frame_frontend_assign_opt(c["poses"][p], ob[a:e], pc, prm)
            assert same_bits((rj[0], rj[1], rj[3], rj[4]), (ra[0], ra[1], ra[3], ra[4])), (name, f)
            if rj[5]["n_dropped"][0] == 0 and rj[5]["n_untestable"][0] == 0:
                assert np.array_equal(rj[2], ra[2]), (name, f)
    print("%-16s frames %d kept %d dropped %d untestable %d; so far: %d frames, %d left after one round, worst |J - exact| / B %.3g" % (
        name, len(fs) - 1, first[2].sum(), first[3].sum(), first[4].sum(), WORST["frames"], WORST["one_round"], WORST["r"]))
    G.map_clear()


# ---- the resident call's defences, and the calls around it
def test_resident_defences(pkg, G, sized):
    """a frame of 257 and a frame with two poses get -1, J = +inf, counts and delta 0; frames with bounds outside [0, n] or a > b, and uncovered
    observations, leave the pre-filled pattern everywhere; an index outside the map (or below -1) makes its pair untestable; the good
    frames between them return what they return alone; the optional outputs may be left out"""
    s = sized; n = 420
    ob = np.concatenate([s["base"], s["base"][:n - 256]]); po = np.zeros(n, dtype=np.int32); poses = np.concatenate([s["poses"], s["poses"] + 0.5])
    set_map(G, s["xy"], s["ty"], s["cov"]); m = len(s["xy"])
    hyp = G.assign_opt(poses, po, ob, [0, 256, n], s["xy"], s["ty"], s["cov"], None, s["prm"])[0]
    po[310] = 1                                                              # the frame [300, 340) names two poses
    hyp[262] = m; hyp[263] = -7; hyp[264] = 2 ** 30                          # outside the map: untestable
    head = [0, 257, 300, 340, 700, 350, -5, 345]
    for fs, good in ((head + [400], [(1, (257, 300)), (7, (345, 400))]),                                               # mean frame 52: the large kernel alone
                     (head + list(range(346, 401)), [(1, (257, 300)), (7, (345, 346)), (30, (368, 369)), (61, (399, 400))])):      # 62 frames, eight to a wave, then the large ones
        defences(pkg, G, s, poses, po, ob, hyp, np.array(fs, dtype=np.int32), good, m, n)
    G.map_clear()


def defences(pkg, G, s, poses, po, ob, hyp, fs, good, m, n):
    b = pkg.binding; nf = len(fs) - 1
    d = Dev(pkg, poses, po, ob, fs, hyp, None); idx, J, nk, nd, nu, dl = d.run(G, s["prm"], s["jc"])
    assert (idx[:257] == -1).all() and np.isinf(J[0]) and nk[0] == nd[0] == nu[0] == 0 and not dl[0:3].any()          # above GS_NN_FRAME_MAX
    assert (idx[300:340] == -1).all() and np.isinf(J[2]) and nk[2] == nd[2] == nu[2] == 0 and not dl[6:9].any()       # two poses
    for f in (3, 4, 5, 6):                                                   # 340..700, 700..350, 350..-5, -5..345: not frames of this call
        assert J[f] == FILL_D and nk[f] == nd[f] == nu[f] == FILL_I and (dl[3 * f:3 * f + 3] == FILL_D).all(), f
    written = np.zeros(n, dtype=bool); written[:340] = True; written[345:400] = True
    assert (idx[~written] == FILL_I).all() and (~written).sum() == 25
    for f, (a, e) in good:
        h = hyp[a:e].copy(); bad = (h < -1) | (h >= m); h[bad] = -1
        alone = flat(*G.joint_compat(poses, po[a:e], ob[a:e], [0, e - a], s["xy"], h, s["cov"], None, s["prm"], s["jc"]))
        assert np.array_equal(idx[a:e], alone[0]) and bits(np.array([J[f]]))[0] == bits(alone[1])[0] and nk[f] == alone[2][0] and nd[f] == alone[3][0], (f, a, e)
        assert nu[f] == alone[4][0] + bad.sum() and same_bits((dl[3 * f:3 * f + 3],), (alone[5],)) and (e - a == 1 or nk[f] > 0)
    assert nu[1] >= 3 and (idx[262:265] == -1).all()
    lib = b.lib(); only = b.DeviceArray(np.full(n, FILL_I, dtype=np.int32))  # the optional outputs left out: the index alone is written, and the same
    assert lib.gs_joint_compat_resident(G.h, n, d.p.ptr, 2, d.po.ptr, d.ob.ptr, nf, d.fs.ptr, None, C.byref(s["prm"]), C.byref(s["jc"]), d.hyp.ptr, only.ptr,
                                        None, None, None, None, None) == 0
    G.synchronize(); assert np.array_equal(only.to_host(np.int32, n), idx); only.free()
    shifted = C.c_void_p(d.ob.ptr.value + 8)
    assert lib.gs_joint_compat_resident(G.h, n - 1, d.p.ptr, 2, d.po.ptr, shifted, nf, d.fs.ptr, None, C.byref(s["prm"]), C.byref(s["jc"]), d.hyp.ptr, d.idx.ptr,
                                        None, None, None, None, None) == -1
    d.free()


def test_the_existing_calls_are_unchanged_by_joint_calls(pkg, G):
    c = dict(ns.case("map257")); b = pkg.binding; prm = b.nn_params(); jc = b.jc_params(); order, fs = ar.frames_by_pose(c["pose_of"])
    po = np.ascontiguousarray(c["pose_of"][order]); ob = np.ascontiguousarray(c["obs"][order]); k0 = int(fs[1])
    set_map(G, c["map_xy"], c["map_ty"], c["map_cov"])
    def existing():
        out = tuple(G.assign_opt(c["poses"], po, ob, fs, c["map_xy"], c["map_ty"], c["map_cov"], c["pose_cov"], prm))
        out += tuple(G.associate_nn(c["poses"], po, ob, c["map_xy"], c["map_ty"], c["map_cov"], c["pose_cov"], prm))
        out += tuple(G.assign_nn(c["poses"], po, ob, fs, c["map_xy"], c["map_ty"], c["map_cov"], c["pose_cov"], prm))
        return out + tuple(G.frame_frontend_assign_opt(c["poses"][0], ob[:k0], c["pose_cov"][0], prm)) + tuple(G.frame_frontend_nn(c["poses"][0], ob[:k0], c["pose_cov"][0], prm))
    before = existing(); assert (before[0] >= 0).any()
    G.joint_compat(c["poses"], po, ob, fs, c["map_xy"], before[0], c["map_cov"], c["pose_cov"], prm, jc); assert same_bits(existing(), before)
    G.frame_frontend_jc(c["poses"][0], ob[:k0], c["pose_cov"][0], prm, jc); assert same_bits(existing(), before)
    d = Dev(pkg, c["poses"], po, ob, fs, before[0], c["pose_cov"]); d.run(G, prm, jc); d.free(); assert same_bits(existing(), before)
    G.map_clear()
