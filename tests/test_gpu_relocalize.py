"""GPU tests of relocalisation (k_reloc_seed / k_reloc_pick of gs_reloc.hip): a frame's pose found on the map without a prior.

THREE paths — gs_relocalize_batch, gs_relocalize_resident, gs_frame_frontend_relocalize frame by frame — BOTH scoring searches (the hashed
grid and the walk over the whole map: gs_debug_options.assoc_grid forces either) and any slicing of the cones over workgroups
(gs_debug_relocalize) must agree bit for bit.  Every frame is held to relocalize_ref.run, the header restated in numpy float64, fed the
device's OWN z (the bits the front-end frame calls return as out_zxy; see test_where_the_device_s_z_comes_from): tx, ty, count, cost, seed,
second_count, the runner-up's tx and ty, n_seeds, status, index and e2 bit for bit; theta against numpy.arctan2 of the reference's (s, c) within relocalize_ref.THETA_ULPS (the libm allowance of
DESIGN 22, stated there).  Where a scene was synthesised from a known pose the independent checker holds the returned pose within
inlier_radius of it and index to the truth's matches.  The scenes (relocalize_shapes.py) are the smallest at which each part can go wrong.

Measured on an MI355X (the tests print these figures with -s): all 31 purpose-made scenes and the 100 frames of 'hundred' bit for bit on every
path, 117 frames held to a known pose; the largest |theta - numpy.arctan2| seen is 1.95 u |theta| against the allowance of 10; the file runs in
a few seconds.  With z read from gs_polar_to_xy_batch instead of the frame calls, 8 of the 100 frames of 'hundred' differ from the reference in
the last bits of e2 / cost (15 of its 907 observations have another last bit of z there): test_where_the_device_s_z_comes_from."""
import numpy as np
import pytest

import relocalize_ref as rr
import relocalize_shapes as rs

pytestmark = pytest.mark.gpu
FILL_I, FILL_D = 12345, 777.0
STATS = {"frames": 0, "truth": 0, "theta": 0.0}


@pytest.fixture(scope="module")
def G(pkg):
    if pkg.device_count() < 1:
        pytest.fail("no gfx950 device visible: the HIP path cannot run")
    g = pkg.Graph(lidar_to_cog=rs.LIDAR)
    yield g
    g.close()
    print("\nrelocalisation: %d frames held bit for bit to the reference, %d of them to a known pose; largest |theta - numpy.arctan2| %.3g u |theta|" % (
        STATS["frames"], STATS["truth"], STATS["theta"]))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


KEYS = ("pose", "count", "cost", "seed", "second_count", "second_pose", "n_seeds", "status")


def flat(rec, idx, e2):
    return tuple(np.asarray(rec[k]).reshape(-1) for k in KEYS) + (np.asarray(idx), np.asarray(e2))


def zfun_of(G):
    """obs -> the device's own z: the bits the front-end frame calls return as out_zxy (gs_frame_frontend_assign: the out-of-line A0 function every
    kernel of this family calls), 256 observations a call.  NOT gs_polar_to_xy_batch: see test_where_the_device_s_z_comes_from"""
    def zfun(obs):
        obs = np.ascontiguousarray(obs, dtype=np.float64).reshape(-1, 4)
        parts = [G.frame_frontend_assign([0.0, 0.0, 0.0], obs[a:a + 256])[0] for a in range(0, len(obs), 256)]
        return np.concatenate(parts) if parts else np.zeros((0, 2))
    return zfun


def test_where_the_device_s_z_comes_from(pkg, G):
    """The reference is fed the device's own z.  gs_polar_to_xy_batch (the A0 kernel, the conversion inlined) and the front-end frame calls (the
    out-of-line A0 function the association, assignment, joint-test, localisation and relocalisation kernels share) are one formula but, as
    compiled, NOT one rounding: measured on an MI355X they differ in the last bit of z for 15 of the 907 observations of the scene 'hundred'
    (the existing calls gs_polar_to_xy_batch and gs_frame_frontend_assign against each other; nothing of relocalisation is involved), and with
    gs_polar_to_xy_batch's z the reference then differs from the device in the last bits of e2 / cost on 8 of its 100 frames, on none of the
    other 31 scenes.  So z is read from the frame call; where the two agree the choice changes nothing.  This test holds what the choice rests
    on: the frame call's z is within 2 ulp of gs_polar_to_xy_batch's everywhere, and equal to it for most observations."""
    c = rs.scene("hundred"); ob = c["obs"]
    zb = G.polar_to_xy(ob[:, 0], ob[:, 1], ob[:, 2]); zf = zfun_of(G)(ob)
    differ = int((bits(zb) != bits(zf)).any(axis=1).sum())
    print("z: %d of %d observations differ between gs_polar_to_xy_batch and the frame call" % (differ, len(ob)))
    assert np.all(np.abs(zb - zf) <= 2 * np.spacing(np.abs(zb))) and differ <= len(ob) // 10


def set_map(G, xy, ty):
    G.map_clear()
    if len(ty):
        G.map_append(xy, ty)
    assert G.map_size() == len(ty)


class Dev:
    """a call's inputs in device memory, every output pre-filled with a pattern"""

    def __init__(self, pkg, obs, frame_start, n=None):
        DA = pkg.binding.DeviceArray; f = lambda a, t: DA(np.ascontiguousarray(a, dtype=t))
        self.n = len(obs) if n is None else n; self.nf = len(frame_start) - 1; nf = max(self.nf, 1); m = max(len(obs), 1)
        self.ob = f(obs if len(obs) else np.zeros((1, 4)), np.float64); self.fs = f(frame_start, np.int32)
        self.pose, self.sp = f(np.full(3 * nf, FILL_D), np.float64), f(np.full(3 * nf, FILL_D), np.float64)
        self.cost = f(np.full(nf, FILL_D), np.float64); self.ns = f(np.full(nf, FILL_I), np.int64); self.seed = f(np.full(4 * nf, FILL_I), np.int32)
        self.count, self.sc, self.st = (f(np.full(nf, FILL_I), np.int32) for _ in range(3))
        self.idx = f(np.full(m, FILL_I), np.int32); self.e2 = f(np.full(m, FILL_D), np.float64); self.m = m

    def run(self, G, prm, second=True):
        G.relocalize_resident(self.ob, self.n, self.nf, self.fs, self.pose, self.count, self.cost, self.seed, self.sc if second else None,
                              self.sp if second else None, self.ns, self.st, self.idx, self.e2, prm); G.synchronize()
        nf = self.nf
        return (self.pose.to_host(np.float64, 3 * nf), self.count.to_host(np.int32, nf), self.cost.to_host(np.float64, nf), self.seed.to_host(np.int32, 4 * nf),
                self.sc.to_host(np.int32, nf), self.sp.to_host(np.float64, 3 * nf), self.ns.to_host(np.int64, nf), self.st.to_host(np.int32, nf),
                self.idx.to_host(np.int32, self.m), self.e2.to_host(np.float64, self.m))

    def free(self):
        for a in (self.ob, self.fs, self.pose, self.sp, self.cost, self.ns, self.seed, self.count, self.sc, self.st, self.idx, self.e2):
            a.free()


def paths(pkg, G, c, prm):
    """{path: flat result}: the batch and the resident call with each scoring search, in the scene's slicing and in two others; leaves the map resident"""
    out = {}
    set_map(G, c["map_xy"], c["map_ty"])
    d = Dev(pkg, c["obs"], c["frame_start"])
    n = len(c["obs"])
    for grid in (1, 0):
        G.set_debug(assoc_grid=grid)
        for sl in sorted({c["slice"], 0, 7, max(1, len(c["map_ty"]))}):
            if len(c["map_ty"]) > 600 and sl == 7:                               # (a slice of 7 on the large maps: thousands of workgroups that say nothing new)
                continue
            G.debug_relocalize(sl)
            out["batch grid %d slice %d" % (grid, sl)] = flat(*G.relocalize(c["obs"], c["frame_start"], c["map_xy"], c["map_ty"], prm))
            r = d.run(G, prm)
            out["resident grid %d slice %d" % (grid, sl)] = r[:8] + (r[8][:n], r[9][:n])
    G.set_debug(assoc_grid=-1); G.debug_relocalize(0)
    out["batch auto"] = flat(*G.relocalize(c["obs"], c["frame_start"], c["map_xy"], c["map_ty"], prm))
    d.free()
    return out


def all_agree(res, tag):
    first = res["batch auto"]
    for path, r in res.items():
        assert same_bits(first, r), (tag, path, "differs from batch auto", [int((bits(x) != bits(y)).sum()) for x, y in zip(first, r)])
    return first


def unflat(r):
    rec = {k: r[t] for t, k in enumerate(KEYS)}
    rec["pose"] = rec["pose"].reshape(-1, 3); rec["second_pose"] = rec["second_pose"].reshape(-1, 3); rec["seed"] = rec["seed"].reshape(-1, 4)
    return rec, r[8], r[9]


def hold(c, z, r, tag, prm_kw):
    """every frame of the flat result r against the reference and, where the scene has one, against the truth"""
    rec, idx, e2 = unflat(r)
    frames = rr.run(z, c["obs"][:, 3], c["frame_start"], c["map_xy"], c["map_ty"], **prm_kw)
    R = rr.params_of(**prm_kw)["inlier_radius"]
    for f, o in enumerate(frames):
        a, b = int(c["frame_start"][f]), int(c["frame_start"][f + 1])
        bad = rr.failures(o, rec, f, idx[a:b], e2[a:b])
        assert not bad, (tag, "frame %d" % f, bad)
        STATS["frames"] += 1
        for got, want in ((rec["pose"][f][2], o["pose"][2]), (rec["second_pose"][f][2], o["second_pose"][2])):
            if want != 0.0:
                STATS["theta"] = max(STATS["theta"], abs(got - want) / (rr.U * abs(want)))
        if c["status"][f] is not None:
            assert rec["status"][f] == c["status"][f], (tag, f, rec["status"][f])
        if c["truth"][f] is not None:
            pose, tidx = c["truth"][f]
            bad = rr.check_truth(rec["pose"][f], idx[a:b], pose, tidx, z[a:b], R)
            assert not bad, (tag, "frame %d" % f, bad)
            STATS["truth"] += 1
    return frames, rec, idx, e2


def run_scene(pkg, G, name):
    zfun = zfun_of(G); c = rs.scene(name, zfun); z = zfun(c["obs"])
    prm = pkg.binding.reloc_params(**c["params"])
    first = all_agree(paths(pkg, G, c, prm), name)
    return (c, z) + hold(c, z, first, name, c["params"])


SCENES = [n for n in rs.NAMES if n != "hundred"]


@pytest.mark.parametrize("name", SCENES)
def test_every_path_agrees_and_matches_the_reference(pkg, G, name):
    c, z, frames, rec, idx, e2 = run_scene(pkg, G, name)
    o = frames[0]
    print("%-14s status %d count %3d second %3d seeds %6d cost %.3g" % (name, rec["status"][0], rec["count"][0], rec["second_count"][0], rec["n_seeds"][0], rec["cost"][0]))
    if name == "small_frames":
        assert list(rec["status"]) == [2, 2, 2] and list(rec["count"]) == [0, 0, 0] and np.all(np.isinf(rec["cost"])) and np.all(rec["pose"] == 0.0)
        assert np.all(rec["seed"] == -1) and np.all(idx == -1) and np.all(np.isinf(e2)) and list(rec["n_seeds"]) == [0, 0, 0]
    if name == "two_on_two":
        assert (rec["n_seeds"][0], rec["count"][0], rec["second_count"][0], rec["status"][0]) == (2, 2, 2, 1)
    if name == "equal_r2":
        r2 = z[:, 0] * z[:, 0] + z[:, 1] * z[:, 1]
        assert r2[1] == r2[2] and list(rec["seed"][0][:2]) == [0, 1] and rec["count"][0] == 4                  # equal r2 bit for bit: the lower index is the seed
    if name in ("square", "twins"):
        assert rec["second_count"][0] == rec["count"][0] == (4 if name == "square" else 8)
    if name == "twins":
        assert all(int(t) % 2 == 0 for t in rec["seed"][0]) and list(idx) == [0, 0, 2, 2, 4, 4, 6, 6]        # exact ties: the key's (u, v, p, q) decides
    if name == "heading_pi":
        assert rec["pose"][0][2] == np.pi                                        # s = +0, c = -1 exactly
    if name.startswith("line") and name != "line300s":
        assert rec["n_seeds"][0] == max(0, 2 * (int(name[4:]) - 3))
    if name in ("nan_cone", "nan_query"):
        assert rec["count"][0] == 7 and (idx == -1).sum() == 1


def test_a_hundred_frames_in_one_call_equal_each_alone(pkg, G):
    """neighbour independence: frame f of the call of 100 is bitwise the call of that frame alone (u, v move with the frame's position)"""
    c, z, frames, rec, idx, e2 = run_scene(pkg, G, "hundred")
    amb = int((rec["second_count"] == rec["count"]).sum())
    print("hundred: %d of 100 frames have a runner-up of the winner's count; n_seeds %d .. %d" % (amb, rec["n_seeds"].min(), rec["n_seeds"].max()))
    for f in range(0, 100, 7):
        a, b = int(c["frame_start"][f]), int(c["frame_start"][f + 1])
        r1, i1, e1 = G.relocalize(c["obs"][a:b], [0, b - a], c["map_xy"], c["map_ty"])
        sd = rec["seed"][f].copy(); sd[:2] -= a
        want = (rec["pose"][f], rec["count"][f:f + 1], rec["cost"][f:f + 1], sd, rec["second_count"][f:f + 1], rec["second_pose"][f], rec["n_seeds"][f:f + 1],
                rec["status"][f:f + 1], idx[a:b], e2[a:b])
        assert same_bits(flat(r1, i1, e1), want), f


def test_no_second_pointer_skips_the_second_pass_and_changes_nothing_else(pkg, G):
    zfun = zfun_of(G); c = rs.scene("track8", zfun)
    full = flat(*G.relocalize(c["obs"], c["frame_start"], c["map_xy"], c["map_ty"]))
    r, i, e = G.relocalize(c["obs"], c["frame_start"], c["map_xy"], c["map_ty"], second=False)
    assert r["second_count"][0] == 0 and np.all(r["second_pose"] == 0.0)         # (the binding's zeros: nothing was written)
    part = flat(r, i, e)
    assert same_bits(full[:4] + full[6:], part[:4] + part[6:])
    set_map(G, c["map_xy"], c["map_ty"]); d = Dev(pkg, c["obs"], c["frame_start"]); got = d.run(G, None, second=False); d.free()
    assert same_bits(full[:4] + full[6:], got[:4] + got[6:]) and np.all(got[4] == FILL_I) and np.all(got[5] == FILL_D)


def test_the_resident_defences_against_a_pre_filled_pattern(pkg, G):
    """bad frame bounds read and write nothing; a frame of 257 gets status 4 and -1 / +inf; observations that no frame covers are not written"""
    zfun = zfun_of(G); c = rs.scene("track8", zfun); k = len(c["obs"])
    big = np.tile(c["obs"], (40, 1))[:300]                                        # 300 observations: [0, 8) a good frame, [10, 267) one of 257, the rest uncovered
    fs = np.array([0, k, 10, 267], dtype=np.int32)                               # as frames: [0, 8), [8, 10) (2 observations), [10, 267)
    set_map(G, c["map_xy"], c["map_ty"])
    d = Dev(pkg, big, fs); r = d.run(G, None); d.free()
    rec, idx, e2 = unflat(r)
    alone = flat(*G.relocalize(c["obs"], c["frame_start"], c["map_xy"], c["map_ty"]))
    assert same_bits([x[:len(y)] for x, y in zip(r[:8], alone[:8])], alone[:8]) and same_bits((idx[:k], e2[:k]), alone[8:])
    assert rec["status"][2] == 4 and rec["count"][2] == 0 and np.isinf(rec["cost"][2]) and np.all(rec["pose"][2] == 0.0) and np.all(rec["seed"][2] == -1)
    assert rec["second_count"][2] == 0 and np.all(rec["second_pose"][2] == 0.0) and rec["n_seeds"][2] == 0
    assert np.all(idx[10:267] == -1) and np.all(np.isinf(e2[10:267]))
    assert np.all(idx[267:] == FILL_I) and np.all(e2[267:] == FILL_D)            # uncovered: not written
    # frames whose bounds are not 0 <= a <= b <= n: nothing of them is written, the good frame beside them is
    for bad in ([0, k, -1, 5], [0, k, 9, 8], [0, k, k, 301]):
        d = Dev(pkg, big, np.array(bad, dtype=np.int32)); r = d.run(G, None); d.free()
        rec, idx, e2 = unflat(r)
        assert rec["status"][0] == alone[7][0] and same_bits((idx[:k],), (alone[8],)), bad
        covered = np.zeros(300, dtype=bool); refused = 0
        for f in range(3):
            a, b = bad[f], bad[f + 1]
            if 0 <= a <= b <= 300:
                covered[a:b] = True
                continue
            refused += 1
            assert rec["status"][f] == FILL_I and rec["count"][f] == FILL_I and rec["cost"][f] == FILL_D and np.all(rec["pose"][f] == FILL_D), (bad, f)
            assert rec["second_count"][f] == FILL_I and rec["n_seeds"][f] == FILL_I and np.all(rec["seed"][f] == FILL_I), (bad, f)
        assert refused >= 1 and np.all(idx[~covered] == FILL_I) and np.all(e2[~covered] == FILL_D) and np.all(idx[covered] != FILL_I), bad
    # batch: the same frame of 257 is refused on the host
    with pytest.raises(pkg.binding.GsError) as e:
        G.relocalize(big, [0, k, 10, 267, 300], c["map_xy"], c["map_ty"])
    assert e.value.code == -1


def test_the_frame_call(pkg, G):
    """its search outputs equal the resident call's; its chain outputs are bitwise gs_frame_frontend_localize's from the returned pose and the same prior"""
    b = pkg.binding; zfun = zfun_of(G); sx, st = 0.5, 0.1
    prior = np.diag([sx * sx, sx * sx, st * st]).reshape(9)
    for name in ("track8", "twelve", "map2049", "frame65", "heading_pi", "nan_query", "two_on_two", "line3"):
        c = rs.scene(name, zfun); prm = b.reloc_params(**c["params"]); set_map(G, c["map_xy"], c["map_ty"])
        for grid in (-1, 0, 1):
            G.set_debug(assoc_grid=grid)
            r = G.frame_frontend_relocalize(c["obs"], sx, st, prm)
            d = Dev(pkg, c["obs"], c["frame_start"]); res = d.run(G, prm); d.free()
            assert same_bits(flat(*r[:3]), res), (name, grid, "the frame call's search differs from the resident call")
            if r[0]["status"][0] < 2:
                chain = G.frame_frontend_localize(r[0]["pose"][0], c["obs"], prior)
                got = r[3:]
                assert same_bits(got[:5], chain[:5]), (name, grid)
                assert same_bits([got[5][k] for k in sorted(got[5])], [chain[5][k] for k in sorted(chain[5])]), (name, grid)
                assert same_bits([got[6][k] for k in sorted(got[6])], [chain[6][k] for k in sorted(chain[6])]), (name, grid)
                if name in ("track8", "twelve"):
                    pose, tidx = c["truth"][0]                                  # the chain lands on the truth and keeps the true matches
                    assert got[6]["status"][0] == 0 and np.hypot(*(got[6]["pose"][0][:2] - pose[:2])) < 0.05, (name, got[6])
                    assert np.array_equal(got[2][tidx >= 0], tidx[tidx >= 0]), (name, got[2], tidx)
            else:                                                                # no seed: the chain found an empty frame
                z, gx, idx, d2, na, jr, lr = r[3:]
                assert np.all(z == 0.0) and np.all(gx == 0.0) and np.all(idx == -1) and np.all(np.isinf(d2)) and np.all(na == 0)
                assert jr["n_kept"][0] == 0 and jr["joint_d2"][0] == 0.0 and lr["status"][0] == 2 and lr["n_pairs"][0] == 0
        G.set_debug(assoc_grid=-1)
    # k == 0: nothing is launched
    r = G.frame_frontend_relocalize(np.zeros((0, 4)), sx, st)
    assert r[0]["status"][0] == 2 and r[0]["count"][0] == 0 and np.isinf(r[0]["cost"][0]) and r[0]["n_seeds"][0] == 0 and r[9]["status"][0] == 2
    assert np.array_equal(r[9]["cov"][0], prior) and np.all(r[9]["pose"][0] == 0.0)
    with pytest.raises(b.GsError) as e:
        G.frame_frontend_relocalize(np.tile(rs.OBS2[:1], (257, 1)), sx, st)
    assert e.value.code == -1


def test_the_existing_calls_are_unchanged_by_it(pkg, G):
    """one existing front-end call and one gs_iterate before and after relocalising: identical bits"""
    zfun = zfun_of(G); c = rs.scene("track8", zfun); truth = c["truth"][0][0]
    set_map(G, c["map_xy"], c["map_ty"])
    existing = lambda: G.frame_frontend_assign(truth, c["obs"], np.diag([0.04, 0.04, 0.01]).reshape(9))
    before = existing()
    G.relocalize(c["obs"], c["frame_start"], c["map_xy"], c["map_ty"]); assert same_bits(existing(), before)
    d = Dev(pkg, c["obs"], c["frame_start"]); d.run(G, None); d.free(); assert same_bits(existing(), before)
    G.frame_frontend_relocalize(c["obs"], 0.5, 0.1); assert same_bits(existing(), before)
    G.map_clear()
    t = pkg.track.generate(50, 30); fe = pkg.Graph(device=0); g = pkg.track.bench_graph(t, fe); fe.close(); out = []
    for reloc in (False, True):
        H = pkg.Graph(device=0); H.load_bench_graph(g)
        if reloc:
            H.relocalize(c["obs"], c["frame_start"], c["map_xy"], c["map_ty"])
            H.map_append(c["map_xy"], c["map_ty"]); H.frame_frontend_relocalize(c["obs"], 0.5, 0.1)
        H.initialize_optimization(); H.iterate(); out.append((H.poses(), H.landmarks())); H.close()
    assert same_bits(out[0], out[1])
