"""CPU tests of relocalisation: the header declares and the library exports it, gs_reloc_params_default, every host-side refusal on a host-only
handle, the numpy reference (relocalize_ref.py) alone on every purpose-made scene (relocalize_shapes.py) held by the independent checker, the
symmetric scenes' tie order, and the teeth of the two checkers.  Nothing here runs a kernel."""
import ctypes as C

import numpy as np
import pytest

import relocalize_ref as rr
import relocalize_shapes as rs

NEW_FUNCS = ("gs_reloc_params_default", "gs_relocalize_batch", "gs_relocalize_resident", "gs_frame_frontend_relocalize", "gs_debug_relocalize",
             "gs_debug_time_relocalize_resident")


def test_the_header_declares_and_the_library_exports(pkg):
    names = pkg.binding.declared_symbols(); L = pkg.binding.lib()
    for f in NEW_FUNCS:
        assert f in names, f
        assert hasattr(L, f), f
    for f in ("relocalize", "relocalize_resident", "frame_frontend_relocalize", "time_relocalize_resident", "debug_relocalize"):
        assert hasattr(pkg.Graph, f), f


def test_the_default_params(pkg):
    b = pkg.binding; p = b.reloc_params()
    assert C.sizeof(b.RelocParams) == 64 and p.struct_size == 64 and b.RELOC_SEED_MAX == 16
    assert (p.seed_obs, p.min_inliers, p.reserved) == (12, 4, 0)
    assert (p.min_baseline, p.length_tol, p.inlier_radius, p.type_tol, p.distinct_xy, p.distinct_cos) == (2.0, 0.3, 0.5, 1e-4, 2.0, 0.98006657784124163)
    assert abs(p.distinct_cos - np.cos(0.2)) < 1e-16
    assert {k: getattr(p, k) for k in rr.DEFAULTS} == rr.DEFAULTS                # the reference's defaults are the library's
    assert b.lib().gs_reloc_params_default(None) == -1
    assert b.reloc_params(seed_obs=3, length_tol=0.1).seed_obs == 3
    with pytest.raises(AttributeError):
        b.reloc_params(nothing=1)


def test_refusals_on_a_host_only_handle(pkg):
    b = pkg.binding; L = b.lib(); G = pkg.Graph(device=-2)
    ob = np.array([[10.0, 0, 5, 1], [20.0, 0, 6, 2]]); xy = np.ones((3, 2)); ty = np.ones(3, dtype=np.int32); fs = np.array([0, 1, 2], dtype=np.int32)
    def code(fn, *a, **kw):
        with pytest.raises(b.GsError) as e:
            fn(*a, **kw)
        return e.value.code
    da = C.c_void_p(4096)                                                        # never dereferenced: every refusal below is decided on the host
    prm = b.reloc_params()
    res = lambda **kw: L.gs_relocalize_resident(*[kw.get(k, v) for k, v in (("g", G.h), ("n", 2), ("ob", da), ("nf", 2), ("fs", da), ("prm", C.byref(prm)),
                                                                              ("pose", None), ("count", None), ("cost", None), ("seed", None), ("sc", None), ("sp", None),
                                                                              ("ns", None), ("st", None), ("idx", None), ("e2", None))])
    frame = lambda *a, **kw: G.frame_frontend_relocalize(ob, 1.0, 0.2, *a, **kw)
    # good arguments: GS_ERR_NO_DEVICE; every output is optional
    assert code(G.relocalize, ob, fs, xy, ty) == -4 and code(frame) == -4 and code(G.relocalize, ob, fs, xy, ty, second=False) == -4
    assert code(G.relocalize, ob, [0, 0, 2, 2], xy, ty) == -4                    # empty frames are allowed
    assert res() == -4 and res(pose=da, count=da, cost=da, seed=da, sc=da, sp=da, ns=da, st=da, idx=da, e2=da) == -4
    # gs_reloc_params: the size, seed_obs outside 2 .. 16, min_inliers < 2, a non-finite or non-positive length, distinct_cos outside [-1, 1]
    bad = [dict(struct_size=0), dict(struct_size=72), dict(seed_obs=1), dict(seed_obs=17), dict(seed_obs=-3), dict(min_inliers=1), dict(min_inliers=0),
           dict(distinct_cos=1.0000001), dict(distinct_cos=-1.5), dict(distinct_cos=float("nan")), dict(type_tol=float("nan")), dict(type_tol=float("inf"))]
    bad += [{k: v} for k in ("min_baseline", "length_tol", "inlier_radius", "distinct_xy") for v in (0.0, -1e-30, float("nan"), float("inf"), -float("inf"))]
    for kw in bad:
        p = b.reloc_params(**kw)
        assert code(G.relocalize, ob, fs, xy, ty, p) == -1, kw
        assert code(frame, p) == -1, kw
        assert res(prm=C.byref(p)) == -1, kw
    for kw in (dict(seed_obs=2), dict(seed_obs=16), dict(min_inliers=2), dict(distinct_cos=1.0), dict(distinct_cos=-1.0), dict(min_baseline=1e-300)):
        p = b.reloc_params(**kw)
        assert code(G.relocalize, ob, fs, xy, ty, p) == -4 and res(prm=C.byref(p)) == -4 and code(frame, p) == -4, kw
    # the frame call also checks the prior sigmas and the chain's three structs
    for sx, st in ((-1.0, 0.1), (1.0, -0.1), (float("nan"), 0.1), (1.0, float("inf"))):
        assert code(G.frame_frontend_relocalize, ob, sx, st) == -1, (sx, st)
    assert code(G.frame_frontend_relocalize, ob, 0.0, 0.0) == -4
    assert code(frame, params=b.nn_params(gate_chi2=-1.0)) == -1 and code(frame, loc=b.loc_params(max_iterations=0)) == -1
    t = b.jc_params(); t.gate[3] = -0.5
    assert code(frame, jc=t) == -1
    # pointers, counts, alignment (resident)
    assert res(ob=C.c_void_p(4096 + 8)) == -1
    for k in ("g", "ob", "fs", "prm"):
        assert res(**{k: None}) == -1, k
    assert res(n=-1) == -1 and res(nf=-1) == -1
    # the frames (batch), as gs_assign_nn_batch checks them
    for f in ([1, 1, 2], [0, 2, 1, 2], [0, 1, 1], [0, 1, 3], [0, 2, 1]):
        assert code(G.relocalize, ob, f, xy, ty) == -1, f
    big = np.tile(ob[:1], (300, 1))
    assert code(G.relocalize, big, [0, 257, 300], xy, ty) == -1 and code(G.relocalize, big, [0, 44, 300], xy, ty) == -4
    assert code(G.frame_frontend_relocalize, big[:257], 1.0, 0.2) == -1 and code(G.frame_frontend_relocalize, big[:256], 1.0, 0.2) == -4
    dp = C.POINTER(C.c_double); ip = C.POINTER(C.c_int32)
    args = lambda **kw: [kw.get(k, v) for k, v in (("g", G.h), ("n", 2), ("ob", ob.ctypes.data_as(dp)), ("nf", 2), ("fs", fs.ctypes.data_as(ip)), ("m", 3),
                                                   ("xy", xy.ctypes.data_as(dp)), ("ty", ty.ctypes.data_as(ip)), ("prm", C.byref(prm)))] + [None] * 10
    assert L.gs_relocalize_batch(*args()) == -4
    for k in ("g", "ob", "fs", "xy", "ty", "prm"):
        assert L.gs_relocalize_batch(*args(**{k: None})) == -1, k
    assert L.gs_relocalize_batch(*args(n=-1)) == -1 and L.gs_relocalize_batch(*args(m=-1)) == -1 and L.gs_relocalize_batch(*args(nf=-1)) == -1
    assert L.gs_debug_relocalize(G.h, -1) == -1 and L.gs_debug_relocalize(None, 0) == -1 and L.gs_debug_relocalize(G.h, 16) == 0 and L.gs_debug_relocalize(G.h, 0) == 0
    ms = C.c_double()
    tm = lambda reps: L.gs_debug_time_relocalize_resident(G.h, 2, da, 2, da, C.byref(prm), *([None] * 10), reps, C.byref(ms))
    assert tm(0) == -1 and tm(3) == -4
    G.close()


@pytest.fixture(scope="module")
def census():
    """scene -> (the scene, its z, the reference's frames)"""
    out = {}
    for name in rs.NAMES:
        c = rs.scene(name); z = rs.default_z(c["obs"])
        out[name] = (c, z, rr.run(z, c["obs"][:, 3], c["frame_start"], c["map_xy"], c["map_ty"], **c["params"]))
    return out


def test_the_reference_alone_recovers_the_truth_on_every_scene(census):
    held = 0
    for name, (c, z, frames) in census.items():
        R = rr.params_of(**c["params"])["inlier_radius"]
        for f, o in enumerate(frames):
            a, b = c["frame_start"][f], c["frame_start"][f + 1]
            if c["status"][f] is not None:
                assert o["status"] == c["status"][f], (name, f, o["status"])
            if c["truth"][f] is not None:
                pose, idx = c["truth"][f]
                assert not rr.check_truth(o["pose"], o["index"], pose, idx, z[a:b], R), (name, f, rr.check_truth(o["pose"], o["index"], pose, idx, z[a:b], R))
                assert o["count"] == int((idx >= 0).sum()), (name, f)
                held += 1
            assert o["count"] == int((o["index"] >= 0).sum()) and (o["status"] == 2) == (o["n_seeds"] == 0), (name, f)
            cost = 0.0
            for e in o["e2"][o["index"] >= 0]:
                cost = cost + e
            assert o["cost"] == (cost if o["status"] != 2 else rr.INF), (name, f)
        o = frames[0]
        print("%-14s frames %3d status %d count %3d second %3d seeds %5d cost %.3g" % (name, len(frames), o["status"], o["count"], o["second_count"], o["n_seeds"], o["cost"]))
    assert held >= 110
    # what the scenes were made for
    hundred = census["hundred"][2]
    assert all(o["status"] == 0 for o in hundred)
    amb = sum(o["second_count"] == o["count"] for o in hundred)
    print("hundred: %d of 100 frames have a runner-up of the winner's count; runner-up counts %d .. %d against winners %d .. %d" % (
        amb, min(o["second_count"] for o in hundred), max(o["second_count"] for o in hundred), min(o["count"] for o in hundred), max(o["count"] for o in hundred)))
    assert all(o["second_count"] >= 2 for o in hundred)                          # the track repeats itself: the ambiguity output is not decoration
    assert [o["status"] for o in census["small_frames"][2]] == [2, 2, 2]
    o = census["two_on_two"][2][0]
    assert (o["n_seeds"], o["count"], o["second_count"], o["status"]) == (2, 2, 2, 1)
    assert census["twelve"][0]["frame_start"][1] == 12 and census["thirteen"][0]["frame_start"][1] == 13
    c, z, fr = census["equal_r2"]; r2 = z[:, 0] * z[:, 0] + z[:, 1] * z[:, 1]
    assert r2[1] == r2[2] and r2[0] < r2[1] < r2[3] and list(fr[0]["seed"][:2]) == [0, 1] and fr[0]["count"] == 4
    for n in rs.LINES:
        assert census["line%d" % n][2][0]["n_seeds"] == max(0, 2 * (n - 3)), n
    fills = sorted(set(sum((rs.ring_fill(n) for n in rs.LINES), [])))
    assert {0, 1, 63, 64, 65, 66, 128}.issubset(fills) and max(fills) > 128, fills    # a wave's ring: empty, one, around the drain at 64, full, wrapped
    assert len(rs.ring_fill(300, 3, 16)) // 4 == 19                              # line300s: 19 records a frame
    assert census["heading_pi"][2][0]["pose"][2] == np.pi and census["heading_pi"][2][0]["s"] == 0.0 and census["heading_pi"][2][0]["c"] == -1.0
    assert census["heading_minus"][2][0]["pose"][2] < -3.0
    assert census["nan_cone"][2][0]["count"] == 7 and census["nan_query"][2][0]["count"] == 7


def test_the_symmetric_scenes_tie_order(census):
    """an exact square fed to the reference as z itself: the eight poses that map the square onto itself tie in (count, cost) = (4, 0) exactly where
    the arithmetic is exact, and the key's (u, v, p, q) decides; the twins scene ties through equal cones and equal observations"""
    z = rs.SQUARE.copy(); ty = np.ones(4)
    fr = rr.run(z, ty, [0, 4], z, np.ones(4, dtype=np.int32))[0]                # the cones ARE the observations: the identity is a seed, cost 0
    assert (fr["count"], fr["cost"], fr["second_count"], fr["n_seeds"]) == (4, 0.0, 4, 40)
    assert list(fr["seed"]) == [0, 1, 0, 1] and list(fr["pose"]) == [0.0, 0.0, 0.0] and list(fr["index"]) == [0, 1, 2, 3]
    # with the first two cones exchanged in the map the four rotations of the square are the seeds (0, 1, 1, 0), (0, 1, 0, 2), (0, 1, 2, 3) and
    # (0, 1, 3, 1), all of count 4 and cost 0 (quarter turns of these numbers are exact): the smallest key wins, which is no longer the identity
    sw = z[[1, 0, 2, 3]]
    fr = rr.run(z, ty, [0, 4], sw, np.ones(4, dtype=np.int32))[0]
    assert (fr["count"], fr["cost"], fr["second_count"]) == (4, 0.0, 4) and list(fr["seed"]) == [0, 1, 0, 2] and list(fr["index"]) == [0, 2, 3, 1]
    assert (fr["c"], fr["s"]) == (0.0, -1.0)
    c, zz, frames = census["twins"]; o = frames[0]
    assert o["count"] == 8 and o["second_count"] == 8 and o["n_seeds"] == 640
    assert all(int(t) % 2 == 0 for t in o["seed"])                               # of two equal observations, of two equal cones: the lower (the costs decide the rest)
    assert list(o["index"]) == [0, 0, 2, 2, 4, 4, 6, 6]
    o = census["square"][2][0]
    assert o["count"] == 4 and o["second_count"] == 4 and o["n_seeds"] == 40


def test_the_checkers_have_teeth(pkg, census):
    """the reference's own answer passes both checkers; a perturbed one fails them"""
    b = pkg.binding
    for name in ("track8", "twelve", "map1023", "frame65", "heading_pi", "nan_query", "twins"):
        c, z, frames = census[name]; o = frames[0]; n = len(c["obs"])
        rec = b._reloc_record(1)
        rec["pose"][0] = o["pose"]; rec["count"][0] = o["count"]; rec["cost"][0] = o["cost"]; rec["seed"][0] = o["seed"]; rec["second_count"][0] = o["second_count"]
        rec["second_pose"][0] = o["second_pose"]; rec["n_seeds"][0] = o["n_seeds"]; rec["status"][0] = o["status"]
        assert not rr.failures(o, rec, 0, o["index"], o["e2"]), (name, rr.failures(o, rec, 0, o["index"], o["e2"]))
        def broken(field, value, idx=None, e2=None):
            r = {k: v.copy() for k, v in rec.items()}
            if field is not None:
                r[field][0] = value
            return rr.failures(o, r, 0, o["index"] if idx is None else idx, o["e2"] if e2 is None else e2)
        assert any("pose xy" in w for w in broken("pose", o["pose"] + np.array([np.spacing(o["pose"][0]), 0.0, 0.0]))), name      # one ulp of tx
        assert any("theta" in w for w in broken("pose", o["pose"] + np.array([0.0, 0.0, 16 * np.spacing(abs(o["pose"][2]) + 1e-300)]))), name
        assert not broken("pose", o["pose"] + np.array([0.0, 0.0, np.spacing(o["pose"][2])])), name                                # an ulp of theta is libm's
        assert any("cost" in w for w in broken("cost", np.nextafter(o["cost"], 1.0))), name
        assert any("count" in w for w in broken("count", o["count"] - 1)) and any("n_seeds" in w for w in broken("n_seeds", o["n_seeds"] + 1)), name
        assert any("second_count" in w for w in broken("second_count", o["second_count"] + 1)) and any("status" in w for w in broken("status", 1 - o["status"])), name
        sd = o["seed"].copy(); sd[3] += 1
        assert any("seed" in w for w in broken("seed", sd)), name
        ix = o["index"].copy(); ix[0] = ix[0] + 1
        e = o["e2"].copy(); e[0] = np.nextafter(e[0], 1.0)
        assert any("index" in w for w in broken(None, None, idx=ix)) and any("e2" in w for w in broken(None, None, e2=e)), name
        # the independent checker: a pose off by a little more than the radius, a heading off by the radius at the farthest cone, a wrong match
        pose, idx = c["truth"][0]; R = 0.5
        assert not rr.check_truth(o["pose"], o["index"], pose, idx, z, R)
        assert rr.check_truth(o["pose"] + np.array([1.01 * R, 0.0, 0.0]), o["index"], pose, idx, z, R)
        assert rr.check_truth(o["pose"] + np.array([0.0, 0.0, 2 * R / 3.0]), o["index"], pose, idx, z, R)
        assert rr.check_truth(o["pose"], ix, pose, idx, z, R)
