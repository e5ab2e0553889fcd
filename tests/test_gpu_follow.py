"""GPU tests of frame following (k_follow_stage / k_follow_update of gs_follow.hip around the chain of gs_assoc_nn.hip).

Per scene of follow_shapes: gs_follow_batch, gs_follow_resident and a sequence of gs_frame_frontend_follow calls return identical bits, with the
hashed grid and with the whole-map search.  Then, for EVERY step and EVERY hypothesis that tracked at it: the device's prior is inside
follow_ref.predict_exact's bound (theta- bit for bit); the device's own priors, fed to the existing gs_assign_opt_batch ->
gs_joint_compat_batch -> gs_localize_batch with every hypothesis a frame of its own, give bitwise the chain record and the pruned index of the
step; and follow_ref.update, fed those chain records, gives bitwise the step's decisions, the final state, best and n_tracking.

Measured on an MI355X (the tests print these figures with -s): over the 20 scenes 118 predicted priors held to the exact prediction, the largest
|device - exact| / B 0.424 (cov_null, step 2, hypothesis 1, the heading variance); 265 hypothesis-steps bitwise equal to the chain's own calls; in
the truth scene the hypothesis one cone spacing along is rejected at step 0 with chi2 7.85 on 3 pairs and lost at step 2; the file runs in about
1.2 seconds."""
import ctypes as C

import numpy as np
import pytest

import follow_ref as fr
import follow_shapes as fs

pytestmark = pytest.mark.gpu
WORST = {"r": 0.0, "where": "", "priors": 0, "chains": 0}
STATE_KEYS = ("sum_chi2", "hits", "frames_hit", "frames_missed", "misses", "state", "state_step", "duplicate_of")


@pytest.fixture(scope="module")
def G(pkg):
    if pkg.device_count() < 1:
        pytest.fail("no gfx950 device visible: the HIP path cannot run")
    g = pkg.Graph(lidar_to_cog=fs.LIDAR)
    yield g
    g.close()
    print("\nframe following: %d priors held to the exact prediction, largest |device - exact| / B %.3g (%s); %d hypothesis-steps equal to the chain's calls"
          % (WORST["priors"], WORST["r"], WORST["where"], WORST["chains"]))


def blocks(b, sc, **follow):
    f = dict(sc["follow"]); f.update(follow)
    return b.nn_params(**sc["params"]), b.jc_params(), b.loc_params(**sc["loc"]), b.follow_params(**f)


def set_map(G, sc):
    G.map_clear(); G.map_append(sc["map_xy"], sc["map_ty"])
    assert G.map_size() == len(sc["map_ty"])


def raw(res):
    """a result's bytes, NaN-proof"""
    return (res["steps"].tobytes(), None if res["index"] is None else res["index"].tobytes(), res["state"].tobytes(), res["best"], res["n_tracking"])


def run_batch(G, sc, blk, poses=None, covs=None, index=True):
    prm, jc, loc, fp = blk
    poses = sc["poses"] if poses is None else poses
    return G.follow(poses, sc["obs"], sc["frame_start"], sc["motion"], sc["map_xy"], sc["map_ty"], sc["covs"] if covs is None else covs, sc["motion_cov"],
                    None, prm, jc, loc, fp, index)


def run_resident(pkg, G, sc, blk, frame_start=None, frame_cap=None, fill=None):
    """the resident call over the scene (the map must be resident); fill: the outputs' pattern before the call"""
    b = pkg.binding; DA = b.DeviceArray; prm, jc, loc, fp = blk
    nh, n, ns = len(sc["poses"]), len(sc["obs"]), len(sc["frames"])
    fsa = sc["frame_start"] if frame_start is None else np.asarray(frame_start, dtype=np.int32)
    cap = int(np.diff(sc["frame_start"]).max()) if frame_cap is None and ns else (frame_cap or 0)
    steps = np.zeros((ns, nh), dtype=b.FOLLOW_STEP); idx = np.zeros((nh, max(n, 1)), dtype=np.int32); state = np.zeros(nh, dtype=b.FOLLOW_STATE); best = np.zeros(2, dtype=np.int32)
    if fill is not None:
        steps.view(np.uint8)[...] = fill; idx.view(np.uint8)[...] = fill; state.view(np.uint8)[...] = fill; best.view(np.uint8)[...] = fill
    d = dict(poses=DA(sc["poses"]), obs=DA(sc["obs"]) if n else DA(nbytes=32), fs=DA(fsa), mo=DA(sc["motion"]) if ns > 1 else None,
             cv=None if sc["covs"] is None else DA(sc["covs"]), mq=None if sc["motion_cov"] is None or ns < 2 else DA(sc["motion_cov"]),
             steps=DA(steps), idx=DA(idx), state=DA(state), best=DA(best))
    G.follow_resident(d["poses"], nh, d["obs"], n, ns, d["fs"], cap, d["mo"], d["cv"], d["mq"], d["steps"], d["idx"], d["state"], d["best"], prm, jc, loc, fp)
    G.synchronize()
    out = dict(steps=d["steps"].to_host(np.uint8, steps.nbytes).view(b.FOLLOW_STEP).reshape(ns, nh), index=d["idx"].to_host(np.int32, idx.size).reshape(nh, -1)[:, :n],
               state=d["state"].to_host(np.uint8, state.nbytes).view(b.FOLLOW_STATE))
    b2 = d["best"].to_host(np.int32, 2); out["best"], out["n_tracking"] = int(b2[0]), int(b2[1])
    for a in d.values():
        if a is not None:
            a.free()
    return out


def run_frames(pkg, G, sc, blk):
    """gs_follow_set, then one gs_frame_frontend_follow per frame (the map must be resident)"""
    b = pkg.binding; prm, jc, loc, fp = blk; nh, n = len(sc["poses"]), len(sc["obs"])
    G.follow_set(sc["poses"], sc["covs"])
    steps, idx = [], np.zeros((nh, n), dtype=np.int32); best, nt = 0, nh
    for t, ob in enumerate(sc["frames"]):
        s, ix, best, nt = G.frame_frontend_follow(ob, sc["motion"][t - 1] if t else None, sc["motion_cov"][t - 1] if t and sc["motion_cov"] is not None else None,
                                                  prm, jc, loc, fp)
        steps.append(s); a = sc["frame_start"][t]; idx[:, a:a + len(ob)] = ix
    state, gb, gn = G.follow_get()
    if sc["frames"]:
        assert (gb, gn) == (best, nt)
    return dict(steps=np.stack(steps) if steps else np.zeros((0, nh), dtype=b.FOLLOW_STEP), index=idx, state=state, best=gb, n_tracking=gn)


def chain_of(G, sc, blk, t, priors_pose, priors_cov):
    """the existing batch calls over len(priors) frames that each hold frame t: (pruned index [m, k], n_kept [m], localisation record)"""
    prm, jc, loc, _ = blk; ob = sc["frames"][t]; k, m = len(ob), len(priors_pose)
    obs = np.tile(ob, (m, 1)); po = np.repeat(np.arange(m, dtype=np.int32), k); fst = (np.arange(m + 1) * k).astype(np.int32)
    a = G.assign_opt(priors_pose, po, obs, fst, sc["map_xy"], sc["map_ty"], None, priors_cov, prm)[0]
    j, jr = G.joint_compat(priors_pose, po, obs, fst, sc["map_xy"], a, None, priors_cov, prm, jc)
    lr = G.localize(priors_pose, po, obs, fst, sc["map_xy"], j, None, priors_cov, prm, loc)
    return j.reshape(m, k), jr["n_kept"], lr


def check_run(pkg, G, sc, blk, res):
    """every step and every hypothesis that tracked at it: the prior, the chain, the update — nothing is left out"""
    b = pkg.binding; nh = len(sc["poses"]); fp = dict(fr.DEFAULTS); fp.update(sc["follow"]); fp.update({k: getattr(blk[3], k) for k in fr.DEFAULTS})
    gate = np.array(blk[1].gate[:])
    st = fr.new_state(sc["poses"], sc["covs"]); steps = res["steps"]
    for t in range(len(sc["frames"])):
        tracking = [h for h in range(nh) if st["state"][h] == fr.TRACKING]
        assert [h for h in range(nh) if steps[t, h]["status"] != -1] == tracking, (sc["name"], t, "who tracks")
        priors = {}
        for h in tracking:
            r = steps[t, h]; pp, pc = r["prior_pose"], r["prior_cov"]
            assert pc.reshape(3, 3).tobytes() == pc.reshape(3, 3).T.copy().tobytes(), (sc["name"], t, h, "the prior covariance is not bitwise symmetric")
            if t == 0:
                assert pp.tobytes() == st["pose"][h].tobytes() and pc.tobytes() == st["cov"][h].tobytes(), (sc["name"], h, "step 0's prior is the given state")
            else:
                qu = None if sc["motion_cov"] is None else sc["motion_cov"][t - 1]
                assert pp[2].tobytes() == fr.predict64(st["pose"][h], st["cov"][h], sc["motion"][t - 1], qu)[0][2].tobytes(), (sc["name"], t, h, "theta-")
                if np.isfinite(st["pose"][h]).all():
                    xm, ym, _, S = fr.predict_exact(st["pose"][h], st["cov"][h], sc["motion"][t - 1], qu)
                    for what, dev, ref in [("x", pp[0], xm), ("y", pp[1], ym)] + [("cov%d" % e, pc[fr.UP[e]], S[e]) for e in range(6)]:
                        ok, ratio = fr.inside(dev, ref)
                        assert ok, (sc["name"], t, h, what, float(dev), ratio)
                        if ratio > WORST["r"]:
                            WORST["r"], WORST["where"] = ratio, "%s step %d hyp %d %s" % (sc["name"], t, h, what)
                    WORST["priors"] += 1
                else:
                    assert not np.isfinite(pp[:2]).all(), (sc["name"], t, h, "a NaN pose predicts a finite one")
            priors[h] = (pp.copy(), pc.copy())
        chain = {}
        k = len(sc["frames"][t]); a = sc["frame_start"][t]
        if tracking and k:
            j, kept, lr = chain_of(G, sc, blk, t, np.stack([priors[h][0] for h in tracking]), np.stack([priors[h][1] for h in tracking]))
            for m, h in enumerate(tracking):
                chain[h] = dict(pose=lr["pose"][m], cov=lr["cov"][m], chi2=lr["chi2"][m], n_pairs=lr["n_pairs"][m], iterations=lr["iterations"][m],
                                status=lr["status"][m], n_kept=kept[m])
                assert res["index"][h, a:a + k].tobytes() == j[m].tobytes(), (sc["name"], t, h, "the pruned index")
                WORST["chains"] += 1
        else:
            chain = {h: fr.empty_record(*priors[h]) for h in tracking}
        for h in range(nh):
            if h not in tracking:
                assert np.all(res["index"][h, a:a + k] == -1), (sc["name"], t, h, "a retired hypothesis has an index")
        recs, best, nt = fr.update(st, t, priors, chain, gate, fp)
        for h, r in enumerate(recs):
            bad = fr.mismatches(steps[t, h], r)
            assert not bad, (sc["name"], t, h, bad, steps[t, h], r)
    assert res["state"]["pose"].tobytes() == st["pose"].tobytes() and res["state"]["cov"].tobytes() == st["cov"].tobytes(), (sc["name"], "final pose / cov")
    for key in STATE_KEYS:
        assert res["state"][key].tobytes() == np.ascontiguousarray(st[key]).tobytes(), (sc["name"], "final", key, res["state"][key], st[key])
    assert (res["best"], res["n_tracking"]) == (fr.best_of(st), int((st["state"] == fr.TRACKING).sum())), (sc["name"], "best / n_tracking")
    for key, want in sc["expect"].items():
        if key == "best":
            assert res["best"] == want, (sc["name"], "best", res["best"])
        else:
            for h, w in enumerate(want):
                assert w is None or int(res["state"][key][h]) == w, (sc["name"], key, h, int(res["state"][key][h]), w)
    return st


@pytest.mark.parametrize("name", fs.NAMES)
def test_scene_three_paths_both_searches_and_the_reference(pkg, G, name):
    sc = fs.scene(name); blk = blocks(pkg.binding, sc); set_map(G, sc)
    res = {}
    for grid in (-1, 0, 1):
        G.set_debug(assoc_grid=grid)
        res["batch %d" % grid] = run_batch(G, sc, blk)
        res["resident %d" % grid] = run_resident(pkg, G, sc, blk)
        res["frames %d" % grid] = run_frames(pkg, G, sc, blk)
    G.set_debug(assoc_grid=-1)
    first = res["batch -1"]
    for path, r in res.items():
        assert raw(r) == raw(first), (name, path, "differs from the batch call")
    check_run(pkg, G, sc, blk, first)


def test_sixty_four_hypotheses_equal_each_alone(pkg, G):
    sc = fs.scene("h64_s12"); blk = blocks(pkg.binding, sc, merge_xy=0.0); set_map(G, sc)
    all_ = run_batch(G, sc, blk)
    assert np.all(all_["state"]["state"] != fr.DUPLICATE)
    for h in range(len(sc["poses"])):
        one = run_batch(G, sc, blk, poses=sc["poses"][h:h + 1], covs=sc["covs"][h:h + 1])
        assert one["steps"][:, 0].tobytes() == all_["steps"][:, h].tobytes(), (h, "steps")
        assert one["index"][0].tobytes() == all_["index"][h].tobytes() and one["state"][0].tobytes() == all_["state"][h].tobytes(), (h, "index / state")


def test_truth_scene(pkg, G):
    sc = fs.scene("truth"); blk = blocks(pkg.binding, sc); set_map(G, sc)
    r = run_batch(G, sc, blk); gate = np.array(blk[1].gate[:]); cl = __import__("relocalize_shapes").track()[2]
    assert r["best"] == 0 and np.all(r["steps"][:, 0]["accepted"] == 1) and r["state"]["state"][0] == fr.TRACKING
    end = cl[fs.AT + 11]
    assert np.hypot(*(r["state"]["pose"][0, :2] - end[:2])) < 0.05
    assert np.all(r["steps"][:, 0]["chi2"] < 0.5 * gate[r["steps"][:, 0]["n_pairs"]])
    assert r["state"]["state"][2] == fr.LOST and r["state"]["state_step"][2] == blk[3].max_misses - 1 and r["state"]["hits"][2] == 0
    print("\ntruth scene: hypothesis 1 (one cone spacing along) ends in state %d at step %d, accepted %s, chi2 %s" % (
        r["state"]["state"][1], r["state"]["state_step"][1], r["steps"][:, 1]["accepted"].tolist(), np.round(r["steps"][:, 1]["chi2"], 2).tolist()))


def test_resident_defences_write_nothing(pkg, G):
    sc = fs.scene("h2_s2"); blk = blocks(pkg.binding, sc); set_map(G, sc); n = len(sc["obs"]); a = int(sc["frame_start"][1])
    good = run_resident(pkg, G, sc, blk, fill=0x5a)
    assert raw(good) == raw(run_batch(G, sc, blk))
    for bad in ([0, a, n + 1], [0, a, a - 1], [0, -1, n], [0, a, n]):
        cap = 1 if bad == [0, a, n] else None                                  # the last: good bounds, a frame above frame_cap
        r = run_resident(pkg, G, sc, blk, frame_start=bad, frame_cap=cap, fill=0x5a)
        # the bounds (a .. bad[2]) of step 1 are no frame (and, with bad[1] = -1 or the cap, those of step 0): that step left the pattern
        skipped = [t for t in range(2) if not (0 <= bad[t] <= bad[t + 1] <= n and bad[t + 1] - bad[t] <= (cap or 256))]
        assert skipped, bad
        for t in skipped:
            assert np.all(r["steps"][t].view(np.uint8) == 0x5a), (bad, t, "a step that is no frame wrote its records")
        if 0 not in skipped:
            assert r["steps"][0].tobytes() == good["steps"][0].tobytes(), (bad, "step 0 is the good run's")
            assert r["index"][:, :a].tobytes() == good["index"][:, :a].tobytes() and np.all(r["index"][:, a:].view(np.uint8) == 0x5a)
            assert r["state"]["frames_hit"].tolist() == good["steps"][0]["accepted"].tolist()
        else:
            assert np.all(r["index"].view(np.uint8) == 0x5a) and np.all(r["state"]["frames_hit"] == 0) and np.all(r["state"]["frames_missed"] == 0)


def test_null_outputs_and_refusals_on_the_device(pkg, G):
    b = pkg.binding; sc = fs.scene("h2_s2"); prm, jc, loc, fp = blocks(b, sc); set_map(G, sc); L = G.L
    rc = L.gs_follow_batch(G.h, 2, sc["poses"].ctypes.data_as(C.POINTER(C.c_double)), None, 2, len(sc["obs"]), sc["obs"].ctypes.data_as(C.POINTER(C.c_double)),
                           sc["frame_start"].ctypes.data_as(C.POINTER(C.c_int32)), sc["motion"].ctypes.data_as(C.POINTER(C.c_double)), None, len(sc["map_ty"]),
                           sc["map_xy"].ctypes.data_as(C.POINTER(C.c_double)), sc["map_ty"].ctypes.data_as(C.POINTER(C.c_int32)), None, C.byref(prm), C.byref(jc),
                           C.byref(loc), C.byref(fp), None, None, None, None, None)
    assert rc == 0
    DA = b.DeviceArray; d = [DA(sc["poses"]), DA(sc["obs"]), DA(sc["frame_start"]), DA(sc["motion"])]
    G.follow_resident(d[0], 2, d[1], len(sc["obs"]), 2, d[2], 8, d[3]); G.synchronize()
    for a in d:
        a.free()
    G.follow_set(sc["poses"])
    assert L.gs_frame_frontend_follow(G.h, None, None, sc["frames"][0].ctypes.data_as(C.POINTER(C.c_double)), 8, C.byref(prm), C.byref(jc), C.byref(loc), C.byref(fp),
                                      None, None, None, None) == 0
    with pytest.raises(b.GsError):                                             # a second frame without a motion record
        G.frame_frontend_follow(sc["frames"][1])
    G.follow_set(sc["poses"])
    with pytest.raises(b.GsError):                                             # a first frame with one
        G.frame_frontend_follow(sc["frames"][0], sc["motion"][0])
    fresh = pkg.Graph(lidar_to_cog=fs.LIDAR)
    with pytest.raises(b.GsError):
        fresh.frame_frontend_follow(sc["frames"][0])
    with pytest.raises(b.GsError):
        fresh.follow_get()
    fresh.close()


def test_other_calls_are_unchanged_by_a_follow_call(pkg, G):
    import localize_shapes as ls
    c = ls.scene("rotation"); b = pkg.binding; prm = b.nn_params(**c["params"]); g = pkg.Graph(lidar_to_cog=ls.LIDAR)
    g.map_clear(); g.map_append(c["map_xy"], c["map_ty"])
    before = g.frame_frontend_localize(c["poses"][0], c["obs"], c["pose_cov"], prm)
    t = pkg.track.generate(50, 30); gb = pkg.track.bench_graph(t, g); S = pkg.Graph(device=0); S.load_bench_graph(gb); S.optimize(1); p0 = S.poses().copy(); S.close()
    sc = fs.scene("h2_s2"); run_batch(g, sc, blocks(b, sc))
    g.map_clear(); g.map_append(sc["map_xy"], sc["map_ty"]); run_frames(pkg, g, sc, blocks(b, sc))
    g.map_clear(); g.map_append(c["map_xy"], c["map_ty"])
    after = g.frame_frontend_localize(c["poses"][0], c["obs"], c["pose_cov"], prm)
    for x, y in zip(before[:5], after[:5]):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    for key in before[6]:
        assert np.asarray(before[6][key]).tobytes() == np.asarray(after[6][key]).tobytes(), key
    S = pkg.Graph(device=0); S.load_bench_graph(gb); S.follow_set(sc["poses"]); S.optimize(1)
    assert S.poses().tobytes() == p0.tobytes(), "gs_iterate after a follow call on the same handle"
    S.close(); g.close()
