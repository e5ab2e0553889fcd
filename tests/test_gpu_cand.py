"""GPU tests of the cone candidates (k_cand_init / k_cand_stage / k_cand_update of gs_cand.hip around the minimum-cost association of
gs_assoc_nn.hip).

Per scene of cand_shapes: gs_cand_batch, gs_cand_resident and a sequence of gs_frame_frontend_candidates calls return identical bits.  Then,
for EVERY step: the device's own table before the step (gs_cand_get between the live calls), fed to the existing gs_assign_opt_batch as a map
with the masked frame, gives bitwise every slot an observation fused with; and cand_ref.StepCheck, fed that table and that association, gives
bitwise every decision, counter, id and untouched slot, and holds every fused and spawned value inside its bound B = 2 e.

The figures the tests print with -s (the largest fraction of a bound reached, the number of values held) are recorded in DESIGN.md section 30."""
import ctypes as C

import numpy as np
import pytest

import cand_ref as cr
import cand_shapes as cs

pytestmark = pytest.mark.gpu
WORST = {"r": 0.0, "where": "", "values": 0, "steps": 0}


@pytest.fixture(scope="module")
def G(pkg):
    if pkg.device_count() < 1:
        pytest.fail("no gfx950 device visible: the HIP path cannot run")
    g = pkg.Graph(lidar_to_cog=cs.LIDAR)
    yield g
    g.close()
    print("\ncone candidates: %d steps checked, %d fused / spawned values held to the exact ones, largest |device - exact| / B %.3g (%s)"
          % (WORST["steps"], WORST["values"], WORST["r"], WORST["where"]))


def blocks(b, sc, **cand):
    c = dict(sc["cand"]); c.update(cand)
    return b.nn_params(**sc["params"]), b.cand_params(**c)


def raw(res):
    """a result's bytes, NaN-proof"""
    return (res["steps"].tobytes(), res["cand_id"].tobytes(), res["cand_slot"].tobytes(), res["table"].tobytes(), res["n_live"])


def run_batch(G, sc, blk):
    return G.cand(sc["poses"], sc["obs"], sc["frame_start"], sc["in_idx_all"], sc["pose_covs"], sc["records"], blk[0], blk[1])


def run_resident(pkg, G, sc, blk, frame_start=None, frame_cap=None, fill=None):
    """the resident call over the scene; fill: the outputs' pattern before the call"""
    b = pkg.binding; DA = b.DeviceArray; n, ns = len(sc["obs"]), len(sc["frames"])
    fsa = sc["frame_start"] if frame_start is None else np.asarray(frame_start, dtype=np.int32)
    cap = int(np.diff(sc["frame_start"]).max()) if frame_cap is None and ns else (frame_cap or 0)
    steps = np.zeros(ns, dtype=b.CAND_STEP); cid = np.zeros(max(n, 1), dtype=np.int32); slot = np.zeros(max(n, 1), dtype=np.int32)
    tab = np.zeros(b.CAND_MAX, dtype=b.CAND); meta = np.zeros(4, dtype=np.int32)
    if fill is not None:
        for a in (steps, cid, slot, tab, meta):
            a.view(np.uint8)[...] = fill
    rec = sc["records"]
    d = dict(obs=DA(sc["obs"]) if n else DA(nbytes=32), fs=DA(fsa), poses=DA(sc["poses"]) if ns else DA(nbytes=32),
             pc=None if sc["pose_covs"] is None else DA(sc["pose_covs"]), ii=None if sc["in_idx_all"] is None or n == 0 else DA(sc["in_idx_all"]),
             rec=None if rec is None else DA(rec.view(np.uint8)), steps=DA(steps.view(np.uint8)) if ns else DA(nbytes=64), cid=DA(cid), slot=DA(slot),
             tab=DA(tab.view(np.uint8)), meta=DA(meta))
    G.cand_resident(d["obs"], n, ns, d["fs"], cap, d["poses"], d["pc"], d["ii"], 0 if rec is None else len(rec), d["rec"], d["steps"], d["cid"], d["slot"],
                    d["tab"], d["meta"], blk[0], blk[1])
    G.synchronize()
    out = dict(steps=d["steps"].to_host(np.uint8, steps.nbytes).view(b.CAND_STEP) if ns else steps, cand_id=d["cid"].to_host(np.int32, len(cid))[:n],
               cand_slot=d["slot"].to_host(np.int32, len(slot))[:n], table=d["tab"].to_host(np.uint8, tab.nbytes).view(b.CAND))
    m = d["meta"].to_host(np.int32, 4); out["meta"] = m; out["n_live"] = int(m[2])
    for a in d.values():
        if a is not None:
            a.free()
    return out


def run_frames(pkg, G, sc, blk):
    """gs_cand_set, then one gs_frame_frontend_candidates per frame, the table read before and after each"""
    b = pkg.binding; n = len(sc["obs"])
    G.cand_set(sc["records"])
    steps = np.zeros(len(sc["frames"]), dtype=b.CAND_STEP); cid = np.zeros(n, dtype=np.int32); slot = np.zeros(n, dtype=np.int32); tables, metas = [], []
    tab, ni, t, nl = G.cand_get(); tables.append(tab); metas.append([ni, t, nl])
    for t, ob in enumerate(sc["frames"]):
        ii = None if sc["in_idx"] is None else sc["in_idx"][t]; pc = None if sc["pose_covs"] is None else sc["pose_covs"][t]
        s, ci, sl = G.frame_frontend_candidates(sc["poses"][t], ob, ii, pc, blk[0], blk[1])
        a = sc["frame_start"][t]; steps[t] = s; cid[a:a + len(ob)] = ci; slot[a:a + len(ob)] = sl
        tab, ni, tt, nl = G.cand_get(); tables.append(tab); metas.append([ni, tt, nl])
    return dict(steps=steps, cand_id=cid, cand_slot=slot, table=tables[-1], n_live=metas[-1][2], tables=tables, metas=metas)


def check_run(G, sc, blk, live):
    """every step of the live run: the association over the device's own table, then the reference — nothing is left out"""
    prm = cs.nn_params_of(sc); cp = dict(sc["cand"]); cp.update({k: getattr(blk[1], k) for k in cr.DEFAULTS})
    tab0, meta0 = cr.load(sc["records"])
    assert live["tables"][0].tobytes() == tab0.tobytes() and live["metas"][0] == meta0, (sc["name"], "the loaded table")
    for t, ob in enumerate(sc["frames"]):
        before, after = live["tables"][t], live["tables"][t + 1]; k = len(ob); a = sc["frame_start"][t]
        ii = None if sc["in_idx"] is None else sc["in_idx"][t]; pc = None if sc["pose_covs"] is None else sc["pose_covs"][t]
        if k:
            mx, mt, mc = cr.as_map(before)
            idx, _, na = G.assign_opt(sc["poses"][t:t + 1], np.zeros(k, dtype=np.int32), cr.masked(ob, ii), [0, k], mx, mt, mc, None if pc is None else pc.reshape(1, 9), blk[0])
        else:
            idx, na = np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
        got_slot = live["cand_slot"][a:a + k]
        assert got_slot[idx >= 0].tobytes() == idx[idx >= 0].tobytes(), (sc["name"], t, "the slots fused with are not gs_assign_opt_batch's over the device's table")
        assert all(before[s]["state"] == cr.FREE for s in got_slot[(idx < 0) & (got_slot >= 0)]), (sc["name"], t, "a spawn into a slot that was not free")
        chk = cr.StepCheck(before, live["metas"][t], ob, ii, sc["poses"][t], pc, idx, na, prm, cp, sc["lidar"])
        bad = chk.failures(after, live["metas"][t + 1], live["steps"][t], live["cand_id"][a:a + k], got_slot)
        assert not bad, (sc["name"], t, bad[:3])
        WORST["steps"] += 1; WORST["values"] += 5 * len(chk.values)
        if chk.worst > WORST["r"]:
            WORST["r"], WORST["where"] = chk.worst, "%s step %d" % (sc["name"], t)


@pytest.mark.parametrize("name", cs.NAMES)
def test_scene_three_paths_and_the_reference(pkg, G, name):
    sc = cs.scene(name); blk = blocks(pkg.binding, sc)
    live = run_frames(pkg, G, sc, blk); batch = run_batch(G, sc, blk); res = run_resident(pkg, G, sc, blk)
    assert raw(live) == raw(batch), (name, "the live calls differ from the batch call")
    assert raw(res) == raw(batch), (name, "the resident call differs from the batch call")
    assert G.cand_get()[0].tobytes() == live["table"].tobytes(), (name, "a batch or resident run disturbed the live table")
    check_run(G, sc, blk, live)


def test_truth_scene_equals_the_replay(pkg, G):
    sc = cs.scene("truth"); blk = blocks(pkg.binding, sc); r = run_batch(G, sc, blk)
    rp = cr.replay(None, sc["poses"], None, sc["frames"], sc["in_idx"], cs.nn_params_of(sc), sc["cand"], sc["lidar"])
    for t, rec in enumerate(rp["steps"]):
        for key in cr.STEP_KEYS:
            assert int(r["steps"][t][key]) == rec[key], (t, key, int(r["steps"][t][key]), rec[key])
    assert r["cand_id"].tobytes() == np.concatenate(rp["cand_id"]).tobytes() and r["cand_slot"].tobytes() == np.concatenate(rp["cand_slot"]).tobytes()
    for key in cr.INT_KEYS:
        assert r["table"][key].tobytes() == rp["table"][key].tobytes(), key
    live = r["table"]["state"] != cr.FREE
    assert np.allclose(r["table"]["xy"][live], rp["table"]["xy"][live], rtol=0, atol=1e-9) and r["n_live"] == rp["meta"][2]
    assert int((r["table"]["state"] == cr.CONFIRMED).sum()) >= 5


def test_resident_defences_write_nothing(pkg, G):
    sc = cs.scene("steps2"); blk = blocks(pkg.binding, sc); n = len(sc["obs"]); a = int(sc["frame_start"][1])
    good = run_resident(pkg, G, sc, blk, fill=0x5a)
    assert raw(good) == raw(run_batch(G, sc, blk))
    for bad in ([0, a, n + 1], [0, a, a - 1], [0, -1, n], [0, a, n]):
        cap = 1 if bad == [0, a, n] else None                                  # the last: good bounds, a frame above frame_cap
        r = run_resident(pkg, G, sc, blk, frame_start=bad, frame_cap=cap, fill=0x5a)
        skipped = [t for t in range(2) if not (0 <= bad[t] <= bad[t + 1] <= n and bad[t + 1] - bad[t] <= (cap or 256))]
        assert skipped, bad
        for t in skipped:
            assert np.all(r["steps"][t:t + 1].view(np.uint8) == 0x5a), (bad, t, "a step that is no frame wrote its record")
        assert int(r["meta"][1]) == 2 - len(skipped), (bad, "a step that is no frame advanced t")
        if 0 not in skipped:
            assert r["steps"][0].tobytes() == good["steps"][0].tobytes(), (bad, "step 0 is the good run's")
            assert r["cand_id"][:a].tobytes() == good["cand_id"][:a].tobytes() and np.all(r["cand_id"][a:].view(np.uint8) == 0x5a)
            assert np.all(r["cand_slot"][a:].view(np.uint8) == 0x5a) and r["n_live"] == int(good["steps"][0]["n_live"])
        else:
            assert np.all(r["cand_id"].view(np.uint8) == 0x5a) and np.all(r["cand_slot"].view(np.uint8) == 0x5a) and r["n_live"] == 0
            assert r["table"].tobytes() == cr.load(None)[0].tobytes(), (bad, "no step ran, yet the table is not the loaded one")


def test_null_outputs_work(pkg, G):
    b = pkg.binding; sc = cs.scene("steps2"); prm, cp = blocks(b, sc); L = G.L; dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    assert L.gs_cand_batch(G.h, 2, len(sc["obs"]), sc["obs"].ctypes.data_as(dp), sc["frame_start"].ctypes.data_as(ip), sc["poses"].ctypes.data_as(dp), None, None,
                           0, None, C.byref(prm), C.byref(cp), None, None, None, None, None) == 0
    DA = b.DeviceArray; d = [DA(sc["obs"]), DA(sc["frame_start"]), DA(sc["poses"])]
    G.cand_resident(d[0], len(sc["obs"]), 2, d[1], 8, d[2], params=prm, cand=cp); G.synchronize()
    for a in d:
        a.free()
    G.cand_clear()
    assert L.gs_frame_frontend_candidates(G.h, sc["poses"][0].ctypes.data_as(dp), None, sc["frames"][0].ctypes.data_as(dp), 8, None, C.byref(prm), C.byref(cp),
                                          None, None, None) == 0
    assert L.gs_cand_get(G.h, None, None, None, None) == 0
    tab, ni, t, nl = G.cand_get()
    assert (ni, t, nl) == (8, 1, 8), "the frame call with no outputs still ran its step"
    fresh = pkg.Graph(lidar_to_cog=cs.LIDAR)                                  # a handle that never set a table: an empty one
    tab, ni, t, nl = fresh.cand_get()
    assert tab.tobytes() == cr.load(None)[0].tobytes() and (ni, t, nl) == (0, 0, 0) and len(fresh.cand_take_confirmed()) == 0
    fresh.close()


def test_take_confirmed_frees_exactly_the_confirmed_slots(pkg, G):
    b = pkg.binding; sc = cs.scene("steps12"); blk = blocks(b, sc); run_frames(pkg, G, sc, blk)
    before, ni, t, nl = G.cand_get(); conf = np.flatnonzero(before["state"] == cr.CONFIRMED)
    assert len(conf) >= 2
    n = C.c_int32(0); small = np.zeros(1, dtype=b.CAND)
    assert G.L.gs_cand_take_confirmed(G.h, 1, small.ctypes.data_as(C.c_void_p), C.byref(n)) == -1 and G.cand_get()[0].tobytes() == before.tobytes(), "cap too small: nothing changes"
    got = G.cand_take_confirmed()
    assert got["id"].tolist() == sorted(before["id"][conf].tolist()) and all(got[i].tobytes() == before[before["id"] == got[i]["id"]][0].tobytes() for i in range(len(got)))
    after, ni2, t2, nl2 = G.cand_get(); want = before.copy(); want[conf] = cr.free_record()
    assert after.tobytes() == want.tobytes() and (ni2, t2, nl2) == (ni, t, nl - len(conf))
    assert len(G.cand_take_confirmed()) == 0
    # the freed slots are invisible to the next step and free for its spawners
    s, ci, sl = G.frame_frontend_candidates(sc["poses"][0], sc["frames"][0], None, None, *blk)
    assert int(s["n_fused"]) == int((want["state"] != cr.FREE).sum()) and sorted(sl[ci >= ni]) == sorted(conf.tolist())[:int(s["n_spawned"])]


def test_promote_makes_the_next_association_explain_the_cones(pkg, G):
    b = pkg.binding; sc = cs.scene("steps3"); blk = blocks(b, sc); run_frames(pkg, G, sc, blk)
    G.map_clear(); rec, first = G.cand_promote()
    assert first == 0 and len(rec) == 6 and G.map_size() == 6 and np.all(rec["state"] == cr.CONFIRMED)
    assert G.map_cov(0).reshape(-1, 4).tobytes() == rec["cov"].tobytes()
    idx = G.frame_frontend_assign_opt(sc["poses"][2], sc["frames"][2], None, blk[0])[2]
    explained = idx >= 0
    assert int(explained.sum()) == 6, "the promoted cones explain their observations"
    s, ci, sl = G.frame_frontend_candidates(sc["poses"][2], sc["frames"][2], idx, None, *blk)
    assert int(s["n_unexplained"]) == 2 and np.all(ci[explained] == -1) and int(s["n_fused"]) == 2, "what is left for the candidates are the two tentative cones"
    G.map_clear()


def test_other_calls_are_unchanged_by_a_candidate_run(pkg, G):
    import follow_shapes as fs
    import localize_shapes as ls
    c = ls.scene("rotation"); b = pkg.binding; prm = b.nn_params(**c["params"]); g = pkg.Graph(lidar_to_cog=ls.LIDAR)
    g.map_clear(); g.map_append(c["map_xy"], c["map_ty"])
    before = g.frame_frontend_localize(c["poses"][0], c["obs"], c["pose_cov"], prm)
    fsc = fs.scene("h2_s2"); fb = (b.nn_params(**fsc["params"]), b.jc_params(), b.loc_params(**fsc["loc"]), b.follow_params(**fsc["follow"]))
    follow = lambda: g.follow(fsc["poses"], fsc["obs"], fsc["frame_start"], fsc["motion"], fsc["map_xy"], fsc["map_ty"], fsc["covs"], fsc["motion_cov"], None, *fb)
    f0 = follow()
    t = pkg.track.generate(50, 30); gb = pkg.track.bench_graph(t, g); S = pkg.Graph(device=0); S.load_bench_graph(gb); S.optimize(1); p0 = S.poses().copy(); S.close()
    sc = cs.scene("steps3"); blk = blocks(b, sc); run_batch(g, sc, blk); run_frames(pkg, g, sc, blk)
    after = g.frame_frontend_localize(c["poses"][0], c["obs"], c["pose_cov"], prm)
    for x, y in zip(before[:5], after[:5]):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    for key in before[6]:
        assert np.asarray(before[6][key]).tobytes() == np.asarray(after[6][key]).tobytes(), key
    f1 = follow()
    assert f0["steps"].tobytes() == f1["steps"].tobytes() and f0["state"].tobytes() == f1["state"].tobytes() and f0["index"].tobytes() == f1["index"].tobytes()
    S = pkg.Graph(device=0); S.load_bench_graph(gb); S.cand_set(sc["records"]); S.frame_frontend_candidates(sc["poses"][0], sc["frames"][0]); S.optimize(1)
    assert S.poses().tobytes() == p0.tobytes(), "gs_iterate after a candidate call on the same handle"
    S.close(); g.close()
