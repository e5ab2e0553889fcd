"""CPU tests of the cone candidates: the fusion's algebra in 40 digits, the float64 step inside the reference's bound, each rule on hand-made
records, the float64 replay of the truth scene (and the margins the GPU test rests on), that the checker rejects no scene, every refusal of the
new calls and GS_ERR_NO_DEVICE on a host-only handle, the defaults, struct sizes and exported symbols, the checker's teeth, and the host layout
helper under AddressSanitizer / UndefinedBehaviorSanitizer as a stand-alone program."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import cand_ref as cr
import cand_shapes as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
mp = cr.MP
MARGIN = 1e-6


def _spd(rng, scale):
    a = rng.normal(size=(2, 2)); m = a @ a.T * scale + np.eye(2) * scale * 0.1
    return m


def test_fusion_algebra_in_forty_digits():
    """K A (the form the kernel runs) equals C - K C (the textbook form, which cancels) and the information-form fusion (C^-1 + A^-1)^-1,
    and l + K (g - l) equals C+ (C^-1 l + A^-1 g), in 40-digit arithmetic"""
    rng = np.random.default_rng(4)
    with mp.workdps(40):
        for _ in range(30):
            Cn, An = _spd(rng, 10.0 ** rng.uniform(-4, 0)), _spd(rng, 10.0 ** rng.uniform(-4, 0)); l, g = rng.normal(0, 20, 2), rng.normal(0, 20, 2)
            Cm = mp.matrix(Cn.tolist()); Am = mp.matrix(An.tolist()); lm, gm = mp.matrix(l.tolist()), mp.matrix(g.tolist())
            K = Cm * (Cm + Am) ** -1
            KA, CKC, info = K * Am, Cm - K * Cm, (Cm ** -1 + Am ** -1) ** -1
            scale = max(abs(KA[r, c]) for r in range(2) for c in range(2))
            for r in range(2):
                for c in range(2):
                    assert abs(KA[r, c] - CKC[r, c]) <= mp.mpf(10) ** -30 * scale and abs(KA[r, c] - info[r, c]) <= mp.mpf(10) ** -30 * scale
            lp = lm + K * (gm - lm); li = info * (Cm ** -1 * lm + Am ** -1 * gm)
            assert all(abs(lp[r] - li[r]) <= mp.mpf(10) ** -28 * (1 + abs(lp[r])) for r in range(2))
            # and the header's lines (cand_ref._fuse) are that K A: float64 inside 1e-9 of it for these well-conditioned blocks
            x, y, c00, c01, c11 = cr.fuse64(l, Cn.reshape(4), g, [An[0, 0], An[0, 1], An[1, 1]])
            for got, want in ((x, lp[0]), (y, lp[1]), (c00, KA[0, 0]), (c01, KA[0, 1]), (c11, KA[1, 1])):
                assert abs(mp.mpf(float(got)) - want) <= 1e-9 * (abs(want) + scale)


def _as_device(sc):
    """the float64 replay of a scene, and every step checked by the reference as a device run would be: (replay, the largest fraction of a bound)"""
    prm = cs.nn_params_of(sc); cp = sc["cand"]
    rp = cr.replay(sc["records"], sc["poses"], sc["pose_covs"], sc["frames"], sc["in_idx"], prm, cp, sc["lidar"])
    tab, meta = cr.load(sc["records"]); worst = 0.0
    for t, frame in enumerate(sc["frames"]):
        ii = None if sc["in_idx"] is None else sc["in_idx"][t]; pc = None if sc["pose_covs"] is None else sc["pose_covs"][t]
        slot, na, _, _ = cr.associate64(tab, sc["poses"][t], pc, frame, ii, prm, sc["lidar"], [])
        chk = cr.StepCheck(tab, meta, frame, ii, sc["poses"][t], pc, slot, na, prm, cp, sc["lidar"])
        after = rp["tables"][t]; m = chk.meta if t + 1 < len(sc["frames"]) else rp["meta"]
        bad = chk.failures(after, m, rp["steps"][t], rp["cand_id"][t], rp["cand_slot"][t])
        assert not bad, (sc["name"], t, bad[:3])
        worst = max(worst, chk.worst); tab, meta = after, chk.meta
    assert meta == rp["meta"]
    return rp, worst


@pytest.mark.parametrize("name", [n for n in cs.NAMES if n != "truth"])
def test_no_scene_is_rejected_and_the_float64_step_stays_inside_the_bound(name):
    """cand_ref.StepCheck over the float64 replay of every scene: no decision inside its band (it would raise Rejected), every integer bit for
    bit, every fused and spawned value inside B = 2 e — and not at 0 where something was fused: the bound is not vacuous"""
    sc = cs.scene(name); rp, worst = _as_device(sc)
    assert worst < 1.0
    if any(r["n_fused"] for r in rp["steps"]):
        assert worst > 0.0
    assert min(rp["margins"], default=1.0) > MARGIN, (name, min(rp["margins"]))


def _run(records, frames, cand=None, in_idx=None, pose=cs.POSE0, params=None):
    sc = cs.pack("hand", [pose] * len(frames), frames, records=records, in_idx=in_idx, params=params, cand=cand)
    return cr.replay(sc["records"], sc["poses"], None, sc["frames"], sc["in_idx"], cs.nn_params_of(sc), sc["cand"], sc["lidar"])


def test_rules_on_hand_made_records():
    P = cs.POSE0; at = lambda z: cs.ahead(P, [z])[0]; obs = lambda zs, ty=None: cs.see(P, cs.ahead(P, zs), ty if ty is not None else [1] * len(zs))
    none = np.zeros((0, 4))
    # confirmation at exactly confirm_hits: a record with 1 hit is tentative after its second, confirmed by its third
    r = _run([cr.record(at([8.0, 0.5]), id=5, hits=1)], [obs([[8.0, 0.5]])] * 2)
    assert [int(t[0]["state"]) for t in r["tables"]] == [1, 2] and [int(t[0]["hits"]) for t in r["tables"]] == [2, 3]
    assert [s["step"] for s in r["steps"]] == [1, 2], "a loaded table goes on counting behind its largest last_step"
    assert int(r["table"][0]["confirm_step"]) == 2 and [s["n_confirmed"] for s in r["steps"]] == [0, 1] and r["cand_id"][0].tolist() == [5]
    # a hit resets misses; an unseen slot (behind the car) keeps its misses; a visible one counts
    r = _run([cr.record(at([8.0, 0.5]), id=0, misses=2, last_step=3), cr.record(at([-8.0, 0.0]), id=1, misses=2, last_step=3), cr.record(at([6.0, 2.0]), id=2, misses=0, last_step=3)],
             [obs([[8.0, 0.5]])], cand=dict(max_misses=5))
    assert r["table"]["misses"][:3].tolist() == [0, 2, 1] and r["steps"][0]["n_missed"] == 1 and r["steps"][0]["step"] == 4 and r["table"]["last_step"][:3].tolist() == [4, 3, 3]
    # a confirmed slot never retires; a tentative one beside it does, at exactly max_misses
    r = _run([cr.record(at([6.0, 1.0]), id=0, state=cr.CONFIRMED, misses=7, confirm_step=0), cr.record(at([6.0, -1.0]), id=1, misses=1)], [none, none])
    assert [int(t[0]["state"]) for t in r["tables"]] == [2, 2] and int(r["table"][0]["misses"]) == 9
    assert [int(t[1]["state"]) for t in r["tables"]] == [1, 0] and [s["n_retired"] for s in r["steps"]] == [0, 1] and r["steps"][1]["n_live"] == 1
    assert np.isnan(r["table"][1]["xy"]).all() and int(r["table"][1]["id"]) == -1
    # a retired slot is not reused in the same step, but in the next
    sc = cs.scene("retire_spawn"); r = cr.replay(sc["records"], sc["poses"], None, sc["frames"], None, cs.nn_params_of(sc), sc["cand"], sc["lidar"])
    assert r["cand_slot"][0].tolist() == [1] and r["steps"][0]["n_retired"] == 1 and r["steps"][0]["n_spawned"] == 1 and r["cand_slot"][1].tolist() == [1, 0]
    assert r["cand_id"][0].tolist() == [10] and r["cand_id"][1].tolist() == [10, 11]
    # spawn order (ascending observation into ascending free slot) and the table-full drop
    sc = cs.scene("free_255_256_1023"); r = cr.replay(sc["records"], sc["poses"], None, sc["frames"], None, cs.nn_params_of(sc), sc["cand"], sc["lidar"])
    assert r["cand_slot"][0].tolist() == [255, 256, 1023, -1] and r["cand_id"][0].tolist() == [1023, 1024, 1025, -1]
    assert (r["steps"][0]["n_spawned"], r["steps"][0]["n_dropped"], r["steps"][0]["n_live"]) == (3, 1, 1024)
    assert r["cand_slot"][1].tolist() == [255, 256, 1023, -1] and (r["steps"][1]["n_fused"], r["steps"][1]["n_dropped"]) == (3, 1)
    # contested: two observations admissible to one slot, one fuses, the other does nothing
    sc = cs.scene("contested"); r = cr.replay(sc["records"], sc["poses"], None, sc["frames"], None, cs.nn_params_of(sc), sc["cand"], sc["lidar"])
    s = r["steps"][0]; assert (s["n_fused"], s["n_contested"], s["n_spawned"]) == (1, 1, 1) and r["cand_slot"][0].tolist() == [0, -1, 1]
    # out of spawn range
    sc = cs.scene("far"); r = cr.replay(sc["records"], sc["poses"], None, sc["frames"], None, cs.nn_params_of(sc), sc["cand"], sc["lidar"])
    s = r["steps"][0]; assert (s["n_spawned"], s["n_far"]) == (1, 2) and r["cand_slot"][0].tolist() == [0, -1, -1]
    # a type mismatch spawns beside a candidate
    sc = cs.scene("type_mismatch"); r = cr.replay(sc["records"], sc["poses"], None, sc["frames"], None, cs.nn_params_of(sc), sc["cand"], sc["lidar"])
    assert r["cand_slot"][0].tolist() == [1] and r["cand_slot"][1].tolist() == [1, 0] and r["table"]["type"][:2].tolist() == [1, 2]
    assert np.hypot(*(r["table"][0]["xy"] - r["table"][1]["xy"])) < 1e-5        # (A0 carries a float pi: a round trip is good to 1e-7)
    # explained observations and invalid queries are counted in nothing but n_unexplained
    sc = cs.scene("nan_obs"); r = cr.replay(sc["records"], sc["poses"], None, sc["frames"], None, cs.nn_params_of(sc), sc["cand"], sc["lidar"])
    s = r["steps"][0]; assert (s["n_unexplained"], s["n_spawned"], s["n_fused"], s["n_contested"], s["n_far"], s["n_dropped"]) == (5, 2, 0, 0, 0, 0)


def test_replay_of_the_truth_scene():
    sc = cs.scene("truth"); prm = cs.nn_params_of(sc); cp = sc["cand"]
    rp = cr.replay(None, sc["poses"], None, sc["frames"], sc["in_idx"], prm, cp, sc["lidar"])
    assert min(rp["margins"]) > MARGIN, "a gate, Euclidean or visibility decision of the truth scene is closer than the stated margin"
    # which candidate id belongs to which truth cone (or false detection -1 - f): by the observation that spawned it
    owner = {}; sightings = {}
    for t, who in enumerate(sc["seen"]):
        for i, w in enumerate(who):
            if w >= 0 and not sc["mapped"][w]:
                sightings[w] = sightings.get(w, 0) + 1
            cid = int(rp["cand_id"][t][i])
            if sc["in_idx"][t][i] >= 0:
                assert cid == -1
                continue
            assert cid >= 0, (t, i, "an unexplained observation neither fused nor spawned")
            assert owner.setdefault(cid, int(w)) == int(w), (t, i, "a candidate fused with another cone's observation")
    assert len(set(owner.values())) == len(owner), "two candidates for one cone"
    final = {int(r["id"]): r for r in rp["table"] if r["state"] != cr.FREE}
    confirmed = {owner[i] for i, r in final.items() if r["state"] == cr.CONFIRMED}
    want = {w for w, n in sightings.items() if n >= cp["confirm_hits"]}
    assert want and want <= confirmed, ("an unmapped cone seen %d times or more is not confirmed" % cp["confirm_hits"], sorted(want - confirmed))
    assert all(w >= 0 for w in confirmed), "a false detection was confirmed"
    for i, r in final.items():
        if r["state"] == cr.CONFIRMED:
            d = r["xy"] - sc["truth_xy"][owner[i]]; Cm = r["cov"].reshape(2, 2)
            assert d @ np.linalg.solve(Cm, d) < prm["gate_chi2"], (owner[i], "a confirmed cone is outside the gate of the truth under its own covariance")
    for t0, f in sc["false_at"].items():
        cid = [c for c, w in owner.items() if w == -1 - f]; assert len(cid) == 1
        alive = [any(int(r["id"]) == cid[0] for r in tab if r["state"] != cr.FREE) for tab in rp["tables"]]
        assert alive[t0:t0 + cp["max_misses"]] == [True] * cp["max_misses"] and not any(alive[t0 + cp["max_misses"]:]), (f, alive)
        assert rp["steps"][t0 + cp["max_misses"]]["n_retired"] >= 1
    print("\ntruth scene: %d unmapped cones confirmed, %d tentative at the end, smallest decision margin %.3g" % (
        len(confirmed), sum(r["state"] == cr.TENTATIVE for r in final.values()), min(rp["margins"])))


def test_truth_scene_is_not_rejected():
    _as_device(cs.scene("truth"))


def test_defaults_struct_sizes_and_symbols(pkg):
    b = pkg.binding; p = b.cand_params()
    assert (p.struct_size, p.confirm_hits, p.max_misses, p.spawn_range, p.view_range, p.view_cos) == (40, 3, 3, 67.0, 12.0, 0.5)
    assert C.sizeof(b.CandParams) == 40 and tuple(cr.DEFAULTS.values()) == (3, 3, 67.0, 12.0, 0.5)
    assert b.CAND.itemsize == 80 and b.CAND_STEP.itemsize == 48 and b.CAND == cr.CAND and b.CAND_MAX == 1024 == cr.CAND_MAX
    hdr = open(os.path.join(ROOT, "include", "graphslam.h")).read()
    assert "#define GS_CAND_MAX 1024" in hdr
    L = b.lib()
    for name in ("gs_cand_params_default", "gs_cand_batch", "gs_cand_resident", "gs_cand_clear", "gs_cand_set", "gs_cand_get", "gs_cand_take_confirmed",
                 "gs_frame_frontend_candidates", "gs_debug_time_cand_resident"):
        assert hasattr(L, name) and name in b.declared_symbols(), name
    assert L.gs_cand_params_default(None) == -1                              # GS_ERR_INVALID


def test_refusals_and_no_device(pkg):
    """every refusal comes before the device is touched: a host-only handle sees GS_ERR_INVALID for each and GS_ERR_NO_DEVICE for a good call"""
    b = pkg.binding; g = b.Graph(device=-2); sc = cs.scene("steps2"); INVALID, NO_DEVICE = -1, -4

    def code(fn):
        try:
            fn()
        except b.GsError as e:
            return e.code
        return 0

    def batch(fs_=sc["frame_start"], obs=sc["obs"], prm=None, cp=None, table=None):
        return code(lambda: g.cand(sc["poses"], obs, fs_, None, None, table, prm, cp))
    bad = lambda p, **kw: [setattr(p, k, v) for k, v in kw.items()] and p
    assert batch() == NO_DEVICE
    assert batch(prm=bad(b.nn_params(), struct_size=8)) == INVALID and batch(cp=bad(b.cand_params(), struct_size=32)) == INVALID
    assert batch(prm=bad(b.nn_params(), gate_chi2=-1.0)) == INVALID
    for kw in (dict(confirm_hits=0), dict(max_misses=0), dict(spawn_range=0.0), dict(spawn_range=float("inf")), dict(view_range=-1.0), dict(view_range=float("nan")),
               dict(view_cos=1.0000001), dict(view_cos=-1.5), dict(view_cos=float("nan"))):
        assert batch(cp=bad(b.cand_params(), **kw)) == INVALID, kw
    assert batch(cp=b.cand_params(view_cos=-1.0, confirm_hits=1, max_misses=1)) == NO_DEVICE and batch(cp=b.cand_params(view_cos=1.0)) == NO_DEVICE
    assert batch(fs_=np.array([0, 9, 8], dtype=np.int32)) == INVALID and batch(fs_=np.array([1, 8, 16], dtype=np.int32)) == INVALID
    big = np.tile(sc["obs"][:1], (258, 1))
    assert batch(obs=big, fs_=np.array([0, 257, 258], dtype=np.int32)) == INVALID
    rec = np.array([cr.record((1.0, 2.0))]); rec["state"] = 3
    assert batch(table=rec) == INVALID and code(lambda: g.cand_set(rec)) == INVALID
    rec["state"] = 1
    assert batch(table=rec) == NO_DEVICE and code(lambda: g.cand_set(rec)) == NO_DEVICE
    L = b.lib(); too_many = np.zeros(1025, dtype=b.CAND)
    assert L.gs_cand_set(g.h, 1025, too_many.ctypes.data_as(C.c_void_p)) == INVALID and L.gs_cand_set(g.h, 1, None) == INVALID
    assert code(g.cand_clear) == NO_DEVICE and code(g.cand_get) == NO_DEVICE and code(g.cand_take_confirmed) == NO_DEVICE
    assert code(lambda: g.frame_frontend_candidates(cs.POSE0, sc["frames"][0])) == NO_DEVICE
    assert code(lambda: g.frame_frontend_candidates(cs.POSE0, np.tile(sc["obs"][:1], (257, 1)))) == INVALID
    assert code(lambda: g.frame_frontend_candidates(cs.POSE0, sc["frames"][0], cand=bad(b.cand_params(), max_misses=0))) == INVALID
    prm, cp = b.nn_params(), b.cand_params()
    res = lambda obs, fs_, cap, poses, c, n_in=0, tab=None: L.gs_cand_resident(g.h, 2, 16, obs, fs_, cap, poses, None, None, n_in, tab, C.byref(prm), C.byref(c),
                                                                               None, None, None, None, None)
    assert res(64, 64, 8, 64, cp) == NO_DEVICE and res(72, 64, 8, 64, cp) == INVALID and res(64, 64, 257, 64, cp) == INVALID and res(64, None, 8, 64, cp) == INVALID
    assert res(64, 64, 8, None, cp) == INVALID and res(64, 64, 8, 64, cp, 1025, 64) == INVALID and res(64, 64, 8, 64, cp, 1, None) == INVALID
    assert res(64, 64, 8, 64, bad(b.cand_params(), confirm_hits=-1)) == INVALID
    n = C.c_int32(0)
    assert L.gs_cand_take_confirmed(g.h, -1, None, C.byref(n)) == INVALID and L.gs_cand_take_confirmed(g.h, 4, None, C.byref(n)) == INVALID
    g.close()


def test_the_checker_has_teeth():
    sc = cs.scene("cov_full"); prm = cs.nn_params_of(sc); cp = sc["cand"]
    rp = cr.replay(sc["records"], sc["poses"], sc["pose_covs"], sc["frames"], sc["in_idx"], prm, cp, sc["lidar"])
    t = 1; before = rp["tables"][0]; meta = [6, 1, 6]
    slot, na, _, _ = cr.associate64(before, sc["poses"][t], sc["pose_covs"][t], sc["frames"][t], None, prm, sc["lidar"], [])
    chk = cr.StepCheck(before, meta, sc["frames"][t], None, sc["poses"][t], sc["pose_covs"][t], slot, na, prm, cp, sc["lidar"])
    good = (rp["tables"][t], chk.meta, rp["steps"][t], rp["cand_id"][t], rp["cand_slot"][t])
    assert chk.failures(*good) == [] and chk.rec["n_fused"] == 6
    for field, e in (("xy", 0), ("xy", 1), ("cov", 0), ("cov", 3)):                      # a value off by a few parts in 1e12: far outside B
        tab = good[0].copy(); tab[field][2, e] *= 1.0 + 4e-12
        assert chk.failures(tab, *good[1:]), (field, e)
    tab = good[0].copy(); tab["cov"][2, 1] = np.nextafter(tab["cov"][2, 1], 1.0)          # cov[1] != cov[2]
    assert chk.failures(tab, *good[1:])
    tab = good[0].copy(); tab["xy"][700, 0] = 1.0                                         # a slot nothing touched
    assert chk.failures(tab, *good[1:])
    for key in cr.INT_KEYS:
        tab = good[0].copy(); tab[key][3] += 1
        assert chk.failures(tab, *good[1:]), key
    for key in cr.STEP_KEYS:
        rec = dict(good[2]); rec[key] += 1
        assert chk.failures(good[0], good[1], rec, good[3], good[4]), key
    ids = good[3].copy(); ids[0] += 1
    assert chk.failures(good[0], good[1], good[2], ids, good[4])
    sl = good[4].copy(); sl[5] = -1
    assert chk.failures(good[0], good[1], good[2], good[3], sl)
    assert chk.failures(good[0], [chk.meta[0] + 1] + chk.meta[1:], *good[2:])
    # a decision inside its band is rejected, not decided: a slot exactly on the view's range, and one exactly on its cone
    for z, kw in (([12.0, 0.0], {}), ([3.0, 4.0], dict(view_cos=0.6))):
        pose = np.zeros(3); tabz, metaz = cr.load([cr.record(z)])
        with pytest.raises(cr.Rejected):
            cr.StepCheck(tabz, metaz, np.zeros((0, 4)), None, pose, None, [], [], prm, cr.params_of(**kw), sc["lidar"])
    tabz, metaz = cr.load([cr.record([-5.0, 0.0])])                                        # all-round: exactly behind is visible, and decided
    assert cr.StepCheck(tabz, metaz, np.zeros((0, 4)), None, np.zeros(3), None, [], [], prm, cr.params_of(view_cos=-1.0), sc["lidar"]).rec["n_missed"] == 1


def test_layout_helper_under_address_and_undefined_sanitizers(tmp_path):
    """tests/cand_layout_san.cpp: a stand-alone program (its own main, no HIP, nothing loaded into python) around csrc/gs_cand_host.hpp"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "cand_layout_san")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "opendlv-logic-cfsd18-sensation-slam_amd", "csrc"), os.path.join(ROOT, "tests", "cand_layout_san.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "cand layout: ok" in out.stdout, out.stdout + out.stderr
