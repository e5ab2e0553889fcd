"""CPU tests of frame following: the reference's own prediction against a 40-digit evaluation and against finite differences of the motion
model, the update and duplicate rules on hand-made records, the float64 replay of the truth scene (the margins the GPU test rests on), every
refusal of the new calls and GS_ERR_NO_DEVICE on a host-only handle, the defaults and struct sizes, the checkers' teeth, and the host layout
helper under AddressSanitizer / UndefinedBehaviorSanitizer as a stand-alone program."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import follow_ref as fr
import follow_shapes as fs
import relocalize_shapes as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
mp = fr.MP


def _cases():
    rng = np.random.default_rng(2)
    out = [(np.array([35.0, 29.0, 3.1]), fs.COV0, np.array([5.0, 0.2, 0.1]), fs.QU_FULL), (np.array([-3.0, 2.0, fr.PI]), fs.COV0, np.array([0.0, 0.0, 0.0]), None),
           (np.array([1.0, 1.0, -3.1]), np.zeros(9), np.array([1.0, -2.0, -0.2]), fs.QU_DIAG)]
    for _ in range(20):
        A = rng.normal(size=(3, 3)); P = (A @ A.T * 0.01).reshape(9); B = rng.normal(size=(3, 3)); Q = (B @ B.T * 1e-3).reshape(9)
        out.append((rng.uniform(-50, 50, 3) * [1, 1, 0.06], P, rng.normal(0, 3, 3) * [1, 1, 0.1], Q))
    return out


def test_prediction_against_forty_digits():
    """predict64 (float64, the header's order) lands inside the bound predict_exact derives around a 40-digit evaluation written independently
    of it (matrix products, not the header's lines); theta- is g2o's normalisation of the float64 sum"""
    worst = 0.0
    with mp.workdps(40):
        for pose, P, u, Q in _cases():
            p64, c64 = fr.predict64(pose, P, u, Q)
            xm, ym, th, S = fr.predict_exact(pose, P, u, Q)
            t = mp.mpf(float(pose[2])); c, s = mp.cos(t), mp.sin(t)
            p = c * mp.mpf(float(u[0])) - s * mp.mpf(float(u[1])); q = s * mp.mpf(float(u[0])) + c * mp.mpf(float(u[1]))
            F = mp.matrix([[1, 0, -q], [0, 1, p], [0, 0, 1]]); W = mp.matrix([[c, -s, 0], [s, c, 0], [0, 0, 1]])
            Pm = mp.matrix(3, 3); Qm = mp.matrix(3, 3); Pf = fr.mirror(P); Qf = np.zeros(9) if Q is None else fr.mirror(Q)
            for r in range(3):
                for k in range(3):
                    Pm[r, k] = mp.mpf(float(Pf[3 * r + k])); Qm[r, k] = mp.mpf(float(Qf[3 * r + k]))
            Sm = F * Pm * F.T + W * Qm * W.T
            exact = [mp.mpf(float(pose[0])) + p, mp.mpf(float(pose[1])) + q] + [Sm[r, k] for r, k in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
            for ref, ex, got in zip([xm, ym] + S, exact, [p64[0], p64[1]] + [c64[e] for e in fr.UP]):
                assert abs(ref.v - ex) <= mp.mpf(2) ** -100 * (1 + abs(ex)), "the E arithmetic's value is not the exact one"
                ok, ratio = fr.inside(got, ref); worst = max(worst, ratio)
                assert ok, (pose, got, float(ref.v), ratio)
            assert c64.reshape(3, 3).tobytes() == c64.reshape(3, 3).T.copy().tobytes()
            want = float(pose[2]) + float(u[2]); assert -fr.PI <= th < fr.PI and abs(np.sin(th) - np.sin(want)) < 1e-12 and abs(np.cos(th) - np.cos(want)) < 1e-12
    assert 0.0 < worst < 1.0
    assert fr.normalize(fr.PI) == -fr.PI and fr.normalize(3.1 + 0.1) == (3.1 + 0.1) - 2.0 * fr.PI and fr.normalize(-fr.PI) == -fr.PI


def test_prediction_covariance_against_finite_differences():
    def f(x, u):
        c, s = np.cos(x[2]), np.sin(x[2])
        return np.array([x[0] + c * u[0] - s * u[1], x[1] + s * u[0] + c * u[1], x[2] + u[2]])
    for pose, P, u, Q in _cases():
        h = 1e-6; Jx = np.zeros((3, 3)); Ju = np.zeros((3, 3))
        for k in range(3):
            e = np.zeros(3); e[k] = h
            Jx[:, k] = (f(pose + e, u) - f(pose - e, u)) / (2 * h); Ju[:, k] = (f(pose, u + e) - f(pose, u - e)) / (2 * h)
        want = Jx @ fr.mirror(P).reshape(3, 3) @ Jx.T + (0 if Q is None else Ju @ fr.mirror(Q).reshape(3, 3) @ Ju.T)
        got = fr.predict64(pose, P, u, Q)[1].reshape(3, 3)
        assert np.allclose(got, want, rtol=1e-6, atol=1e-9 * (1 + np.abs(want).max()))


GATE = np.concatenate([[0.0], 6.0 + 2.5 * np.arange(256)])


def _chain(pose, chi2=1.0, n_pairs=5, status=0):
    return dict(pose=np.array(pose, dtype=np.float64), cov=np.full(9, 0.25), chi2=chi2, n_pairs=n_pairs, iterations=2, status=status, n_kept=n_pairs)


def test_update_rules_on_hand_made_records():
    fp = fr.params_of(max_misses=2)
    st = fr.new_state([[0, 0, 0], [10, 0, 0], [20, 0, 0], [30, 0, 0]])
    pri = {h: (st["pose"][h] + [1.0, 0, 0], np.full(9, 0.5)) for h in range(4)}
    # 0 accepted; 1 above its gate; 2 too few pairs; 3 status 2
    ch = {0: _chain([1.1, 0, 0]), 1: _chain([11, 0, 0], chi2=GATE[5] * 1.0000001), 2: _chain([21, 0, 0], n_pairs=2), 3: _chain([31, 0, 0], status=2)}
    recs, best, nt = fr.update(st, 0, pri, ch, GATE, fp)
    assert [r["accepted"] for r in recs] == [1, 0, 0, 0] and best == 0 and nt == 4
    assert st["pose"][0].tolist() == [1.1, 0, 0] and st["pose"][1].tolist() == [11.0, 0, 0] and st["cov"][1].tolist() == [0.5] * 9      # dead reckoning
    assert st["hits"].tolist() == [5, 0, 0, 0] and st["misses"].tolist() == [0, 1, 1, 1] and st["frames_missed"].tolist() == [0, 1, 1, 1]
    # chi2 exactly AT the gate is accepted, a NaN is not; the run counter goes back to 0 on a hit, the second miss in a row loses
    pri = {h: (st["pose"][h].copy(), st["cov"][h].copy()) for h in range(4)}
    ch = {0: _chain(st["pose"][0], chi2=np.nan), 1: _chain(st["pose"][1], chi2=GATE[5]), 2: _chain(st["pose"][2], n_pairs=2), 3: _chain(st["pose"][3], status=1, n_pairs=3)}
    recs, best, nt = fr.update(st, 1, pri, ch, GATE, fp)
    assert [r["accepted"] for r in recs] == [0, 1, 0, 1] and st["misses"].tolist() == [1, 0, 2, 0]
    assert st["state"].tolist() == [0, 0, 1, 0] and st["state_step"].tolist() == [-1, -1, 1, -1] and nt == 3
    assert best == 0 and st["hits"].tolist() == [5, 5, 0, 3]                   # hits tie between 0 and 1: the smaller sum_chi2 (1.0 < the gate)
    # latched: the lost one is frozen whatever the chain says, and its record is the frozen pose with status -1
    frozen = st["pose"][2].copy()
    pri = {h: (st["pose"][h].copy(), st["cov"][h].copy()) for h in (0, 1, 3)}
    ch = {h: _chain(st["pose"][h]) for h in (0, 1, 3)}
    recs, best, nt = fr.update(st, 2, pri, ch, GATE, fp)
    assert recs[2]["status"] == -1 and recs[2]["accepted"] == 0 and recs[2]["state"] == 1 and recs[2]["pose"].tolist() == frozen.tolist()
    assert st["state_step"][2] == 1 and st["frames_missed"][2] == 2
    assert best == 0 and st["hits"].tolist() == [10, 10, 0, 8]                  # still the tie; 0 has 1.0 + 1.0, 1 has the gate + 1.0


def test_the_sequential_merge():
    fp = fr.params_of()
    for poses, want_state, want_of in (([[0, 0, 0], [0.3, 0, 0], [0.6, 0, 0]], [0, 2, 0], [-1, 0, -1]),          # 2 is near 1 only, and 1 is gone
                                       ([[0, 0, 0], [0.6, 0, 0], [0.3, 0, 0]], [0, 0, 2], [-1, -1, 0]),          # 2 is near both: the smallest d
                                       ([[0, 0, 3.1], [0.1, 0, -3.1], [0.1, 0, 2.9]], [0, 2, 0], [-1, 0, -1]),   # the angle wraps; 0.2 rad is too far
                                       ([[0, 0, 0], [0.5, 0, 0], [np.nan, 0, 0]], [0, 0, 0], [-1, -1, -1])):     # at the radius is not inside; NaN is near nobody
        st = fr.new_state(poses); pri = {h: (st["pose"][h].copy(), st["cov"][h].copy()) for h in range(3)}
        recs, best, nt = fr.update(st, 4, pri, {h: fr.empty_record(*pri[h]) for h in range(3)}, GATE, fp)
        assert st["state"].tolist() == want_state and st["duplicate_of"].tolist() == want_of, poses
        assert [int(s) for s in st["state_step"]] == [4 if w == 2 else -1 for w in want_state] and [r["state"] for r in recs] == want_state
    st = fr.new_state([[0, 0, 0], [0, 0, 0]]); pri = {h: (st["pose"][h].copy(), st["cov"][h].copy()) for h in range(2)}
    fr.update(st, 0, pri, {h: fr.empty_record(*pri[h]) for h in range(2)}, GATE, fr.params_of(merge_xy=0.0))
    assert st["state"].tolist() == [0, 0], "merge_xy = 0 switches the pass off"


def test_the_checkers_have_teeth():
    st = fr.new_state([[1, 2, 0.5]]); pri = {0: (st["pose"][0].copy(), np.full(9, 0.5))}
    recs, _, _ = fr.update(st, 0, pri, {0: _chain([1.1, 2, 0.5])}, GATE, fr.params_of())
    good = dict(recs[0]); assert fr.mismatches(good, recs[0]) == []
    for key in fr.REC_F:
        bad = dict(good); v = np.array(bad[key], dtype=np.float64).reshape(-1).copy(); v.view(np.int64)[-1] ^= 1; bad[key] = v
        assert fr.mismatches(bad, recs[0]) == [key], key
    for key in fr.REC_I:
        bad = dict(good); bad[key] = good[key] + 1
        assert fr.mismatches(bad, recs[0]) == [key], key
    xm, ym, _, S = fr.predict_exact([35.0, 29.0, 0.7], fs.COV0, [5.0, 0.2, 0.1], fs.QU_FULL)
    for ref in [xm, ym] + S:
        assert fr.inside(float(ref.v), ref)[0] and not fr.inside(float(ref.v + 3 * 2 * ref.e + abs(ref.v) * 2.0 ** -50), ref)[0]


def _replay(sc, gate):
    prm = dict(fr.nr.DEFAULTS); prm.update(sc["params"]); prm["lidar"] = sc["lidar"]
    loc = dict(max_iterations=5, tol_xy=1e-6, tol_theta=1e-8); loc.update(sc["loc"])
    return fr.replay(sc["poses"], sc["covs"], sc["frames"], sc["motion"], sc["motion_cov"], sc["map_xy"], sc["map_ty"], sc["map_cov"], prm, gate, loc,
                     fr.params_of(**sc["follow"]))


def test_replay_of_the_truth_scene(pkg):
    """the margins the GPU test rests on: the true hypothesis stays below HALF its gate in every step, the far one has NO admissible pair
    at all — neither can be decided by rounding.  What the one-spacing-off hypothesis does is printed, not asserted."""
    sc = fs.scene("truth"); gate = np.array(pkg.binding.jc_params().gate[:])
    steps, st, best, nt = _replay(sc, gate); cl = rs.track()[2]
    assert best == 0 and all(steps[t][0]["accepted"] == 1 for t in range(12)) and st["state"][0] == fr.TRACKING
    assert all(steps[t][0]["n_pairs"] >= 8 and steps[t][0]["chi2"] < 0.5 * gate[steps[t][0]["n_pairs"]] for t in range(12))
    assert np.hypot(*(st["pose"][0, :2] - cl[fs.AT + 11, :2])) < 0.05 and abs(fr.normalize(st["pose"][0, 2] - cl[fs.AT + 11, 2])) < 0.01
    assert st["state"][2] == fr.LOST and st["state_step"][2] == fr.DEFAULTS["max_misses"] - 1 and st["hits"][2] == 0
    assert all(np.all(np.isinf(steps[t][2]["d2"])) for t in range(3)), "the far hypothesis must have no admissible pair at all"
    print("\none spacing off: state %d at step %d; accepted %s; chi2 / gate %s" % (
        st["state"][1], st["state_step"][1], [steps[t][1]["accepted"] for t in range(12)],
        [round(steps[t][1]["chi2"] / gate[steps[t][1]["n_pairs"]], 2) if steps[t][1]["n_pairs"] else None for t in range(12)]))


@pytest.mark.parametrize("name", ["row3", "same_pose", "lost_frozen", "miss_hit", "min_pairs_high"])
def test_replay_of_the_scenes_built_for_one_thing(pkg, name):
    sc = fs.scene(name); steps, st, best, nt = _replay(sc, np.array(pkg.binding.jc_params().gate[:]))
    for key, want in sc["expect"].items():
        assert [int(v) for v in st[key]] == want, (name, key, st[key])
    if name == "lost_frozen":
        assert [steps[t][0]["status"] for t in range(5)] == [2, 2, 2, -1, -1] and best == -1 and nt == 0
    if name == "miss_hit":
        assert [steps[t][0]["accepted"] for t in range(3)] == [1, 0, 1]


def test_defaults_and_struct_sizes(pkg):
    b = pkg.binding; p = b.follow_params()
    assert (p.struct_size, p.min_pairs, p.max_misses, p.merge_xy, p.merge_theta) == (32, 3, 3, 0.5, 0.1) == (C.sizeof(b.FollowParams),) + tuple(fr.DEFAULTS.values())
    assert b.FOLLOW_STATE.itemsize == 136 and b.FOLLOW_STEP.itemsize == 224 and b.FOLLOW_HYP_MAX == 64
    hdr = open(os.path.join(ROOT, "include", "graphslam.h")).read()
    assert "#define GS_FOLLOW_HYP_MAX 64" in hdr
    assert b.lib().gs_follow_params_default(None) == -1                     # GS_ERR_INVALID


def test_refusals_and_no_device(pkg):
    """every refusal comes before the device is touched: a host-only handle sees GS_ERR_INVALID for each and GS_ERR_NO_DEVICE for a good call"""
    b = pkg.binding; g = b.Graph(device=-2); sc = fs.scene("h2_s2"); INVALID, NO_DEVICE = -1, -4

    def code(fn):
        try:
            fn()
        except b.GsError as e:
            return e.code
        return 0

    def batch(poses=sc["poses"], fs_=sc["frame_start"], obs=sc["obs"], prm=None, jc=None, loc=None, fp=None):
        return code(lambda: g.follow(poses, obs, fs_, sc["motion"], sc["map_xy"], sc["map_ty"], None, None, None, prm, jc, loc, fp))
    assert batch() == NO_DEVICE
    bad = lambda p, **kw: [setattr(p, k, v) for k, v in kw.items()] and p
    assert batch(prm=bad(b.nn_params(), struct_size=8)) == INVALID and batch(jc=bad(b.jc_params(), struct_size=8)) == INVALID
    assert batch(loc=bad(b.loc_params(), struct_size=8)) == INVALID and batch(fp=bad(b.follow_params(), struct_size=24)) == INVALID
    assert batch(loc=bad(b.loc_params(), max_iterations=0)) == INVALID and batch(prm=bad(b.nn_params(), gate_chi2=-1.0)) == INVALID
    for kw in (dict(min_pairs=0), dict(max_misses=0), dict(merge_xy=-0.5), dict(merge_theta=-1e-9), dict(merge_xy=float("nan")), dict(merge_theta=float("inf"))):
        assert batch(fp=bad(b.follow_params(), **kw)) == INVALID, kw
    assert batch(fp=b.follow_params(merge_xy=0.0, merge_theta=0.0)) == NO_DEVICE, "merge values of 0 are legal"
    assert batch(poses=np.zeros((65, 3))) == INVALID and batch(poses=np.zeros((0, 3))) == INVALID
    assert batch(fs_=np.array([0, 9, 8], dtype=np.int32)) == INVALID and batch(fs_=np.array([1, 8, 13], dtype=np.int32)) == INVALID
    assert batch(fs_=np.array([0, 8, 12], dtype=np.int32)) == INVALID
    big = np.tile(sc["obs"][:1], (258, 1))
    assert batch(obs=big, fs_=np.array([0, 257, 258], dtype=np.int32)) == INVALID
    assert code(lambda: g.follow_set(sc["poses"])) == NO_DEVICE and code(lambda: g.follow_set(np.zeros((65, 3)))) == INVALID
    assert code(lambda: g.follow_get()) == NO_DEVICE
    assert code(lambda: g.frame_frontend_follow(sc["frames"][0])) == NO_DEVICE
    assert code(lambda: g.frame_frontend_follow(np.tile(sc["obs"][:1], (257, 1)))) == INVALID
    assert code(lambda: g.frame_frontend_follow(sc["frames"][0], follow=bad(b.follow_params(), min_pairs=0))) == INVALID
    L = b.lib(); prm, jc, loc, fp = b.nn_params(), b.jc_params(), b.loc_params(), b.follow_params()
    res = lambda poses, obs, cap, f: L.gs_follow_resident(g.h, 2, poses, None, 2, 13, obs, 64, cap, 64, None, C.byref(prm), C.byref(jc), C.byref(loc), C.byref(f), None, None, None, None)
    assert res(64, 64, 8, fp) == NO_DEVICE and res(64, 72, 8, fp) == INVALID and res(64, 64, 257, fp) == INVALID and res(None, 64, 8, fp) == INVALID
    assert res(64, 64, 8, bad(b.follow_params(), max_misses=-1)) == INVALID
    g.close()


def test_layout_helper_under_address_and_undefined_sanitizers(tmp_path):
    """tests/follow_layout_san.cpp: a stand-alone program (its own main, no HIP, nothing loaded into python) around csrc/gs_follow_host.hpp"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "follow_layout_san")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "opendlv-logic-cfsd18-sensation-slam_amd", "csrc"), os.path.join(ROOT, "tests", "follow_layout_san.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "follow layout: ok" in out.stdout, out.stdout + out.stderr
