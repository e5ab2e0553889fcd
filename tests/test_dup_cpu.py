"""CPU tests of the map twins: the fusion's algebra in 40 digits, the float64 replay of every scene inside the reference's bounds with no scene
rejected, the truth scene's facts, the remap's properties, every refusal of the new calls and GS_ERR_NO_DEVICE on a host-only handle, the
defaults, struct sizes and exported symbols, the checker's teeth, gs_merge_landmarks on a host-only handle against a fresh handle built with
the merged insertions, and the host helpers under AddressSanitizer / UndefinedBehaviorSanitizer as a stand-alone program."""
import ctypes as C
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import dup_ref as dr
import dup_shapes as ds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("opendlv-logic-cfsd18-sensation-slam_amd")
B = pkg.binding
mp = dr.MP
GS_OK, GS_ERR_INVALID, GS_ERR_UNKNOWN_ID, GS_ERR_NO_DEVICE = 0, -1, -3, -4      # include/graphslam.h


@pytest.fixture(scope="module", autouse=True)
def _library(pkg):
    """the session's package fixture builds the native library where it is missing"""
    return pkg


@pytest.fixture(scope="module")
def host():
    g = pkg.Graph(device=-2)
    yield g
    g.close()


def _spd(rng, scale):
    a = rng.normal(size=(2, 2))
    return a @ a.T * scale + np.eye(2) * scale * 0.1


def test_fusion_algebra_in_forty_digits():
    """K B with K = A S^-1 (the form the kernel runs) is the parallel sum (A^-1 + B^-1)^-1, and l_a + K (l_b - l_a) the information-weighted
    mean, in 40-digit arithmetic; the float64 replay's fused values sit within 1e-9 of them for well-conditioned blocks"""
    rng = np.random.default_rng(31)
    with mp.workdps(40):
        for _ in range(30):
            An, Bn = _spd(rng, 10.0 ** rng.uniform(-4, 0)), _spd(rng, 10.0 ** rng.uniform(-4, 0)); la = rng.normal(0, 20, 2); lb = la + rng.normal(0, 0.05, 2)
            An[1, 0] = An[0, 1]; Bn[1, 0] = Bn[0, 1]
            Am, Bm = mp.matrix(An.tolist()), mp.matrix(Bn.tolist()); lam, lbm = mp.matrix(la.tolist()), mp.matrix(lb.tolist())
            K = Am * (Am + Bm) ** -1
            KB, par = K * Bm, (Am ** -1 + Bm ** -1) ** -1
            scale = max(abs(KB[r, c]) for r in range(2) for c in range(2))
            assert all(abs(KB[r, c] - par[r, c]) <= mp.mpf(10) ** -30 * scale for r in range(2) for c in range(2))
            lp = lam + K * (lbm - lam); li = par * (Am ** -1 * lam + Bm ** -1 * lbm)
            assert all(abs(lp[r] - li[r]) <= mp.mpf(10) ** -28 * (1 + abs(lp[r])) for r in range(2))
            rp = dr.replay([la, lb], [1, 1], [An.reshape(4), Bn.reshape(4)], dict(ds.DEFAULTS, sigma_floor=0.0, gate_chi2=1e30))
            assert rp["info"]["n_pairs"] == 1
            for got, want in ((rp["xy"][0, 0], lp[0]), (rp["xy"][0, 1], lp[1]), (rp["cov"][0, 0], KB[0, 0]), (rp["cov"][0, 1], KB[0, 1]), (rp["cov"][0, 3], KB[1, 1])):
                assert abs(mp.mpf(float(got)) - want) <= 1e-9 * (abs(want) + scale)


def test_two_cones_of_zero_covariance_fuse_to_half_the_floor():
    rp = dr.replay([[1.0, 2.0], [1.0625, 2.0]], [1, 1], np.zeros((2, 4)), ds.DEFAULTS)
    s2 = 0.05 * 0.05
    assert rp["info"] == dict(n_in=2, n_out=1, n_pairs=1, n_ambiguous=0)
    assert np.allclose(rp["cov"][0], [s2 / 2, 0, 0, s2 / 2], rtol=1e-15, atol=0) and np.allclose(rp["xy"][0], [1.03125, 2.0], rtol=1e-15)


@pytest.fixture(scope="module")
def refs():
    """the exact reference of every scene, made once (a Rejected scene raises here)"""
    return {name: dr.make(ds.scene(name), ds.params_of(ds.scene(name))) for name in ds.NAMES}


@pytest.mark.parametrize("name", ds.NAMES)
def test_no_scene_is_rejected_and_the_float64_replay_stays_inside_the_bounds(name, refs):
    sc = ds.scene(name); ref = refs[name]
    rp = dr.replay(sc["xy"], sc["ty"], sc["cov"], ds.params_of(sc))
    bad = ref.twins_failures(rp["twin"], rp["d2"], rp["second"], rp["nadm"]) + ref.merge_failures(rp["xy"], rp["ty"], rp["cov"], rp["remap"], rp["info"])
    assert not bad, (name, bad[:3])
    assert ref.worst < 1.0
    if ref.info["n_pairs"] and name not in ("type_ignored",):
        assert ref.worst > 0.0                                                 # the bound is not vacuous
    assert sorted(rp["pairs"]) == sorted(ref.twin_pairs)


def test_the_scenes_hold_what_they_are_named_for(refs):
    n = lambda name: refs[name].info
    assert refs["straddle"].twin_pairs == [(255, 256)] and refs["ends"].twin_pairs == [(0, 599)]
    assert refs["triplet"].twin_pairs == [(7, 21)] and refs["triplet"].twin[30] == 21 and refs["triplet"].nadm[21] == 2
    t = refs["tie"]
    assert t.nadm[3] == 2 and t.twin[3] == 5 and t.d2[3][0] == t.second[3][0] and t.twin_pairs == [(3, 5)] and t.info["n_ambiguous"] == 1
    assert refs["tie_exclusive"].twin_pairs == [] and refs["tie_exclusive"].nadm[3] == 2
    assert n("type_mismatch")["n_pairs"] == 0 and refs["type_ignored"].twin_pairs == [(2, 11)] and refs["type_ignored"].d2[2][0] == 0
    for name in ("gate_not_distance", "distance_not_gate", "zero_floor_zero_cov"):
        assert n(name)["n_pairs"] == 0 and not refs[name].nadm.any(), name
    assert refs["gate_not_distance"].n_values == 0 and refs["distance_not_gate"].n_values == 1
    assert refs["nan_between"].twin_pairs == [(4, 6)] and refs["nan_between"].twin[5] == -1
    assert n("zero_cov")["n_pairs"] > 0 and n("no_cov")["n_pairs"] > 0 and n("anisotropic")["n_pairs"] > 0
    assert n("all_paired") == dict(n_in=512, n_out=256, n_pairs=256, n_ambiguous=0)
    for size in ds.SIZES:
        assert n("n%d" % size)["n_in"] == size and (size < 2 or n("n%d" % size)["n_pairs"] > 0)


def test_the_triplet_needs_two_rounds_in_float64():
    sc = ds.scene("triplet"); p = ds.params_of(sc)
    r1 = dr.replay(sc["xy"], sc["ty"], sc["cov"], p); r2 = dr.replay(r1["xy"], r1["ty"], r1["cov"], p); r3 = dr.replay(r2["xy"], r2["ty"], r2["cov"], p)
    assert (r1["info"]["n_pairs"], r2["info"]["n_pairs"], r3["info"]["n_pairs"]) == (1, 1, 0) and r3["info"]["n_out"] == 38


def test_truth_scene_facts(refs):
    """the rule finds exactly the 40 planted pairs, no cone has more than one admissible neighbour, the largest planted d2 is 4.668 (1.32 inside
    the gate), and the track's smallest same-type spacing, 1.57 m, is above max_distance"""
    sc, planted = ds.truth(); ref = refs["truth"]
    assert ref.twin_pairs == planted and ref.info == dict(n_in=160, n_out=120, n_pairs=40, n_ambiguous=0)
    assert ref.nadm.max() == 1
    worst = max(float(ref.d2[a][0]) for a, _ in planted)
    assert abs(worst - 4.668) < 5e-4 and abs((ds.DEFAULTS["gate_chi2"] - worst) - 1.32) < 5e-3
    xy, ty = sc["xy"][:120], sc["ty"][:120]
    d = np.hypot(xy[:, None, 0] - xy[None, :, 0], xy[:, None, 1] - xy[None, :, 1]); d[ty[:, None] != ty[None, :]] = np.inf; np.fill_diagonal(d, np.inf)
    assert abs(d.min() - 1.57) < 5e-3 and d.min() > ds.DEFAULTS["max_distance"]


@pytest.mark.parametrize("name", ds.NAMES)
def test_remap_properties(name, refs):
    ref = refs[name]; rm = ref.remap; dropped = {b for _, b in ref.twin_pairs}
    kept = [i for i in range(ref.n) if i not in dropped]
    assert list(rm[kept]) == list(range(len(kept)))                            # monotone, gap-free on the kept cones
    assert all(rm[b] == rm[a] and a < b for a, b in ref.twin_pairs)
    assert ref.info["n_out"] == ref.info["n_in"] - ref.info["n_pairs"] == len(kept)
    assert len({x for pr in ref.twin_pairs for x in pr}) == 2 * len(ref.twin_pairs)                # disjoint


# ---- the checker's teeth
def _replayed(name):
    sc = ds.scene(name)
    return dr.replay(sc["xy"], sc["ty"], sc["cov"], ds.params_of(sc))


def test_checker_catches_a_perturbed_fused_position(refs):
    ref = refs["straddle"]; rp = _replayed("straddle"); k = int(ref.remap[255])
    xy = rp["xy"].copy(); xy[k, 0] = np.nextafter(xy[k, 0], np.inf) + 1e-9
    assert ref.merge_failures(xy, rp["ty"], rp["cov"], rp["remap"], rp["info"])
    cv = rp["cov"].copy(); cv[k, 3] *= 1 + 1e-9
    assert ref.merge_failures(rp["xy"], rp["ty"], cv, rp["remap"], rp["info"])
    assert not ref.merge_failures(rp["xy"], rp["ty"], rp["cov"], rp["remap"], rp["info"])


def test_checker_catches_a_swapped_keeper(refs):
    """the same fusion with b as the keeper: the fused cone lands at b's place in the order, with b's remap"""
    ref = refs["ends"]; sc = ds.scene("ends"); rp = _replayed("ends")
    order = list(range(1, 600))                                                # cone 0 dropped, 599 kept
    xy = sc["xy"][order].copy(); ty = sc["ty"][order].copy(); cv = sc["cov"][order].copy()
    xy[-1] = rp["xy"][0]; cv[-1] = rp["cov"][0]
    rm = np.arange(-1, 599, dtype=np.int32); rm[0] = 598
    assert ref.merge_failures(xy, ty, cv, rm, rp["info"])


def test_checker_catches_a_wrong_remap_entry_a_wrong_twin_and_a_wrong_count(refs):
    ref = refs["n257"]; rp = _replayed("n257")
    rm = rp["remap"].copy(); rm[100] += 1
    assert ref.merge_failures(rp["xy"], rp["ty"], rp["cov"], rm, rp["info"])
    a, b = ref.twin_pairs[0]
    tw = rp["twin"].copy(); tw[a] = -1
    assert ref.twins_failures(tw, rp["d2"], rp["second"], rp["nadm"])
    d2 = rp["d2"].copy(); d2[a] *= 1 + 1e-9
    assert ref.twins_failures(rp["twin"], d2, rp["second"], rp["nadm"])
    na = rp["nadm"].copy(); na[b] += 1
    assert ref.twins_failures(rp["twin"], rp["d2"], rp["second"], na)
    info = dict(rp["info"], n_ambiguous=rp["info"]["n_ambiguous"] + 1)
    assert ref.merge_failures(rp["xy"], rp["ty"], rp["cov"], rp["remap"], info)


def test_reference_rejects_a_decision_inside_its_band():
    """a cone exactly max_distance from its partner, and two candidates with equal d2 that are no mirror images"""
    with pytest.raises(dr.Rejected):
        dr.Ref([[0.0, 0.0], [1.0, 0.0]], [1, 1], np.full((2, 4), [0.5, 0, 0, 0.5]), ds.DEFAULTS)
    with pytest.raises(dr.Rejected):
        dr.Ref([[0.0, 0.0], [0.25, 0.0], [0.0, 0.25]], [1, 1, 1], np.full((3, 4), [0.0072, 0, 0, 0.0072]), ds.DEFAULTS)


# ---- defaults, sizes, symbols, refusals
def test_defaults_struct_sizes_and_symbols():
    p = B.dup_params()
    assert C.sizeof(B.DupParams) == 40 == p.struct_size and B.DUP_INFO.itemsize == 16
    got = {k: getattr(p, k) for k in ds.DEFAULTS}
    assert got == ds.DEFAULTS and got["gate_chi2"] == B.nn_params().gate_chi2 and got["sigma_floor"] == B.nn_params().sigma_xy
    L = B.lib(); names = B.declared_symbols()
    for s in ("gs_dup_params_default", "gs_map_twins_batch", "gs_map_twins_resident", "gs_map_merge_twins_batch", "gs_map_merge_twins", "gs_map_get_xy",
              "gs_merge_landmarks", "gs_debug_time_map_twins_resident", "gs_debug_time_map_merge_twins"):
        assert s in names and hasattr(L, s), s
    hdr = open(os.path.join(ROOT, "include", "graphslam.h")).read()
    assert "#define GS_DUP_MAP_MAX %d" % B.DUP_MAP_MAX in hdr and B.DUP_MAP_MAX >= 65536
    assert L.gs_dup_params_default(None) == GS_ERR_INVALID
    with pytest.raises(AttributeError):
        B.dup_params(sigma=1.0)


def _rc(fn, *a):
    return fn(*a)


def test_every_refusal_comes_before_the_device(host):
    """on a host-only handle a bad argument is GS_ERR_INVALID and a good call GS_ERR_NO_DEVICE: the refusals are decided first"""
    L = B.lib(); h = host.h; INV, NODEV = GS_ERR_INVALID, GS_ERR_NO_DEVICE
    xy = np.zeros((4, 2)); ty = np.zeros(4, dtype=np.int32); cv = np.zeros((4, 4)); tw = np.zeros(4, dtype=np.int32); d = np.zeros(4)
    oxy = np.zeros((4, 2)); oty = np.zeros(4, dtype=np.int32); rm = np.zeros(4, dtype=np.int32); info = np.zeros(1, dtype=B.DUP_INFO)
    _d, _i = B._d, B._i
    good = B.dup_params()
    bad = []
    for k, v in (("struct_size", 39), ("gate_chi2", 0.0), ("gate_chi2", float("nan")), ("max_distance", -1.0), ("max_distance", float("inf")),
                 ("sigma_floor", -0.01), ("sigma_floor", float("nan")), ("require_same_type", 2), ("exclusive", -1)):
        p = B.dup_params(); setattr(p, k, v); bad.append(C.byref(p))
    calls = {
        "twins_batch": lambda p, n=4, x=xy, t=tw: L.gs_map_twins_batch(h, n, None if x is None else _d(x), _i(ty), _d(cv), p, None if t is None else _i(t), _d(d), None, None),
        "twins_resident": lambda p: L.gs_map_twins_resident(h, p, None, None, None, None),
        "merge_batch": lambda p, n=4, x=oxy: L.gs_map_merge_twins_batch(h, n, _d(xy), _i(ty), None, p, None if x is None else _d(x), _i(oty), None, _i(rm),
                                                                        info.ctypes.data_as(C.c_void_p)),
        "merge": lambda p: L.gs_map_merge_twins(h, p, 4, _i(rm), None),
    }
    for name, f in calls.items():
        assert f(C.byref(good)) == NODEV, name
        assert f(None) == INV, name
        for p in bad:
            assert f(p) == INV, name
    assert calls["twins_batch"](C.byref(good), n=-1) == INV and calls["twins_batch"](C.byref(good), x=None) == INV and calls["twins_batch"](C.byref(good), t=None) == INV
    assert calls["twins_batch"](C.byref(good), n=B.DUP_MAP_MAX + 1) == INV and calls["merge_batch"](C.byref(good), n=B.DUP_MAP_MAX + 1) == INV
    assert calls["merge_batch"](C.byref(good), n=-1) == INV and calls["merge_batch"](C.byref(good), x=None) == INV
    assert L.gs_map_twins_batch(None, 0, None, None, None, C.byref(good), None, None, None, None) == INV
    assert L.gs_map_merge_twins(None, C.byref(good), 0, None, None) == INV and L.gs_map_twins_resident(None, C.byref(good), None, None, None, None) == INV
    assert L.gs_map_get_xy(h, 0, 0, None, None) == NODEV and L.gs_map_get_xy(h, 0, 1, _d(oxy), None) == INV and L.gs_map_get_xy(h, -1, 0, None, None) == INV
    assert L.gs_merge_landmarks(None, 0, 1) == INV


# ---- gs_merge_landmarks on a host-only handle
POSES = 6
LMS = (100, 7, 42, 3, 18)


def _insert(g, skip=None, to=None):
    """a small graph: odometry chain, Cartesian and polar observation edges, landmark priors; landmark `skip` is left out and what hangs on it
    points at `to`"""
    at = lambda l: to if l == skip else l
    for p in range(POSES):
        g.add_pose(50 + p, [p * 1.5, 0.1 * p, 0.05 * p])
    g.set_fixed_pose(50)
    for l in LMS:
        if l != skip:
            g.add_landmark(l, [0.3 * l, 4.0 - 0.1 * l])
    for p in range(POSES - 1):
        g.add_odometry_edge(50 + p, 51 + p, [1.5, 0.1, 0.05], np.eye(3) * (2.0 + p))
    e = 0
    for p in range(POSES):
        for l in LMS:
            e += 1
            if e % 3 == 0:
                continue
            if e % 5 == 0:
                g.add_range_bearing_edge(50 + p, at(l), [2.0 + 0.1 * e, 0.01 * e], np.diag([4.0, 30.0 + e]))
            elif e % 7 == 0:
                g.add_bearing_edge(50 + p, at(l), 0.02 * e, 25.0)
            else:
                g.add_observation_edge(50 + p, at(l), [0.2 * e, 1.0 - 0.1 * e], [[3.0 + e, 0.5], [0.5, 2.0]])
    for l in (7, 42, 18, 42):
        g.add_landmark_prior(at(l), [0.3 * l, 4.0], [[1.0 + l, 0.0], [0.0, 2.0]])
    off = [1, 4, 9, 12]
    g.set_edges_active("observation", off, None)
    return off


def _state(g):
    n, m = g.n_poses, g.n_landmarks
    pid = np.zeros(n, dtype=np.int32); pe = np.zeros((n, 3)); lid = np.zeros(m, dtype=np.int32); le = np.zeros((m, 2))
    g._check(g.L.gs_get_poses(g.h, n, B._i(pid), B._d(pe))); g._check(g.L.gs_get_landmarks(g.h, m, B._i(lid), B._d(le)))
    g.plan_build_host()
    return dict(pid=pid.tolist(), pe=pe.tobytes(), lid=lid.tolist(), le=le.tobytes(), counts=(n, m, g.n_pp, g.n_pl, g.n_landmark_priors, g.num_polar_edges()),
                polar=[a.tolist() for a in g.polar_edges()], active=g.edges_active("observation").tolist(), plan=g.plan_export().tobytes(),
                isolated=g.find_isolated_vertex())


@pytest.mark.parametrize("keep,drop", [(100, 42), (42, 7), (7, 18), (18, 3), (3, 18)])
def test_merge_landmarks_equals_a_fresh_handle_with_the_merged_insertions(keep, drop):
    a = pkg.Graph(device=-2); b = pkg.Graph(device=-2)
    try:
        off = _insert(a); _insert(b, skip=drop, to=keep)
        before = a.get_landmark(keep).tobytes()
        a.merge_landmarks(keep, drop)
        sa, sb = _state(a), _state(b)
        assert sa == sb
        assert a.n_landmarks == len(LMS) - 1 and a.n_landmark_priors == 4 and a.num_polar_edges() == b.num_polar_edges() > 0
        assert a.get_landmark(keep).tobytes() == before                        # keep's estimate is untouched
        assert [i for i, f in enumerate(sa["active"]) if not f] == off         # the flags stayed with their edges
        with pytest.raises(B.GsError) as e:
            a.get_landmark(drop)
        assert e.value.code == GS_ERR_UNKNOWN_ID
        a.add_landmark(drop, [0.0, 0.0])                                       # the id is free again
    finally:
        a.close(); b.close()


def test_merge_landmarks_refusals():
    g = pkg.Graph(device=-2)
    try:
        _insert(g); L = g.L
        assert L.gs_merge_landmarks(g.h, 7, 999) == GS_ERR_UNKNOWN_ID and L.gs_merge_landmarks(g.h, 999, 7) == GS_ERR_UNKNOWN_ID
        assert L.gs_merge_landmarks(g.h, 999, 999) == GS_ERR_UNKNOWN_ID
        assert L.gs_merge_landmarks(g.h, 7, 7) == GS_ERR_INVALID
        g.set_fixed_landmark(42)
        assert L.gs_merge_landmarks(g.h, 7, 42) == GS_ERR_INVALID          # drop fixed, keep free
        assert g.n_landmarks == len(LMS)
        g.set_fixed_landmark(7)
        assert L.gs_merge_landmarks(g.h, 7, 42) == GS_OK                   # both fixed
        assert L.gs_merge_landmarks(g.h, 7, 3) == GS_OK                    # keep fixed, drop free
        assert g.n_landmarks == len(LMS) - 2
    finally:
        g.close()
    g = pkg.Graph(device=-2)                                                   # a sharded handle (which takes no priors)
    try:
        g.add_landmark(1, [0.0, 0.0]); g.add_landmark(2, [0.1, 0.0])
        g.dist_configure(0, 2)
        assert g.L.gs_merge_landmarks(g.h, 1, 2) == GS_ERR_INVALID and g.n_landmarks == 2
    finally:
        g.close()


def test_layout_and_graph_merge_under_address_and_undefined_sanitizers(tmp_path):
    """tests/dup_layout_san.cpp: a stand-alone program (its own main, no HIP, nothing loaded into python) around csrc/gs_dup_host.hpp"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "dup_layout_san")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "opendlv-logic-cfsd18-sensation-slam_amd", "csrc"), os.path.join(ROOT, "tests", "dup_layout_san.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0 and "dup layout: ok" in out.stdout, out.stdout + out.stderr
