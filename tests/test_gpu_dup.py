"""GPU tests of the map twins (k_dup_nearest / k_dup_fuse / k_dup_scan / k_dup_scatter of gs_dup.hip).

Per scene of dup_shapes: the batch and the resident query return identical bits, the batch and the in-place consolidation return identical
bits, the resident query changes nothing and writes exactly [0, n) of pre-filled outputs, and dup_ref holds every decision, counter, remap
entry and untouched cone bit for bit and every d2, l+ and C+ inside its bound B = 2 e.  Across scenes: the symmetry of a pair's d2, a second
consolidation of the truth scene, the triplet's two rounds, NULL outputs.  After a consolidation: a frame that saw both copies of a cone, the
resident association and relocalisation against a handle whose map was appended already consolidated (the grids' invalidation), and a lap
graph whose loop is closed by merging the two vertices of one cone.  A twins query leaves the other paths of a handle alone.

The figures printed with -s (pair values held, the largest |device - exact| / B) are recorded in DESIGN.md section 31."""
import ctypes as C

import numpy as np
import pytest

import cand_shapes as cs
import dup_ref as dr
import dup_shapes as ds
import relocalize_shapes as rs

pytestmark = pytest.mark.gpu
WORST = {"r": 0.0, "where": "", "values": 0, "fused": 0}
FILL = 0x5A
REFS = {}


def ref_of(name):
    if name not in REFS:
        REFS[name] = dr.make(ds.scene(name), ds.params_of(ds.scene(name)))
    return REFS[name]


@pytest.fixture(scope="module")
def G(pkg):
    if pkg.device_count() < 1:
        pytest.fail("no gfx950 device visible: the HIP path cannot run")
    g = pkg.Graph(lidar_to_cog=rs.LIDAR)
    yield g
    g.close()
    print("\nmap twins: %d pair values and %d fused values held to the exact ones, largest |device - exact| / B %.3g (%s)"
          % (WORST["values"], WORST["fused"], WORST["r"], WORST["where"]))


@pytest.fixture(scope="module")
def Gplain(pkg):
    """a handle that never sets a map covariance"""
    g = pkg.Graph(lidar_to_cog=rs.LIDAR)
    yield g
    g.close()


def set_map(g, xy, ty, cov):
    g.map_clear()
    if len(ty):
        g.map_append(xy, ty)
        if cov is not None:
            g.map_set_cov(0, cov)
    assert g.map_size() == len(ty)


def map_bytes(g):
    xy, ty = g.map_xy()
    return xy.tobytes(), ty.tobytes(), g.map_cov().tobytes()


def resident_query(pkg, g, p, n, only_twin=False):
    """gs_map_twins_resident into outputs of n + 8 entries pre-filled with a pattern: (twin, d2, second, nadm) of [0, n), and the tails"""
    DA = pkg.binding.DeviceArray; m = n + 8
    ti = np.zeros(m, dtype=np.int32); ti.view(np.uint8)[...] = FILL; td = np.zeros(m); td.view(np.uint8)[...] = FILL
    d = [DA(ti), DA(td), DA(td), DA(ti)]
    g.map_twins_resident(d[0], None if only_twin else d[1], None if only_twin else d[2], None if only_twin else d[3], p); g.synchronize()
    out = [d[0].to_host(np.int32, m), d[1].to_host(np.float64, m), d[2].to_host(np.float64, m), d[3].to_host(np.int32, m)]
    for a in d:
        a.free()
    return [a[:n] for a in out], [a[n:] for a in out], (ti, td)


@pytest.mark.parametrize("name", ds.NAMES)
def test_scene_every_path_and_the_reference(pkg, G, Gplain, name):
    sc = ds.scene(name); b = pkg.binding; p = b.dup_params(**sc["params"]); n = len(sc["ty"]); ref = ref_of(name)
    g = Gplain if sc["cov"] is None else G
    batch = g.map_twins(sc["xy"], sc["ty"], sc["cov"], p)
    set_map(g, sc["xy"], sc["ty"], sc["cov"])
    before = map_bytes(g)
    res, tails, (ti, td) = resident_query(pkg, g, p, n)
    assert [a.tobytes() for a in res] == [a.tobytes() for a in batch], (name, "the resident query differs from the batch query")
    assert all(t.tobytes() == (ti if t.dtype == np.int32 else td)[n:].tobytes() for t in tails), (name, "the resident query wrote beyond [0, n)")
    assert map_bytes(g) == before, (name, "the resident query changed the map")
    twin, d2, second, nadm = batch
    bad = ref.twins_failures(twin, d2, second, nadm)
    assert not bad, (name, bad[:3])
    for a, bb in ref.twin_pairs:                                               # both ends of a pair see identical bits
        assert d2[a].tobytes() == d2[bb].tobytes(), (name, a, bb)
    mxy, mty, mcv, remap, info = g.map_merge_twins_batch(sc["xy"], sc["ty"], sc["cov"], p)
    rremap, rinfo = g.map_merge_twins(p)
    assert g.map_size() == int(rinfo["n_out"]) == len(mty)
    rxy, rty = g.map_xy(); rcv = g.map_cov()
    assert (rxy.tobytes(), rty.tobytes(), rremap.tobytes(), rinfo.tobytes()) == (mxy.tobytes(), mty.tobytes(), remap.tobytes(), info.tobytes()), (name, "in place differs from batch")
    if sc["cov"] is not None:
        assert rcv.tobytes() == mcv.tobytes(), (name, "in place differs from batch: cov")
    else:
        assert mcv is None and not rcv.any(), (name, "a covariance where none was given")
    bad = ref.merge_failures(mxy, mty, None if mcv is None else mcv.reshape(-1, 4), remap, info)
    assert not bad, (name, bad[:3])
    WORST["values"] += ref.n_values; WORST["fused"] += (5 if mcv is not None else 2) * len(ref.twin_pairs)
    if ref.worst > WORST["r"]:
        WORST["r"], WORST["where"] = ref.worst, name


def test_truth_scene_facts_of_the_reference_then_of_the_device(pkg, G):
    sc, planted = ds.truth(); ref = ref_of("truth")
    assert ref.twin_pairs == planted and ref.nadm.max() == 1 and ref.info == dict(n_in=160, n_out=120, n_pairs=40, n_ambiguous=0)
    twin, d2, second, nadm = G.map_twins(sc["xy"], sc["ty"], sc["cov"])
    assert [(a, int(twin[a])) for a in range(160) if twin[a] > a and twin[twin[a]] == a] == planted
    assert nadm.max() == 1 and np.isinf(second).all() and abs(d2[np.isfinite(d2)].max() - 4.668) < 5e-4
    assert sorted(np.flatnonzero(twin < 0)) == sorted(set(range(120)) - {a for a, _ in planted})
    # a second consolidation of the consolidated map finds nothing and leaves every bit alone
    set_map(G, sc["xy"], sc["ty"], sc["cov"])
    remap, info = G.map_merge_twins()
    assert (int(info["n_pairs"]), G.map_size()) == (40, 120)
    once = map_bytes(G)
    remap2, info2 = G.map_merge_twins()
    assert (int(info2["n_in"]), int(info2["n_out"]), int(info2["n_pairs"]), int(info2["n_ambiguous"])) == (120, 120, 0, 0)
    assert map_bytes(G) == once and remap2.tolist() == list(range(120))


def test_the_triplet_needs_exactly_two_rounds(pkg, G):
    sc = ds.scene("triplet"); set_map(G, sc["xy"], sc["ty"], sc["cov"])
    rounds = []
    for _ in range(3):
        _, info = G.map_merge_twins(); rounds.append(int(info["n_pairs"]))
    assert rounds == [1, 1, 0] and G.map_size() == 38
    p = ds.params_of(sc); r1 = dr.replay(sc["xy"], sc["ty"], sc["cov"], p); r2 = dr.replay(r1["xy"], r1["ty"], r1["cov"], p)
    xy, ty = G.map_xy()
    assert ty.tolist() == r2["ty"].tolist() and np.allclose(xy, r2["xy"], rtol=0, atol=1e-12) and np.allclose(G.map_cov().reshape(-1, 4), r2["cov"], rtol=1e-12, atol=0)


def test_null_outputs(pkg, G):
    sc = ds.scene("n257"); b = pkg.binding; L = b.lib(); p = b.dup_params(); n = 257; _d, _i = b._d, b._i
    full = G.map_twins(sc["xy"], sc["ty"], sc["cov"], p)
    tw = np.zeros(n, dtype=np.int32)
    assert L.gs_map_twins_batch(G.h, n, _d(sc["xy"]), _i(sc["ty"]), _d(sc["cov"]), C.byref(p), _i(tw), None, None, None) == 0
    assert tw.tobytes() == full[0].tobytes()
    set_map(G, sc["xy"], sc["ty"], sc["cov"])
    res, _, _ = resident_query(pkg, G, p, n, only_twin=True)
    assert res[0].tobytes() == full[0].tobytes()
    mxy, mty, mcv, remap, info = G.map_merge_twins_batch(sc["xy"], sc["ty"], sc["cov"], p)
    oxy = np.zeros((n, 2)); oty = np.zeros(n, dtype=np.int32)
    assert L.gs_map_merge_twins_batch(G.h, n, _d(sc["xy"]), _i(sc["ty"]), _d(sc["cov"]), C.byref(p), _d(oxy), _i(oty), None, None, None) == 0
    k = len(mty)
    assert oxy[:k].tobytes() == mxy.tobytes() and oty[:k].tobytes() == mty.tobytes() and np.isnan(oxy[k:]).all() and not oty[k:].any()
    assert L.gs_map_merge_twins(G.h, C.byref(p), 0, None, None) == 0 and G.map_size() == k
    assert G.map_xy()[0].tobytes() == mxy.tobytes() and G.map_cov().tobytes() == mcv.tobytes()
    rm = np.zeros(4, dtype=np.int32)
    assert L.gs_map_merge_twins(G.h, C.byref(p), 4, _i(rm), None) == -9 and G.map_size() == k          # GS_ERR_CAPACITY, nothing changes


def _seen_from(pose, xy, ty):
    c, s = np.cos(pose[2]), np.sin(pose[2]); d = xy - pose[:2]
    return rs.obs_of_xy(np.stack([d[:, 0] * c + d[:, 1] * s, -d[:, 0] * s + d[:, 1] * c], axis=1), ty)


def test_a_frame_that_saw_both_copies_gives_the_cone_to_one_observation(pkg, G):
    sc, planted = ds.truth(); _, _, poses = rs.track()
    set_map(G, sc["xy"], sc["ty"], sc["cov"])
    pose = poses[58]; both = [0, 120]
    ob = _seen_from(pose, sc["xy"][both], sc["ty"][both])
    _, _, idx, _, na = G.frame_frontend_assign_opt(pose, ob)
    assert sorted(idx.tolist()) == both and na.tolist() == [2, 2]              # the two copies go to two observations
    remap, _ = G.map_merge_twins()
    assert remap[0] == remap[120] == 0
    _, _, idx, _, na = G.frame_frontend_assign_opt(pose, ob)
    assert sorted(idx.tolist()) == [-1, 0] and na.tolist() == [1, 1]


def test_resident_calls_over_the_consolidated_map_equal_a_map_appended_consolidated(pkg, G):
    """the association's and the relocalisation's grids are built before the consolidation: they must not outlive it"""
    b = pkg.binding; DA = b.DeviceArray; sc, _ = ds.truth(); xy0, ty0, poses = rs.track(); rng = np.random.default_rng(8)
    frames = [rs.view(xy0, ty0, poses[at] + np.array([0.3, -0.2, 0.03]), 8, rng)[0] for at in (3, 17, 40)]
    obs = np.concatenate(frames); n = len(obs); fs = np.array([0, 8, 16, 24], dtype=np.int32)
    ps = np.stack([poses[at] + np.array([0.3, -0.2, 0.03]) for at in (3, 17, 40)]); po = np.repeat(np.arange(3, dtype=np.int32), 8)
    d_obs, d_fs, d_ps, d_po = DA(obs), DA(fs), DA(ps), DA(po)

    def run(g):
        o = dict(idx=DA(np.zeros(n, dtype=np.int32)), d2=DA(np.zeros(n)), sec=DA(np.zeros(n)), pose=DA(np.zeros(9)), count=DA(np.zeros(3, dtype=np.int32)),
                 cost=DA(np.zeros(3)), ridx=DA(np.zeros(n, dtype=np.int32)))
        g.associate_nn_resident(d_ps, 3, d_po, d_obs, n, o["idx"], o["d2"], o["sec"])
        g.relocalize_resident(d_obs, n, 3, d_fs, o["pose"], o["count"], o["cost"], d_index=o["ridx"]); g.synchronize()
        out = (o["idx"].to_host(np.int32, n), o["d2"].to_host(np.float64, n), o["sec"].to_host(np.float64, n), o["pose"].to_host(np.float64, 9),
               o["count"].to_host(np.int32, 3), o["cost"].to_host(np.float64, 3), o["ridx"].to_host(np.int32, n))
        for a in o.values():
            a.free()
        return out

    set_map(G, sc["xy"], sc["ty"], sc["cov"])
    stale = run(G)                                                             # builds both grids over the 160 cones
    G.map_merge_twins()
    got = run(G)
    mxy, mty, mcv, _, _ = G.map_merge_twins_batch(sc["xy"], sc["ty"], sc["cov"])
    H = pkg.Graph(lidar_to_cog=rs.LIDAR)
    try:
        set_map(H, mxy, mty, mcv.reshape(-1, 4)); want = run(H)
    finally:
        H.close()
    for a in (d_obs, d_fs, d_ps, d_po):
        a.free()
    assert [a.tobytes() for a in got] == [a.tobytes() for a in want]
    assert (got[0] >= 0).sum() >= 20 and (got[4] >= 4).all() and got[0].max() < 120 and stale[0].max() >= 0


# ---- the closed loop
N_POSES, N_CONES, TWIN_ID = 24, 12, 12


def _lap():
    """24 poses on a circle of 10 m, 12 cones on one of 12 m; a pose sees its four nearest cones exactly.  Cone 0 is entered under a second id
    (12) by the poses of the last third of the lap.  Returns the insertions as lists."""
    a = 2 * np.pi * np.arange(N_POSES) / N_POSES
    poses = np.stack([10 * np.cos(a), 10 * np.sin(a), a + np.pi / 2], axis=1)
    ca = 2 * np.pi * np.arange(N_CONES) / N_CONES
    cones = np.stack([12 * np.cos(ca), 12 * np.sin(ca)], axis=1)
    rng = np.random.default_rng(24)
    pose_est = poses + rng.normal(0, [0.05, 0.05, 0.01], (N_POSES, 3)); pose_est[0] = poses[0]
    lm_est = np.concatenate([cones, cones[:1]]) + rng.normal(0, 0.08, (N_CONES + 1, 2))
    pp, pl = [], []
    for p in range(N_POSES - 1):
        d = poses[p + 1] - poses[p]; c, s = np.cos(poses[p, 2]), np.sin(poses[p, 2])
        pp.append((p, p + 1, [c * d[0] + s * d[1], -s * d[0] + c * d[1], d[2]]))
    for p in range(N_POSES):
        d = cones - poses[p, :2]; c, s = np.cos(poses[p, 2]), np.sin(poses[p, 2])
        for l in np.argsort(np.hypot(d[:, 0], d[:, 1]))[:4]:
            lid = TWIN_ID if (l == 0 and p >= 2 * N_POSES // 3) else int(l)
            pl.append((p, lid, [c * d[l, 0] + s * d[l, 1], -s * d[l, 0] + c * d[l, 1]]))
    return pose_est, lm_est, pp, pl


def _build(g, pose_est, lm_est, pp, pl, merged):
    g.add_poses(np.arange(N_POSES), pose_est)
    g.add_landmarks(np.arange(len(lm_est)), lm_est)
    g.set_fixed_pose(0)
    for i, j, z in pp:
        g.add_odometry_edge(i, j, z, np.eye(3) * 400.0)
    for p, l, z in pl:
        g.add_observation_edge(p, 0 if (merged and l == TWIN_ID) else l, z, np.eye(2) * 100.0)


def test_the_loop_is_closed_by_merging_the_two_vertices_of_one_cone(pkg):
    pose_est, lm_est, pp, pl = _lap()
    assert sum(1 for _, l, _ in pl if l == TWIN_ID) >= 2 and sum(1 for _, l, _ in pl if l == 0) >= 2
    g = pkg.Graph(lidar_to_cog=rs.LIDAR); f = pkg.Graph(lidar_to_cog=rs.LIDAR)
    try:
        _build(g, pose_est, lm_est, pp, pl, merged=False)
        done, _ = g.optimize(10)
        assert done == 10
        g.compute_marginals()
        lm_ids = np.arange(N_CONES + 1, dtype=np.int32)
        g.map_append(g.landmarks(), np.ones(N_CONES + 1, dtype=np.int32)); g.map_set_cov_from_marginals(0, lm_ids)
        remap, new_ids, info = g.map_consolidate(lm_ids)
        assert (int(info["n_in"]), int(info["n_out"]), int(info["n_pairs"])) == (13, 12, 1)
        assert remap.tolist() == list(range(12)) + [0] and new_ids.tolist() == list(range(12))                 # exactly that pair
        assert g.n_landmarks == N_CONES and g.map_size() == N_CONES
        assert g.get_landmark(0).tobytes() == g.map_xy()[0][0].tobytes()       # the keeper carries the fused position
        assert g.find_isolated_vertex() is None
        _build(f, g.poses(), g.landmarks(), pp, pl, merged=True)               # the merged insertions, the same starting estimates
        done_g, st_g = g.optimize(10); done_f, st_f = f.optimize(10)
        assert done_g == done_f == 10
        assert g.poses().tobytes() == f.poses().tobytes() and g.landmarks().tobytes() == f.landmarks().tobytes()
        assert st_g.chi2_final < 1e-12 * max(st_g.chi2_initial, 1.0) or st_g.chi2_final < 1e-9
    finally:
        g.close(); f.close()


# ---- a twins query leaves the other paths of a handle alone
def test_a_twins_query_leaves_the_other_paths_alone(pkg, bench_graphs):
    b = pkg.binding; sc, _ = ds.truth(); _, _, poses = rs.track(); cn = cs.scene(cs.NAMES[0])
    t, bg = bench_graphs(50, 30)
    ob = _seen_from(poses[58], sc["xy"][:6], sc["ty"][:6])

    def run(query):
        g = pkg.Graph(lidar_to_cog=cs.LIDAR)
        try:
            set_map(g, sc["xy"], sc["ty"], sc["cov"])
            g.load_bench_graph(bg); g.initialize_optimization()
            if query:
                DA = b.DeviceArray; d = DA(np.zeros(160, dtype=np.int32))
                g.map_twins_resident(d); g.synchronize(); d.free()
                g.map_twins(sc["xy"], sc["ty"], sc["cov"])
            fe = g.frame_frontend_assign_opt(poses[58], ob)
            cd = g.cand(cn["poses"], cn["obs"], cn["frame_start"], cn["in_idx_all"], cn["pose_covs"], cn["records"], b.nn_params(**cn["params"]), b.cand_params(**cn["cand"]))
            g.iterate(); g.sync_estimates()
            return ([a.tobytes() for a in fe], [cd[k].tobytes() for k in ("steps", "cand_id", "cand_slot", "table")], g.poses().tobytes(), g.landmarks().tobytes(),
                    map_bytes(g))
        finally:
            g.close()

    assert run(False) == run(True)


# ---- gs_merge_landmarks on the device, with polar edges and priors on the dropped landmark and on landmarks behind it
LM_ORDER = [0, 1, 2, 3, TWIN_ID] + list(range(4, N_CONES))                   # the twin in the middle: eight landmarks move down by one


def test_merge_landmarks_with_polar_edges_and_priors_equals_a_fresh_handle(pkg):
    """every polar edge and every prior of the dropped landmark, and of the eight landmarks behind it, must reach the device under its new
    landmark index: ten iterations, every edge's chi2 and every prior's are bitwise those of a fresh handle with the merged insertions"""
    pose_est, lm_all, pp, pl = _lap()
    ids = np.array(LM_ORDER, dtype=np.int32); est = lm_all[ids]
    n_polar_twin = sum(1 for e, (_, l, _) in enumerate(pl) if l == TWIN_ID and e % 3 != 2)
    n_polar_behind = sum(1 for e, (_, l, _) in enumerate(pl) if 4 <= l < N_CONES and e % 3 != 2)
    assert n_polar_twin >= 2 and n_polar_behind >= 20
    g = pkg.Graph(lidar_to_cog=rs.LIDAR); f = pkg.Graph(lidar_to_cog=rs.LIDAR)
    try:
        prior_z = {l: lm_all[l] for l in (TWIN_ID, 7, 11, 4)}

        def build(h, lm_ids, lm_est, merged):
            rng = np.random.default_rng(77); at = lambda l: 0 if (merged and l == TWIN_ID) else l
            h.add_poses(np.arange(N_POSES), pose_est if not merged else g_poses)
            h.add_landmarks(lm_ids, lm_est)
            h.set_fixed_pose(0)
            for i, j, z in pp:
                h.add_odometry_edge(i, j, np.asarray(z) + rng.normal(0, [0.01, 0.01, 0.002]), np.eye(3) * 400.0)
            for e, (p, l, z) in enumerate(pl):
                z = np.asarray(z) + rng.normal(0, 0.02, 2)
                if e % 3 == 0:
                    h.add_range_bearing_edge(p, at(l), [np.hypot(z[0], z[1]), np.arctan2(z[1], z[0])], np.diag([100.0, 900.0]))
                elif e % 3 == 1:
                    h.add_bearing_edge(p, at(l), np.arctan2(z[1], z[0]), 900.0)
                else:
                    h.add_observation_edge(p, at(l), z, np.eye(2) * 100.0)
            for l in (TWIN_ID, 7, 11, TWIN_ID, 4):
                h.add_landmark_prior(at(l), prior_z[l], [[4.0, 0.5], [0.5, 3.0]])
            h.set_edges_active("observation", [5, 40], None)

        g_poses = None
        build(g, ids, est, merged=False)
        done, _ = g.optimize(3)                                                # the plan, the polar and the prior tables are on the device
        assert done == 3 and g.num_polar_edges() == sum(1 for e in range(len(pl)) if e % 3 != 2)
        g.merge_landmarks(0, TWIN_ID)
        assert g.n_landmarks == N_CONES and g.n_landmark_priors == 5 and g.find_isolated_vertex() is None
        g_poses = g.poses(); g_lms = g.landmarks()
        build(f, np.arange(N_CONES, dtype=np.int32), g_lms, merged=True)
        assert g.edges_active("observation").tolist() == f.edges_active("observation").tolist()
        assert [a.tolist() for a in g.polar_edges()] == [a.tolist() for a in f.polar_edges()]
        for h in (g, f):
            done, _ = h.optimize(10)
            assert done == 10
        assert g.poses().tobytes() == f.poses().tobytes() and g.landmarks().tobytes() == f.landmarks().tobytes()
        sg, wg = g.edge_chi2("observation"); sf, wf = f.edge_chi2("observation")
        assert sg.tobytes() == sf.tobytes() and wg.tobytes() == wf.tobytes() and sg.max() > 0
        assert g.edge_chi2("odometry")[0].tobytes() == f.edge_chi2("odometry")[0].tobytes()
        assert g.prior_chi2("landmark").tobytes() == f.prior_chi2("landmark").tobytes() and g.prior_chi2("landmark").max() > 0
        assert g.chi2() == f.chi2()
    finally:
        g.close(); f.close()


def test_a_max_distance_whose_square_is_not_a_normal_number(pkg, Gplain):
    """sqrt(0) < 1e-160 holds, so two coincident cones are twins: the search's first look must not stand in the rule's way"""
    p = pkg.binding.dup_params(max_distance=1e-160)
    twin, d2, second, nadm = Gplain.map_twins([[1.0, 2.0], [1.0, 2.0], [5.0, 5.0], [1.0, 2.0 + 1e-10]], [1, 1, 1, 1], None, p)
    assert twin.tolist() == [1, 0, -1, -1] and d2[:2].tolist() == [0.0, 0.0] and nadm.tolist() == [1, 1, 0, 0] and np.isinf(second).all()
