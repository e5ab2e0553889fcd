"""GPU tests of the marginal covariances (gs_compute_marginals): the selected inversion of the device factor against the inverse
of the oracle's H at the same estimates, over every factor form and launch mode, growth, the side-effect rules and the errors.

Tolerance.  The CPU-vs-CPU spread of these blocks, relative to the block's largest entry: numpy's dense inverse against columns of
the reference's Eigen LDL^T (oracle EigenSolver(0), analysed once) is 1.2e-13 / 4.1e-13 at 50/30 (cond H 9e4) and 3.4e-10 / 2.7e-10
at 1k/200 (cond H 7e7), at the initial estimates / after optimize(10).  The other graphs here, against the supernodal replay of
tests/selinv_exec.py: 2e-11 / 6e-12 on the K = 16 / 24 tracks of 400 poses, 8.9e-10 on the 600-pose growth graph (cond H 1e8).  The
bound is about 10x the largest: REL = 1e-8.  At cfg3 (10k / 2k after optimize(10): marginal variances up to 3e6 along a 10k-pose chain)
the Eigen LDL^T columns and scipy's sparse LU columns differ by 2.5e-7 on the sampled blocks, the replay and scipy by 6.4e-7: REL3 = 1e-5."""
import numpy as np
import pytest

from conftest import append_tail, make_oracle_graph, split_for_growth
import selinv_exec as sx

pytestmark = pytest.mark.gpu
REL = 1e-8
REL3 = 1e-5


def fresh(pkg, g, debug=None, **kw):
    G = pkg.Graph(device=0, debug=debug, **kw)
    G.load_bench_graph(g)
    return G


def blocks_of(G):
    return G.pose_covariances(), G.landmark_covariances(), G.odometry_edge_covariances(), G.observation_edge_covariances()


def rel_err(a, b):
    """largest error of a block relative to the largest entry of the reference block (zero blocks: absolute)"""
    a = a.reshape(len(a), -1); b = b.reshape(len(b), -1)
    if not len(b):
        return 0.0
    sc = np.abs(b).max(1)
    return float((np.abs(a - b).max(1) / np.where(sc > 0, sc, 1.0)).max())


def oracle_at(po, g, G):
    """the oracle graph at the handle's current estimates -> dense H, oracle offsets"""
    og = make_oracle_graph(po, g)
    og.set_poses(G.poses()); og.set_landmarks(G.landmarks())
    return sx.dense_system(og)


def check_against_dense(po, g, G):
    H, po_, lo_ = oracle_at(po, g, G)
    ref = sx.reference_blocks(np.linalg.inv(H), po_, lo_, g)
    got = blocks_of(G)
    for name, a, b in zip(("poses", "landmarks", "odometry edges", "observation edges"), got, ref):
        assert a.shape == b.shape
        e = rel_err(a, b)
        assert e < REL, (name, e)
    for blk in list(got[0][np.asarray(po_) >= 0]) + list(got[1][np.asarray(lo_) >= 0]):     # SPD diagonal blocks
        assert np.array_equal(blk, blk.T) and np.linalg.eigvalsh(blk).min() > 0
    return got


@pytest.mark.parametrize("N,M", [(50, 30), (1000, 200)])
def test_diagonal_and_cross_blocks_equal_the_dense_inverse(pkg, po, bench_graphs, N, M):
    _, g = bench_graphs(N, M)
    G = fresh(pkg, g)
    info = G.compute_marginals()                                    # at the initial estimates
    assert info["numeric_failure"] == 0 and info["sigma_bytes"] > 0 and info["ms_total"] > 0
    check_against_dense(po, g, G)
    G.optimize(10)
    G.compute_marginals()                                           # after optimize(10)
    got = check_against_dense(po, g, G)
    # single pairs through gs_get_covariance_block: the same numbers as the arrays
    rng = np.random.default_rng(1)
    for k in rng.choice(len(g["pp_i"]), 8, replace=False):
        i, j = int(g["pp_i"][k]), int(g["pp_j"][k])
        assert np.array_equal(G.covariance_block("pose", i, "pose", j), got[2][k])
        assert np.array_equal(G.covariance_block("pose", j, "pose", i), got[2][k].T)
    for k in rng.choice(len(g["pl_p"]), 8, replace=False):
        p, l = int(g["pl_p"][k]), int(g["pl_l"][k])
        assert np.array_equal(G.covariance_block("pose", p, "landmark", l), got[3][k])
        assert np.array_equal(G.covariance_block("landmark", l, "landmark", l), got[1][l])
    G.close()


def test_a_pair_outside_the_pattern_is_refused(pkg, bench_graphs):
    from plan_exec import Plan
    _, g = bench_graphs(1000, 200)
    G = fresh(pkg, g); G.compute_marginals()
    P = Plan(G.plan_export()); rows = sx.Rows(P)
    far = next(q for q in range(600, 1000) if P.pose_gidx[q] >= 0 and rows.place(int(P.pose_gidx[5]), int(P.pose_gidx[q])) is None)
    with pytest.raises(pkg.GsError) as e:
        G.covariance_block("pose", 5, "pose", far)
    assert e.value.code == -11
    G.close()


def test_cfg3_sample_against_columns_of_the_reference_solver(pkg, po, bench_graphs):
    """10k / 2k: 256 poses, 256 landmarks and their edges against columns of H^-1 from the reference's Eigen LDL^T (analysed once)"""
    _, g = bench_graphs(10000, 2000)
    G = fresh(pkg, g); G.optimize(10); G.compute_marginals()
    got = blocks_of(G)
    og = make_oracle_graph(po, g); og.set_poses(G.poses()); og.set_landmarks(G.landmarks())
    n, colptr, rowind, values, _ = og.build_system()
    po_ = np.zeros(og.n_poses, dtype=np.int32); lo_ = np.zeros(og.n_landmarks, dtype=np.int32)
    from oracle.pyoracle import _i
    og.L.orc_vertex_offsets(og.g, _i(po_), _i(lo_))
    rng = np.random.default_rng(3)
    ps = rng.choice(np.flatnonzero(po_ >= 0), 256, replace=False); ls = rng.choice(np.flatnonzero(lo_ >= 0), 256, replace=False)
    cols = np.concatenate([po_[p] + np.arange(3) for p in ps] + [lo_[l] + np.arange(2) for l in ls])
    E = po.EigenSolver(0); X = np.zeros((n, len(cols)))
    for k, c in enumerate(cols):
        e = np.zeros(n); e[c] = 1.0
        X[:, k] = E.solve(n, colptr, rowind, values, e, analyze=(k == 0))
    col = {int(c): k for k, c in enumerate(cols)}
    for p in ps:
        ref = X[po_[p]:po_[p] + 3, [col[po_[p] + t] for t in range(3)]]
        assert rel_err(got[0][p][None], ref[None]) < REL3
    for l in ls:
        ref = X[lo_[l]:lo_[l] + 2, [col[lo_[l] + t] for t in range(2)]]
        assert rel_err(got[1][l][None], ref[None]) < REL3
    pset = set(int(p) for p in ps)
    for k in np.flatnonzero(np.isin(g["pl_p"], ps)):
        p, l = int(g["pl_p"][k]), int(g["pl_l"][k])
        if lo_[l] < 0:
            continue
        ref = X[lo_[l]:lo_[l] + 2, [col[po_[p] + t] for t in range(3)]].T          # Sigma(x_p, l) = Sigma(l, x_p)^T
        assert rel_err(got[3][k][None], ref[None]) < REL3
    for k in np.flatnonzero(np.isin(g["pp_j"], ps)):
        i, j = int(g["pp_i"][k]), int(g["pp_j"][k])
        if po_[i] < 0 or j not in pset:
            continue
        ref = X[po_[i]:po_[i] + 3, [col[po_[j] + t] for t in range(3)]]
        assert rel_err(got[2][k][None], ref[None]) < REL3
    G.close()


@pytest.mark.parametrize("kw,debug", [(dict(factor_variant=4), None), (dict(leaf_poses=3), None), (dict(leaf_poses=64), None),
                                      (dict(), dict(tree=0)), (dict(), dict(leaf_kernel=0)), (dict(), dict(block_fronts=0)),
                                      (dict(), dict(leaf_kernel=2)), (dict(), dict(leaf_kernel=2, subtree=1, block_fronts=0)),
                                      (dict(), dict(tickets=1))])
def test_every_factor_form_and_launch_mode(pkg, po, bench_graphs, kw, debug):
    _, g = bench_graphs(1000, 200)
    G = fresh(pkg, g, debug=debug, **kw); G.optimize(3); G.compute_marginals()
    got = check_against_dense(po, g, G)
    if not kw:                                                      # the same variant-3 plan: Sigma bit for bit whatever the launch mode
        A = fresh(pkg, g); A.optimize(3); A.compute_marginals()
        for a, b in zip(blocks_of(A), got):
            assert np.array_equal(a, b)
        A.close()
    G.close()


def test_variant4_fronts_beyond_the_lds(pkg, po):
    """a dense irregular graph whose fronts all hold 182-268 scalars (variant 4 by default): every one takes the HBM form of the inversion
    (k_selinv_big), which works in the front's arena slot (the L L^T form of the panels runs in test_every_factor_form_and_launch_mode)"""
    from conftest import random_graph
    from plan_exec import Plan
    g = random_graph(5, n_poses=80, n_lms=120, obs_per_pose=40, extra_pp=10)
    G = fresh(pkg, g); G.compute_marginals()
    assert G.stats().factor_variant == 4
    f = Plan(G.plan_export()); f = f.npiv + f.nbnd
    assert f.max() > 200
    check_against_dense(po, g, G)
    G.close()


@pytest.mark.parametrize("K", [16, 24])
def test_plans_with_workgroup_fronts(pkg, po, frontend, K):
    t = pkg.track.generate(400, 150, K)
    g = pkg.track.bench_graph(t, frontend)
    G = fresh(pkg, g); G.optimize(3); G.compute_marginals()
    assert G.stats().n_big_fronts > 0
    check_against_dense(po, g, G)
    B = fresh(pkg, g, debug=dict(tree=0)); B.optimize(3); B.compute_marginals()
    for a, b in zip(blocks_of(B), blocks_of(G)):
        assert np.array_equal(a, b)
    G.close(); B.close()


def test_growth_gives_the_marginals_of_a_fresh_build(pkg, po, bench_graphs):
    _, g0 = bench_graphs(1000, 200)
    base, tail, full = split_for_growth(g0, 4, keep=600)
    G = fresh(pkg, base); G.optimize(2)
    G.compute_marginals()
    for k in range(4):
        append_tail(G, tail, (k, k + 1))
        G.initialize_optimization(); assert G.plan_growths() == k + 1, G.growth_refusal()
    G.compute_marginals()
    F = pkg.Graph(device=0); F.load_bench_graph(dict(full, pose_est=G.poses(), lm_est=G.landmarks()))
    F.compute_marginals()
    for a, b in zip(blocks_of(G), blocks_of(F)):
        assert rel_err(a, b) < REL
    check_against_dense(po, dict(full), G)
    G.close(); F.close()


def test_the_call_moves_nothing(pkg, bench_graphs):
    _, g = bench_graphs(1000, 200)
    A = fresh(pkg, g); A.optimize(5)
    B = fresh(pkg, g); B.optimize(5)
    P0, L0 = B.poses().copy(), B.landmarks().copy()
    B.compute_marginals()
    assert np.array_equal(B.poses(), P0) and np.array_equal(B.landmarks(), L0)
    A.optimize(5); B.optimize(5)
    assert np.array_equal(A.poses(), B.poses()) and np.array_equal(A.landmarks(), B.landmarks())
    # the stop rule of optimize_until fires at the same iteration
    C = fresh(pkg, g); D = fresh(pkg, g)
    C.optimize(2); D.optimize(2); D.compute_marginals()
    nc = C.optimize_until(50, 1e-6)[0]; nd = D.optimize_until(50, 1e-6)[0]
    assert nc == nd and np.array_equal(C.poses(), D.poses())
    A.close(); B.close(); C.close(); D.close()


def test_results_go_stale(pkg, bench_graphs):
    _, g = bench_graphs(50, 30)
    getters = lambda G: (G.pose_covariances, G.landmark_covariances, G.odometry_edge_covariances, G.observation_edge_covariances,
                         lambda: G.covariance_block("pose", 2, "pose", 3))

    def stale(G):
        for fn in getters(G):
            with pytest.raises(pkg.GsError) as e:
                fn()
            assert e.value.code == -6
    G = fresh(pkg, g)
    stale(G)
    for act in (lambda: G.optimize(1), lambda: G.iterate(), lambda: G.set_pose_estimate(5, G.get_pose(5) + 0.01),
                lambda: G.set_landmark_estimate(2, G.get_landmark(2)), lambda: G.add_pose(100000, [0.0, 0.0, 0.0])):
        G.compute_marginals()
        G.pose_covariances()                                        # fresh results are served
        act()
        stale(G)
    G.close()
    G = fresh(pkg, g); G.compute_marginals(); G.pose_covariances()
    G.clear()
    stale(G)
    G.close()


def test_error_cases(pkg, bench_graphs):
    # the gauge-free singular system of test_singular_system_returns_zero_and_leaves_the_estimates_like_g2o
    G = pkg.Graph(device=0)
    P0 = np.array([[0.0, 0, 0], [1.1, 0.2, 0.1], [2.3, -0.1, 0.2]])
    G.add_poses([0, 1, 2], P0)
    z = np.array([[1.0, 0, 0], [1.0, 0, 0]]); info = np.tile((np.diag([1.0, 1.0, 0.0])).reshape(1, 9), (2, 1))
    G.add_odometry_edges([0, 1], [1, 2], z, info)
    with pytest.raises(pkg.GsError) as e:
        G.compute_marginals()
    assert e.value.code == -8
    with pytest.raises(pkg.GsError) as e:
        G.pose_covariances()
    assert e.value.code == -6
    assert np.array_equal(G.poses(), P0)
    G.close()
    # fixed vertices: zero blocks, and zero cross blocks
    _, g = bench_graphs(50, 30)
    G = fresh(pkg, g); G.compute_marginals()
    pc, lc, ppc, plc = blocks_of(G)
    for p in g["fixed_poses"]:
        assert not pc[int(p)].any()
        assert not ppc[(g["pp_i"] == p) | (g["pp_j"] == p)].any()
        assert not plc[g["pl_p"] == p].any()
    for l in g["fixed_landmarks"]:
        assert not lc[int(l)].any() and not plc[g["pl_l"] == l].any()
    G.close()
    # a sharded handle is refused
    S = fresh(pkg, g, debug=dict(force_shared_top=2))
    with pytest.raises(pkg.GsError) as e:
        S.compute_marginals()
    assert e.value.code == -1
    S.close()


def test_slam_mirror_map_covariances(pkg):
    """after a lap of the synthetic track: the map's covariances are the landmark blocks of gs_slam_graph, in map order (map cone j is
    the graph's landmark with id j: the reference numbers cones 0, 1, ... as it maps them)"""
    N, M = 120, 60
    t = pkg.track.generate(N, M)
    S = pkg.Slam(same_cone_threshold=1.2, cone_mapping_threshold=67.0)
    for k in range(N):
        S.perform_slam(t["odom_poses"][k], t["obs"][k])
        if k == 10:                                                  # before the loop closure the mirror has no gauge: no covariances
            assert not S.loop_closed
            with pytest.raises(pkg.GsError) as e:
                S.map_covariances()
            assert e.value.code == -6
    assert S.loop_closed
    xy_before = S.map()[0].copy(); pose_before = S.graph.poses().copy()
    C = S.map_covariances()
    assert len(C) == S.map_size > 0
    ids = np.zeros(S.graph.n_landmarks, dtype=np.int32)
    import ctypes
    pkg.binding.lib().gs_get_landmarks(S.graph.h, len(ids), ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                       np.zeros((len(ids), 2)).ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    lc = S.graph.landmark_covariances()
    index = {int(i): k for k, i in enumerate(ids)}
    for j in range(len(C)):
        assert np.array_equal(C[j], lc[index[j]])
    assert np.array_equal(S.map()[0], xy_before) and np.array_equal(S.graph.poses(), pose_before)
    S.close()


def test_cfg4_smoke(pkg, bench_graphs):
    _, g = bench_graphs(100000, 10000)
    G = fresh(pkg, g); G.optimize(10)
    info = G.compute_marginals()
    pc, lc, _, _ = blocks_of(G)
    assert np.isfinite(pc).all() and np.isfinite(lc).all()
    free = np.ones(len(lc), bool); free[g["fixed_landmarks"]] = False
    assert np.linalg.eigvalsh(lc[free]).min() > 0
    # the arena is the packed lower triangles of every front, sum f (f + 1) / 2 doubles
    from plan_exec import Plan
    P = Plan(G.plan_export()); f = (P.npiv + P.nbnd).astype(np.int64)
    assert info["sigma_bytes"] == 8 * int((f * (f + 1) // 2).sum())
    G.close()
