"""CPU tests of the marginal covariances (gs_compute_marginals and its getters) without a GPU: the C-ABI's declarations and
the host-only handle's errors, and a numpy replay of the selected inversion (tests/selinv_exec.py) over the exported plan
against np.linalg.inv of the oracle's dense H — which proves the index maps the device kernels and the extraction tables use."""
import re

import numpy as np
import pytest

from conftest import ROOT, make_oracle_graph, random_graph
from plan_exec import Plan
import selinv_exec as sx

NEW_FUNCS = ["gs_compute_marginals", "gs_get_pose_covariances", "gs_get_landmark_covariances", "gs_get_odometry_edge_covariances",
             "gs_get_observation_edge_covariances", "gs_get_covariance_block", "gs_slam_get_map_covariances"]


def test_header_declares_the_marginals_and_the_library_exports_them(pkg):
    txt = open(pkg.binding.HEADER).read()
    assert re.search(r"#define\s+GS_ERR_OUT_OF_PATTERN\s+-11\b", txt)
    assert re.search(r"typedef struct gs_marginals_info \{.*?int64_t\s+sigma_bytes;.*?\} gs_marginals_info;", txt, re.S)
    assert "computeMarginals" in txt
    L = pkg.binding.lib()
    for name in NEW_FUNCS:
        assert name in pkg.binding.declared_symbols(debug=False), name
        assert hasattr(L, name), name
    assert L.gs_version() == 1
    assert pkg.binding.ERRORS[-11] == "GS_ERR_OUT_OF_PATTERN"


def test_host_only_handle_refuses_the_marginals(pkg, bench_graphs):
    import ctypes as C
    _, g = bench_graphs(50, 30)
    G = pkg.Graph(device=-2); G.load_bench_graph(g)
    L = pkg.binding.lib()
    info = pkg.binding.MarginalsInfo()
    assert L.gs_compute_marginals(G.h, C.byref(info)) == -4               # GS_ERR_NO_DEVICE
    assert L.gs_compute_marginals(G.h, None) == -4
    buf = np.zeros(9 * 64); ids = np.zeros(64, dtype=np.int32)
    dp, ip = buf.ctypes.data_as(C.POINTER(C.c_double)), ids.ctypes.data_as(C.POINTER(C.c_int32))
    assert L.gs_get_pose_covariances(G.h, 64, ip, dp) == -6               # GS_ERR_NOT_INITIALIZED
    assert L.gs_get_landmark_covariances(G.h, 64, ip, dp) == -6
    assert L.gs_get_odometry_edge_covariances(G.h, 64, dp) == -6
    assert L.gs_get_observation_edge_covariances(G.h, 64, dp) == -6
    assert L.gs_get_covariance_block(G.h, 0, 2, 0, 3, dp) == -6
    # null arguments
    assert L.gs_compute_marginals(None, None) == -1
    assert L.gs_get_pose_covariances(G.h, 64, ip, None) == -1
    assert L.gs_get_pose_covariances(None, 64, ip, dp) == -1
    assert L.gs_get_landmark_covariances(G.h, 64, ip, None) == -1
    assert L.gs_get_odometry_edge_covariances(G.h, 64, None) == -1
    assert L.gs_get_observation_edge_covariances(None, 64, dp) == -1
    assert L.gs_get_covariance_block(G.h, 0, 2, 0, 3, None) == -1
    assert L.gs_slam_get_map_covariances(None, 4, dp) == -1
    # the binding raises GsError with those codes
    for fn, code in ((G.compute_marginals, -4), (G.pose_covariances, -6), (G.landmark_covariances, -6),
                     (G.odometry_edge_covariances, -6), (G.observation_edge_covariances, -6),
                     (lambda: G.covariance_block("pose", 2, "landmark", 0), -6)):
        with pytest.raises(pkg.GsError) as e:
            fn()
        assert e.value.code == code
    G.close()
    S = pkg.Slam(device=-2)
    with pytest.raises(pkg.GsError) as e:
        S.map_covariances()
    assert e.value.code == -4
    S.close()


def _replay_vs_dense(pkg, po, g, **kw):
    G = pkg.Graph(device=-2, **kw); G.load_bench_graph(g); G.plan_build_host()
    P = Plan(G.plan_export()); P.check_invariants(); G.close()
    og = make_oracle_graph(po, g)
    blocks = og.linearize_blocks()
    H, po_, lo_ = sx.dense_system(og)
    # the two solvers agree on which vertices are free
    assert np.array_equal(P.pose_gidx >= 0, po_ >= 0) and np.array_equal(P.lm_gidx >= 0, lo_ >= 0)
    Ls, ok = sx.factor(P, blocks)
    assert ok
    Sig = sx.selinv(P, Ls)
    ref = sx.reference_blocks(np.linalg.inv(H), po_, lo_, g)
    got = sx.replay_blocks(P, Sig, g)
    for name, a, b in zip(("poses", "landmarks", "odometry edges", "observation edges"), got, ref):
        assert a.shape == b.shape, name
        scale = np.abs(b).reshape(len(b), -1).max(1) if len(b) else np.zeros(0)
        err = np.abs(a - b).reshape(len(b), -1).max(1) if len(b) else np.zeros(0)
        assert np.all(err <= 1e-8 * np.maximum(scale, 1e-300) + 1e-300), (name, float((err / np.maximum(scale, 1e-300)).max()))
    return P


@pytest.mark.parametrize("N,M,leaf", [(50, 30, 0), (1000, 200, 0), (1000, 200, 3)])
def test_selinv_replay_matches_the_dense_inverse_on_tracks(pkg, po, bench_graphs, N, M, leaf):
    _, g = bench_graphs(N, M)
    _replay_vs_dense(pkg, po, g, leaf_poses=leaf)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_selinv_replay_matches_the_dense_inverse_on_irregular_graphs(pkg, po, seed):
    _replay_vs_dense(pkg, po, random_graph(seed))


def test_selinv_replay_with_extra_fixed_vertices(pkg, po):
    g = random_graph(7, n_poses=60, n_lms=30)
    g["fixed_poses"] = np.array([0, 17, 41], dtype=np.int32); g["fixed_landmarks"] = np.array([3, 11], dtype=np.int32)
    _replay_vs_dense(pkg, po, g)


def test_selinv_replay_with_fronts_beyond_159_scalars(pkg, po):
    P = _replay_vs_dense(pkg, po, random_graph(5, n_poses=80, n_lms=120, obs_per_pose=40, extra_pp=10))
    assert int((P.npiv + P.nbnd).max()) > 200


@pytest.mark.parametrize("K", [16, 24])
def test_selinv_replay_on_plans_with_workgroup_fronts(pkg, po, frontend, K):
    t = pkg.track.generate(300, 120, K)
    g = pkg.track.bench_graph(t, frontend)
    P = _replay_vs_dense(pkg, po, g)
    assert int((P.npiv + P.nbnd).max()) > 63


def test_a_pair_outside_the_pattern_is_reported_as_such(pkg, po, bench_graphs):
    """the replay's own rule (the host's too): a pair none of whose fronts holds both vertices is outside the pattern"""
    _, g = bench_graphs(1000, 200)
    G = pkg.Graph(device=-2); G.load_bench_graph(g); G.plan_build_host(); P = Plan(G.plan_export()); G.close()
    rows = sx.Rows(P)
    a, b = int(P.pose_gidx[5]), int(P.pose_gidx[900])
    assert rows.place(a, b) is None
    assert rows.place(a, a + 1) is not None
