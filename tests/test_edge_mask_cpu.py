"""Edge deactivation without a GPU: the C-ABI surface on host-only handles (flags, counts, every error code, the sharded refusals,
gs_find_isolated_vertex against its restatement), the checker's equivalence (tests/edge_mask_ref.py: an inactive edge is an edge with
zero information) pinned against the oracle on the graph with those edges physically left out, the condition of the GPU suite's
outlier-rejection test, and the host rules (csrc/gs_edge_mask_host.hpp) under the host sanitizers in a stand-alone program."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import edge_mask_ref as em
import robust_ref as rr
from conftest import make_oracle_graph, random_graph
import lm_ref
from test_lm_cpu import starts
from test_robust_cpu import OUTLIER_DELTA, outlier_case

NEW_FUNCS = ["gs_set_edge_active", "gs_set_edges_active", "gs_get_edges_active", "gs_activate_all_edges", "gs_num_inactive_edges",
             "gs_find_isolated_vertex", "gs_deactivate_edges_above"]
BLOCKS = ("Hpp_diag", "Hll_diag", "Hpp_off", "Hpl", "b_pose", "b_lm")
GAP_MIN = 1e-6
HUBER_ITERATIONS = 10
MASK_SEED = 21            # seed of the masks the GPU suite uses (edge_mask_ref.random_masks)
LM_ITERATIONS = 5


def refused(b, code, fn, *a):
    with pytest.raises(b.GsError) as e:
        fn(*a)
    assert e.value.code == code, (getattr(fn, "__name__", fn), a, e.value.code)
    return str(e.value)


def test_header_declares_the_calls_and_the_library_exports_them(pkg):
    names = pkg.binding.declared_symbols()
    L = pkg.binding.lib()
    for f in NEW_FUNCS:
        assert f in names, f
        assert hasattr(L, f), f
    for m in ("set_edge_active", "set_edges_active", "edges_active", "activate_all_edges", "n_inactive_edges", "find_isolated_vertex", "deactivate_edges_above"):
        assert hasattr(pkg.Graph, m), m


def test_flags_counts_and_errors_on_a_host_only_handle(pkg, bench_graphs):
    b = pkg.binding
    _, g = bench_graphs(50, 30)
    G = pkg.Graph(device=-2); G.load_bench_graph(g)
    Epp, Epl = G.n_pp, G.n_pl
    assert G.edges_active("odometry").all() and G.edges_active("observation").all() and len(G.edges_active(0)) == Epp and len(G.edges_active(1)) == Epl
    assert G.n_inactive_edges("odometry") == 0 and G.n_inactive_edges("observation") == 0
    G.set_edge_active("observation", 7, False); G.set_edge_active("odometry", 3, False); G.set_edge_active("observation", 7, False)
    assert G.n_inactive_edges(1) == 1 and G.n_inactive_edges(0) == 1
    a = G.edges_active("observation"); assert not a[7] and a.sum() == Epl - 1
    G.set_edges_active("observation", [1, 2, 7, Epl - 1])                        # active = NULL: all off
    assert G.n_inactive_edges(1) == 4 and not G.edges_active(1)[[1, 2, 7, Epl - 1]].any()
    G.set_edges_active("observation", [1, 2, 5], [True, False, False])
    assert G.n_inactive_edges(1) == 4 and np.flatnonzero(~G.edges_active(1)).tolist() == [2, 5, 7, Epl - 1]
    G.set_edge_active(1, 5, True); assert G.n_inactive_edges(1) == 3
    G.set_edges_active("odometry", []); assert G.n_inactive_edges(0) == 1
    # changing flags is not a structural change: the plan built before stays the plan
    G.plan_build_host(); before = G.plan_export()
    G.set_edge_active("observation", 11, False); G.plan_build_host()
    assert np.array_equal(G.plan_export(), before)
    G.set_edge_active("observation", 11, True)
    # errors
    refused(b, -1, G.set_edge_active, 2, 0, False); refused(b, -1, G.set_edge_active, -1, 0, False)
    refused(b, -1, G.set_edge_active, "observation", Epl, False); refused(b, -1, G.set_edge_active, "observation", -1, True); refused(b, -1, G.set_edge_active, "odometry", Epp, True)
    refused(b, -1, G.set_edges_active, "observation", [0, Epl]); refused(b, -1, G.set_edges_active, 5, [0])
    assert G.edges_active(1)[0]                                                  # all or nothing: the bulk call with a bad index changed no flag
    refused(b, -1, G.edges_active, 2); refused(b, -1, G.n_inactive_edges, 2)
    L = b.lib(); idx = (C.c_int32 * 1)(0); out = (C.c_uint8 * (Epl + 1))()
    assert L.gs_set_edge_active(None, 0, 0, 0) == -1 and L.gs_set_edges_active(None, 0, 0, None, None) == -1 and L.gs_get_edges_active(None, 0, 0, None) == -1
    assert L.gs_activate_all_edges(None) == -1 and L.gs_num_inactive_edges(None, 0) == -1 and L.gs_find_isolated_vertex(None, None, None) == -1
    assert L.gs_deactivate_edges_above(None, 0, 1.0, 0, None) == -1
    assert L.gs_set_edges_active(G.h, 1, 1, None, None) == -1 and L.gs_set_edges_active(G.h, 1, -1, idx, None) == -1 and L.gs_set_edges_active(G.h, 1, 0, None, None) == 0
    assert L.gs_get_edges_active(G.h, 1, Epl - 1, out) == -9 and L.gs_get_edges_active(G.h, 1, Epl, out) == Epl and L.gs_get_edges_active(G.h, 1, 0, None) == Epl
    # gs_deactivate_edges_above: argument errors first, then no device
    refused(b, -1, G.deactivate_edges_above, 2, 1.0); refused(b, -1, G.deactivate_edges_above, "observation", -1.0)
    for bad in (float("nan"), float("inf")):
        refused(b, -1, G.deactivate_edges_above, "observation", bad)
    refused(b, -4, G.deactivate_edges_above, "observation", 1.0); refused(b, -4, G.deactivate_edges_above, "odometry", 0.0, True)
    assert G.n_inactive_edges(1) == 3 and G.n_inactive_edges(0) == 1
    # flags survive added edges (which are active) ...
    off = np.flatnonzero(~G.edges_active(1)).tolist()
    G.add_observation_edge(4, 2, [1.0, 2.0], np.eye(2)); G.add_odometry_edge(5, 9, [0.1, 0.2, 0.0], np.eye(3))
    a = G.edges_active(1); assert len(a) == Epl + 1 and a[Epl] and np.flatnonzero(~a).tolist() == off and G.edges_active(0)[Epp] and not G.edges_active(0)[3]
    G.set_edge_active(1, Epl, False); assert G.n_inactive_edges(1) == 4
    G.activate_all_edges()
    assert G.n_inactive_edges(0) == 0 and G.n_inactive_edges(1) == 0 and G.edges_active(1).all() and G.edges_active(0).all()
    G.activate_all_edges()
    # ... and are gone after gs_clear
    G.set_edge_active(1, 3, False); G.clear()
    assert G.n_inactive_edges(1) == 0 and len(G.edges_active(1)) == 0
    G.load_bench_graph(g)
    assert G.edges_active(1).all() and G.n_inactive_edges(1) == 0
    G.close()


def test_sharded_refusals_both_ways(pkg, bench_graphs):
    b = pkg.binding
    _, g = bench_graphs(50, 30)
    G = pkg.Graph(device=-2); G.load_bench_graph(g)
    G.set_edge_active("observation", 4, False)
    msg = refused(b, -1, G.dist_configure, 0, 2); assert "inactive" in msg
    G.dist_configure(0, 1)                                                           # world 1 is not a shard
    G.activate_all_edges(); G.dist_configure(0, 2)
    refused(b, -1, G.set_edge_active, "observation", 4, False); refused(b, -1, G.set_edges_active, "odometry", [1, 2]); refused(b, -1, G.set_edges_active, "odometry", [1, 2], [True, False])
    G.set_edge_active("observation", 4, True); G.set_edges_active("odometry", [1, 2], [True, True]); G.set_edges_active("odometry", [])      # nothing switched off: accepted
    assert G.n_inactive_edges(0) == 0 and G.n_inactive_edges(1) == 0
    G.dist_configure(0, 1); G.set_edge_active("observation", 4, False); assert G.n_inactive_edges(1) == 1
    G.close()


def handle_isolated(G):
    r = G.find_isolated_vertex()
    return None if r is None else (r[0], r[1])


def test_find_isolated_vertex_agrees_with_the_restatement(pkg):
    g = random_graph(7)
    Epp, Epl = len(g["pp_i"]), len(g["pl_p"])
    G = pkg.Graph(device=-2); G.load_bench_graph(g)
    assert handle_isolated(G) is None and em.isolated_vertex(g, np.ones(Epp, bool), np.ones(Epl, bool)) is None
    rng = np.random.default_rng(11); found = 0
    for share in (0.1, 0.3, 0.5, 0.7, 0.8, 0.9, 0.95, 1.0):
        for _ in range(6):
            a_pp = rng.random(Epp) >= share; a_pl = rng.random(Epl) >= share
            G.activate_all_edges(); G.set_edges_active("odometry", np.arange(Epp), a_pp); G.set_edges_active("observation", np.arange(Epl), a_pl)
            assert np.array_equal(G.edges_active(0), a_pp) and np.array_equal(G.edges_active(1), a_pl)
            ref = em.isolated_vertex(g, a_pp, a_pl)
            assert handle_isolated(G) == ref, (share, ref)
            found += ref is not None
    assert found >= 10
    # a landmark with all its edges off (vertex ids = indices in these graphs) ...
    l = 5; assert l not in g["fixed_landmarks"]
    a_pl = np.asarray(g["pl_l"]) != l
    G.activate_all_edges(); G.set_edges_active("observation", np.flatnonzero(~a_pl))
    assert handle_isolated(G) == ("landmark", l) == em.isolated_vertex(g, np.ones(Epp, bool), a_pl)
    # ... the same landmark with a prior is not isolated ...
    G.add_landmark_prior(l, [0.0, 0.0], np.eye(2))
    assert handle_isolated(G) is None and em.isolated_vertex(g, np.ones(Epp, bool), a_pl, lm_prior=[l]) is None
    G.clear_priors(); assert handle_isolated(G) == ("landmark", l)
    # ... and neither is a fixed vertex
    f = int(g["fixed_landmarks"][0]); a_pl = np.asarray(g["pl_l"]) != f
    G.activate_all_edges(); G.set_edges_active("observation", np.flatnonzero(~a_pl))
    assert handle_isolated(G) is None and em.isolated_vertex(g, np.ones(Epp, bool), a_pl) is None
    # a pose: every edge of pose 9 off; poses are reported before landmarks
    p = 9; a_pp = (np.asarray(g["pp_i"]) != p) & (np.asarray(g["pp_j"]) != p); a_pl = (np.asarray(g["pl_p"]) != p) & (np.asarray(g["pl_l"]) != l)
    G.activate_all_edges(); G.set_edges_active("odometry", np.flatnonzero(~a_pp)); G.set_edges_active("observation", np.flatnonzero(~a_pl))
    assert handle_isolated(G) == ("pose", p) == em.isolated_vertex(g, a_pp, a_pl)
    G.add_pose_xy_prior(p, [0.0, 0.0], np.eye(2)); assert handle_isolated(G) == ("landmark", l)
    G.close()


def test_keep_connected_restatement(po):
    """the plain-Python rule on random_graph(7): with keep_connected no vertex is isolated and every skipped candidate would isolate one;
    without it every active candidate goes"""
    g = random_graph(7); Epp, Epl = len(g["pp_i"]), len(g["pl_p"])
    rng = np.random.default_rng(3)
    a_pp, a_pl = np.ones(Epp, bool), np.ones(Epl, bool); skipped = 0
    for kd, n in ((0, Epp), (1, Epl)):                                           # the observation edges on top of the odometry edges' result
        cand = rng.random(n) < 0.9
        b_pp, b_pl, off2 = em.deactivate(g, a_pp, a_pl, kd, cand, False)
        assert np.array_equal(off2, np.flatnonzero(cand)) and np.array_equal((b_pp, b_pl)[kd], ~cand)
        a_pp, a_pl, off = em.deactivate(g, a_pp, a_pl, kd, cand, True)
        assert em.isolated_vertex(g, a_pp, a_pl) is None and len(off) > 0 and cand[off].all()
        act = (a_pp, a_pl)[kd]
        for k in np.flatnonzero(cand & act):
            t = act.copy(); t[k] = False
            assert em.isolated_vertex(g, *((t, a_pl) if kd == 0 else (a_pp, t))) is not None
        skipped += len(np.flatnonzero(cand & act))
    assert skipped > 0


@pytest.mark.parametrize("name", ["bench50", "random"])
def test_zero_information_is_the_edge_left_out(po, bench_graphs, name):
    """masked(): blocks, b and chi2 of the oracle on the masked graph against the oracle on the graph with those edges physically left out
    (edge order mapped; the blocks of the masked edges exactly zero).  Bound: 1e-12 of the array's largest entry (the two sums differ by
    added zeros only), chi2 1e-12 relative."""
    g = random_graph(7) if name == "random" else bench_graphs(50, 30)[1]
    a_pp, a_pl = em.random_masks(g, 21)
    assert (~a_pp).sum() > 0 and (~a_pl).sum() > 0
    A = make_oracle_graph(po, em.masked(g, a_pp, a_pl)); B = make_oracle_graph(po, em.without(g, a_pp, a_pl))
    Ba, Bb = A.linearize_blocks(), B.linearize_blocks()
    figs = {}
    for k in BLOCKS:
        got = Ba[k]
        if k == "Hpp_off":
            assert not got[~a_pp].any(); got = got[a_pp]
        if k == "Hpl":
            assert not got[~a_pl].any(); got = got[a_pl]
        figs[k] = float(np.abs(got - Bb[k]).max() / np.abs(Bb[k]).max())
    e_chi = abs(A.chi2() - B.chi2()) / B.chi2()
    plain = make_oracle_graph(po, g).chi2()
    print("%s masked vs left out (%d + %d edges off): " % (name, (~a_pp).sum(), (~a_pl).sum()) + " ".join("%s %.2e" % kv for kv in figs.items()) + " chi2 %.2e (%.8g, unmasked %.8g)" % (e_chi, A.chi2(), plain))
    for k, v in figs.items():
        assert v <= 1e-12, k
    assert e_chi <= 1e-12 and A.chi2() < plain
    # the per-edge values of the checker with the edges' own information, masked by hand, sum to the masked oracle's chi2
    s_pp, s_pl = rr.edge_s(g, g["pose_est"], g["lm_est"]); c_pp, c_pl = rr.active(g)
    assert abs(s_pp[a_pp & c_pp].sum() + s_pl[a_pl & c_pl].sum() - A.chi2()) <= 1e-12 * A.chi2()


_huber = {}


def huber_outlier_state(po, bench_graphs):
    """outlier_case after HUBER_ITERATIONS Huber iterations (delta = OUTLIER_DELTA, observation edges, oracle IRLS): (xP, xL, graph, the
    re-targeted edges, poses, landmarks, per-edge s of the observation edges there).  Built once, left unchanged."""
    if not _huber:
        xP, xL, go, pick = outlier_case(po, bench_graphs)
        P, L, _, _ = rr.irls(po, go, {"observation": ("huber", OUTLIER_DELTA)}, HUBER_ITERATIONS, make_oracle_graph)
        _huber["x"] = (xP, xL, go, pick, P, L, rr.edge_s(go, P, L)[1])
    return _huber["x"]


def test_outlier_case_has_a_gap_to_cut_at(po, bench_graphs):
    """Condition of test_gpu_edge_mask.py's rejection test, on the CPU: after the Huber iterations the sorted per-edge s of the
    observation edges of outlier_case has, from delta^2 up (edge_mask_ref.widest_gap_threshold), a widest relative gap of at least 1e-6 —
    the test cuts at its midpoint, so a device s that differs from the checker's by rounding (1e-11) selects the same set — and cutting
    there isolates no vertex.  Measured with the committed generators: inliers up to s = 2.03e-3, re-targeted edges from 5.43e-2,
    threshold 2.82e-2, relative gap 0.963, the 400 edges above are the 400 re-targeted ones."""
    xP, xL, go, pick, P, L, s = huber_outlier_state(po, bench_graphs)
    thr, gap = em.widest_gap_threshold(s, OUTLIER_DELTA ** 2)
    above = np.flatnonzero(s > thr)
    print("outlier case after %d Huber iterations: threshold %.6g, relative gap %.3g, %d of %d edges above (%d re-targeted, %d of them above); largest below %.4g smallest above %.4g"
          % (HUBER_ITERATIONS, thr, gap, len(above), len(s), len(pick), np.isin(above, pick).sum(), s[s <= thr].max(), s[s > thr].min()))
    assert gap >= GAP_MIN and 0 < len(above) < len(s) // 2
    a_pl = np.ones(len(s), bool); a_pl[above] = False
    assert em.isolated_vertex(go, np.ones(len(go["pp_i"]), bool), a_pl) is None


def lm_mask_case(po, bench_graphs):
    """(graph, act_pp, act_pl, x1 poses, x1 landmarks): the perturbed start of test_gpu_lm.py (seed 1) with the bench 1000 / 200 masks"""
    g, _, _, P1, L1, _, _ = starts(po, bench_graphs, 1)
    a_pp, a_pl = em.random_masks(g, MASK_SEED)
    return g, a_pp, a_pl, P1, L1


def test_lm_case_condition_with_the_checker_alone(po, bench_graphs):
    """The LM trajectory the GPU suite compares: from x1 on masked(g), default parameters, five iterations.  Every trial has a margin
    >= 1e-3; the accepted chi2 is finite and non-increasing."""
    g, a_pp, a_pl, P1, L1 = lm_mask_case(po, bench_graphs)
    r = lm_ref.run(po, em.masked(g, a_pp, a_pl), LM_ITERATIONS, poses=P1, lms=L1)
    print("LM on the masked graph: trials %s, min margin %.3g\n%s" % (r["n_trials"].tolist(), r["min_margin"], lm_ref.describe(r)))
    seq = np.r_[r["chi2"], r["chi2_final"]]
    assert r["accepted"] == LM_ITERATIONS and not r["terminated"]
    assert all(t["margin"] >= lm_ref.MIN_MARGIN for t in r["trials"])
    assert np.all(np.isfinite(seq)) and np.all(np.diff(seq) <= 0)


def test_host_rules_under_address_and_undefined_sanitizers(tmp_path):
    """tests/edge_mask_san.cpp: a stand-alone program (its own main, no HIP, nothing loaded into python) over csrc/gs_edge_mask_host.hpp —
    growth of the flag store, the isolated-vertex scan and keep_connected on random graphs, the device bookkeeping — built with
    -fsanitize=address,undefined and run."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "edge_mask_san.cpp"); exe = str(tmp_path / "edge_mask_san")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "edge mask host: ok" in out.stdout, out.stdout + out.stderr
