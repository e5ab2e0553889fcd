"""Prior edges without a GPU: the checker's equivalence (tests/prior_ref.py: a prior is an edge from an auxiliary fixed pose at the
origin) pinned against plain numpy, the C-ABI surface on host-only handles, and the conditions of the trajectories that
test_gpu_prior.py compares — established here with the oracle alone."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import lm_ref
import prior_ref as pr
from conftest import make_oracle_graph, random_graph
from test_lm_cpu import starts

NEW_FUNCS = ["gs_add_pose_prior", "gs_add_pose_xy_prior", "gs_add_landmark_prior", "gs_add_pose_priors", "gs_add_pose_xy_priors",
             "gs_add_landmark_priors", "gs_num_pose_priors", "gs_num_landmark_priors", "gs_clear_priors", "gs_get_prior_chi2"]
LM_ITERATIONS = 6
SOFT_GAUGE_Z = np.array([0.3, -0.2, 0.1])                       # the strong SE2 prior that replaces the fixed flags (test 4 of the GPU suite)
SOFT_GAUGE_W = 1e4 * np.array([[2.0, 0.3, 0.1], [0.3, 1.5, -0.2], [0.1, -0.2, 1.0]])


def graph_named(bench_graphs, name):
    return random_graph(7) if name == "random" else bench_graphs(*{"bench50": (50, 30), "bench1000": (1000, 200)}[name])[1]


def gauge_free(g):
    """the graph with no fixed vertex and one strong SE2 prior on pose 0"""
    gf = dict(g, fixed_poses=np.zeros(0, dtype=np.int32), fixed_landmarks=np.zeros(0, dtype=np.int32))
    z = np.asarray(g["pose_est"], dtype=np.float64)[0] + SOFT_GAUGE_Z
    return gf, dict(pose=[(0, z, SOFT_GAUGE_W, False)], lm=[])


_lm_case = {}


def lm_case(po, bench_graphs):
    """(graph, prior set, x1 poses, x1 landmarks): the perturbed start of test_gpu_lm.py (seed 1, one Gauss-Newton step from x0) with the
    graph's prior set; run from there with the default parameters (lambda_0 = tau max diag)"""
    if not _lm_case:
        g, _, _, P1, L1, _, _ = starts(po, bench_graphs, 1)
        _lm_case["x"] = (g, pr.prior_set(g), P1, L1)
    return _lm_case["x"]


LM_REJECTION_LAMBDA0 = 1e-12
LM_REJECTION_TRIALS = [1, 1, 1, 1, 10, 1]
_lm_rejection_case = {}


def lm_rejection_case(po, bench_graphs):
    """the same with seed 2's x1 and initial_lambda = 1e-12: the checker rejects nine trials of iteration 4 and accepts its tenth"""
    if not _lm_rejection_case:
        g, _, _, P1, L1, _, _ = starts(po, bench_graphs, 2)
        _lm_rejection_case["x"] = (g, pr.prior_set(g), P1, L1)
    return _lm_rejection_case["x"]


def lm_checker(po, g, pri, P, L, iterations=LM_ITERATIONS, **kw):
    return lm_ref.run(po, pr.augment(g, pri), iterations, poses=np.vstack([P, np.zeros((1, 3))]), lms=L, **kw)


def rel_to_largest(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), np.abs(a).max(), 1e-300))


# ---------------------------------------------------------------- the equivalence
def single(kind, g):
    rng = np.random.default_rng(5)
    P, L = np.asarray(g["pose_est"]), np.asarray(g["lm_est"])
    if kind == "se2":
        return dict(pose=[(5, P[5] + [0.3, -0.4, 0.7], pr.spd(rng, 3, 0.5), False)], lm=[])
    if kind == "xy":
        z, W = pr.embed_xy(P[6, :2] + [0.2, 0.5], pr.spd(rng, 2, 0.5)); return dict(pose=[(6, z, W, True)], lm=[])
    return dict(pose=[], lm=[(4, L[4] + [-0.3, 0.25], pr.spd(rng, 2, 0.5))])


@pytest.mark.parametrize("name", ["bench50", "random"])
@pytest.mark.parametrize("which", ["se2", "xy", "lm", "set"])
def test_a_prior_is_the_edge_from_an_auxiliary_fixed_pose_at_the_origin(po, bench_graphs, name, which):
    """numpy e, J, J^T W J, -J^T W e, e^T W e of the priors against linearize_blocks() / chi2() of the augmented minus the plain oracle
    graph: 1e-12 of the largest entry of the compared array (the difference of two sums that share every other term).  One prior of
    each kind alone — its block IS the difference —, then the whole set (several priors per vertex, priors on fixed vertices)."""
    g = graph_named(bench_graphs, name)
    pri = pr.prior_set(g) if which == "set" else single(which, g)
    P, L = np.asarray(g["pose_est"], dtype=np.float64), np.asarray(g["lm_est"], dtype=np.float64)
    plain = make_oracle_graph(po, g); aug = make_oracle_graph(po, pr.augment(g, pri))
    B0 = plain.linearize_blocks(); B1 = pr.strip(aug.linearize_blocks(), g)
    Hp, bp, Hl, bl, chi = pr.contributions(g, pri, P, L)
    figs = dict(Hpp_diag=rel_to_largest(B1["Hpp_diag"] - B0["Hpp_diag"], Hp) if Hp.any() else float(np.abs(B1["Hpp_diag"] - B0["Hpp_diag"]).max()),
                b_pose=rel_to_largest(B1["b_pose"] - B0["b_pose"], bp) if bp.any() else float(np.abs(B1["b_pose"] - B0["b_pose"]).max()),
                Hll_diag=rel_to_largest(B1["Hll_diag"] - B0["Hll_diag"], Hl) if Hl.any() else float(np.abs(B1["Hll_diag"] - B0["Hll_diag"]).max()),
                b_lm=rel_to_largest(B1["b_lm"] - B0["b_lm"], bl) if bl.any() else float(np.abs(B1["b_lm"] - B0["b_lm"]).max()))
    # relative to the largest entry of the arrays the difference was taken of
    scale = {k: max(np.abs(B1[k]).max(), 1e-300) for k in figs}
    abs_err = dict(Hpp_diag=np.abs(B1["Hpp_diag"] - B0["Hpp_diag"] - Hp).max(), b_pose=np.abs(B1["b_pose"] - B0["b_pose"] - bp).max(),
                   Hll_diag=np.abs(B1["Hll_diag"] - B0["Hll_diag"] - Hl).max(), b_lm=np.abs(B1["b_lm"] - B0["b_lm"] - bl).max())
    e_chi = abs((aug.chi2() - plain.chi2()) - chi) / aug.chi2()
    print("%s %s: " % (name, which) + " ".join("%s %.2e" % (k, abs_err[k] / scale[k]) for k in figs) + " chi2 %.2e (prior share %.4g of %.6g)" % (e_chi, chi, aug.chi2()))
    for k in figs:
        assert abs_err[k] <= 1e-12 * scale[k], k
    assert e_chi <= 1e-12
    assert np.array_equal(B1["Hpp_off"], B0["Hpp_off"]) and np.array_equal(B1["Hpl"], B0["Hpl"])      # no off-diagonal block moves
    if which != "set":
        (tp, tl) = pr.terms(pri, P, L); e, J, H, b, c = (tp + tl)[0]
        if which == "lm":
            assert np.array_equal(J, np.eye(2)) and np.allclose(H, pri["lm"][0][2], rtol=0, atol=0)
        if which == "xy":
            assert np.array_equal(J, np.eye(3)) and np.array_equal(e[:2], P[6, :2] - pri["pose"][0][1][:2]) and H[2].tolist() == [0, 0, 0] and b[2] == 0
        if which == "se2":
            z = pri["pose"][0][1]; c_, s_ = np.cos(z[2]), np.sin(z[2])
            assert np.allclose(J, [[c_, s_, 0], [-s_, c_, 0], [0, 0, 1]], rtol=0, atol=0)


# ---------------------------------------------------------------- C-ABI on host-only handles
def test_header_declares_the_priors_and_the_library_exports_them(pkg):
    names = pkg.binding.declared_symbols()
    L = pkg.binding.lib()
    for f in NEW_FUNCS:
        assert f in names, f
        assert hasattr(L, f), f
    st = pkg.binding.Stats()
    assert hasattr(st, "n_pose_priors") and hasattr(st, "n_landmark_priors")


def test_abi_on_a_host_only_handle(pkg, bench_graphs):
    b = pkg.binding
    _, g = bench_graphs(50, 30)
    G = pkg.Graph(device=-2); G.load_bench_graph(g)
    I3 = np.eye(3); I2 = np.eye(2)
    assert G.n_pose_priors == 0 and G.n_landmark_priors == 0
    G.add_pose_prior(3, [1, 2, 0.5], 2 * I3); G.add_pose_xy_prior(4, [1, 2], I2); G.add_landmark_prior(5, [0, 1], I2)
    G.add_pose_prior(0, [0, 0, 0], I3); G.add_landmark_prior(0, [0, 0], I2)          # fixed vertices: accepted
    G.add_pose_prior(3, [1, 2, 0.6], I3)                                             # a second one on the same pose
    assert G.n_pose_priors == 4 and G.n_landmark_priors == 2                         # XY priors count as pose priors
    G.add_pose_priors([7, 8], [[0, 0, 0], [1, 1, 1]], [I3, I3]); G.add_pose_xy_priors([9], [[0, 0]], [I2]); G.add_landmark_priors([6, 7], [[0, 0], [1, 1]], [I2, I2])
    assert G.n_pose_priors == 7 and G.n_landmark_priors == 4
    # adding priors is not a structural change: the plan built before stays the plan
    G.plan_build_host(); before = G.plan_export()
    G.add_pose_xy_prior(10, [0, 0], I2); G.plan_build_host()
    assert np.array_equal(G.plan_export(), before)
    st = G.stats()
    assert st.n_pose_priors == 8 and st.n_landmark_priors == 4 and st.struct_size == C.sizeof(b.Stats)
    # errors
    def refused(code, fn, *a):
        with pytest.raises(b.GsError) as e:
            fn(*a)
        assert e.value.code == code, (fn.__name__, a, e.value.code)
    refused(-3, G.add_pose_prior, 10 ** 6, [0, 0, 0], I3); refused(-3, G.add_pose_xy_prior, -7, [0, 0], I2); refused(-3, G.add_landmark_prior, 10 ** 6, [0, 0], I2)
    refused(-3, G.add_pose_priors, [3, 10 ** 6], [[0, 0, 0]] * 2, [I3, I3])
    for bad in (float("nan"), float("inf")):
        refused(-1, G.add_pose_prior, 3, [bad, 0, 0], I3); refused(-1, G.add_pose_prior, 3, [0, 0, bad], I3)
        refused(-1, G.add_pose_xy_prior, 3, [0, bad], I2); refused(-1, G.add_landmark_prior, 3, [bad, 0], I2)
    asym3 = I3.copy(); asym3[0, 1] = 0.5; asym2 = I2.copy(); asym2[1, 0] = 0.25
    refused(-1, G.add_pose_prior, 3, [0, 0, 0], asym3); refused(-1, G.add_pose_xy_prior, 3, [0, 0], asym2); refused(-1, G.add_landmark_prior, 3, [0, 0], asym2)
    nan3 = I3.copy(); nan3[0, 1] = nan3[1, 0] = float("nan")
    refused(-1, G.add_pose_prior, 3, [0, 0, 0], nan3)
    L = b.lib(); z = (C.c_double * 3)(0, 0, 0); w = (C.c_double * 9)(*I3.reshape(9)); ids = (C.c_int32 * 1)(3)
    assert L.gs_add_pose_prior(G.h, 3, None, w) == -1 and L.gs_add_pose_prior(G.h, 3, z, None) == -1 and L.gs_add_pose_prior(None, 3, z, w) == -1
    assert L.gs_add_pose_xy_prior(G.h, 3, None, w) == -1 and L.gs_add_landmark_prior(G.h, 3, z, None) == -1
    assert L.gs_add_pose_priors(G.h, 1, ids, z, None) == -1 and L.gs_add_pose_xy_priors(G.h, 1, None, z, w) == -1 and L.gs_add_landmark_priors(G.h, 1, ids, None, w) == -1
    assert L.gs_num_pose_priors(None) == -1 and L.gs_num_landmark_priors(None) == -1 and L.gs_clear_priors(None) == -1 and L.gs_get_prior_chi2(None, 0, 0, None) == -1
    assert G.n_pose_priors == 9 and G.n_landmark_priors == 4                         # (the bulk call that failed on its second id kept its first)
    refused(-4, G.prior_chi2, "pose"); refused(-4, G.prior_chi2, 1)                  # GS_ERR_NO_DEVICE
    assert L.gs_get_prior_chi2(G.h, 2, 0, None) == -1
    # shards: refused in both orders
    refused(-1, G.dist_configure, 0, 2)
    G.dist_configure(0, 1)                                                           # world 1 is not a shard
    G.clear_priors()
    assert G.n_pose_priors == 0 and G.n_landmark_priors == 0 and G.n_poses == 50      # nothing else goes
    G.dist_configure(0, 2)
    refused(-1, G.add_pose_prior, 3, [0, 0, 0], I3); refused(-1, G.add_pose_xy_prior, 3, [0, 0], I2); refused(-1, G.add_landmark_prior, 3, [0, 0], I2)
    assert G.n_pose_priors == 0
    G.dist_configure(0, 1)
    G.add_pose_prior(3, [0, 0, 0], I3); G.add_landmark_prior(5, [0, 1], I2)
    G.clear()                                                                        # gs_clear drops them with their vertices
    assert G.n_pose_priors == 0 and G.n_landmark_priors == 0 and G.n_poses == 0
    G.close()


# ---------------------------------------------------------------- the conditions of the compared trajectories
@pytest.mark.parametrize("name", ["bench50", "bench1000"])
def test_gauge_free_case_converges_with_the_oracle_alone(po, bench_graphs, name):
    """No fixed vertex, one strong SE2 prior on pose 0: ten oracle Gauss-Newton iterations on the augmented graph; chi2 at the
    linearisation points finite and non-increasing."""
    gf, pri = gauge_free(graph_named(bench_graphs, name))
    og = make_oracle_graph(po, pr.augment(gf, pri)); done, chi, _ = og.optimize(10, ordering=1)
    seq = np.r_[chi, og.chi2()]
    print("%s gauge-free: chi2 %s" % (name, " ".join("%.8g" % v for v in seq)))
    assert done == 10 and np.all(np.isfinite(seq)) and np.all(np.diff(seq) <= 1e-9 * seq[:-1])


@pytest.mark.parametrize("name", ["bench50", "bench1000", "track400_K16"])
def test_prior_set_case_converges_with_the_oracle_alone(pkg, po, frontend, bench_graphs, name):
    """The graphs whose optimize(10) trajectory the GPU suite compares, with their prior sets.  (random_graph(7) is not among them: its
    measurements are random, Gauss-Newton wanders on it — chi2 9 064, 8 915, 9 884, 9 537, 10 857 ... — with or without priors; the GPU
    suite compares its system, chi2 and ONE step's increment.)"""
    g = pkg.track.bench_graph(pkg.track.generate(400, 150, 16), frontend) if name == "track400_K16" else graph_named(bench_graphs, name)
    pri = pr.prior_set(g)
    og = make_oracle_graph(po, pr.augment(g, pri)); done, chi, _ = og.optimize(10, ordering=1)
    seq = np.r_[chi, og.chi2()]
    print("%s with its prior set: chi2 %s" % (name, " ".join("%.8g" % v for v in seq)))
    assert done == 10 and np.all(np.isfinite(seq)) and np.all(np.diff(seq) <= 1e-9 * seq[:-1])


def test_lm_case_condition_with_the_checker_alone(po, bench_graphs):
    """The LM trajectory the GPU suite compares: from x1 (test_lm_cpu.starts, seed 1) with the bench 1000 / 200 prior set, default
    parameters, six iterations.  Every trial has a margin >= 1e-3; the accepted chi2 is finite and non-increasing."""
    g, pri, P1, L1 = lm_case(po, bench_graphs)
    r = lm_checker(po, g, pri, P1, L1)
    print("LM with priors: trials %s, min margin %.3g\n%s" % (r["n_trials"].tolist(), r["min_margin"], lm_ref.describe(r)))
    seq = np.r_[r["chi2"], r["chi2_final"]]
    assert r["accepted"] == LM_ITERATIONS and not r["terminated"]
    assert all(t["margin"] >= lm_ref.MIN_MARGIN for t in r["trials"])
    assert np.all(np.isfinite(seq)) and np.all(np.diff(seq) <= 0)


def test_lm_rejection_case_condition_with_the_checker_alone(po, bench_graphs):
    """The rejected-trial trajectory the GPU suite compares: seed 2's x1 with the prior set, initial_lambda = 1e-12, six iterations.
    Measured with the committed generators: trials per iteration [1, 1, 1, 1, 10, 1], nine rejections, smallest margin 2.5e-2; chi2 at the
    accepted points 919 834 -> 16 090 -> 3 678 -> 1 919 -> 1 738 -> 1 490 -> 1 450.  Asserted: the counts, margin >= 1e-3 on EVERY
    trial, a finite and decreasing accepted chi2."""
    g, pri, P1, L1 = lm_rejection_case(po, bench_graphs)
    r = lm_checker(po, g, pri, P1, L1, initial_lambda=LM_REJECTION_LAMBDA0)
    print("LM with priors, rejections: trials %s, min margin %.3g\n%s" % (r["n_trials"].tolist(), r["min_margin"], lm_ref.describe(r)))
    seq = np.r_[r["chi2"], r["chi2_final"]]
    assert r["n_trials"].tolist() == LM_REJECTION_TRIALS and r["rejected"] == 9 and r["accepted"] == LM_ITERATIONS and not r["terminated"]
    assert all(t["margin"] >= lm_ref.MIN_MARGIN for t in r["trials"])
    assert np.all(np.isfinite(seq)) and np.all(np.diff(seq) < 0)


# ---------------------------------------------------------------- the host table builder under the sanitizers
def test_host_table_builder_under_address_and_undefined_sanitizers(tmp_path):
    """tests/prior_tables_san.cpp: a stand-alone program (its own main, no HIP, nothing loaded into python) over csrc/gs_prior_host.hpp —
    grouping by vertex, structure-of-arrays packing, the refusals, the upload rule — built with -fsanitize=address,undefined and run."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "prior_tables_san.cpp"); exe = str(tmp_path / "prior_tables_san")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "prior tables: ok" in out.stdout, out.stdout + out.stderr
