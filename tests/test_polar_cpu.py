"""Polar observation edges without a GPU: the checker's equivalence (tests/polar_ref.py: at given estimates a polar edge is the Cartesian
edge with information Jd^T Omega Jd and measurement d - Jd^-1 e) pinned against plain numpy, the analytic Jacobians against central
differences, the C-ABI surface on host-only handles, the host tables under the sanitizers, and the conditions of the trajectories that
test_gpu_polar.py compares — established here with the oracle alone."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import lm_ref
import polar_ref as plr
import robust_ref as rr
from conftest import make_oracle_graph, random_graph
from test_lm_cpu import starts

NEW_FUNCS = ["gs_add_range_bearing_edge", "gs_add_bearing_edge", "gs_add_range_bearing_edges", "gs_add_bearing_edges", "gs_num_polar_edges",
             "gs_get_polar_edges"]
LM_ITERATIONS = 6
START_SIGMA = (0.05, 0.005)                                      # metres (poses and cones), radians


def graph_named(bench_graphs, name):
    return random_graph(7) if name == "random" else bench_graphs(*{"bench50": (50, 30), "bench1000": (1000, 200)}[name])[1]


def start_of(g):
    """the estimates the compared trajectories start from: the graph's own perturbed by N(0, 0.05 m) in position (poses and cones) and
    N(0, 0.005 rad) in heading, seed 11"""
    rng = np.random.default_rng(11)
    P = np.array(g["pose_est"], dtype=np.float64) + rng.normal(0, 1, np.shape(g["pose_est"])) * [START_SIGMA[0], START_SIGMA[0], START_SIGMA[1]]
    L = np.array(g["lm_est"], dtype=np.float64) + rng.normal(0, START_SIGMA[0], np.shape(g["lm_est"]))
    return P, L


_lm_case = {}


def lm_case(po, bench_graphs):
    """(graph, polar set, x1 poses, x1 landmarks): the perturbed start of test_gpu_lm.py (seed 1, one Gauss-Newton step from x0)"""
    if not _lm_case:
        g, _, _, P1, L1, _, _ = starts(po, bench_graphs, 1)
        _lm_case["x"] = (g, plr.polar_set(g), P1, L1)
    return _lm_case["x"]


# ---------------------------------------------------------------- the equivalence
@pytest.mark.parametrize("name", ["bench50", "random", "bench1000"])
@pytest.mark.parametrize("kernel", [None, "huber"])
def test_terms_match_the_oracle_on_the_cartesianised_graph(po, bench_graphs, name, kernel):
    """numpy A^T W A, A^T W B, B^T W B, -A^T W e, -B^T W e, rho(s) of the polar edges against linearize_blocks() / chi2 of the oracle on
    cartesianised() minus the oracle on the carriers (the same graph with zero information on the polar edges): 1e-12 of the largest
    entry of the compared array — the bound of test_prior_cpu.py."""
    g = graph_named(bench_graphs, name); pol = plr.polar_set(g)
    P, L = start_of(g)
    kernels = {"observation": ("huber", float(np.median(np.sqrt(plr.edge_s(g, pol, P, L)))))} if kernel else None
    full = plr.oracle_at(po, g, pol, P, L, kernels).linearize_blocks()
    gc = plr.carriers(g, pol, P, L)
    base = make_oracle_graph(po, rr.reweighted(gc, P, L, kernels) if kernels else gc).linearize_blocks()
    con = plr.contributions(g, pol, P, L, kernels)
    figs = {k: float(np.abs(full[k] - base[k] - con[k]).max() / np.abs(full[k]).max()) for k in ("Hpp_diag", "Hll_diag", "Hpl", "b_pose", "b_lm")}
    chi_full = plr.chi2_at(po, g, pol, P, L, kernels)
    chi_base = rr.robust_chi2(gc, P, L, kernels) if kernels else make_oracle_graph(po, gc).chi2()
    e_chi = abs(chi_full - chi_base - con["chi2"]) / chi_full
    print("%s %s: " % (name, kernel) + " ".join("%s %.2e" % kv for kv in figs.items()) + " chi2 %.2e (polar share %.6g of %.6g; %d polar edges of %d)"
          % (e_chi, con["chi2"], chi_full, len(pol["idx"]), len(g["pl_p"])))
    for k, v in figs.items():
        assert v <= 1e-12, k
    assert e_chi <= 1e-12 and con["chi2"] > 0
    assert np.array_equal(full["Hpp_off"], base["Hpp_off"])
    other = np.ones(len(g["pl_p"]), dtype=bool); other[pol["idx"]] = False
    assert np.array_equal(full["Hpl"][other], base["Hpl"][other]) and np.abs(con["Hpl"][pol["idx"]]).max() > 0
    if kernel:
        assert (rr.weight(kernels["observation"], plr.terms(g, pol, P, L)["s"]) < 1).any()


def test_jacobians_match_central_differences():
    """A and B of terms() against central differences of e (h = 1e-6) over 2000 random edges: within 1e-6 of max(1, |J|) — an error in an
    entry is O(1), the noise of the differences is ~1e-9.  The theta column of A is exactly (0, -1)."""
    rng = np.random.default_rng(3); n = 2000
    P = np.c_[rng.uniform(-20, 20, (n, 2)), rng.uniform(-4, 4, n)]
    rad = rng.uniform(0.5, 25, n); ang = rng.uniform(-np.pi, np.pi, n)
    L = P[:, :2] + np.c_[rad * np.cos(ang), rad * np.sin(ang)]
    g = dict(pl_p=np.arange(n), pl_l=np.arange(n), fixed_poses=[], fixed_landmarks=[])
    pol = dict(idx=np.arange(n), model=np.ones(n, dtype=np.int32), z=np.c_[rng.uniform(0.5, 25, n), rng.uniform(-np.pi, np.pi, n)], W=np.tile(np.eye(2), (n, 1, 1)))
    t = plr.terms(g, pol, P, L)
    h = 1e-6; worst = 0.0
    def diff(x_plus, x_minus):
        d = plr.terms(g, pol, *x_plus)["e"] - plr.terms(g, pol, *x_minus)["e"]
        d[:, 1] = rr.normalize_theta(d[:, 1])
        return d / (2 * h)
    for c in range(3):
        dP = np.zeros_like(P); dP[:, c] = h
        num = diff((P + dP, L), (P - dP, L))
        worst = max(worst, float((np.abs(num - t["A"][:, :, c]) / np.maximum(1.0, np.abs(t["A"][:, :, c]))).max()))
    for c in range(2):
        dL = np.zeros_like(L); dL[:, c] = h
        num = diff((P, L + dL), (P, L - dL))
        worst = max(worst, float((np.abs(num - t["B"][:, :, c]) / np.maximum(1.0, np.abs(t["B"][:, :, c]))).max()))
    print("analytic Jacobians against central differences over %d edges: worst %.2e" % (n, worst))
    assert worst <= 1e-6
    assert np.all(t["A"][:, 0, 2] == 0.0) and np.all(t["A"][:, 1, 2] == -1.0)


def test_bearing_only_is_the_range_bearing_edge_with_the_embedded_omega(bench_graphs):
    """bit for bit: contributions of a bearing-only set (z_r = 0, Omega = [[0, 0], [0, w]]) and of the same entries marked range-bearing"""
    g = graph_named(bench_graphs, "bench50"); pol = plr.polar_set(g)
    b = plr.subset(pol, pol["model"] == plr.BEARING)
    assert len(b["idx"]) > 0 and np.all(b["z"][:, 0] == 0) and np.all(b["W"][:, 0, :] == 0) and np.all(b["W"][:, :, 0] == 0) and np.all(b["W"][:, 1, 1] > 0)
    as_rb = dict(b, model=np.full(len(b["idx"]), plr.RANGE_BEARING, dtype=np.int32))
    P, L = start_of(g)
    c0, c1 = plr.contributions(g, b, P, L), plr.contributions(g, as_rb, P, L)
    for k in ("Hpp_diag", "Hll_diag", "Hpl", "b_pose", "b_lm"):
        assert np.array_equal(c0[k], c1[k]), k
    assert c0["chi2"] == c1["chi2"]
    g0, g1 = plr.cartesianised(g, b, P, L), plr.cartesianised(g, as_rb, P, L)
    assert np.array_equal(g0["pl_info"], g1["pl_info"])
    # (the Cartesian measurement differs — e_r := 0 for the bearing-only model keeps it near the cone — and does not matter: Omega's range row is zero)
    s0 = rr.edge_s(g0, P, L)[1][b["idx"]]; s1 = rr.edge_s(g1, P, L)[1][b["idx"]]
    assert np.abs(s0 - s1).max() <= 1e-9 * np.abs(s0).max()


# ---------------------------------------------------------------- the conditions of the compared trajectories
@pytest.mark.parametrize("name", ["bench50", "bench1000"])
def test_compared_trajectories_converge_in_the_checker(po, bench_graphs, name):
    """ten undamped iterations from start_of(): the last two chi2 agree to 1e-9 relative"""
    g = graph_named(bench_graphs, name); pol = plr.polar_set(g)
    P0, L0 = start_of(g)
    P, L, chi, _, chi_end = plr.gauss_newton(po, g, pol, 10, P0, L0)
    seq = np.r_[chi, chi_end]
    print("%s with its polar set (%d range-bearing, %d bearing-only of %d): chi2 %s" % (name, (pol["model"] == 1).sum(), (pol["model"] == 2).sum(), len(g["pl_p"]),
                                                                                       " ".join("%.8g" % v for v in seq)))
    assert np.all(np.isfinite(seq)) and abs(seq[-1] - seq[-2]) <= 1e-9 * seq[-1]


def test_lm_restatement_is_lm_ref_on_a_graph_without_polar_edges(po, bench_graphs):
    """lm_run over polar_ref.system_at against lm_ref.run on a graph WITHOUT polar edges: identical logs"""
    g, _, _, P1, L1, _, _ = starts(po, bench_graphs, 1)
    a = lm_ref.run(po, g, 3, poses=P1, lms=L1); b = plr.lm_run(po, g, plr.empty_set(), 3, poses=P1, lms=L1)
    assert a["n_trials"].tolist() == b["n_trials"].tolist() and np.array_equal(a["chi2"], b["chi2"]) and np.array_equal(a["lam"], b["lam"])
    assert np.array_equal(a["P"], b["P"]) and np.array_equal(a["L"], b["L"]) and a["chi2_final"] == b["chi2_final"] and a["lambda_final"] == b["lambda_final"]
    for ta, tb in zip(a["trials"], b["trials"]):
        assert ta["chi_old"] == tb["chi_old"] and ta["chi_new"] == tb["chi_new"] and ta["rho"] == tb["rho"] and ta["accepted"] == tb["accepted"]


def test_lm_case_condition_with_the_checker_alone(po, bench_graphs):
    """The LM trajectory the GPU suite compares: from x1 (test_lm_cpu.starts, seed 1) with the bench 1000 / 200 polar set, default
    parameters, six iterations.  Every trial has a margin >= lm_ref.MIN_MARGIN."""
    g, pol, P1, L1 = lm_case(po, bench_graphs)
    r = plr.lm_run(po, g, pol, LM_ITERATIONS, poses=P1, lms=L1)
    print("LM with polar edges: trials %s, min margin %.3g\n%s" % (r["n_trials"].tolist(), r["min_margin"], lm_ref.describe(r)))
    assert not r["terminated"] and all(t["margin"] >= lm_ref.MIN_MARGIN for t in r["trials"])
    assert np.all(np.isfinite(np.r_[r["chi2"], r["chi2_final"]]))


# ---------------------------------------------------------------- C-ABI on host-only handles
def test_header_declares_the_polar_edges_and_the_library_exports_them(pkg):
    names = pkg.binding.declared_symbols()
    L = pkg.binding.lib()
    for f in NEW_FUNCS:
        assert f in names, f
        assert hasattr(L, f), f


def test_abi_on_a_host_only_handle(pkg, bench_graphs):
    b = pkg.binding
    _, g = bench_graphs(50, 30)
    G = pkg.Graph(device=-2); G.load_bench_graph(g)
    E0 = len(g["pl_p"]); I2 = np.eye(2)
    assert G.num_polar_edges() == 0 and G.n_pl == E0
    G.add_range_bearing_edge(3, 5, [2.0, 0.5], [[4.0, 0.1], [0.1, 9.0]])
    G.add_bearing_edge(4, 5, 7.0, 3.0)                                              # (z_beta is normalised when stored; any finite value goes)
    G.add_observation_edge(4, 6, [1, 2], I2)                                         # a Cartesian edge in between takes its own index
    G.add_range_bearing_edges([5, 6], [7, 8], [[1.0, 0.1], [0.0, -0.2]], [I2, 2 * I2])   # z_r = 0 is allowed
    G.add_bearing_edges([7, 0], [9, 0], [0.3, -0.3], [1.0, 0.0])                     # information 0 is allowed; fixed vertices are accepted
    idx, model = G.polar_edges()
    assert G.num_polar_edges() == 6 and idx.tolist() == [E0, E0 + 1, E0 + 3, E0 + 4, E0 + 5, E0 + 6] and model.tolist() == [1, 2, 1, 1, 2, 2]
    assert G.n_pl == E0 + 7                                                          # gs_num_observation_edges counts the carriers
    L = b.lib()
    assert L.gs_get_polar_edges(G.h, 0, None, None) == 6                             # either pointer may be NULL
    one = (C.c_int32 * 6)()
    assert L.gs_get_polar_edges(G.h, 6, one, None) == 6 and list(one) == idx.tolist()
    assert L.gs_get_polar_edges(G.h, 6, None, one) == 6 and list(one) == model.tolist()
    assert L.gs_get_polar_edges(G.h, 5, one, None) == -9                             # GS_ERR_CAPACITY
    # a polar edge is an observation edge: the flag calls name it by its observation index
    G.set_edge_active("observation", E0 + 1, False); assert G.n_inactive_edges("observation") == 1 and not G.edges_active("observation")[E0 + 1]
    G.activate_all_edges()
    G.plan_build_host()                                                              # the structure phase takes the carriers like any observation edge
    # errors: each refused edge leaves no carrier behind
    def refused(code, fn, *a):
        n_pl, n_pol = G.n_pl, G.num_polar_edges()
        with pytest.raises(b.GsError) as e:
            fn(*a)
        assert e.value.code == code, (fn.__name__, a, e.value.code)
        assert G.n_pl == n_pl and G.num_polar_edges() == n_pol, (fn.__name__, a)
    refused(-3, G.add_range_bearing_edge, 10 ** 6, 5, [1, 0], I2); refused(-3, G.add_range_bearing_edge, 3, 10 ** 6, [1, 0], I2)
    refused(-3, G.add_bearing_edge, -7, 5, 0.1, 1.0); refused(-3, G.add_bearing_edge, 3, 10 ** 6, 0.1, 1.0)
    for bad in (float("nan"), float("inf"), -float("inf")):
        refused(-1, G.add_range_bearing_edge, 3, 5, [bad, 0], I2); refused(-1, G.add_range_bearing_edge, 3, 5, [1, bad], I2)
        refused(-1, G.add_bearing_edge, 3, 5, bad, 1.0); refused(-1, G.add_bearing_edge, 3, 5, 0.1, bad)
        W = I2.copy(); W[0, 0] = bad; refused(-1, G.add_range_bearing_edge, 3, 5, [1, 0], W)
        W = I2.copy(); W[0, 1] = W[1, 0] = bad; refused(-1, G.add_range_bearing_edge, 3, 5, [1, 0], W)
    refused(-1, G.add_range_bearing_edge, 3, 5, [-1e-9, 0], I2)                      # z_r < 0
    refused(-1, G.add_bearing_edge, 3, 5, 0.1, -1e-9)                                # omega < 0
    asym = I2.copy(); asym[1, 0] = 0.25
    refused(-1, G.add_range_bearing_edge, 3, 5, [1, 0], asym)
    z = (C.c_double * 2)(1, 0); w = (C.c_double * 4)(1, 0, 0, 1); ids = (C.c_int32 * 1)(3); n0, p0 = G.n_pl, G.num_polar_edges()
    assert L.gs_add_range_bearing_edge(G.h, 3, 5, None, w) == -1 and L.gs_add_range_bearing_edge(G.h, 3, 5, z, None) == -1
    assert L.gs_add_range_bearing_edge(None, 3, 5, z, w) == -1 and L.gs_add_bearing_edge(None, 3, 5, 0.1, 1.0) == -1
    assert L.gs_add_range_bearing_edges(G.h, 1, None, ids, z, w) == -1 and L.gs_add_range_bearing_edges(G.h, 1, ids, None, z, w) == -1
    assert L.gs_add_range_bearing_edges(G.h, 1, ids, ids, None, w) == -1 and L.gs_add_range_bearing_edges(G.h, 1, ids, ids, z, None) == -1      # information is required
    assert L.gs_add_bearing_edges(G.h, 1, None, ids, z, w) == -1 and L.gs_add_bearing_edges(G.h, 1, ids, None, z, w) == -1
    assert L.gs_add_bearing_edges(G.h, 1, ids, ids, None, w) == -1 and L.gs_add_bearing_edges(G.h, 1, ids, ids, z, None) == -1
    assert L.gs_num_polar_edges(None) == -1 and L.gs_get_polar_edges(None, 0, None, None) == -1
    assert G.n_pl == n0 and G.num_polar_edges() == p0
    # a bulk call that fails on its second edge keeps its first
    with pytest.raises(b.GsError) as e:
        G.add_bearing_edges([3, 10 ** 6], [5, 5], [0.1, 0.2], [1.0, 1.0])
    assert e.value.code == -3 and G.num_polar_edges() == p0 + 1 and G.n_pl == n0 + 1
    # the computing calls on a host-only handle: GS_ERR_NO_DEVICE as before
    refused(-4, G.chi2); refused(-4, G.edge_chi2, "observation")
    # shards: refused in both orders
    refused(-1, G.dist_configure, 0, 2)
    G.dist_configure(0, 1)                                                           # world 1 is not a shard
    G.clear()                                                                        # gs_clear drops the polar edges with everything else
    assert G.num_polar_edges() == 0 and G.n_pl == 0 and G.n_poses == 0
    G.load_bench_graph(g); G.dist_configure(0, 2)
    refused(-1, G.add_range_bearing_edge, 3, 5, [1, 0], I2); refused(-1, G.add_bearing_edge, 3, 5, 0.1, 1.0)
    G.dist_configure(0, 1)
    G.add_bearing_edge(3, 5, 0.1, 1.0)
    assert G.num_polar_edges() == 1 and G.polar_edges()[0].tolist() == [E0]
    G.close()


# ---------------------------------------------------------------- the host tables under the sanitizers
def test_host_tables_under_address_and_undefined_sanitizers(tmp_path):
    """tests/polar_tables_san.cpp: a stand-alone program (its own main, no HIP, nothing loaded into python) over csrc/gs_polar_host.hpp —
    the empty store, a pose with many edges, tail locations, inactive flags, the refusals, the upload rule — built with
    -fsanitize=address,undefined and run."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "polar_tables_san.cpp"); exe = str(tmp_path / "polar_tables_san")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "polar tables: ok" in out.stdout, out.stdout + out.stderr
