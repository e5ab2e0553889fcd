"""Polar observation edges on the GPU (gs_add_range_bearing_edge / gs_add_bearing_edge, csrc/gs_polar.hip) against the checker
tests/polar_ref.py: the UNCHANGED CPU oracle on the graph whose polar edges are rewritten, at the estimates in question, as the
Cartesian edges that are equivalent there (test_polar_cpu.py pins that equivalence against plain numpy and central differences and
establishes, without a GPU, that the compared trajectories converge and that every compared LM trial has a margin >= 1e-3).

Tolerances are the project's existing bars: H / b arrays 1e-11 of the array's largest entry, chi2 and estimates 1e-9, per-edge s 1e-11 of
the largest, increments 1e-8 of the largest increment (1e-9 on the random graph), LM max(4 x the plain gs_optimize yardstick, 1e-9),
marginals REL of test_gpu_marginals.py.  Every test prints its figures before it asserts (-s); the printed run is
profiles/polar_gpu_suite.txt.

Polar set per graph (polar_ref.polar_set): a third of the observation edges range-bearing, a seventh bearing-only, z taken from the
Cartesian z, Omega_bb scaled by r^2 and the cross terms by r; all edges of one cone polar, all edges of one pose polar, one polar edge on
a fixed cone and one on the fixed pose (where the graph has them).  The bench graphs start from test_polar_cpu.start_of()."""
import numpy as np
import pytest

import lm_ref
import polar_ref as plr
import prior_ref as pr
import robust_ref as rr
import selinv_exec as sx
from conftest import make_oracle_graph, random_graph, split_for_growth
from test_gpu_marginals import REL, rel_err
from test_polar_cpu import LM_ITERATIONS, lm_case, start_of

pytestmark = pytest.mark.gpu


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300))


def fresh(pkg, g, pol=None, debug=None, **kw):
    G = pkg.Graph(device=0, debug=debug, **kw)
    return plr.load(G, g, pol if pol is not None else plr.empty_set())


_graphs = {}
NAMES = ["bench50", "bench1000", "random", "track400_K16"]


def graph_of(pkg, bench_graphs, frontend, name):
    """(graph at its start estimates, its polar set), built once per name and left unchanged"""
    if name not in _graphs:
        if name == "random":
            g = random_graph(7)
        elif name == "track400_K16":
            g = pkg.track.bench_graph(pkg.track.generate(400, 150, 16), frontend)
        else:
            g = bench_graphs(*{"bench50": (50, 30), "bench1000": (1000, 200)}[name])[1]
        if name != "random":
            P, L = start_of(g); g = dict(g, pose_est=P, lm_est=L)
        _graphs[name] = (g, plr.polar_set(g))
    return _graphs[name]


_gn = {}


def checker_run(po, name, g, pol, iterations):
    """the checker's Gauss-Newton trajectory, computed once per (graph, length)"""
    if (name, iterations) not in _gn:
        _gn[(name, iterations)] = plr.gauss_newton(po, g, pol, iterations)
    return _gn[(name, iterations)]


# ---------------------------------------------------------------- 1. the system
@pytest.mark.parametrize("gather", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_system_with_polar_edges_matches_the_checker(pkg, po, bench_graphs, frontend, name, gather):
    """linearize() + export_system(): every array against the oracle on the cartesianised graph (1e-11 of the array's largest entry);
    the off-diagonal pose-pose blocks bit-identical to a handle loaded with the Cartesian carriers only, whose H_pl rows of the polar
    edges are zero.  bench50: fewer than 256 carrying poses (the one-launch chi2 total); bench1000: more (two launches)."""
    g, pol = graph_of(pkg, bench_graphs, frontend, name)
    ref = plr.oracle_at(po, g, pol, g["pose_est"], g["lm_est"]).linearize_blocks()
    G = fresh(pkg, g, pol, linearize_gather=gather)
    G.linearize(); S = G.export_system()
    figs = {k: rel(S[k], ref[k]) for k in ref}
    C = fresh(pkg, plr.carriers(g, pol), linearize_gather=gather); C.linearize(); S0 = C.export_system()
    n_carrying = len(np.unique(np.asarray(g["pl_p"])[pol["idx"]]))
    print("%s gather=%d: " % (name, gather) + " ".join("%s %.2e" % kv for kv in figs.items()) + " | %d polar edges on %d poses" % (len(pol["idx"]), n_carrying))
    assert G.num_polar_edges() == len(pol["idx"]) and np.array_equal(G.polar_edges()[0], pol["idx"]) and np.array_equal(G.polar_edges()[1], pol["model"])
    for k, v in figs.items():
        assert v < 1e-11, k
    assert np.array_equal(S["Hpp_off"], S0["Hpp_off"])
    assert np.abs(S0["Hpl"][pol["idx"]]).max() == 0.0 and np.abs(S["Hpl"][pol["idx"]]).max() > 0
    other = np.ones(len(g["pl_p"]), dtype=bool); other[pol["idx"]] = False
    assert np.array_equal(S["Hpl"][other], S0["Hpl"][other])
    assert (n_carrying < 256) == (name in ("bench50", "random"))
    G.close(); C.close()


# ---------------------------------------------------------------- 2. chi2 and per-edge s / weight
def grown_with_polar_tail(pkg, g0, h=6, keep=600, **kw):
    """a handle grown by the last h poses of the stretch's first `keep` poses (test_gpu_lm.py's grown plan: 1000 / 200, keep = 600, 6 poses),
    polar edges in the base AND in the tail, from the perturbed start; returns (handle, full graph, its polar set, first tail edge, first tail pose, first tail cone)"""
    base, tail, full = split_for_growth(g0, h, keep)
    pol = plr.polar_set(full)
    Eb, Nb, Mb = len(base["pl_p"]), len(base["pose_est"]), len(base["lm_est"])
    G = fresh(pkg, base, plr.subset(pol, pol["idx"] < Eb), **kw); G.initialize_optimization()
    G.add_poses(np.arange(Nb, Nb + h), tail["pose_est"])
    if len(tail["lm_est"]):
        G.add_landmarks(Mb + np.arange(len(tail["lm_est"])), tail["lm_est"])
    G.add_odometry_edges(tail["pp_i"], tail["pp_j"], tail["pp_z"], tail["pp_info"])
    plr.add_edges(G, full, pol, first=Eb)
    G.initialize_optimization()
    assert G.plan_growths() > 0, G.growth_refusal()
    return G, full, pol, Eb, Nb, Mb


@pytest.mark.parametrize("name,gather", [(n, k) for n in NAMES for k in (0, 1)] + [("grown", 0)])
def test_chi2_and_per_edge_values(pkg, po, bench_graphs, frontend, name, gather):
    """gs_chi2 against the checker (1e-9) and gs_get_edge_chi2(observation) against numpy (s: 1e-11 of the largest; weight exactly 1
    without a kernel), at the initial estimates and after two iterations.  Grown plan: polar edges on an old pose, from a tail pose to an
    old cone and from a tail pose to a tail cone."""
    if name == "grown":
        G, g, pol, Eb, Nb, Mb = grown_with_polar_tail(pkg, graph_of(pkg, bench_graphs, frontend, "bench1000")[0])
        pp, ll = np.asarray(g["pl_p"])[pol["idx"]], np.asarray(g["pl_l"])[pol["idx"]]
        kinds = ((pp < Nb).sum(), ((pp >= Nb) & (ll < Mb)).sum(), ((pp >= Nb) & (ll >= Mb)).sum())
        print("grown: polar edges on old poses %d, tail pose -> old cone %d, tail pose -> tail cone %d" % kinds)
        assert all(k > 0 for k in kinds)
    else:
        g, pol = graph_of(pkg, bench_graphs, frontend, name)
        G = fresh(pkg, g, pol, linearize_gather=gather)
    for step in (0, 2):
        if step:
            done, _ = G.optimize(step); assert done == step
        P, L = G.poses(), G.landmarks()
        chi_o = plr.chi2_at(po, g, pol, P, L); chi = G.chi2()
        s_ref = plr.edge_s(g, pol, P, L); s, w = G.edge_chi2("observation")
        share = plr.contributions(g, pol, P, L)["chi2"]
        print("%s gather=%d after %d iterations: chi2 %.10g (checker %.10g, rel %.2e, polar share %.6g) per-edge s %.2e (%d edges, %d polar)"
              % (name, gather, step, chi, chi_o, abs(chi - chi_o) / chi_o, share, rel(s, s_ref), len(s), len(pol["idx"])))
        assert abs(chi - chi_o) <= 1e-9 * chi_o and share > 0
        assert len(s) == len(g["pl_p"]) == G.n_pl and rel(s, s_ref) < 1e-11 and np.all(w == 1.0) and np.all(s[pol["idx"]] > 0)
    if name == "grown":
        assert G.plan_growths() > 0 and G.growth_refusal() == ""
    G.close()


# ---------------------------------------------------------------- 3. one increment
@pytest.mark.parametrize("name,gather", [(n, 0) for n in NAMES] + [("bench50", 1), ("random", 1)])
def test_one_increment_matches_the_checker(pkg, po, bench_graphs, frontend, name, gather):
    """initialize_optimization() + iterate() + export_delta() against one oracle step on the cartesianised graph: 1e-8 of the largest
    increment (1e-9 on the random graph, which is compared for this one increment only: Gauss-Newton wanders on it)"""
    g, pol = graph_of(pkg, bench_graphs, frontend, name)
    og = plr.oracle_at(po, g, pol, g["pose_est"], g["lm_est"]); done, _, _ = og.optimize(1, ordering=1); assert done == 1
    dp_o, dl_o = og.delta()
    G = fresh(pkg, g, pol, linearize_gather=gather); G.initialize_optimization(); assert G.iterate() == 1; G.synchronize(); G.sync_estimates()
    dp, dl = G.export_delta(); sc = max(np.abs(dp_o).max(), np.abs(dl_o).max())
    e_inc = max(np.abs(dp - dp_o).max(), np.abs(dl - dl_o).max()) / sc
    print("%s gather=%d: increment %.2e of the largest (%.3g); estimates %.2e" % (name, gather, e_inc, sc, max(rel(G.poses(), og.poses()), rel(G.landmarks(), og.landmarks()))))
    assert e_inc < (1e-9 if name == "random" else 1e-8)
    assert rel(G.poses(), og.poses()) < 1e-9 and rel(G.landmarks(), og.landmarks()) < 1e-9
    G.close()


# ---------------------------------------------------------------- 4. trajectories
@pytest.mark.parametrize("name,variant,gather", [(n, v, k) for n in ("bench50", "bench1000") for v in (3, 4) for k in (0, 1)])
def test_trajectories_match_the_checker(pkg, po, bench_graphs, frontend, name, variant, gather):
    """optimize(10): estimates and chi2 against the checker's re-cartesianised Gauss-Newton (1e-9); whole-tree and per-level launches
    (tree = 0) bitwise equal; optimize_until(30, 1e-6) stops where the checker's chi2 sequence says"""
    g, pol = graph_of(pkg, bench_graphs, frontend, name)
    Po, Lo, chi_o, _, chi_end = checker_run(po, name, g, pol, 10)
    A = fresh(pkg, g, pol, factor_variant=variant, linearize_gather=gather); da, sa = A.optimize(10)
    B = fresh(pkg, g, pol, factor_variant=variant, linearize_gather=gather, debug=dict(tree=0)); db, sb = B.optimize(10)
    U = fresh(pkg, g, pol, factor_variant=variant, linearize_gather=gather); du, su = U.optimize_until(30, 1e-6)
    stop = rr.stop_iteration(chi_o, 1e-6, 30)
    Pu, Lu, _, _, _ = checker_run(po, name, g, pol, stop) if stop < 10 else (None, None, None, None, None)
    e_p, e_l = rel(A.poses(), Po), rel(A.landmarks(), Lo)
    e_c0, e_c = abs(sa.chi2_initial - chi_o[0]) / chi_o[0], abs(sa.chi2_final - chi_end) / chi_end
    same = np.array_equal(A.poses(), B.poses()) and np.array_equal(A.landmarks(), B.landmarks()) and sa.chi2_final == sb.chi2_final
    print("%s v%d gather=%d optimize(10): poses %.2e landmarks %.2e chi2_initial %.2e chi2_final %.2e (%.10g -> %.10g); tree=0 bit-identical %s; optimize_until stopped after %d (checker %d)"
          % (name, variant, gather, e_p, e_l, e_c0, e_c, sa.chi2_initial, sa.chi2_final, same, du, stop))
    assert da == 10 and db == 10 and e_p < 1e-9 and e_l < 1e-9 and e_c0 <= 1e-9 and e_c <= 1e-9 and same
    assert stop < 10 and du == stop and rel(U.poses(), Pu) < 1e-9 and rel(U.landmarks(), Lu) < 1e-9
    A.close(); B.close(); U.close()


# ---------------------------------------------------------------- 5. a grown plan
def test_grown_plan_with_polar_edges(pkg, po, bench_graphs, frontend):
    """optimize(5) on the grown handle (polar edges in the base and in the tail) against the checker on the full graph: 1e-9"""
    G, g, pol, Eb, Nb, Mb = grown_with_polar_tail(pkg, graph_of(pkg, bench_graphs, frontend, "bench1000")[0])
    Po, Lo, chi_o, _, chi_end = plr.gauss_newton(po, g, pol, 5)
    done, st = G.optimize(5)
    e_p, e_l, e_c0, e_c = rel(G.poses(), Po), rel(G.landmarks(), Lo), abs(st.chi2_initial - chi_o[0]) / chi_o[0], abs(st.chi2_final - chi_end) / chi_end
    print("grown + polar optimize(5): poses %.2e landmarks %.2e chi2_initial %.2e chi2_final %.2e (%.10g -> %.10g); growths %d, %d polar edges in the tail"
          % (e_p, e_l, e_c0, e_c, st.chi2_initial, st.chi2_final, G.plan_growths(), (pol["idx"] >= Eb).sum()))
    assert G.plan_growths() > 0 and G.growth_refusal() == ""
    assert done == 5 and e_p < 1e-9 and e_l < 1e-9 and e_c0 <= 1e-9 and e_c <= 1e-9
    G.close()


# ---------------------------------------------------------------- 6. composition
@pytest.mark.parametrize("gather", [0, 1])
def test_huber_on_the_observation_kind_weights_the_polar_edges(pkg, po, bench_graphs, frontend, gather):
    """Huber on the observation edges, delta = the median sqrt(s) of the kind at the start: system 1e-11, chi2 1e-9, per-edge weights,
    optimize(3) 1e-9 against the checker (reweighted() on the cartesianised graph sees the same s)"""
    g, pol = graph_of(pkg, bench_graphs, frontend, "bench1000")
    P, L = g["pose_est"], g["lm_est"]
    kernel = ("huber", float(np.median(np.sqrt(plr.edge_s(g, pol, P, L))))); kernels = {"observation": kernel}
    G = fresh(pkg, g, pol, linearize_gather=gather); G.set_robust_kernel("observation", *kernel)
    ref = plr.oracle_at(po, g, pol, P, L, kernels).linearize_blocks()
    G.linearize(); S = G.export_system()
    figs = {k: rel(S[k], ref[k]) for k in ref}
    chi, chi_o = G.chi2(), plr.chi2_at(po, g, pol, P, L, kernels)
    s, w = G.edge_chi2("observation"); w_ref = rr.weight(kernel, plr.edge_s(g, pol, P, L))
    Po, Lo, chi_seq, _, chi_end = plr.gauss_newton(po, g, pol, 3, kernels=kernels)
    done, st = G.optimize(3)
    e_p, e_l = rel(G.poses(), Po), rel(G.landmarks(), Lo)
    print("huber + polar gather=%d: " % gather + " ".join("%s %.2e" % kv for kv in figs.items()) + " chi2 %.2e weights %.2e (%d polar edges down-weighted) | optimize(3) poses %.2e landmarks %.2e chi2 %.2e"
          % (abs(chi - chi_o) / chi_o, rel(w, w_ref), int((w[pol["idx"]] < 1).sum()), e_p, e_l, abs(st.chi2_final - chi_end) / chi_end))
    for k, v in figs.items():
        assert v < 1e-11, k
    assert abs(chi - chi_o) <= 1e-9 * chi_o and rel(w, w_ref) < 1e-11 and (w[pol["idx"]] < 1).any() and (w[pol["idx"]] == 1).any()
    assert done == 3 and e_p < 1e-9 and e_l < 1e-9 and abs(st.chi2_final - chi_end) <= 1e-9 * chi_end
    G.close()


@pytest.mark.parametrize("gather", [0, 1])
def test_priors_and_polar_edges_together(pkg, po, bench_graphs, frontend, gather):
    """the prior set of test_gpu_prior.py on top of the polar set: system (1e-11) and chi2 (1e-9) against the oracle on the cartesianised
    graph augmented by the prior edges"""
    g, pol = graph_of(pkg, bench_graphs, frontend, "bench1000")
    pri = pr.prior_set(g)
    og = make_oracle_graph(po, pr.augment(plr.cartesianised(g, pol, g["pose_est"], g["lm_est"]), pri))
    ref = pr.strip(og.linearize_blocks(), g)
    G = fresh(pkg, g, pol, linearize_gather=gather); pr.add_to(G, pri)
    G.linearize(); S = G.export_system(); chi = G.chi2()
    figs = {k: rel(S[k], ref[k]) for k in ref}
    print("priors + polar gather=%d: " % gather + " ".join("%s %.2e" % kv for kv in figs.items()) + " chi2 %.2e" % (abs(chi - og.chi2()) / og.chi2()))
    for k, v in figs.items():
        assert v < 1e-11, k
    assert abs(chi - og.chi2()) <= 1e-9 * og.chi2()
    G.close()


def test_lm_with_polar_edges_matches_the_restated_loop(pkg, po, bench_graphs):
    """optimize_lm(6) from the perturbed start of test_gpu_lm.py (x1, seed 1) with the bench 1000 / 200 polar set against
    polar_ref.lm_run: trial counts exactly, lambda[], chi2[] and the estimates within max(4 x the plain gs_optimize(6) yardstick, 1e-9);
    the margin >= 1e-3 asserted on every compared trial"""
    g, pol, P1, L1 = lm_case(po, bench_graphs)
    r = plr.lm_run(po, g, pol, LM_ITERATIONS, poses=P1, lms=L1)
    assert all(t["margin"] >= lm_ref.MIN_MARGIN for t in r["trials"])
    gs = dict(g, pose_est=P1, lm_est=L1)
    A = fresh(pkg, gs, pol); done, sa = A.optimize(LM_ITERATIONS); assert done == LM_ITERATIONS
    Po, Lo, _, _, chi_end = plr.gauss_newton(po, gs, pol, LM_ITERATIONS)
    y_est = max(rel(A.poses(), Po), rel(A.landmarks(), Lo)); y_chi = abs(sa.chi2_final - chi_end) / chi_end
    A.close()
    tol_est, tol_chi = max(4 * y_est, 1e-9), max(4 * y_chi, 4 * y_est, 1e-9)
    G = fresh(pkg, gs, pol); done, st, info = G.optimize_lm(LM_ITERATIONS)
    e_chi = float(np.abs(info["chi2"] / r["chi2"] - 1).max()); e_lam = float(np.abs(info["lambda"] / r["lam"] - 1).max())
    e_est = max(rel(G.poses(), r["P"]), rel(G.landmarks(), r["L"])); e_fin = abs(st.chi2_final - r["chi2_final"]) / r["chi2_final"]
    print("LM with polar edges: trials GPU %s checker %s min margin %.2e | plain(6) estimates %.2e chi2 %.2e | LM chi2[] %.2e lambda[] %.2e estimates %.2e chi2_final %.2e lambda_0 %.6e / %.6e"
          % (info["n_trials"].tolist(), r["n_trials"].tolist(), r["min_margin"], y_est, y_chi, e_chi, e_lam, e_est, e_fin, info["lambda_initial"], r["lambda_initial"]))
    assert done == LM_ITERATIONS and info["n_trials"].tolist() == r["n_trials"].tolist() and info["rejected"] == r["rejected"] and info["terminated"] == 0
    assert e_chi <= tol_chi and e_lam <= tol_chi and e_fin <= tol_chi and e_est <= tol_est
    G.close()


def test_marginals_with_polar_edges_match_the_dense_inverse(pkg, po, bench_graphs, frontend):
    """compute_marginals() after optimize(3) on bench 50 / 30: every covariance block against the dense inverse of the checker's H at the
    handle's estimates (REL); the H_pl rows of the polar edges are named by their observation index"""
    g, pol = graph_of(pkg, bench_graphs, frontend, "bench50")
    G = fresh(pkg, g, pol); G.optimize(3); G.compute_marginals()
    ga = plr.cartesianised(g, pol, G.poses(), G.landmarks())
    H, po_, lo_ = sx.dense_system(make_oracle_graph(po, ga))
    ref = sx.reference_blocks(np.linalg.inv(H), po_, lo_, ga)
    got = (G.pose_covariances(), G.landmark_covariances(), G.odometry_edge_covariances(), G.observation_edge_covariances())
    figs = {k: rel_err(a, b) for k, a, b in zip(("poses", "landmarks", "odometry edges", "observation edges"), got, ref)}
    figs["polar observation edges"] = rel_err(got[3][pol["idx"]], ref[3][pol["idx"]])
    print("marginals with polar edges: " + " ".join("%s %.2e" % kv for kv in figs.items()) + " | cond(H) %.2e" % np.linalg.cond(H))
    for k, v in figs.items():
        assert v < REL, k
    G.close()


@pytest.mark.parametrize("gather", [0, 1])
def test_a_polar_edge_switched_off_and_on_again(pkg, po, bench_graphs, frontend, gather):
    """gs_set_edge_active on polar edges (a range-bearing and a bearing-only one) and on a Cartesian edge: the system and chi2 of the graph
    without them (1e-11 / 1e-9), gs_get_edge_chi2 reports their own s with weight 0; switched on again: bit-identical to a handle that
    never had the flag"""
    g, pol = graph_of(pkg, bench_graphs, frontend, "bench1000")
    P, L = g["pose_est"], g["lm_est"]
    k_rb = int(pol["idx"][pol["model"] == plr.RANGE_BEARING][40]); k_b = int(pol["idx"][pol["model"] == plr.BEARING][9])
    k_c = int(np.setdiff1d(np.arange(len(g["pl_p"])), pol["idx"])[25]); off = [k_rb, k_b, k_c]
    F = fresh(pkg, g, pol, linearize_gather=gather); F.linearize(); S_on = F.export_system(); chi_on = F.chi2()
    G = fresh(pkg, g, pol, linearize_gather=gather)
    G.set_edge_active("observation", k_rb, False); G.set_edges_active("observation", [k_b, k_c])
    ref = plr.oracle_at(po, g, pol, P, L, off=off).linearize_blocks()
    G.linearize(); S = G.export_system(); chi, chi_o = G.chi2(), plr.chi2_at(po, g, pol, P, L, off=off)
    figs = {k: rel(S[k], ref[k]) for k in ref}
    s, w = G.edge_chi2("observation"); s_ref = plr.edge_s(g, pol, P, L)
    G.activate_all_edges(); G.linearize(); S_again = G.export_system(); chi_again = G.chi2()
    same = all(np.array_equal(S_again[k], S_on[k]) for k in S_on) and chi_again == chi_on
    print("polar edges off, gather=%d: " % gather + " ".join("%s %.2e" % kv for kv in figs.items()) + " chi2 %.2e per-edge s %.2e weights off %s | on again bit-identical %s"
          % (abs(chi - chi_o) / chi_o, rel(s, s_ref), w[off].tolist(), same))
    for k, v in figs.items():
        assert v < 1e-11, k
    assert abs(chi - chi_o) <= 1e-9 * chi_o and chi < chi_on
    assert np.abs(S["Hpl"][off]).max() == 0.0 and rel(s, s_ref) < 1e-11 and np.all(w[off] == 0.0) and np.all(np.delete(w, off) == 1.0) and np.all(s[off] > 0)
    assert same
    # gs_deactivate_edges_above never selects a polar edge: its gate sees the carrier's zero information
    n_off = G.deactivate_edges_above("observation", 0.0)
    act = G.edges_active("observation")
    assert n_off > 0 and np.all(act[pol["idx"]]) and not act[np.setdiff1d(np.arange(len(act)), pol["idx"])].any()
    G.close(); F.close()


# ---------------------------------------------------------------- 7. nothing for nothing
def test_a_handle_without_polar_edges_is_bit_identical(pkg, bench_graphs, frontend):
    """Two handles after optimize(10): never touched; empty bulk calls of both kinds.  Estimates and chi2 bitwise equal, the launch
    schedule unchanged, no polar edge reported."""
    g, pol = graph_of(pkg, bench_graphs, frontend, "bench1000")
    A = pkg.Graph(device=0); A.load_bench_graph(g)
    B = pkg.Graph(device=0); B.load_bench_graph(g)
    B.add_range_bearing_edges([], [], np.zeros((0, 2)), np.zeros((0, 4))); B.add_bearing_edges([], [], np.zeros(0), np.zeros(0))
    outs = []
    for H in (A, B):
        done, st = H.optimize(10); assert done == 10
        outs.append((H.poses(), H.landmarks(), st.chi2_final, H.debug_schedule()["raw"], H.num_polar_edges()))
    same = np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and outs[0][2] == outs[1][2] and np.array_equal(outs[0][3], outs[1][3])
    print("no polar edges: chi2 %.17g; two handles bit-identical %s" % (outs[0][2], same))
    assert same and outs[0][4] == 0 and outs[1][4] == 0
    A.close(); B.close()


def test_sharded_handles_are_refused(pkg, bench_graphs):
    b = pkg.binding
    g = bench_graphs(50, 30)[1]
    G = pkg.Graph(device=0); G.load_bench_graph(g)
    G.add_bearing_edge(5, 5, 0.1, 1.0)
    with pytest.raises(b.GsError) as e:
        G.dist_configure(0, 2)
    assert e.value.code == -1 and "polar" in str(e.value)
    G.clear(); G.load_bench_graph(g); G.dist_configure(0, 2)
    n = G.n_pl
    for call in (lambda: G.add_range_bearing_edge(5, 5, [1.0, 0.1], np.eye(2)), lambda: G.add_bearing_edge(5, 5, 0.1, 1.0)):
        with pytest.raises(b.GsError) as e:
            call()
        assert e.value.code == -1 and "shard" in str(e.value)
    assert G.n_pl == n and G.num_polar_edges() == 0
    G.close()


# ---------------------------------------------------------------- the chi2 finish at the one / two workgroup boundary
@pytest.mark.parametrize("gather", [0, 1])
def test_chi2_finish_at_the_workgroup_boundary(pkg, bench_graphs, gather):
    """One range-bearing edge each on 255, 256 and 257 free poses of a 300-pose / 40-cone graph, to a cone the pose has no edge to: the
    pose side is one workgroup of 255 and of 256 listed poses (its total added by the pass itself) and two workgroups at 257 (partials,
    then the totalling kernel).  The pairs beyond the count are added as what a carrier is — a Cartesian edge with zero information —, so
    the three handles have one structure.  The handle's chi2 minus the graph's own chi2 is the sum of the per-edge values (1e-9 of
    chi2, the bar of test_chi2_and_per_prior_chi2), and the exported diagonal blocks and right-hand sides of the first 255 carrying
    poses do not depend on the count, bit for bit."""
    g = bench_graphs(300, 40)[1]
    rng = np.random.default_rng(257)
    P = np.asarray(g["pose_est"], dtype=np.float64).reshape(-1, 3); L = np.asarray(g["lm_est"], dtype=np.float64).reshape(-1, 2)
    pl_p, pl_l = np.asarray(g["pl_p"], dtype=np.int64), np.asarray(g["pl_l"], dtype=np.int64)
    free = np.setdiff1d(np.arange(len(P)), np.asarray(g["fixed_poses"], dtype=np.int64))[:257]
    free_l = np.setdiff1d(np.arange(len(L)), np.asarray(g["fixed_landmarks"], dtype=np.int64))
    cone = np.array([np.setdiff1d(free_l, pl_l[pl_p == p])[0] for p in free])           # (the lowest index among the free cones p does not observe)
    assert len(free) == 257
    d = L[cone] - P[free, :2]; th = P[free, 2]
    dx, dy = np.cos(th) * d[:, 0] + np.sin(th) * d[:, 1], np.cos(th) * d[:, 1] - np.sin(th) * d[:, 0]
    z = np.stack([np.hypot(dx, dy), np.arctan2(dy, dx)], 1) + rng.normal(0, 0.05, (257, 2))
    assert np.all(z[:, 0] > 0)
    W = np.stack([pr.spd(rng, 2, 0.3) for _ in range(257)])
    G0 = pkg.Graph(device=0, linearize_gather=gather); G0.load_bench_graph(g); chi0 = G0.chi2(); G0.close()
    blocks = {}
    for count in (255, 256, 257):
        G = pkg.Graph(device=0, linearize_gather=gather); G.load_bench_graph(g)
        G.add_range_bearing_edges(free[:count], cone[:count], z[:count], W[:count].reshape(-1, 4))
        if count < 257:
            G.add_observation_edges(free[count:], cone[count:], np.zeros((257 - count, 2)), np.zeros((257 - count, 4)))
        chi = G.chi2(); s, w = G.edge_chi2("observation"); idx, _ = G.polar_edges()
        G.linearize(); S = G.export_system()
        blocks[count] = (S["Hpp_diag"][free[:255]].copy(), S["b_pose"][free[:255]].copy())
        print("gather=%d %d polar edges: chi2 %.10g without %.10g difference %.10g sum of the per-edge values %.10g (rel %.2e)"
              % (gather, count, chi, chi0, chi - chi0, s[idx].sum(), abs((chi - chi0) - s[idx].sum()) / chi))
        assert len(idx) == count and np.all(s[idx] > 0) and np.all(w == 1.0) and np.all(s[len(pl_p) + count:] == 0.0)
        assert abs((chi - chi0) - s[idx].sum()) <= 1e-9 * chi
        G.close()
    for count in (256, 257):
        assert np.array_equal(blocks[count][0], blocks[255][0]) and np.array_equal(blocks[count][1], blocks[255][1]), count
