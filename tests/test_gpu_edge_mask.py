"""Edge deactivation on the GPU (gs_set_edge_active ... gs_deactivate_edges_above, csrc/gs_edge_mask.hip) against the checker
tests/edge_mask_ref.py: the UNCHANGED CPU oracle on the graph whose inactive edges carry zero information (test_edge_mask_cpu.py pins
that equivalence, and establishes without a GPU the conditions of the rejection and LM cases).

Graphs: bench 50/30, random_graph(7), bench 1000/200 (the per-edge kernels span several workgroups) and a grown plan (tail slots),
each on the fused and the linearize_gather = 1 paths.  Masks switch off about 10 % of each kind by a seeded RNG such that no vertex is
isolated (asserted on the CPU, edge_mask_ref.random_masks).

Tolerances.  Items 1, 2: none — the device arrays are the same, so the bits are.  Item 3: the yardstick is the SAME comparison with no
mask on the same graph, taken inside the test (as test_gpu_robust.py); the masked comparison may be 4 x that, with test_gpu_parity.py's
bounds as floors: blocks and per-edge values 1e-11 of the array's largest entry, chi2 1e-10, increments 1e-8 (1e-9 on the random
graph), estimates 1e-9.  Items 4 - 6: the bars of the features' own GPU tests.  Every test prints its figures before it asserts (-s);
the printed run is profiles/edge_mask_gpu_suite.txt."""
import numpy as np
import pytest

import edge_mask_ref as em
import lm_ref
import prior_ref as pr
import robust_ref as rr
from conftest import append_tail, make_oracle_graph, random_graph, split_for_growth
from test_edge_mask_cpu import BLOCKS, GAP_MIN, HUBER_ITERATIONS, LM_ITERATIONS, MASK_SEED, huber_outlier_state, lm_mask_case
from test_gpu_marginals import check_against_dense
from test_robust_cpu import OUTLIER_DELTA, lm_rmse, perturbed

pytestmark = pytest.mark.gpu

NAMES = ["bench50", "random", "bench1000", "grown"]
GROW_H, GROW_KEEP = 6, 600
PATHS = [(n, k) for n in NAMES for k in (0, 1) if not (n == "grown" and k == 1)]     # (a plan built for the gather kernels has no room to grow: the tail is the fused path's)


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300))


_cases = {}


def case(bench_graphs, name):
    """(graph in the handle's edge order, act_pp, act_pl, base, tail), built once per name and left unchanged; on the grown plan the
    last odometry edge and the last observation edge — tail slots — are among the candidates"""
    if name not in _cases:
        base = tail = None
        if name == "random":
            g = random_graph(7)
        elif name == "grown":
            base, tail, g = split_for_growth(bench_graphs(1000, 200)[1], GROW_H, GROW_KEEP)
        else:
            g = bench_graphs(*{"bench50": (50, 30), "bench1000": (1000, 200)}[name])[1]
        a_pp, a_pl = em.random_masks(g, MASK_SEED)
        if name == "grown":
            for kd, n in ((0, len(a_pp)), (1, len(a_pl))):
                cand = np.zeros(n, bool); cand[[n - 1, n - 3]] = True
                a_pp, a_pl, _ = em.deactivate(g, a_pp, a_pl, kd, cand, True)
            assert not a_pp[len(base["pp_i"]):].all() and not a_pl[len(base["pl_p"]):].all()
        assert em.isolated_vertex(g, a_pp, a_pl) is None and (~a_pp).sum() > 0 and (~a_pl).sum() > 0
        _cases[name] = (g, a_pp, a_pl, base, tail)
    return _cases[name]


def handle(pkg, name, g, base, tail, **kw):
    """a handle holding g: loaded whole, or (grown) the base built, then the tail's six poses and their cones absorbed by a growth step"""
    G = pkg.Graph(device=0, **kw)
    if name != "grown":
        G.load_bench_graph(g); return G
    nb_pp, nb_pl = len(base["pp_i"]), len(base["pl_p"])
    b = dict(base, pp_info=np.asarray(g["pp_info"])[:nb_pp], pl_info=np.asarray(g["pl_info"])[:nb_pl])      # (g may carry other information than base / tail: zeros)
    t = dict(tail, pp_info=np.asarray(g["pp_info"])[nb_pp:], pl_info=np.asarray(g["pl_info"])[nb_pl:])
    G.load_bench_graph(b); G.initialize_optimization()
    append_tail(G, t); G.initialize_optimization()
    assert G.plan_growths() > 0, G.growth_refusal()
    return G


def switch_off(G, a_pp, a_pl):
    G.set_edges_active("odometry", np.flatnonzero(~a_pp)); G.set_edges_active("observation", np.flatnonzero(~a_pl))


def three_iterations(G):
    """(behind system_of: the plan is on the device — a gs_initialize_optimization here would rebuild a grown plan from scratch)"""
    for _ in range(3):
        assert G.iterate() == 1
    G.synchronize(); G.sync_estimates()
    return G.poses(), G.landmarks()


def same_bits(a, b):
    return bool(np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True))


def system_of(G):
    """(export_system() of a fresh linearisation, chi2); a grown plan exports the whole graph's system, tail arenas included"""
    G.linearize()
    return G.export_system(), G.chi2()


# ---------------------------------------------------------------- 1. bit for bit against zero-information edges
@pytest.mark.parametrize("name,gather", PATHS)
def test_masked_handle_equals_zero_information_edges_bit_for_bit(pkg, bench_graphs, name, gather):
    """A handle with the mask against a fresh handle built with the same edges given all-zero information: export_system, chi2 and the
    estimates after three gs_iterate — identical bits, no tolerance (the device arrays are the same)."""
    g, a_pp, a_pl, base, tail = case(bench_graphs, name)
    A = handle(pkg, name, g, base, tail, linearize_gather=gather); switch_off(A, a_pp, a_pl)
    Z = handle(pkg, name, em.masked(g, a_pp, a_pl), base, tail, linearize_gather=gather)
    SA, ca = system_of(A); SZ, cz = system_of(Z)
    sys_same = {k: same_bits(SA[k], SZ[k]) for k in SA}
    zero_blocks = not SA["Hpl"][~a_pl].any() and not SA["Hpp_off"][~a_pp].any()
    assert len(SA) == len(BLOCKS) == len(SZ) and (name != "grown" or (A.plan_growths() > 0 and not a_pl[len(base["pl_p"]):].all()))
    PA, LA = three_iterations(A); PZ, LZ = three_iterations(Z)
    print("%s gather=%d (%d + %d edges off): system %s chi2 %.17g / %.17g estimates after 3 iterations %s %s; growths %d"
          % (name, gather, (~a_pp).sum(), (~a_pl).sum(), sys_same, ca, cz, same_bits(PA, PZ), same_bits(LA, LZ), A.plan_growths()))
    assert all(sys_same.values()) and ca == cz and zero_blocks
    assert same_bits(PA, PZ) and same_bits(LA, LZ) and np.isfinite(PA).all()
    assert A.n_inactive_edges(0) == (~a_pp).sum() and A.n_inactive_edges(1) == (~a_pl).sum() and Z.n_inactive_edges(1) == 0
    A.close(); Z.close()


# ---------------------------------------------------------------- 2. reactivation restores everything
@pytest.mark.parametrize("name,gather", PATHS)
def test_reactivation_restores_everything(pkg, bench_graphs, name, gather):
    """Deactivate (and let the device see it), activate_all_edges, then against a handle that never had a mask: export_system, chi2 and
    three iterations bit for bit."""
    g, a_pp, a_pl, base, tail = case(bench_graphs, name)
    A = handle(pkg, name, g, base, tail, linearize_gather=gather); switch_off(A, a_pp, a_pl)
    _, c_masked = system_of(A)
    A.activate_all_edges()
    U = handle(pkg, name, g, base, tail, linearize_gather=gather)
    SA, ca = system_of(A); SU, cu = system_of(U)
    sys_same = {k: same_bits(SA[k], SU[k]) for k in SA}
    PA, LA = three_iterations(A); PU, LU = three_iterations(U)
    print("%s gather=%d: masked chi2 %.10g, after activate_all %.17g, never masked %.17g; system %s estimates %s %s"
          % (name, gather, c_masked, ca, cu, sys_same, same_bits(PA, PU), same_bits(LA, LU)))
    assert c_masked < cu and ca == cu and all(sys_same.values()) and same_bits(PA, PU) and same_bits(LA, LU)
    assert A.n_inactive_edges(0) == 0 and A.n_inactive_edges(1) == 0 and A.edges_active(1).all()
    A.close(); U.close()


# ---------------------------------------------------------------- 3. against the oracle on masked(g)
def oracle_figures(pkg, po, name, gather, g, a_pp, a_pl, base, tail, iterate):
    """GPU against the oracle on masked(g): blocks, chi2, per-edge s (the edges' OWN information: the unmasked reference s) and weight,
    one increment, and (iterate) the estimates after ten iterations"""
    gm = em.masked(g, a_pp, a_pl)
    G = handle(pkg, name, g, base, tail, linearize_gather=gather); switch_off(G, a_pp, a_pl)
    out = {}
    S, chi = system_of(G)
    ref = make_oracle_graph(po, gm).linearize_blocks()
    for k in S:
        out[k] = rel(S[k], ref[k])
    chi_o = make_oracle_graph(po, gm).chi2(); out["chi2"] = abs(chi - chi_o) / chi_o
    s_ref = dict(zip(("odometry", "observation"), rr.edge_s(g, g["pose_est"], g["lm_est"])))
    w_bad = 0
    for kind, act in (("odometry", a_pp), ("observation", a_pl)):
        s, w = G.edge_chi2(kind)
        out["s_" + kind] = rel(s, s_ref[kind])
        w_bad += int((w[~act] != 0).sum() + (w[act] != 1).sum())
    og = make_oracle_graph(po, gm); og.build_system(); og.apply_update(og.solve_ldlt(1)); dp_o, dl_o = og.delta()
    done, _ = G.optimize(1); assert done == 1
    dp, dl = G.export_delta(); sc = max(np.abs(dp_o).max(), np.abs(dl_o).max())
    out["increment"] = float(max(np.abs(dp - dp_o).max(), np.abs(dl - dl_o).max()) / sc)
    if iterate:
        og = make_oracle_graph(po, gm); d_o, _, _ = og.optimize(10, ordering=1); assert d_o == 10
        done, st = G.optimize(9); assert done == 9
        out["estimates"] = max(rel(G.poses(), og.poses()), rel(G.landmarks(), og.landmarks()))
        out["chi2_final"] = abs(st.chi2_final - og.chi2()) / og.chi2()
    G.close()
    return out, w_bad


def floor_of(key, name):
    if key.startswith("chi2"):
        return 1e-10
    if key == "increment":
        return 1e-9 if name == "random" else 1e-8
    if key == "estimates":
        return 1e-9
    return 1e-11


@pytest.mark.parametrize("name,gather", PATHS)
def test_masked_handle_matches_the_oracle_on_the_masked_graph(pkg, po, bench_graphs, name, gather):
    g, a_pp, a_pl, base, tail = case(bench_graphs, name)
    iterate = name != "random"                                      # (random_graph(7): Gauss-Newton wanders on it, test_prior_cpu.py; system, chi2 and one increment)
    ones = (np.ones_like(a_pp), np.ones_like(a_pl))
    plain, wp = oracle_figures(pkg, po, name, gather, g, ones[0], ones[1], base, tail, iterate)
    got, wb = oracle_figures(pkg, po, name, gather, g, a_pp, a_pl, base, tail, iterate)
    print("%s gather=%d no mask %s" % (name, gather, " ".join("%s=%.2g" % kv for kv in plain.items())))
    print("%s gather=%d masked  %s | weights off their value: %d" % (name, gather, " ".join("%s=%.2g" % kv for kv in got.items()), wb))
    for k, v in got.items():
        assert v <= max(4 * plain[k], floor_of(k, name)), (k, v, plain[k])
    assert wb == 0 and wp == 0                                      # weight 0 on the inactive edges, 1 elsewhere (no kernel set)


# ---------------------------------------------------------------- 4. the flags survive uploads
def zero_rows(S, a_pp, a_pl):
    return not S["Hpl"][~a_pl].any() and not S["Hpp_off"][~a_pp].any()


@pytest.mark.parametrize("gather", [0, 1])
def test_flags_survive_a_full_structure_phase(pkg, po, bench_graphs, gather):
    """Deactivate, then an edge between two old vertices: a full structure phase uploads every edge's information again; the inactive
    edges' blocks are still zero and the system matches the oracle (1e-11, chi2 1e-10)."""
    g, a_pp, a_pl, _, _ = case(bench_graphs, "bench1000")
    G = handle(pkg, "bench1000", g, None, None, linearize_gather=gather); switch_off(G, a_pp, a_pl)
    _, c0 = system_of(G)
    P = np.asarray(g["pose_est"]); i, j = 10, 500
    z = rr.se2_compose(rr.se2_inverse(P[i:i + 1]), P[j:j + 1])[0] + [0.05, -0.03, 0.01]
    G.add_odometry_edge(i, j, z, np.eye(3))
    g2 = dict(g, pp_i=np.r_[g["pp_i"], i].astype(np.int32), pp_j=np.r_[g["pp_j"], j].astype(np.int32), pp_z=np.vstack([np.asarray(g["pp_z"]).reshape(-1, 3), z]),
              pp_info=np.vstack([np.asarray(g["pp_info"]).reshape(-1, 9), np.eye(3).reshape(1, 9)]))
    b_pp = np.r_[a_pp, True]
    S, chi = system_of(G)
    assert G.plan_growths() == 0 and G.growth_refusal() != ""       # not absorbed by growth: a full phase
    gm = em.masked(g2, b_pp, a_pl); ref = make_oracle_graph(po, gm).linearize_blocks(); chi_o = make_oracle_graph(po, gm).chi2()
    figs = {k: rel(S[k], ref[k]) for k in BLOCKS}
    print("full phase, gather=%d: %s chi2 %.2e (%.10g, before the edge %.10g); flags %d + %d" % (gather, " ".join("%s %.2e" % kv for kv in figs.items()),
                                                                                                  abs(chi - chi_o) / chi_o, chi, c0, G.n_inactive_edges(0), G.n_inactive_edges(1)))
    assert zero_rows(S, b_pp, a_pl) and all(v < 1e-11 for v in figs.values()) and abs(chi - chi_o) <= 1e-10 * chi_o
    assert np.array_equal(G.edges_active(0), b_pp) and np.array_equal(G.edges_active(1), a_pl)
    G.close()


def test_flags_survive_a_growth_step(pkg, po, bench_graphs):
    """Deactivate on a grown plan (tail slots among the inactive edges), then one more keyframe: absorbed by growth (plan_growths
    increases), the flags are what they were, the new edges are active.  The inactive edges are seen in the exported blocks (exact
    zeros on them, the rest 1e-11 against the oracle on the masked graph), chi2 1e-10, the per-edge s 1e-11 and weights, and three
    iterations 1e-9."""
    g0 = bench_graphs(1000, 200)[1]
    base, tail, full7 = split_for_growth(g0, GROW_H + 1, GROW_KEEP)
    _, _, full = split_for_growth(g0, GROW_H, GROW_KEEP - 1)        # what the handle holds after its first growth step: the stretch without its last pose
    a_pp, a_pl = em.random_masks(full, MASK_SEED)
    for kd, n in ((0, len(a_pp)), (1, len(a_pl))):
        cand = np.zeros(n, bool); cand[[n - 1, n - 3]] = True
        a_pp, a_pl, _ = em.deactivate(full, a_pp, a_pl, kd, cand, True)
    G = pkg.Graph(device=0); G.load_bench_graph(base); G.initialize_optimization()
    append_tail(G, tail, poses=(0, GROW_H)); G.initialize_optimization()
    n0 = G.plan_growths(); assert n0 > 0, G.growth_refusal()
    assert G.n_pp == len(a_pp) and G.n_pl == len(a_pl) and not a_pl[len(base["pl_p"]):].all()
    switch_off(G, a_pp, a_pl)
    c0 = G.chi2(); assert G.plan_growths() == n0
    chi_o = make_oracle_graph(po, em.masked(full, a_pp, a_pl)).chi2(); e0 = abs(c0 - chi_o) / chi_o
    append_tail(G, tail, poses=(GROW_H, GROW_H + 1)); G.initialize_optimization()
    assert G.plan_growths() == n0 + 1 and G.growth_refusal() == "", G.growth_refusal()
    full_now = dict(full7, lm_est=np.asarray(full7["lm_est"])[:G.n_landmarks])
    b_pp = np.r_[a_pp, np.ones(G.n_pp - len(a_pp), bool)]; b_pl = np.r_[a_pl, np.ones(G.n_pl - len(a_pl), bool)]
    assert np.array_equal(G.edges_active(0), b_pp) and np.array_equal(G.edges_active(1), b_pl) and len(b_pl) == len(full_now["pl_p"]) and len(b_pl) > len(a_pl)
    chi = G.chi2()
    gm = em.masked(full_now, b_pp, b_pl); chi_o = make_oracle_graph(po, gm).chi2()
    s, w = G.edge_chi2("observation"); s_ref = rr.edge_s(full_now, full_now["pose_est"], full_now["lm_est"])[1]
    G.linearize(); S = G.export_system(); ref = make_oracle_graph(po, gm).linearize_blocks()
    figs = {k: rel(S[k], ref[k]) for k in BLOCKS}
    print("growth step: exported blocks against the oracle on the masked graph: %s" % " ".join("%s %.2e" % kv for kv in figs.items()))
    assert zero_rows(S, b_pp, b_pl) and all(v < 1e-11 for v in figs.values()) and G.plan_growths() == n0 + 1
    done, st = G.optimize(3); og = make_oracle_graph(po, gm); og.optimize(3, ordering=1)
    e_p, e_l = rel(G.poses(), og.poses()), rel(G.landmarks(), og.landmarks())
    print("growth step: growths %d -> %d; chi2 before %.2e after %.2e; per-edge s %.2e, weight 0 on %d edges; optimize(3) poses %.2e landmarks %.2e"
          % (n0, G.plan_growths(), e0, abs(chi - chi_o) / chi_o, rel(s, s_ref), int((w == 0).sum()), e_p, e_l))
    assert e0 <= 1e-10 and abs(chi - chi_o) <= 1e-10 * chi_o
    assert rel(s, s_ref) < 1e-11 and np.array_equal(w == 0, ~b_pl)
    assert done == 3 and e_p < 1e-9 and e_l < 1e-9
    G.close()


# ---------------------------------------------------------------- 5. with the rest
def test_with_huber_on_the_observation_edges(pkg, po, bench_graphs):
    """Mask + Huber (delta = the median sqrt(s) of the kind at the start, as test_gpu_robust.py): the checker re-weights with the edges'
    own information, then masks.  System 1e-11, chi2 1e-9, weights of the active edges against the checker, 0 on the inactive ones."""
    g, a_pp, a_pl, _, _ = case(bench_graphs, "bench1000")
    P, L = perturbed(g, 1); gs = dict(g, pose_est=P, lm_est=L)
    kernels = {"observation": ("huber", rr.median_deltas(g, P, L)[1])}
    G = handle(pkg, "bench1000", gs, None, None); switch_off(G, a_pp, a_pl); G.set_robust_kernel("observation", *kernels["observation"])
    gm = em.masked(rr.reweighted(g, P, L, kernels), a_pp, a_pl)
    S, chi = system_of(G); ref = make_oracle_graph(po, gm).linearize_blocks()
    figs = {k: rel(S[k], ref[k]) for k in BLOCKS}
    chi_o = rr.robust_chi2(em.masked(g, a_pp, a_pl), P, L, kernels)
    s, w = G.edge_chi2("observation"); s_ref = rr.edge_s(g, P, L)[1]; w_ref = np.where(a_pl, rr.weight(kernels["observation"], s_ref), 0.0)
    print("huber + mask: %s chi2 %.2e s %.2e w %.2e (%d down-weighted, %d inactive)" % (" ".join("%s %.2e" % kv for kv in figs.items()), abs(chi - chi_o) / chi_o,
                                                                                        rel(s, s_ref), np.abs(w - w_ref).max(), int(((w < 1) & (w > 0)).sum()), int((w == 0).sum())))
    assert all(v < 1e-11 for v in figs.values()) and abs(chi - chi_o) <= 1e-9 * chi_o
    assert rel(s, s_ref) < 1e-11 and np.abs(w - w_ref).max() < 1e-11 and np.array_equal(w == 0, ~a_pl) and ((w < 1) & (w > 0)).any()
    G.close()


def test_with_levenberg_marquardt(pkg, po, bench_graphs):
    """optimize_lm(5) from the perturbed start of test_gpu_lm.py (x1, seed 1) with the mask against lm_ref on masked(g): trial counts
    exactly; lambda[], chi2[] and the estimates within max(4 x the plain gs_optimize(5) yardstick on the masked graph, 1e-9)."""
    g, a_pp, a_pl, P1, L1 = lm_mask_case(po, bench_graphs)
    gm = em.masked(g, a_pp, a_pl)
    r = lm_ref.run(po, gm, LM_ITERATIONS, poses=P1, lms=L1)
    assert all(t["margin"] >= lm_ref.MIN_MARGIN for t in r["trials"])
    gs = dict(g, pose_est=P1, lm_est=L1)
    A = handle(pkg, "bench1000", gs, None, None); switch_off(A, a_pp, a_pl); done, sa = A.optimize(LM_ITERATIONS); assert done == LM_ITERATIONS
    og = make_oracle_graph(po, dict(gm, pose_est=P1, lm_est=L1)); og.optimize(LM_ITERATIONS, ordering=1)
    y_est = max(rel(A.poses(), og.poses()), rel(A.landmarks(), og.landmarks())); y_chi = abs(sa.chi2_final - og.chi2()) / og.chi2()
    A.close()
    tol_est, tol_chi = max(4 * y_est, 1e-9), max(4 * y_chi, 4 * y_est, 1e-9)
    G = handle(pkg, "bench1000", gs, None, None); switch_off(G, a_pp, a_pl); done, st, info = G.optimize_lm(LM_ITERATIONS)
    e_chi = float(np.abs(info["chi2"] / r["chi2"] - 1).max()); e_lam = float(np.abs(info["lambda"] / r["lam"] - 1).max())
    e_est = max(rel(G.poses(), r["P"]), rel(G.landmarks(), r["L"])); e_fin = abs(st.chi2_final - r["chi2_final"]) / r["chi2_final"]
    print("LM + mask: trials GPU %s checker %s min margin %.2e | plain(%d) estimates %.2e chi2 %.2e | LM chi2[] %.2e lambda[] %.2e estimates %.2e chi2_final %.2e"
          % (info["n_trials"].tolist(), r["n_trials"].tolist(), r["min_margin"], LM_ITERATIONS, y_est, y_chi, e_chi, e_lam, e_est, e_fin))
    assert done == r["accepted"] and info["n_trials"].tolist() == r["n_trials"].tolist() and info["rejected"] == r["rejected"]
    assert e_chi <= tol_chi and e_lam <= tol_chi and e_fin <= tol_chi and e_est <= tol_est
    G.close()


def test_with_priors(pkg, po, bench_graphs):
    """Mask + the graph's prior set (prior_ref): system 1e-11, chi2 1e-9, three iterations 1e-9 against the oracle on the augmented
    masked graph.  Then every edge of a cone that carries a prior is switched off: not isolated, the iterations run."""
    g, a_pp, a_pl, _, _ = case(bench_graphs, "bench1000")
    pri = pr.prior_set(g); gm = em.masked(g, a_pp, a_pl)
    G = handle(pkg, "bench1000", g, None, None); pr.add_to(G, pri); switch_off(G, a_pp, a_pl)
    S, chi = system_of(G); ref = pr.strip(make_oracle_graph(po, pr.augment(gm, pri)).linearize_blocks(), g)
    figs = {k: rel(S[k], ref[k]) for k in ref}
    chi_o = make_oracle_graph(po, pr.augment(gm, pri)).chi2()
    og = make_oracle_graph(po, pr.augment(gm, pri)); og.optimize(3, ordering=1)
    done, st = G.optimize(3)
    e_p, e_l = rel(G.poses(), og.poses()[:-1]), rel(G.landmarks(), og.landmarks())
    print("priors + mask: %s chi2 %.2e | optimize(3) poses %.2e landmarks %.2e" % (" ".join("%s %.2e" % kv for kv in figs.items()), abs(chi - chi_o) / chi_o, e_p, e_l))
    assert all(v < 1e-11 for v in figs.values()) and abs(chi - chi_o) <= 1e-9 * chi_o and done == 3 and e_p < 1e-9 and e_l < 1e-9
    fixed = set(int(v) for v in g["fixed_landmarks"]); l = next(int(l) for l, _, _ in pri["lm"] if int(l) not in fixed)
    G.set_edges_active("observation", np.flatnonzero(np.asarray(g["pl_l"]) == l))
    assert G.find_isolated_vertex() is None
    done, _ = G.optimize(1); assert done == 1
    G.close()


def test_with_marginals(pkg, po, bench_graphs):
    """compute_marginals with a mask against the dense inverse of the oracle's H on masked(g) (test_gpu_marginals.check_against_dense,
    1e-8 per block); a flag change makes the results stale."""
    g, a_pp, a_pl, _, _ = case(bench_graphs, "bench1000")
    G = handle(pkg, "bench1000", g, None, None); switch_off(G, a_pp, a_pl); G.optimize(3); G.compute_marginals()
    check_against_dense(po, em.masked(g, a_pp, a_pl), G)
    U = handle(pkg, "bench1000", g, None, None); U.optimize(3); U.compute_marginals()
    wider = float(np.trace(G.landmark_covariances().sum(0)) / np.trace(U.landmark_covariances().sum(0)))
    print("marginals + mask: within 1e-8 of the dense inverse; trace of the landmark covariances with / without the mask %.4f" % wider)
    assert wider > 1.0                                               # information was taken away
    G.set_edge_active("observation", int(np.flatnonzero(a_pl)[0]), False)
    with pytest.raises(pkg.binding.GsError) as e:
        G.pose_covariances()
    assert e.value.code == -6
    G.compute_marginals(); G.pose_covariances()
    G.close(); U.close()


# ---------------------------------------------------------------- 6. gs_deactivate_edges_above
def test_rejection_of_the_outlier_edges(pkg, po, bench_graphs):
    """outlier_case (test_robust_cpu.py): Huber iterations as there, then gs_deactivate_edges_above on the observation edges at the
    midpoint of the widest relative gap of the checker's sorted s (from delta^2 up; the gap >= 1e-6 is the input's condition,
    test_edge_mask_cpu.py): the device's set equals the checker's exactly.  Then plain iterations on the inliers: parity with the oracle
    run of the same procedure at item 3's bars, and a landmark RMSE to the clean optimum no worse than the oracle's plain figure."""
    xP, xL, go, pick, P_o, L_o, s_o = huber_outlier_state(po, bench_graphs)
    kernels = {"observation": ("huber", OUTLIER_DELTA)}
    thr, gap = em.widest_gap_threshold(s_o, OUTLIER_DELTA ** 2)
    assert gap >= GAP_MIN
    want = s_o > thr
    Y = handle(pkg, "bench1000", go, None, None); dy, _ = Y.optimize(10); oy = make_oracle_graph(po, go); oy.optimize(10, ordering=1)
    y_est = max(rel(Y.poses(), oy.poses()), rel(Y.landmarks(), oy.landmarks())); plain_rmse_oracle = lm_rmse(oy.landmarks(), xL)
    Y.close()
    G = handle(pkg, "bench1000", go, None, None); G.set_robust_kernel("observation", *kernels["observation"])
    done, _ = G.optimize(HUBER_ITERATIONS); assert done == HUBER_ITERATIONS
    e_huber = max(rel(G.poses(), P_o), rel(G.landmarks(), L_o))
    s_dev, _ = G.edge_chi2("observation")
    n_off = G.deactivate_edges_above("observation", thr)
    got = ~G.edges_active("observation")
    print("rejection: threshold %.6g (gap %.3g), device s vs checker %.2e, Huber estimates %.2e; switched off %d, checker %d, same set %s, re-targeted among them %d of %d"
          % (thr, gap, rel(s_dev, s_o), e_huber, n_off, want.sum(), np.array_equal(got, want), np.isin(np.flatnonzero(got), pick).sum(), len(pick)))
    assert n_off == want.sum() == G.n_inactive_edges("observation") and np.array_equal(got, want)
    assert G.deactivate_edges_above("observation", thr) == 0        # the inactive edges stay inactive and are not counted again
    G.set_robust_kernel("observation", "none")
    done, st = G.optimize(10); assert done == 10
    og = make_oracle_graph(po, dict(em.masked(go, np.ones(len(go["pp_i"]), bool), ~want), pose_est=P_o, lm_est=L_o)); og.optimize(10, ordering=1)
    e_est = max(rel(G.poses(), og.poses()), rel(G.landmarks(), og.landmarks())); e_chi = abs(st.chi2_final - og.chi2()) / og.chi2()
    rmse, rmse_o = lm_rmse(G.landmarks(), xL), lm_rmse(og.landmarks(), xL)
    print("rejection: re-optimised on the inliers: estimates %.2e (plain yardstick %.2e) chi2 %.2e; landmark RMSE to the clean optimum %.3e m (oracle, same procedure %.3e m; oracle plain, no rejection %.4f m)"
          % (e_est, y_est, e_chi, rmse, rmse_o, plain_rmse_oracle))
    assert e_est <= max(4 * y_est, 1e-9) and e_chi <= 1e-10
    assert rmse <= plain_rmse_oracle
    G.close()


def test_keep_connected_spares_a_cones_only_edge(pkg, po, bench_graphs):
    """The outlier graph plus one cone seen once, 3 m off its measurement: a candidate.  keep_connected = 1 leaves that edge active
    (and the device's set equals the restated rule's); keep_connected = 0 switches it off, and the next call that computes refuses."""
    xP, xL, go, pick, P_o, L_o, s_o = huber_outlier_state(po, bench_graphs)
    thr, _ = em.widest_gap_threshold(s_o, OUTLIER_DELTA ** 2)
    M, E = len(go["lm_est"]), len(go["pl_p"]); p = 10
    z = np.asarray(go["pl_z"]).reshape(-1, 2)[np.flatnonzero(np.asarray(go["pl_p"]) == p)[0]]
    c, s_ = np.cos(P_o[p, 2]), np.sin(P_o[p, 2]); l_at = P_o[p, :2] + [c * z[0] - s_ * z[1], s_ * z[0] + c * z[1]] + [3.0, 0.0]
    g2 = dict(go, pose_est=P_o, lm_est=np.vstack([L_o, l_at]), pl_p=np.r_[go["pl_p"], p].astype(np.int32), pl_l=np.r_[go["pl_l"], M].astype(np.int32),
              pl_z=np.vstack([np.asarray(go["pl_z"]).reshape(-1, 2), z]), pl_info=np.vstack([np.asarray(go["pl_info"]).reshape(-1, 4), np.asarray(go["pl_info"]).reshape(-1, 4)[:1]]))
    s_ref = rr.edge_s(g2, g2["pose_est"], g2["lm_est"])[1]
    cand = s_ref > thr
    assert cand[E] and min(abs(s_ref / thr - 1)) > 1e-6
    ones = np.ones(len(g2["pp_i"]), bool)
    for keep in (1, 0):
        _, want, off = em.deactivate(g2, ones, np.ones(E + 1, bool), 1, cand, bool(keep))
        G = handle(pkg, "bench1000", g2, None, None)
        n_off = G.deactivate_edges_above("observation", thr, keep_connected=keep)
        got = G.edges_active("observation")
        print("keep_connected=%d: candidates %d, switched off %d (rule %d), the lone cone's edge active %s, isolated %s" % (keep, cand.sum(), n_off, len(off), got[E], G.find_isolated_vertex()))
        assert n_off == len(off) and np.array_equal(got, want) and got[E] == bool(keep)
        if keep:
            assert G.find_isolated_vertex() is None
            done, _ = G.optimize(2); assert done == 2
        else:
            assert G.find_isolated_vertex() == ("landmark", M)
            with pytest.raises(pkg.binding.GsError) as e:
                G.optimize(1)
            assert e.value.code == -1 and "landmark %d" % M in str(e.value)
        G.close()


# ---------------------------------------------------------------- 7. refusals on the device
@pytest.mark.parametrize("gather", [0, 1])
def test_an_isolated_landmark_is_refused_before_anything_is_launched(pkg, bench_graphs, gather):
    b = pkg.binding
    g = bench_graphs(50, 30)[1]
    G = handle(pkg, "bench50", g, None, None, linearize_gather=gather)
    done, _ = G.optimize(2); assert done == 2
    P0, L0 = G.poses().copy(), G.landmarks().copy()
    l = 7; assert l not in g["fixed_landmarks"]
    edges = np.flatnonzero(np.asarray(g["pl_l"]) == l)
    G.set_edges_active("observation", edges)
    assert G.find_isolated_vertex() == ("landmark", l)
    for call in (lambda: G.optimize(1), G.chi2, G.linearize, G.iterate, G.compute_marginals, lambda: G.edge_chi2("observation"), lambda: G.optimize_lm(1),
                 lambda: G.deactivate_edges_above("observation", 1.0)):
        with pytest.raises(b.GsError) as e:
            call()
        assert e.value.code == -1 and "landmark %d" % l in str(e.value), str(e.value)
    G.sync_estimates()
    assert np.array_equal(G.poses(), P0) and np.array_equal(G.landmarks(), L0)      # the estimates are untouched
    G.set_edge_active("observation", int(edges[0]), True)
    assert G.find_isolated_vertex() is None
    done, _ = G.optimize(1); assert done == 1 and np.isfinite(G.chi2())
    with pytest.raises(b.GsError) as e:                                              # shards: refused on a device handle too
        G.dist_configure(0, 2)
    assert e.value.code == -1 and "inactive" in str(e.value)
    G.close()
