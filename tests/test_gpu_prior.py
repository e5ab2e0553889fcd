"""Prior edges on the GPU (gs_add_pose_prior / gs_add_pose_xy_prior / gs_add_landmark_prior, csrc/gs_prior.hip) against the checker
tests/prior_ref.py: the UNCHANGED CPU oracle on the graph augmented by one auxiliary fixed pose at the origin and one edge per prior
(test_prior_cpu.py pins that equivalence against plain numpy and establishes, without a GPU, that the compared trajectories converge
and that every compared LM trial has a margin >= 1e-3).

Tolerances are the project's existing bars: H / b arrays 1e-11 of the array's largest entry (test_gpu_parity.py), increments 1e-8 of
the largest increment (1e-9 on the random graph), estimates and chi2 1e-9, per-prior chi2 1e-11 of the largest (the bound
test_gpu_robust.py puts on edge_chi2), LM max(4 x the plain gs_optimize yardstick, 1e-9) (test_gpu_lm.py), marginals REL = 1e-8 per block
(test_gpu_marginals.py).  Every test prints its figures before it asserts (-s); the printed run is profiles/prior_gpu_suite.txt.

Prior set per graph (prior_ref.prior_set): SE2 priors with z_theta != 0 and a full Omega on about every 7th pose, XY priors on other
poses, landmark priors on about every 5th cone, two more priors on one pose and one more on one cone, one prior on a fixed pose and one
on a fixed cone."""
import numpy as np
import pytest

import lm_ref
import prior_ref as pr
import robust_ref as rr
import selinv_exec as sx
from conftest import append_tail, make_oracle_graph, random_graph, split_for_growth
from test_gpu_marginals import REL, rel_err
from test_prior_cpu import LM_ITERATIONS, LM_REJECTION_LAMBDA0, LM_REJECTION_TRIALS, gauge_free, lm_case, lm_checker, lm_rejection_case
from test_robust_cpu import perturbed

pytestmark = pytest.mark.gpu


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300))


def fresh(pkg, g, pri=None, debug=None, **kw):
    G = pkg.Graph(device=0, debug=debug, **kw)
    G.load_bench_graph(g)
    if pri is not None:
        pr.add_to(G, pri)
    return G


_graphs = {}


def graph_of(pkg, bench_graphs, frontend, name):
    """(graph, its prior set), built once per name and left unchanged"""
    if name not in _graphs:
        if name == "random":
            g = random_graph(7)
        elif name == "track400_K16":
            g = pkg.track.bench_graph(pkg.track.generate(400, 150, 16), frontend)
        else:
            g = bench_graphs(*{"bench50": (50, 30), "bench1000": (1000, 200)}[name])[1]
        _graphs[name] = (g, pr.prior_set(g))
    return _graphs[name]


def oracle(po, g, pri, P=None, L=None):
    return make_oracle_graph(po, pr.augment(g, pri, P, L))


def carriers(g, pri):
    """boolean masks of the FREE poses / landmarks that carry a prior"""
    cp = np.zeros(len(g["pose_est"]), dtype=bool); cl = np.zeros(len(g["lm_est"]), dtype=bool)
    cp[[p for p, _, _, _ in pri["pose"]]] = True; cl[[l for l, _, _ in pri["lm"]]] = True
    cp[np.asarray(g["fixed_poses"], dtype=np.int64)] = False; cl[np.asarray(g["fixed_landmarks"], dtype=np.int64)] = False
    return cp, cl


NAMES = ["bench50", "bench1000", "random", "track400_K16"]


# ---------------------------------------------------------------- 1. the system
@pytest.mark.parametrize("gather", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_system_with_priors_matches_the_augmented_oracle(pkg, po, bench_graphs, frontend, name, gather):
    """linearize() + export_system(): every array against the augmented oracle's blocks (1e-11 of the array's largest entry); the
    difference to the same handle's export after clear_priors() is non-zero only in the diagonal blocks and b of prior-carrying free
    vertices (exactly zero elsewhere, off-diagonal blocks bit-identical)."""
    g, pri = graph_of(pkg, bench_graphs, frontend, name)
    ref = pr.strip(oracle(po, g, pri).linearize_blocks(), g)
    G = fresh(pkg, g, pri, linearize_gather=gather)
    G.linearize(); S = G.export_system()
    figs = {k: rel(S[k], ref[k]) for k in ref}
    G.clear_priors(); G.linearize(); S0 = G.export_system()
    cp, cl = carriers(g, pri)
    print("%s gather=%d: " % (name, gather) + " ".join("%s %.2e" % kv for kv in figs.items()) + " | carriers %d poses %d cones" % (cp.sum(), cl.sum()))
    for k, v in figs.items():
        assert v < 1e-11, k
    assert np.array_equal(S["Hpp_off"], S0["Hpp_off"]) and np.array_equal(S["Hpl"], S0["Hpl"])
    for key, mask in (("Hpp_diag", cp), ("b_pose", cp), ("Hll_diag", cl), ("b_lm", cl)):
        d = S[key] - S0[key]
        assert np.abs(d[~mask]).max(initial=0.0) == 0.0, key
        assert np.all(np.abs(d[mask]).max(axis=1) > 0), key
    G.close()


# ---------------------------------------------------------------- 2. chi2 and per-prior chi2
def grown_with_tail(pkg, g, h=6, keep=600, extra=0, **kw):
    """a handle grown by the last h poses of the stretch's first keep - extra poses (test_gpu_lm.py's grown plan: 1000 / 200, keep = 600,
    6 poses and 2 cones), and (base, tail, full) of the whole stretch; extra poses stay in `tail` for a later step"""
    base, tail, full = split_for_growth(g, h + extra, keep)
    G = fresh(pkg, base, **kw); G.initialize_optimization()
    new_lms = append_tail(G, tail, poses=(0, h)); G.initialize_optimization()
    assert G.plan_growths() > 0, G.growth_refusal()
    return G, base, tail, full, new_lms


def tail_priors(full, n_tail_poses, n_tail_lms):
    """the full graph's prior set plus priors on an old pose, an old cone, a tail pose and a tail cone"""
    rng = np.random.default_rng(77)
    pri = pr.prior_set(full)
    N, M = len(full["pose_est"]), len(full["lm_est"])
    P, L = np.asarray(full["pose_est"]), np.asarray(full["lm_est"])
    extra_p = [100, N - 1, N - n_tail_poses]; extra_l = [10, M - 1] if n_tail_lms > 0 else [10]
    for p in extra_p:
        z, W = pr.embed_xy(P[p, :2] + rng.normal(0, 0.2, 2), pr.spd(rng, 2, 0.3)); pri["pose"].append((p, z, W, True))
    pri["pose"].append((N - 2, P[N - 2] + rng.normal(0, 0.1, 3), pr.spd(rng, 3, 0.4), False))
    for l in extra_l:
        pri["lm"].append((l, L[l] + rng.normal(0, 0.2, 2), pr.spd(rng, 2, 0.02)))
    return pri


@pytest.mark.parametrize("name,gather", [(n, k) for n in NAMES for k in (0, 1)] + [("grown", 0)])
def test_chi2_and_per_prior_chi2(pkg, po, bench_graphs, frontend, name, gather):
    """gs_chi2 against the augmented oracle (1e-9) and gs_get_prior_chi2 against numpy (1e-11 of the largest), at the initial
    estimates and after two iterations; priors on fixed vertices are reported by the query and stay out of the total.  Grown plan: the
    tail arenas' poses and cones carry priors too."""
    if name == "grown":
        G, base, tail, g, new_lms = grown_with_tail(pkg, bench_graphs(1000, 200)[1])
        assert new_lms > 0
        pri = tail_priors(g, 6, new_lms); pr.add_to(G, pri)
    else:
        g, pri = graph_of(pkg, bench_graphs, frontend, name)
        G = fresh(pkg, g, pri, linearize_gather=gather)
    for step in (0, 2):
        if step:
            done, _ = G.optimize(step); assert done == step
        P, L = G.poses(), G.landmarks()
        chi_o = oracle(po, g, pri, P, L).chi2(); chi = G.chi2()
        cp_ref, cl_ref = pr.chi2_each(pri, P, L)
        cp, cl = G.prior_chi2("pose"), G.prior_chi2("landmark")
        _, _, _, _, share = pr.contributions(g, pri, P, L)
        print("%s gather=%d after %d iterations: chi2 %.10g (oracle %.10g, rel %.2e, prior share %.6g) per-prior pose %.2e (%d) landmark %.2e (%d)"
              % (name, gather, step, chi, chi_o, abs(chi - chi_o) / chi_o, share, rel(cp, cp_ref), len(cp), rel(cl, cl_ref), len(cl)))
        assert abs(chi - chi_o) <= 1e-9 * chi_o
        assert len(cp) == len(pri["pose"]) == G.n_pose_priors and len(cl) == len(pri["lm"]) == G.n_landmark_priors
        assert rel(cp, cp_ref) < 1e-11 and rel(cl, cl_ref) < 1e-11
        assert share > 0 and (name == "grown" or abs((chi - share) - make_oracle_graph(po, dict(g, pose_est=P, lm_est=L)).chi2()) <= 1e-9 * chi)
    if name == "grown":
        assert G.plan_growths() > 0 and G.growth_refusal() == ""
    G.close()


# ---------------------------------------------------------------- 3. iterations
@pytest.mark.parametrize("name,variant,gather", [(n, v, 0) for n in NAMES for v in (3, 4)] + [("bench1000", 3, 1), ("bench1000", 4, 1), ("bench50", 3, 1), ("random", 3, 1)])
def test_iterations_with_priors_match_the_oracle(pkg, po, bench_graphs, frontend, name, variant, gather):
    """(gather = 1: inside an iteration the prior share of chi2 goes into chi2[0] behind k_reduce_chi2, which k_update reads for the
    history — chi2_initial / chi2_final below — and the stop rule.)
    One step's increment (1e-8 of the largest increment; 1e-9 on the random graph) and, on the graphs whose trajectory converges
    (test_prior_cpu.py), the estimates after optimize(10) and the chi2 behind them (1e-9) against the oracle on the augmented graph;
    whole-tree and per-level launches (tree = 0) bitwise equal."""
    g, pri = graph_of(pkg, bench_graphs, frontend, name)
    og = oracle(po, g, pri); og.build_system(); og.apply_update(og.solve_ldlt(1)); dp_o, dl_o = og.delta(); dp_o = dp_o[:-1]
    G = fresh(pkg, g, pri, factor_variant=variant, linearize_gather=gather)
    done, st = G.optimize(1); assert done == 1
    dp, dl = G.export_delta(); sc = max(np.abs(dp_o).max(), np.abs(dl_o).max())
    e_inc = max(np.abs(dp - dp_o).max(), np.abs(dl - dl_o).max()) / sc
    chi_0 = oracle(po, g, pri).chi2(); e_c = abs(st.chi2_initial - chi_0) / chi_0
    print("%s v%d gather=%d: increment %.2e chi2 at the linearisation point %.2e" % (name, variant, gather, e_inc, e_c))
    assert e_c <= 1e-9
    assert e_inc < (1e-9 if name == "random" else 1e-8)
    assert rel(G.poses(), og.poses()[:-1]) < 1e-9 and rel(G.landmarks(), og.landmarks()) < 1e-9
    G.close()
    if name == "random":
        return
    og = oracle(po, g, pri); done, chi_o, _ = og.optimize(10, ordering=1); assert done == 10
    A = fresh(pkg, g, pri, factor_variant=variant, linearize_gather=gather); da, sa = A.optimize(10)
    B = fresh(pkg, g, pri, factor_variant=variant, linearize_gather=gather, debug=dict(tree=0)); db, sb = B.optimize(10)
    U = fresh(pkg, g, pri, factor_variant=variant, linearize_gather=gather); du, su = U.optimize_until(30, 1e-6)
    ou = oracle(po, g, pri); dou, _, failed = ou.optimize_until(30, 1e-6, ordering=1)
    print("%s v%d gather=%d optimize_until(30, 1e-6): stopped after %d (oracle %d), poses %.2e" % (name, variant, gather, du, dou, rel(U.poses(), ou.poses()[:-1])))
    assert du == dou and not failed and rel(U.poses(), ou.poses()[:-1]) < 1e-9 and rel(U.landmarks(), ou.landmarks()) < 1e-9
    U.close()
    e_p, e_l = rel(A.poses(), og.poses()[:-1]), rel(A.landmarks(), og.landmarks())
    e_c0, e_c = abs(sa.chi2_initial - chi_o[0]) / chi_o[0], abs(sa.chi2_final - og.chi2()) / og.chi2()
    same = np.array_equal(A.poses(), B.poses()) and np.array_equal(A.landmarks(), B.landmarks()) and sa.chi2_final == sb.chi2_final
    print("%s v%d gather=%d optimize(10): poses %.2e landmarks %.2e chi2_initial %.2e chi2_final %.2e (%.10g); tree=0 bit-identical %s"
          % (name, variant, gather, e_p, e_l, e_c0, e_c, sa.chi2_final, same))
    assert da == 10 and db == 10 and e_p < 1e-9 and e_l < 1e-9 and e_c0 <= 1e-9 and e_c <= 1e-9 and same
    assert sa.n_pose_priors == len(pri["pose"]) and sa.n_landmark_priors == len(pri["lm"])
    A.close(); B.close()


# ---------------------------------------------------------------- 4. a soft gauge
def marginals_against_dense(po, g, pri, G):
    """the handle's covariance blocks against the dense inverse of the augmented oracle's H at the handle's estimates"""
    ga = pr.augment(g, pri, G.poses(), G.landmarks())
    H, po_, lo_ = sx.dense_system(make_oracle_graph(po, ga))
    ref = sx.reference_blocks(np.linalg.inv(H), po_, lo_, ga)
    N, Epp, Epl = len(g["pose_est"]), len(g["pp_i"]), len(g["pl_p"])
    ref = (ref[0][:N], ref[1], ref[2][:Epp], ref[3][:Epl])
    got = (G.pose_covariances(), G.landmark_covariances(), G.odometry_edge_covariances(), G.observation_edge_covariances())
    return got, {k: rel_err(a, b) for k, a, b in zip(("poses", "landmarks", "odometry edges", "observation edges"), got, ref)}


@pytest.mark.parametrize("name", ["bench50", "bench1000"])
def test_a_strong_prior_in_place_of_the_fixed_flags(pkg, po, bench_graphs, frontend, name):
    """No fixed vertex, one strong SE2 prior on pose 0: optimize(10) against the oracle (1e-9); compute_marginals(): pose 0 has a
    covariance (non-zero, SPD) and every block matches the dense inverse of the oracle's H (REL)."""
    gf, pri = gauge_free(graph_of(pkg, bench_graphs, frontend, name)[0])
    og = oracle(po, gf, pri); done, _, _ = og.optimize(10, ordering=1); assert done == 10
    G = fresh(pkg, gf, pri); done, st = G.optimize(10)
    e_p, e_l, e_c = rel(G.poses(), og.poses()[:-1]), rel(G.landmarks(), og.landmarks()), abs(st.chi2_final - og.chi2()) / og.chi2()
    G.compute_marginals()
    got, figs = marginals_against_dense(po, gf, pri, G)
    print("%s gauge-free: poses %.2e landmarks %.2e chi2 %.2e | marginals " % (name, e_p, e_l, e_c) + " ".join("%s %.2e" % kv for kv in figs.items())
          + " | Sigma(pose 0) diag %s" % np.diag(got[0][0]))
    assert done == 10 and st.n_free_poses == len(gf["pose_est"]) and e_p < 1e-9 and e_l < 1e-9 and e_c <= 1e-9
    assert np.abs(got[0][0]).max() > 0 and np.linalg.eigvalsh(got[0][0]).min() > 0
    for k, v in figs.items():
        assert v < REL, k
    G.close()


# ---------------------------------------------------------------- 5. Levenberg-Marquardt
def test_lm_with_priors_matches_the_checker(pkg, po, bench_graphs):
    """optimize_lm(6) from the perturbed start of test_gpu_lm.py (x1, seed 1) with the bench 1000 / 200 prior set against lm_ref on the
    augmented graph: trial counts exactly, lambda[], chi2[] and the estimates within max(4 x the plain gs_optimize(6) yardstick, 1e-9);
    the margin >= 1e-3 asserted on every compared trial."""
    g, pri, P1, L1 = lm_case(po, bench_graphs)
    r = lm_checker(po, g, pri, P1, L1)
    assert all(t["margin"] >= lm_ref.MIN_MARGIN for t in r["trials"])
    gs = dict(g, pose_est=P1, lm_est=L1)
    A = fresh(pkg, gs, pri); done, sa = A.optimize(LM_ITERATIONS); assert done == LM_ITERATIONS
    og = oracle(po, gs, pri); og.optimize(LM_ITERATIONS, ordering=1)
    y_est = max(rel(A.poses(), og.poses()[:-1]), rel(A.landmarks(), og.landmarks())); y_chi = abs(sa.chi2_final - og.chi2()) / og.chi2()
    A.close()
    tol_est, tol_chi = max(4 * y_est, 1e-9), max(4 * y_chi, 4 * y_est, 1e-9)
    G = fresh(pkg, gs, pri); done, st, info = G.optimize_lm(LM_ITERATIONS)
    e_chi = float(np.abs(info["chi2"] / r["chi2"] - 1).max()); e_lam = float(np.abs(info["lambda"] / r["lam"] - 1).max())
    e_est = max(rel(G.poses(), r["P"][:-1]), rel(G.landmarks(), r["L"])); e_fin = abs(st.chi2_final - r["chi2_final"]) / r["chi2_final"]
    print("LM with priors: trials GPU %s checker %s min margin %.2e | plain(6) estimates %.2e chi2 %.2e | LM chi2[] %.2e lambda[] %.2e estimates %.2e chi2_final %.2e lambda_0 %.6e / %.6e"
          % (info["n_trials"].tolist(), r["n_trials"].tolist(), r["min_margin"], y_est, y_chi, e_chi, e_lam, e_est, e_fin, info["lambda_initial"], r["lambda_initial"]))
    assert done == LM_ITERATIONS and info["n_trials"].tolist() == r["n_trials"].tolist() and info["rejected"] == r["rejected"] and info["terminated"] == 0
    assert abs(info["lambda_initial"] - r["lambda_initial"]) <= 1e-11 * r["lambda_initial"]
    assert e_chi <= tol_chi and e_lam <= tol_chi and e_fin <= tol_chi and e_est <= tol_est
    G.close()


@pytest.mark.parametrize("gather", [0, 1])
def test_lm_with_priors_through_rejected_trials(pkg, po, bench_graphs, gather):
    """The rejected-trial path with priors: restore the estimates, chi_new from the chi2-only prior pass, linearise again, add the priors
    again, damp.  Seed 2's x1 with the prior set and initial_lambda = 1e-12 (test_prior_cpu.py: trials [1, 1, 1, 1, 10, 1], nine
    rejections, every margin >= 2.5e-2) against lm_ref on the augmented graph: trial counts exactly, lambda[], chi2[] and the estimates
    within max(4 x the plain gs_optimize(6) yardstick, 1e-9); both linearisation paths."""
    g, pri, P1, L1 = lm_rejection_case(po, bench_graphs)
    r = lm_checker(po, g, pri, P1, L1, initial_lambda=LM_REJECTION_LAMBDA0)
    assert r["n_trials"].tolist() == LM_REJECTION_TRIALS and all(t["margin"] >= lm_ref.MIN_MARGIN for t in r["trials"])
    gs = dict(g, pose_est=P1, lm_est=L1)
    A = fresh(pkg, gs, pri, linearize_gather=gather); done, sa = A.optimize(LM_ITERATIONS); assert done == LM_ITERATIONS
    og = oracle(po, gs, pri); og.optimize(LM_ITERATIONS, ordering=1)
    y_est = max(rel(A.poses(), og.poses()[:-1]), rel(A.landmarks(), og.landmarks())); y_chi = abs(sa.chi2_final - og.chi2()) / og.chi2()
    A.close()
    tol_est, tol_chi = max(4 * y_est, 1e-9), max(4 * y_chi, 4 * y_est, 1e-9)
    G = fresh(pkg, gs, pri, linearize_gather=gather); done, st, info = G.optimize_lm(LM_ITERATIONS, initial_lambda=LM_REJECTION_LAMBDA0)
    e_chi = float(np.abs(info["chi2"] / r["chi2"] - 1).max()); e_lam = float(np.abs(info["lambda"] / r["lam"] - 1).max())
    e_est = max(rel(G.poses(), r["P"][:-1]), rel(G.landmarks(), r["L"])); e_fin = abs(st.chi2_final - r["chi2_final"]) / r["chi2_final"]
    print("LM with priors, rejections, gather=%d: trials GPU %s checker %s rejected %d / %d min margin %.2e | plain(6) estimates %.2e chi2 %.2e | LM chi2[] %.2e lambda[] %.2e estimates %.2e chi2_final %.2e"
          % (gather, info["n_trials"].tolist(), r["n_trials"].tolist(), info["rejected"], r["rejected"], r["min_margin"], y_est, y_chi, e_chi, e_lam, e_est, e_fin))
    assert done == LM_ITERATIONS and info["n_trials"].tolist() == r["n_trials"].tolist() and info["rejected"] == r["rejected"] == 9 and info["terminated"] == 0
    assert e_chi <= tol_chi and e_lam <= tol_chi and e_fin <= tol_chi and e_est <= tol_est
    assert abs(G.chi2() - st.chi2_final) <= 1e-9 * st.chi2_final
    G.close()


# ---------------------------------------------------------------- 6. marginals with priors on a gauged graph
@pytest.mark.parametrize("name", ["bench50", "bench1000"])
def test_marginals_with_priors_match_the_dense_inverse(pkg, po, bench_graphs, frontend, name):
    g, pri = graph_of(pkg, bench_graphs, frontend, name)
    G = fresh(pkg, g, pri); G.optimize(3); G.compute_marginals()
    got, figs = marginals_against_dense(po, g, pri, G)
    Z = fresh(pkg, g); Z.optimize(3); Z.compute_marginals()
    tighter = float(np.trace(Z.pose_covariances().sum(0)) / np.trace(got[0].sum(0)))
    print("%s marginals with priors: " % name + " ".join("%s %.2e" % kv for kv in figs.items()) + " | trace of the pose covariances without / with priors %.3f" % tighter)
    for k, v in figs.items():
        assert v < REL, k
    assert tighter > 1.0                                             # information was added
    with pytest.raises(pkg.binding.GsError) as e:                    # a change of the priors makes the results stale
        G.add_pose_xy_prior(5, [0, 0], np.eye(2)); G.pose_covariances()
    assert e.value.code == -6
    G.close(); Z.close()


# ---------------------------------------------------------------- 7. growth
def test_priors_do_not_disturb_growth(pkg, po, bench_graphs):
    """On the grown handle (6 tail poses, 2 tail cones): priors on an old pose, an old cone, tail poses and a tail cone, then
    initialize_optimization(): no structure phase of any kind (plan_growths unchanged, no refusal); chi2 and optimize(6) match the oracle and a
    fresh handle holding the same graph and priors (1e-9).  Then one more keyframe WITH its XY prior in the same step: absorbed by growth."""
    g0 = bench_graphs(1000, 200)[1]
    G, base, tail, full7, new_lms = grown_with_tail(pkg, g0, extra=1)
    _, _, full = split_for_growth(g0, 6, 599)                       # what the handle holds now: the stretch without its last pose
    assert G.n_poses == len(full["pose_est"]) and G.n_landmarks == len(full["lm_est"]) and new_lms > 0
    n0 = G.plan_growths()
    pri = tail_priors(full, 6, new_lms); pr.add_to(G, pri)
    G.initialize_optimization()
    assert G.plan_growths() == n0 and n0 > 0 and G.growth_refusal() == ""
    chi, chi_o = G.chi2(), oracle(po, full, pri).chi2()
    og = oracle(po, full, pri); og.optimize(6, ordering=1)
    F = fresh(pkg, full, pri); df, sf = F.optimize(6)
    dg, sg = G.optimize(6)
    figs = (abs(chi - chi_o) / chi_o, rel(G.poses(), og.poses()[:-1]), rel(G.landmarks(), og.landmarks()), abs(sg.chi2_final - og.chi2()) / og.chi2(),
            rel(G.poses(), F.poses()), rel(G.landmarks(), F.landmarks()))
    print("grown + priors: chi2 %.2e | optimize(6) vs oracle poses %.2e landmarks %.2e chi2 %.2e | vs fresh handle poses %.2e landmarks %.2e; growths %d" % (figs + (n0,)))
    assert dg == 6 and df == 6 and sg.n_growths == n0 and all(f <= 1e-9 for f in figs)
    # one more keyframe with its GPS prior in the same step
    more = append_tail(G, tail, poses=(6, 7))
    p_new = len(full7["pose_est"]) - 1
    z, W = pr.embed_xy(np.asarray(full7["pose_est"])[p_new, :2] + [0.1, -0.15], 0.5 * np.eye(2)); pri["pose"].append((p_new, z, W, True))
    G.add_pose_xy_prior(p_new, z[:2], W[:2, :2])
    G.initialize_optimization()
    assert G.plan_growths() == n0 + 1 and G.growth_refusal() == "", G.growth_refusal()
    # (the oracle graph in the handle's edge order: the stretch without its last pose, then that pose's edges)
    full_now = dict(full7, lm_est=np.asarray(full7["lm_est"])[:G.n_landmarks])
    P, L = G.poses(), G.landmarks()
    chi, chi_o = G.chi2(), oracle(po, full_now, pri, P, L).chi2()
    cp = G.prior_chi2("pose"); cp_ref, _ = pr.chi2_each(pri, P, L)
    print("one more keyframe with its XY prior: growths %d (+%d cones), chi2 %.2e, per-prior %.2e" % (G.plan_growths(), more, abs(chi - chi_o) / chi_o, rel(cp, cp_ref)))
    assert abs(chi - chi_o) <= 1e-9 * chi_o and rel(cp, cp_ref) < 1e-11 and cp[-1] > 0
    og = oracle(po, full_now, pri, P, L); og.optimize(2, ordering=1)
    done, st = G.optimize(2)
    assert done == 2 and rel(G.poses(), og.poses()[:-1]) < 1e-9 and rel(G.landmarks(), og.landmarks()) < 1e-9
    G.close(); F.close()


# ---------------------------------------------------------------- 8. no priors, no change
def test_a_handle_without_priors_is_bit_identical(pkg, bench_graphs, frontend):
    """Three handles after optimize(5): never touched; zero priors (empty bulk calls, clear_priors); priors added, used by a chi2 pass,
    then cleared.  Estimates bitwise equal, debug_schedule() unchanged."""
    g, pri = graph_of(pkg, bench_graphs, frontend, "bench1000")
    A = fresh(pkg, g)
    B = fresh(pkg, g); B.add_pose_priors([], np.zeros((0, 3)), np.zeros((0, 9))); B.add_landmark_priors([], np.zeros((0, 2)), np.zeros((0, 4))); B.clear_priors()
    C = fresh(pkg, g, pri); chi_with = C.chi2(); C.clear_priors()
    outs = []
    for H in (A, B, C):
        done, st = H.optimize(5); assert done == 5
        outs.append((H.poses(), H.landmarks(), st.chi2_final, H.debug_schedule()["raw"], st.n_pose_priors + st.n_landmark_priors))
    same = all(np.array_equal(o[0], outs[0][0]) and np.array_equal(o[1], outs[0][1]) and o[2] == outs[0][2] and np.array_equal(o[3], outs[0][3]) for o in outs)
    print("no priors: chi2 with priors %.10g, after clear %.17g; three handles bit-identical %s" % (chi_with, outs[2][2], same))
    assert same and all(o[4] == 0 for o in outs) and chi_with > 0
    for H in (A, B, C):
        H.close()


# ---------------------------------------------------------------- 9. robust kernels + priors
def test_huber_on_observations_leaves_the_priors_at_weight_one(pkg, po, bench_graphs, frontend):
    """Huber on the observation edges (delta = the median sqrt(s) of that kind at the start, as test_gpu_robust.py) with priors: the
    checker re-weights the graph's own edges first and appends the prior edges at weight 1.  System 1e-11, chi2 1e-9, three iterations 1e-9."""
    g, pri = graph_of(pkg, bench_graphs, frontend, "bench1000")
    P, L = perturbed(g, 1)
    kernels = {"observation": ("huber", rr.median_deltas(g, P, L)[1])}
    gs = dict(g, pose_est=P, lm_est=L)
    G = fresh(pkg, gs, pri); G.set_robust_kernel("observation", *kernels["observation"])
    ref = pr.strip(make_oracle_graph(po, pr.augment_robust(g, pri, P, L, kernels)).linearize_blocks(), g)
    G.linearize(); S = G.export_system()
    figs = {k: rel(S[k], ref[k]) for k in ref}
    share = pr.contributions(g, pri, P, L)[4]; chi_o = rr.robust_chi2(g, P, L, kernels) + share; chi = G.chi2()
    s, w = G.edge_chi2("observation")
    Po, Lo = P, L
    for _ in range(3):
        og = make_oracle_graph(po, pr.augment_robust(g, pri, Po, Lo, kernels)); done, _, _ = og.optimize(1, ordering=1); assert done == 1
        Po, Lo = og.poses()[:-1], og.landmarks()
    done, st = G.optimize(3)
    e_p, e_l = rel(G.poses(), Po), rel(G.landmarks(), Lo)
    chi_end = rr.robust_chi2(g, Po, Lo, kernels) + pr.contributions(g, pri, Po, Lo)[4]
    print("huber + priors: " + " ".join("%s %.2e" % kv for kv in figs.items()) + " chi2 %.2e (prior share %.4g of %.6g, %d edges down-weighted) | optimize(3) poses %.2e landmarks %.2e chi2 %.2e"
          % (abs(chi - chi_o) / chi_o, share, chi_o, int((w < 1).sum()), e_p, e_l, abs(st.chi2_final - chi_end) / chi_end))
    for k, v in figs.items():
        assert v < 1e-11, k
    assert (w < 1).any() and abs(chi - chi_o) <= 1e-9 * chi_o
    assert done == 3 and e_p < 1e-9 and e_l < 1e-9 and abs(st.chi2_final - chi_end) <= 1e-9 * chi_end
    G.close()


# ---------------------------------------------------------------- 10. the refused cases on a device handle
@pytest.mark.parametrize("gather", [0, 1])
def test_refusals_on_a_device_handle(pkg, bench_graphs, gather):
    b = pkg.binding
    g = bench_graphs(50, 30)[1]
    G = fresh(pkg, g, linearize_gather=gather)
    G.add_pose_xy_prior(5, [0, 0], np.eye(2))
    with pytest.raises(b.GsError) as e:
        G.dist_configure(0, 2)
    assert e.value.code == -1 and "prior" in str(e.value)
    G.clear_priors(); G.dist_configure(0, 2)
    with pytest.raises(b.GsError) as e:
        G.add_landmark_prior(5, [0, 0], np.eye(2))
    assert e.value.code == -1 and "shard" in str(e.value)
    G.close()
    # a free landmark whose only measurement is a prior: refused at upload, nothing launched, the handle usable again once it is gone
    G = fresh(pkg, g, linearize_gather=gather)
    lone = len(g["lm_est"]); G.add_landmark(lone, [3.0, 4.0]); G.add_landmark_prior(lone, [3.1, 4.2], np.eye(2))
    for call in (G.chi2, G.linearize, lambda: G.optimize(1), G.compute_marginals, lambda: G.prior_chi2("landmark")):
        with pytest.raises(b.GsError) as e:
            call()
        assert e.value.code == -1 and "prior" in str(e.value)
    G.clear_priors()
    assert G.chi2() > 0
    G.close()


# ---------------------------------------------------------------- 11. estimates set on the host together with a prior
def test_estimates_set_with_a_prior_reach_the_device_before_iterate(pkg, po, bench_graphs, frontend):
    """set_*_estimate + add_*_prior + initialize_optimization() + iterate(): initialize_optimization keeps the plan when only priors
    changed, and gs_iterate does not look at the host: the call must have taken the new estimates up with the prior tables.  One
    iteration from the SET estimates against the oracle (1e-9), and bit for bit against a handle loaded with those estimates."""
    g, pri = graph_of(pkg, bench_graphs, frontend, "bench1000")
    P, L = perturbed(g, 3)
    G = fresh(pkg, g); G.initialize_optimization(); assert G.iterate() == 1; G.sync_estimates()
    for i in range(len(P)):
        G.set_pose_estimate(i, P[i])
    for i in range(len(L)):
        G.set_landmark_estimate(i, L[i])
    pr.add_to(G, pri)
    G.initialize_optimization()
    assert G.iterate() == 1
    G.synchronize(); G.sync_estimates()
    gs = dict(g, pose_est=P, lm_est=L)
    F = fresh(pkg, gs, pri); F.initialize_optimization(); assert F.iterate() == 1; F.synchronize(); F.sync_estimates()
    og = oracle(po, gs, pri); og.optimize(1, ordering=1)
    e_p, e_l = rel(G.poses(), og.poses()[:-1]), rel(G.landmarks(), og.landmarks())
    same = np.array_equal(G.poses(), F.poses()) and np.array_equal(G.landmarks(), F.landmarks())
    print("set estimates + priors + initialize + iterate: poses %.2e landmarks %.2e vs oracle; bit-identical to a handle loaded there %s" % (e_p, e_l, same))
    assert e_p < 1e-9 and e_l < 1e-9 and same
    # a refused upload stays pending: initialize_optimization reports it instead of rebuilding
    lone = len(g["lm_est"]); G.add_landmark(lone, [3.0, 4.0]); G.initialize_optimization()
    G.add_landmark_prior(lone, [3.1, 4.2], np.eye(2))
    for _ in range(2):
        with pytest.raises(pkg.binding.GsError) as e:
            G.initialize_optimization()
        assert e.value.code == -1 and "prior" in str(e.value)
    G.close(); F.close()


# ---------------------------------------------------------------- the chi2 finish at the one / two workgroup boundary
@pytest.mark.parametrize("gather", [0, 1])
def test_chi2_finish_at_the_workgroup_boundary(pkg, bench_graphs, gather):
    """One XY prior each on the first 255, 256 and 257 free poses of a 300-pose / 40-cone graph: the pass is one workgroup of 255 and of
    256 threads (its total added by the pass itself) and two workgroups at 257 (partials, then the totalling kernel).  The handle's chi2
    minus the chi2 of the same handle without priors is the sum of the per-prior values (1e-9 of chi2, the bar of
    test_chi2_and_per_prior_chi2), and the exported diagonal blocks and right-hand sides of the first 255 carrying poses do not depend
    on the count, bit for bit."""
    g = bench_graphs(300, 40)[1]
    rng = np.random.default_rng(256)
    P = np.asarray(g["pose_est"], dtype=np.float64).reshape(-1, 3)
    free = np.setdiff1d(np.arange(len(P)), np.asarray(g["fixed_poses"], dtype=np.int64))[:257]
    assert len(free) == 257
    z = P[free, :2] + rng.normal(0, 0.2, (257, 2)); W = np.stack([pr.spd(rng, 2, 0.3) for _ in range(257)])
    blocks = {}
    for count in (255, 256, 257):
        G = fresh(pkg, g, linearize_gather=gather)
        G.add_pose_xy_priors(free[:count], z[:count], W[:count].reshape(-1, 4))
        chi = G.chi2(); each = G.prior_chi2("pose")
        G.linearize(); S = G.export_system()
        blocks[count] = (S["Hpp_diag"][free[:255]].copy(), S["b_pose"][free[:255]].copy())
        G.clear_priors(); chi0 = G.chi2()
        print("gather=%d %d priors: chi2 %.10g without %.10g difference %.10g sum of the per-prior values %.10g (rel %.2e)"
              % (gather, count, chi, chi0, chi - chi0, each.sum(), abs((chi - chi0) - each.sum()) / chi))
        assert len(each) == count and np.all(each > 0)
        assert abs((chi - chi0) - each.sum()) <= 1e-9 * chi
        G.close()
    for count in (256, 257):
        assert np.array_equal(blocks[count][0], blocks[255][0]) and np.array_equal(blocks[count][1], blocks[255][1]), count
