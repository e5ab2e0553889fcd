"""gs_optimize_dogleg (Powell's dogleg with device-side step control) on the GPU against the checker tests/dogleg_ref.py: g2o's
OptimizationAlgorithmDogleg rule (restated from its published text, not pinned against a g2o build) on the CPU oracle.
test_dogleg_cpu.py establishes, without a GPU, that every trial of the compared trajectories is far from a tie — margin
|chi_old - chi_new| / chi_old >= 1e-3, every rho at least 1e-2 from 0, 0.25 and 0.75, every branch comparison decided by 1e-3 relative —
so that a decision is not rounding noise; the tests below assert those conditions again on every trial whose decision they compare.

Tolerances (the policy of test_gpu_lm.py): the yardstick of a comparison is the SAME comparison for plain gs_optimize on the same graph
and estimates (GPU against oracle), measured inside the test; the dogleg may be 4x that (it inherits two Hessian products and more
reductions), with the bound of the corresponding test_gpu_parity.py test as the floor (increments 1e-8 of the largest increment — 1e-9
on the random graph —, estimates and chi2 1e-9).  Every test prints its figures before it asserts (-s); the printed run is
profiles/dogleg_gpu_suite.txt.

Measured on an MI355X (that file): single trials — increment error plain / dogleg GN, DL, SD: 50/30 v3 8.0e-14 / 5.4e-14 6.1e-14 1.4e-13,
1000/200 v3 8.3e-11 / 3.5e-11 3.8e-11 5.6e-13, 1000/200 gather 1.6e-9 / 1.6e-9 1.7e-9 5.6e-13, random 1.8e-14 / 2.2e-15 2.1e-15 3.4e-16,
grown 4.2e-11 / 1.2e-10 6.4e-11 6.1e-13, track400 K16 1.4e-11 / 1.5e-11 2.8e-11 8.5e-14 (variant 4 alike); chi_new at most 1.9e-9 (the
gather path's DL trial, behind its 1.7e-9 increment), delta_final exact or 1 ulp; every trial accepted on both sides.  Trajectories from
x1: trials [4, 1, 1, 1, 1, 1] / [1] * 6 on both sides, kinds equal, chi2[] 8.9e-11 / 5.0e-13, delta[] 1 ulp, estimates 8.2e-12 / 4.7e-13
(plain(6) 1.2e-11); the terminated call bit-identical to its start; the robust / prior / polar / inactive run [5, 1, 1, 1] on both sides,
chi2 sequence 1.6e-12 (plain(4) chi2 8.1e-12)."""
import numpy as np
import pytest

import dogleg_ref as dr
import lm_ref
import polar_ref as plr
import prior_ref as pr
from conftest import make_oracle_graph
from test_dogleg_cpu import DEFAULT_TRIALS, SIDE_ITERATIONS, boundary_terminate, side_case, side_run, x1_run
from test_gpu_lm import fresh, graph_of, handle_of, rel
from test_lm_cpu import BOUNDARY, boundary_start, starts

pytestmark = pytest.mark.gpu
NUMERIC = -8


def kinds(a):
    return [dr.KINDS[int(k)] for k in a]


# ---------------------------------------------------------------- 1. one trial per kind
CASES_1 = [(n, v, 0) for n in ("bench50", "bench1000", "random", "grown", "track400_K16") for v in (3, 4) if not (n == "grown" and v == 4)] + [("bench1000", 3, 1)]
CASES_1 += [(n, 3, gather) for n in ("n255", "n256", "n257") for gather in (0, 1)]     # N + M = 255, 256, 257 (test_lm_cpu.boundary_start): the workgroup boundary of the vertex-parallel kernels


@pytest.mark.parametrize("name,variant,gather", CASES_1)
def test_one_trial_of_each_kind_matches_the_checker(pkg, po, bench_graphs, frontend, name, variant, gather):
    """ONE trial with initial_delta = 1e4 (GN: |h_gn| is below it on every graph here, asserted), 0.5 (|h_gn| + |h_sd|) (DL) and
    0.5 |h_sd| (SD), the two norms taken from the checker: the increment (export_delta), chi_new, delta_final and step_kind against the
    checker's trial.  Yardstick: the plain gs_optimize(1) increment and the chi2 behind it, GPU against oracle, same graph and
    estimates; the dogleg may be 4x that; floor 1e-8 of the largest increment (1e-9 random graph), 1e-9 for chi2 and delta.
    chi_new: every GN trial, and every DL or SD trial that meets it, is held to max(4 x the plain chi2 figure, 1e-9).  The plain figure
    is taken at the full Gauss-Newton step, a stationary point of the quadratic model, where an error of the increment enters chi2 only in
    second order; a DL or SD step ends where the gradient is not zero, so there chi2 inherits the increment's error in first order.  A DL
    or SD trial beyond the bound above must be explained by exactly that: with dx = the increment's measured difference from the checker's
    (itself held to its own bound) and grad chi2 = -2 b at x_try (b of the oracle's linearisation there), its chi_new may differ by at most
    that bound plus 2 sum_i |b_i| |dx_i| / chi_new.  The line printed says which bound a trial was held to.
    The verdict and the delta update are compared where the checker's trial is far from a tie (dogleg_ref.conditions); a rejected trial
    leaves the start's bits.
    Measured on an MI355X: one of the 33 trials needs the first-order term — 1000/200 on the gather path, DL: chi_new 1.9e-9 behind an
    increment error of 1.7e-9 (plain 1.6e-9 there, against 8.3e-11 on the fused path)."""
    g0 = graph_of(pkg, bench_graphs, frontend, name)
    kw = dict(factor_variant=variant, **({"linearize_gather": 1} if gather else {}))
    A, g = handle_of(pkg, g0, name, **kw)
    og = make_oracle_graph(po, g); og.build_system(); og.apply_update(og.solve_ldlt(1)); dp_o, dl_o = og.delta()
    done, st = A.optimize(1); assert done == 1
    dp, dl = A.export_delta(); sc = max(np.abs(dp_o).max(), np.abs(dl_o).max())
    y_inc = max(np.abs(dp - dp_o).max(), np.abs(dl - dl_o).max()) / sc
    y_chi = abs(A.chi2() - og.chi2()) / og.chi2()
    A.close()
    floor = 1e-9 if name == "random" else 1e-8
    tol_inc, tol_chi, tol_del = max(4 * y_inc, floor), max(4 * y_chi, 1e-9), max(4 * y_inc, 1e-9)
    m = dr.Model(po, g)
    pt = dr.Point(m, np.asarray(g["pose_est"], dtype=np.float64), np.asarray(g["lm_est"], dtype=np.float64))
    gn, sd = float(np.linalg.norm(pt.h_gn)), float(np.linalg.norm(pt.h_sd))
    assert sd < gn < 1e4
    for kind, delta in ((dr.GN, 1e4), (dr.DL, 0.5 * (gn + sd)), (dr.SD, 0.5 * sd)):
        t = dr.trial(m, pt, delta)
        assert t["kind"] == kind and min(t["gaps"]) >= dr.MIN_BRANCH_GAP
        G, _ = handle_of(pkg, g0, name, **kw)
        done, st, info = G.optimize_dogleg(1, initial_delta=delta, max_trials=1)
        dp, dl = G.export_delta(); sc = max(np.abs(t["dpose"]).max(), np.abs(t["dlm"]).max())
        e_inc = max(np.abs(dp - t["dpose"]).max(), np.abs(dl - t["dlm"]).max()) / sc
        e_old = abs(info["chi2"][0] - t["chi_old"]) / t["chi_old"]
        e_new = abs(st.chi2_final - t["chi_new"]) / t["chi_new"] if done == 1 else float("nan")
        e_del = abs(info["delta_final"] - t["delta_next"]) / t["delta_next"]
        decided = t["margin"] >= dr.MIN_MARGIN and dr.rho_gap(t["rho"]) >= dr.MIN_RHO_GAP
        first_order = 0.0                                            # a DL / SD trial beyond the plain bound: what the increment's difference explains
        if done == 1 and kind != dr.GN and e_new > tol_chi:
            B = make_oracle_graph(po, dict(g, pose_est=t["P"], lm_est=t["L"])).linearize_blocks()
            first_order = 2.0 * float((np.abs(B["b_pose"]) * np.abs(dp - t["dpose"])).sum() + (np.abs(B["b_lm"]) * np.abs(dl - t["dlm"])).sum()) / t["chi_new"]
        print("%s v%d gather=%d %s delta %.6g (|h_gn| %.6g |h_sd| %.6g): plain increment %.2e chi2 %.2e | dogleg increment %.2e chi_old %.2e chi_new %.2e delta_final %.2e (%.6g) | rho %+.4f margin %.2e accepted %d kind %s%s%s"
              % (name, variant, gather, dr.KINDS[kind], delta, gn, sd, y_inc, y_chi, e_inc, e_old, e_new, e_del, info["delta_final"], t["rho"], t["margin"], done,
                 kinds(info["step_kind"]), "" if decided else " (verdict / delta update not compared: near a tie)",
                 " | chi_new bound %.2e + first-order term %.2e" % (tol_chi, first_order) if first_order else ""))
        assert info["step_kind"].tolist() == [kind] and info["delta"][0] == delta and info["delta_initial"] == delta
        assert e_inc <= tol_inc and e_old <= 1e-9
        assert info["trials"] == 1 and info["rejected"] == 1 - done and info["terminated"] == 1 - done
        assert (info["n_gn"], info["n_sd"], info["n_dl"]) == tuple(done * int(kind == k) for k in (dr.GN, dr.SD, dr.DL))
        if decided:
            assert done == int(t["accepted"]) and e_del <= tol_del
        if done == 1:
            assert e_new <= tol_chi + first_order
            assert rel(G.poses(), t["P"]) <= max(4 * y_inc, 1e-9) and rel(G.landmarks(), t["L"]) <= max(4 * y_inc, 1e-9)
        else:
            assert np.array_equal(G.poses(), g["pose_est"]) and np.array_equal(G.landmarks(), g["lm_est"])
        G.close()


# ---------------------------------------------------------------- 2. trajectories
def plain_yardstick(pkg, po, gs, iterations):
    """plain gs_optimize(iterations) from the start gs against the oracle: (estimates, chi2_final) relative errors"""
    A = fresh(pkg, gs); done, st = A.optimize(iterations); assert done == iterations
    og = make_oracle_graph(po, gs); og.optimize(iterations, ordering=1)
    y_est = max(rel(A.poses(), og.poses()), rel(A.landmarks(), og.landmarks())); y_chi = abs(st.chi2_final - og.chi2()) / og.chi2()
    A.close()
    return y_est, y_chi


@pytest.mark.parametrize("which", ["default", "small"])
def test_trajectory_matches_the_checker(pkg, po, bench_graphs, which):
    """The CPU-established cases (test_dogleg_cpu.py) from x1, 6 iterations: default parameters (trials [4, 1, 1, 1, 1, 1], three
    rejected GN trials, then DL DL GN DL GN GN) and initial_delta = 1 (SD SD SD DL DL DL).  Trial counts, kinds, chi2[] and delta[] per
    iteration, delta_final and the final estimates against the checker; yardstick plain gs_optimize(6) from the same start."""
    g, _, _, P1, L1, _, _ = starts(po, bench_graphs, 1)
    r = x1_run(po, bench_graphs, which); dr.conditions(r)
    gs = dict(g, pose_est=P1, lm_est=L1)
    y_est, y_chi = plain_yardstick(pkg, po, gs, 6)
    tol_est, tol_chi = max(4 * y_est, 1e-9), max(4 * y_chi, 4 * y_est, 1e-9)
    G = fresh(pkg, gs)
    done, st, info = G.optimize_dogleg(6, **({} if which == "default" else {"initial_delta": 1.0}))
    e_chi = float(np.abs(info["chi2"] / r["chi2"] - 1).max()); e_del = float(np.abs(info["delta"] / r["delta"] - 1).max())
    e_est = max(rel(G.poses(), r["P"]), rel(G.landmarks(), r["L"])); e_fin = abs(st.chi2_final - r["chi2_final"]) / r["chi2_final"]
    print("%s: trials GPU %s checker %s, kinds GPU %s checker %s, rejected %d / %d\n  plain(6) estimates %.2e chi2 %.2e | dogleg chi2[] %.2e delta[] %.2e estimates %.2e chi2_final %.2e delta_final %.6g / %.6g"
          % (which, info["n_trials"].tolist(), r["n_trials"].tolist(), kinds(info["step_kind"]), kinds(r["kind"]), info["rejected"], r["rejected"],
             y_est, y_chi, e_chi, e_del, e_est, e_fin, info["delta_final"], r["delta_final"]))
    print("  chi2[] " + " ".join("%.8g" % v for v in info["chi2"]) + " -> %.8g" % st.chi2_final)
    print("  delta[] " + " ".join("%.6g" % v for v in info["delta"]))
    assert done == 6 and info["iterations"] == 6 and info["terminated"] == 0 and st.iterations == 6
    assert info["n_trials"].tolist() == r["n_trials"].tolist() and info["step_kind"].tolist() == r["kind"].tolist()
    assert info["rejected"] == r["rejected"] and info["trials"] == len(r["trials"])
    acc = [t["kind"] for t in r["trials"] if t["accepted"]]
    assert (info["n_gn"], info["n_sd"], info["n_dl"]) == tuple(acc.count(k) for k in (dr.GN, dr.SD, dr.DL))
    assert e_chi <= tol_chi and e_del <= tol_chi and e_fin <= tol_chi and e_est <= tol_est
    assert abs(st.chi2_initial - r["chi2"][0]) <= 1e-9 * r["chi2"][0] and abs(info["delta_final"] / r["delta_final"] - 1) <= tol_chi
    assert np.all(np.diff(np.r_[info["chi2"], st.chi2_final]) < 0)
    if which == "default":
        assert info["n_trials"].tolist() == DEFAULT_TRIALS
    G.close()


def test_terminate_leaves_the_estimates_bit_identical(pkg, po, bench_graphs):
    """max_trials = 3 from x1 with the default initial_delta: the checker rejects all three Gauss-Newton trials (rho -0.2318 each).  The
    call returns 0 with terminated = 1, rejected = 3, delta_final = 1e4 / 8, and every vertex bit-identical to the start."""
    g, _, _, P1, L1, _, _ = starts(po, bench_graphs, 1)
    r = x1_run(po, bench_graphs, "terminate"); dr.conditions(r)
    assert r["terminated"] and r["rejected"] == 3
    G = fresh(pkg, dict(g, pose_est=P1, lm_est=L1))
    done, st, info = G.optimize_dogleg(6, max_trials=3)
    print("terminate: returned %d, terminated %d, rejected %d, trials %d, n_trials %s, kinds %s, delta[] %s, delta_final %.6g, chi2 %.10g (checker %.10g)"
          % (done, info["terminated"], info["rejected"], info["trials"], info["n_trials"].tolist(), kinds(info["step_kind"]), info["delta"].tolist(),
             info["delta_final"], st.chi2_final, r["chi2_final"]))
    assert done == 0 and info["terminated"] == 1 and info["rejected"] == 3 and info["trials"] == 3 and info["iterations"] == 0
    assert info["n_trials"].tolist() == [3] and info["step_kind"].tolist() == [dr.GN] and info["delta"][0] == 2500.0 and info["delta_final"] == 1250.0
    assert np.array_equal(G.poses(), P1) and np.array_equal(G.landmarks(), L1)
    assert st.chi2_initial == st.chi2_final and abs(st.chi2_final - r["chi2_final"]) <= 1e-9 * r["chi2_final"]
    assert abs(G.chi2() - st.chi2_final) <= 1e-12 * st.chi2_final
    G.close()


@pytest.mark.parametrize("total", sorted(BOUNDARY))
def test_terminate_at_the_workgroup_boundary_leaves_the_estimates_bit_identical(pkg, po, bench_graphs, total):
    """The test above at N + M = 255, 256, 257 from test_lm_cpu.boundary_start: one workgroup of the vertex-parallel kernels with an
    idle last thread, exactly one, and a second one whose only thread is a landmark (every total then has two partials, the second from
    a single thread).  The checker rejects all three Gauss-Newton trials (rho -0.148 / -0.688 / -0.239; dogleg_ref.conditions asserted
    here again, test_dogleg_cpu.py asserts them without a GPU); the call returns 0 with terminated = 1, rejected = 3,
    delta_final = 1e4 / 8, and every vertex bit-identical to the start.
    Measured on an MI355X (profiles/trial_scaffold_gpu_suite.txt): so at all three sizes, chi2 equal to the checker's to the 10 digits printed."""
    g, P1, L1 = boundary_start(po, bench_graphs, total)
    r = boundary_terminate(po, g, P1, L1)
    G = fresh(pkg, dict(g, pose_est=P1, lm_est=L1))
    done, st, info = G.optimize_dogleg(6, max_trials=3)
    print("N + M = %d terminate: returned %d, terminated %d, rejected %d, trials %d, n_trials %s, kinds %s, delta[] %s, delta_final %.6g, chi2 %.10g (checker %.10g, rho %.4f)"
          % (total, done, info["terminated"], info["rejected"], info["trials"], info["n_trials"].tolist(), kinds(info["step_kind"]), info["delta"].tolist(),
             info["delta_final"], st.chi2_final, r["chi2_final"], r["trials"][0]["rho"]))
    assert done == 0 and info["terminated"] == 1 and info["rejected"] == 3 and info["trials"] == 3 and info["iterations"] == 0
    assert info["n_trials"].tolist() == [3] and info["step_kind"].tolist() == [dr.GN] and info["delta"][0] == 2500.0 and info["delta_final"] == 1250.0
    assert np.array_equal(G.poses(), P1) and np.array_equal(G.landmarks(), L1)
    assert st.chi2_initial == st.chi2_final and abs(st.chi2_final - r["chi2_final"]) <= 1e-9 * r["chi2_final"]
    G.close()


# ---------------------------------------------------------------- 3. robust kernel and the side passes
def side_handle(pkg, g, P1, L1, kernels, polar, pri, off):
    G = pkg.Graph(device=0)
    plr.load(G, dict(g, pose_est=P1, lm_est=L1), polar)
    for kind, k in kernels.items():
        G.set_robust_kernel(kind, *k)
    pr.add_to(G, pri)
    for k in off:
        G.set_edge_active("observation", int(k), False)
    return G


def test_robust_kernel_prior_polar_and_inactive_edges(pkg, po, bench_graphs):
    """Huber on the observation kind, one pose prior, polar_ref.polar_set and two inactive edges on bench 1000 / 200 from x1, 4
    iterations: the accepted count, the trial counts, the kinds and the chi2 sequence against the checker (margins: test_dogleg_cpu.py).
    Yardstick: four plain Gauss-Newton iterations of the same graph, GPU against the checker's model."""
    m, g, P1, L1, kernels, polar, pri, off = side_case(po, bench_graphs)
    r = side_run(po, bench_graphs); dr.conditions(r)
    A = side_handle(pkg, g, P1, L1, kernels, polar, pri, off); done, st = A.optimize(SIDE_ITERATIONS); assert done == SIDE_ITERATIONS
    P, L = P1, L1
    for _ in range(SIDE_ITERATIONS):
        og, n, colptr, rowind, values, b = m.system(P, L)
        P, L, _, _ = m.step(og, lm_ref._solve(po, n, colptr, rowind, values, b))
    chi_gn = m.chi2(P, L)
    y_est = max(rel(A.poses(), P), rel(A.landmarks(), L)); y_chi = abs(st.chi2_final - chi_gn) / chi_gn
    A.close()
    tol_est, tol_chi = max(4 * y_est, 1e-9), max(4 * y_chi, 4 * y_est, 1e-9)
    G = side_handle(pkg, g, P1, L1, kernels, polar, pri, off)
    done, st, info = G.optimize_dogleg(SIDE_ITERATIONS)
    seq = np.r_[info["chi2"], st.chi2_final]; want = np.r_[r["chi2"], r["chi2_final"]]
    e_chi = float(np.abs(seq / want - 1).max()); e_est = max(rel(G.poses(), r["P"]), rel(G.landmarks(), r["L"]))
    print("huber + prior + polar + inactive: accepted %d / %d trials GPU %s checker %s kinds %s / %s\n  plain(4) estimates %.2e chi2 %.2e | dogleg chi2 sequence %.2e estimates %.2e\n  chi2 %s"
          % (done, r["accepted"], info["n_trials"].tolist(), r["n_trials"].tolist(), kinds(info["step_kind"]), kinds(r["kind"]), y_est, y_chi, e_chi, e_est,
             " ".join("%.8g" % v for v in seq)))
    assert done == r["accepted"] == SIDE_ITERATIONS and info["n_trials"].tolist() == r["n_trials"].tolist() and info["step_kind"].tolist() == r["kind"].tolist()
    assert e_chi <= tol_chi and e_est <= tol_est
    G.close()


# ---------------------------------------------------------------- 4. against Gauss-Newton
def test_decreasing_where_gauss_newton_rises(pkg, po, bench_graphs):
    """From x1 a plain Gauss-Newton step RAISES chi2 (63 935 -> 77 924, the oracle's figure); the dogleg's chi2 is strictly decreasing
    over its accepted points."""
    g, _, _, P1, L1, _, _ = starts(po, bench_graphs, 1)
    gs = dict(g, pose_est=P1, lm_est=L1)
    A = fresh(pkg, gs); done, sa = A.optimize(1); A.close()
    G = fresh(pkg, gs); done, st, info = G.optimize_dogleg(6)
    seq = np.r_[info["chi2"], st.chi2_final]
    print("Gauss-Newton %.8g -> %.8g | dogleg %s (rejected %d)" % (sa.chi2_initial, sa.chi2_final, " ".join("%.8g" % v for v in seq), info["rejected"]))
    assert sa.chi2_final > sa.chi2_initial
    assert done == 6 and np.all(np.diff(seq) < 0) and seq[0] == sa.chi2_initial
    G.close()


# ---------------------------------------------------------------- 5. a zero pivot ends the call
def test_zero_pivot_ends_the_call_with_a_numeric_error(pkg, po, bench_graphs):
    """gs_debug_fail_at_iteration arms code 1 on the first solve of the call (the status-code hook test_gpu_lm.py uses; no singular H is
    built): g2o's "Fail".  The call returns GS_ERR_NUMERIC, the estimates are bit-identical to the start, and a following optimize(2)
    equals a fresh handle's."""
    g, _, _, P1, L1, _, _ = starts(po, bench_graphs, 1)
    gs = dict(g, pose_est=P1, lm_est=L1)
    G = fresh(pkg, gs); G.initialize_optimization()
    G.debug_fail_at_iteration(1, 1)
    with pytest.raises(pkg.binding.GsError) as e:
        G.optimize_dogleg(4)
    print("zero pivot: code %d (%s)" % (e.value.code, e.value))
    assert e.value.code == NUMERIC
    assert np.array_equal(G.poses(), P1) and np.array_equal(G.landmarks(), L1)
    F = fresh(pkg, gs)
    d1, s1 = G.optimize(2); d2, s2 = F.optimize(2)
    assert d1 == d2 == 2 and s1.numeric_failure == 0 and s1.first_failure == 0
    assert np.array_equal(G.poses(), F.poses()) and np.array_equal(G.landmarks(), F.landmarks()) and s1.chi2_final == s2.chi2_final
    G.close(); F.close()


def test_zero_pivot_with_a_second_workgroup_of_one_landmark_ends_the_call(pkg, po, bench_graphs):
    """The test above at N + M = 257 (test_lm_cpu.boundary_start: the second workgroup of the vertex-parallel kernels is one landmark):
    GS_ERR_NUMERIC, the start's bits in every vertex, and a following optimize(2) runs clean."""
    g, P1, L1 = boundary_start(po, bench_graphs, 257)
    G = fresh(pkg, dict(g, pose_est=P1, lm_est=L1)); G.initialize_optimization()
    G.debug_fail_at_iteration(1, 1)
    with pytest.raises(pkg.binding.GsError) as e:
        G.optimize_dogleg(4)
    print("N + M = 257 zero pivot: code %d (%s)" % (e.value.code, e.value))
    assert e.value.code == NUMERIC
    assert np.array_equal(G.poses(), P1) and np.array_equal(G.landmarks(), L1)
    done, st = G.optimize(2); assert done == 2 and st.numeric_failure == 0 and st.first_failure == 0
    G.close()


def test_flag_timeout_falls_back_to_level_launches_and_finishes(pkg, bench_graphs):
    """the branch shared with gs_optimize and gs_optimize_lm: code 2 (a whole-tree launch gave up on a front's flag; the hook sets the
    status word, nothing stalls) on the first trial.  The call falls back to one launch per level, runs the trial again and finishes with
    the estimates of an uninjected handle."""
    _, g = bench_graphs(1000, 200)
    A = fresh(pkg, g); da, sa, ia = A.optimize_dogleg(3)
    G = fresh(pkg, g); G.initialize_optimization()
    G.debug_fail_at_iteration(1, 2)
    done, st, info = G.optimize_dogleg(3)
    print("dogleg through a flag timeout: accepted %d (uninjected %d) first_failure %d fell_back %d numeric_failure %d n_trials %s"
          % (done, da, st.first_failure, st.fell_back, st.numeric_failure, info["n_trials"].tolist()))
    assert st.first_failure == 2 and st.fell_back == 1 and st.numeric_failure == 0
    assert done == 3 and da == 3 and sa.fell_back == 0 and info["n_trials"].tolist() == ia["n_trials"].tolist()
    assert np.array_equal(G.poses(), A.poses()) and np.array_equal(G.landmarks(), A.landmarks())
    A.close(); G.close()


# ---------------------------------------------------------------- 6. no leftover state
def test_no_leftover_state_on_the_handle(pkg, po, bench_graphs):
    """After optimize_dogleg: gs_iterate, then gs_optimize_lm, then compute_marginals on the same handle give, bit for bit, what a handle
    gives that was loaded at the same estimates and ran plain optimize(0); the marginal getters are stale until recomputed; gs_chi2
    equals the call's final chi2.  Launch modes: tree = 0 and a second call from the same start give the first call's bits.
    (That a handle which never calls the new entry points allocates nothing for them is not tested here: gs_stats.device_bytes counts
    the plan's pool only, and the dogleg buffers are an allocation of the handle's own that only dl_reserve makes.)"""
    g, _, _, P1, L1, _, _ = starts(po, bench_graphs, 1)
    gs = dict(g, pose_est=P1, lm_est=L1)
    G = fresh(pkg, gs)
    G.compute_marginals(); G.pose_covariances()
    done, st, info = G.optimize_dogleg(3)
    assert done == 3 and info["rejected"] == 3
    with pytest.raises(pkg.binding.GsError) as e:
        G.pose_covariances()
    assert e.value.code == -6
    chi = G.chi2()
    print("chi2 after the call %.17g, info %.17g, rel %.2e" % (chi, st.chi2_final, abs(chi - st.chi2_final) / chi))
    assert abs(chi - st.chi2_final) <= 1e-9 * chi
    P, L = G.poses(), G.landmarks()
    F = fresh(pkg, dict(g, pose_est=P, lm_est=L)); F.optimize(0)
    assert G.iterate() == 1 and F.iterate() == 1
    G.synchronize(); F.synchronize()                                 # (raises if a failure, stop or dogleg flag were left behind)
    G.sync_estimates(); F.sync_estimates()
    assert np.array_equal(G.poses(), F.poses()) and np.array_equal(G.landmarks(), F.landmarks())
    (d1, s1, i1), (d2, s2, i2) = G.optimize_lm(2), F.optimize_lm(2)
    assert d1 == d2 and s1.chi2_final == s2.chi2_final and all(np.array_equal(i1[k], i2[k]) for k in i1)
    assert np.array_equal(G.poses(), F.poses()) and np.array_equal(G.landmarks(), F.landmarks())
    G.compute_marginals(); F.compute_marginals()
    assert np.array_equal(G.pose_covariances(), F.pose_covariances()) and np.array_equal(G.landmark_covariances(), F.landmark_covariances())
    G.close(); F.close()
    def run(H):
        done, st, info = H.optimize_dogleg(6)
        return done, st.chi2_final, info, H.poses(), H.landmarks()
    A = fresh(pkg, gs); a = run(A)
    B = fresh(pkg, gs, debug=dict(tree=0)); b = run(B); B.close()
    for i, e in enumerate(P1):
        A.set_pose_estimate(i, e)
    for i, e in enumerate(L1):
        A.set_landmark_estimate(i, e)
    c = run(A); A.close()
    for label, o in (("tree=0", b), ("second call", c)):
        same = (o[0] == a[0] and o[1] == a[1] and np.array_equal(o[3], a[3]) and np.array_equal(o[4], a[4]) and
                all(np.array_equal(o[2][k], a[2][k]) for k in a[2]))
        print("%s: accepted %d n_trials %s chi2_final %.17g bit-identical %s" % (label, o[0], o[2]["n_trials"].tolist(), o[1], same))
        assert same
