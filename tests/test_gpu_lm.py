"""gs_optimize_lm (Levenberg-Marquardt with device-side step control) on the GPU against the checker tests/lm_ref.py: g2o's
OptimizationAlgorithmLevenberg rule (restated from its published text, not pinned against a g2o build) on the CPU oracle.
test_lm_cpu.py establishes, without a GPU, that every trial of the compared trajectories has a margin
|chi_old - chi_new| / chi_old >= 1e-3, so that an accept / reject decision is not rounding noise; the tests below assert that margin
again on every trial whose decision they compare and skip none.

Tolerances: the yardstick of a comparison is the SAME comparison for plain gs_optimize on the same graph and estimates (GPU against
oracle), measured inside the test; LM may be 4x that (rho and lambda inherit the relative error of two chi2 values and one more
reduction), with the bound of the corresponding test_gpu_parity.py test as the floor (H blocks 1e-11 of the array's largest entry,
increments 1e-8 of the largest increment — 1e-9 on the random graph —, estimates and chi2 1e-9).  Every test prints its figures
before it asserts (-s); the printed run is profiles/lm_gpu_suite.txt.

The damping-as-factorised test has its GROWN case in test_damping_as_factorised_on_a_grown_plan (gs_export_system reads the tail
arenas, and a trial's chi2 pass on a grown plan writes nothing of H: k_chi2_tail).  The tail arenas are also pinned through what they
decide, on a plan grown by 6 poses AND 2 cones (grown(): an open stretch of the lap):
a six-iteration trajectory with seven rejections against the checker, a terminated call compared bit for bit on every vertex, one
trial at four lambda, and lambda_0 with the largest diagonal entry on a tail pose."""
import numpy as np
import pytest

import lm_ref
import robust_ref as rr
from conftest import append_tail, make_oracle_graph, random_graph, split_for_growth
from test_lm_cpu import BOUNDARY, REJECTION_LAMBDA0, REJECTION_TRIALS, ROBUST_TRIALS, boundary_start, boundary_terminate, robust_case, starts

pytestmark = pytest.mark.gpu
DIAG3 = (0, 4, 8); DIAG2 = (0, 3)


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300))


def fresh(pkg, g, debug=None, **kw):
    G = pkg.Graph(device=0, debug=debug, **kw)
    G.load_bench_graph(g)
    return G


GROWN_H, GROWN_KEEP = 6, 600      # an open stretch of the lap: its last 6 poses discover 2 cones (a closed lap's last poses only re-observe)


def grown(pkg, g, h=GROWN_H, keep=GROWN_KEEP, **kw):
    """a handle whose plan has absorbed the last h poses of the graph's first `keep` poses by growth — tail poses AND tail cones, both
    asserted, so the tail arenas of poses and landmarks are in use — and the full graph it then holds"""
    base, tail, full = split_for_growth(g, h, keep)
    G = fresh(pkg, base, **kw); G.initialize_optimization()
    new_lms = append_tail(G, tail); G.initialize_optimization()
    assert G.plan_growths() > 0, G.growth_refusal()
    assert new_lms > 0 and len(full["lm_est"]) == len(base["lm_est"]) + new_lms
    return G, full


def graph_of(pkg, bench_graphs, frontend, name):
    if name == "random":
        return random_graph(7)
    if name == "track400_K16":
        return pkg.track.bench_graph(pkg.track.generate(400, 150, 16), frontend)
    sizes = {"bench50": (50, 30), "bench1000": (1000, 200), "bench10k": (10000, 2000), "grown": (1000, 200)}
    sizes.update({"n%d" % total: nm[:2] for total, nm in BOUNDARY.items()})      # N + M = 255, 256, 257 (test_lm_cpu.boundary_start)
    return bench_graphs(*sizes[name])[1]


def handle_of(pkg, g, name, **kw):
    """(handle, the graph the handle holds)"""
    if name == "grown":
        return grown(pkg, g, **kw)
    return fresh(pkg, g, **kw), g


def set_start(G, P, L):
    for i, e in enumerate(P):
        G.set_pose_estimate(i, e)
    for i, e in enumerate(L):
        G.set_landmark_estimate(i, e)


def free_masks(g):
    fp = np.ones(len(g["pose_est"]), dtype=bool); fp[np.asarray(g["fixed_poses"], dtype=np.int64)] = False
    fl = np.ones(len(g["lm_est"]), dtype=bool); fl[np.asarray(g["fixed_landmarks"], dtype=np.int64)] = False
    return fp, fl


# ---------------------------------------------------------------- 1. the damping as the factorisation saw it
@pytest.mark.parametrize("gather", [0, 1])
@pytest.mark.parametrize("name", ["bench50", "bench1000", "bench10k", "random", "bench1000-huber"])
def test_damping_as_factorised(pkg, po, bench_graphs, frontend, name, gather):
    """optimize_lm(1, initial_lambda, max_trials = 1), then export_system(): the diagonal blocks minus the oracle's at the same
    estimates are lambda on the free diagonal scalars and 0 elsewhere; off-diagonal blocks and b are the oracle's.  lambda = 0.01 max
    diag(H).  Bound 1e-11 of each array's largest entry (the addition of lambda is one rounding).
    Measured on an MI355X (profiles/lm_gpu_suite.txt), fused and gather alike: H blocks at most 2.4e-14 (10k / 2k, H_pl) and 7.1e-14 with
    Huber; b at most 4.5e-12 (10k / 2k b_pose: the undamped linearisation's own figure, test_gpu_robust.py); the lambda differences
    themselves exact to the bound's 1e-11."""
    huber = name.endswith("-huber")
    g = graph_of(pkg, bench_graphs, frontend, name.split("-")[0])
    kernels = {"observation": ("huber", rr.median_deltas(g, g["pose_est"], g["lm_est"])[1])} if huber else {}
    lam = 0.01 * lm_ref.max_diag(po, g, g["pose_est"], g["lm_est"], kernels)
    ref = make_oracle_graph(po, rr.reweighted(g, g["pose_est"], g["lm_est"], kernels) if huber else g).linearize_blocks()
    G = fresh(pkg, g, linearize_gather=gather)
    if huber:
        G.set_robust_kernel("observation", *kernels["observation"])
    done, st, info = G.optimize_lm(1, initial_lambda=lam, max_trials=1)
    assert info["trials"] == 1 and info["lambda_initial"] == lam
    S = G.export_system()
    fp, fl = free_masks(g)
    want = {k: v.copy() for k, v in ref.items()}
    for c in DIAG3:
        want["Hpp_diag"][fp, c] += lam
    for c in DIAG2:
        want["Hll_diag"][fl, c] += lam
    dpp = (S["Hpp_diag"] - ref["Hpp_diag"]); dll = (S["Hll_diag"] - ref["Hll_diag"])
    figs = {k: rel(S[k], want[k]) for k in want}
    print("%s gather=%d lambda %.6g accepted %d: " % (name, gather, lam, done) + " ".join("%s %.2e" % kv for kv in figs.items()))
    for k, v in figs.items():
        assert v < 1e-11, k
    tol = 1e-11 * np.abs(want["Hpp_diag"]).max()
    assert np.abs(dpp[fp][:, DIAG3] - lam).max() <= tol and np.abs(dpp[~fp]).max(initial=0.0) == 0.0
    assert np.abs(np.delete(dpp, DIAG3, axis=1)).max() <= tol
    tol = 1e-11 * np.abs(want["Hll_diag"]).max()
    assert np.abs(dll[fl][:, DIAG2] - lam).max() <= tol and np.abs(dll[~fl]).max(initial=0.0) == 0.0
    G.close()


def test_damping_as_factorised_on_a_grown_plan(pkg, po, bench_graphs):
    """test_damping_as_factorised on a GROWN handle (gs_export_system used to refuse one): after optimize_lm(1, initial_lambda,
    max_trials = 1) the exported diagonal blocks minus the oracle's at the trial's starting estimates are lambda on every free diagonal
    scalar — on the 6 tail poses and the 2 tail cones too, where the header promises "as it was factorised" — and 0 elsewhere; the
    off-diagonal blocks and b are the oracle's.  lambda = 0.01 max diag(H); bound 1e-11 of each array's largest entry, as there.  (The chi2
    at the trial point used to be a whole linearisation on a grown plan and left the undamped system at x_try: k_chi2_tail.)"""
    G, full = grown(pkg, bench_graphs(1000, 200)[1])
    lam = 0.01 * lm_ref.max_diag(po, full, full["pose_est"], full["lm_est"], {})
    ref = make_oracle_graph(po, full).linearize_blocks()
    done, st, info = G.optimize_lm(1, initial_lambda=lam, max_trials=1)
    assert info["trials"] == 1 and info["lambda_initial"] == lam and G.plan_growths() > 0
    S = G.export_system()
    N, M = len(full["pose_est"]), len(full["lm_est"]); Nb, Mb = N - GROWN_H, M - 2
    assert S["Hpp_diag"].shape == (N, 9) and S["Hll_diag"].shape == (M, 4) and S["Hpl"].shape == (len(full["pl_p"]), 6)
    fp, fl = free_masks(full)
    assert fp[Nb:].all() and fl[Mb:].all()
    want = {k: v.copy() for k, v in ref.items()}
    for c in DIAG3:
        want["Hpp_diag"][fp, c] += lam
    for c in DIAG2:
        want["Hll_diag"][fl, c] += lam
    dpp = (S["Hpp_diag"] - ref["Hpp_diag"]); dll = (S["Hll_diag"] - ref["Hll_diag"])
    figs = {k: rel(S[k], want[k]) for k in want}
    print("grown lambda %.6g accepted %d: " % (lam, done) + " ".join("%s %.2e" % kv for kv in figs.items()) +
          " | lambda on the tail: poses %.3e cones %.3e off" % (np.abs(dpp[Nb:][:, DIAG3] - lam).max(), np.abs(dll[Mb:][:, DIAG2] - lam).max()))
    for k, v in figs.items():
        assert v < 1e-11, k
    tol = 1e-11 * np.abs(want["Hpp_diag"]).max()
    assert np.abs(dpp[fp][:, DIAG3] - lam).max() <= tol and np.abs(dpp[~fp]).max(initial=0.0) == 0.0
    assert np.abs(dpp[Nb:][:, DIAG3] - lam).max() <= tol and np.abs(np.delete(dpp, DIAG3, axis=1)).max() <= tol
    tol = 1e-11 * np.abs(want["Hll_diag"]).max()
    assert np.abs(dll[fl][:, DIAG2] - lam).max() <= tol and np.abs(dll[~fl]).max(initial=0.0) == 0.0
    assert np.abs(dll[Mb:][:, DIAG2] - lam).max() <= tol
    G.close()


# ---------------------------------------------------------------- 2. one trial
@pytest.mark.parametrize("name,variant", [(n, v) for n in ("bench50", "bench1000", "bench10k", "random", "grown", "track400_K16") for v in (3, 4)
                                          if not (n == "grown" and v == 4)] +     # (append-only growth exists for factor_variant 3 only)
                                         [(n + path, 3) for n in ("n255", "n256", "n257") for path in ("", "-gather")])
def test_one_trial_increment_and_chi2_match_the_checker(pkg, po, bench_graphs, frontend, name, variant):
    """The increment (export_delta) and chi_new of ONE trial against the checker's, lambda in {1e-12 max diag, the default 1e-5 max
    diag, 1e3 max diag} and — added, so that a large lambda is fully asserted too — 1e1 max diag (margins 4.7e-3 .. 2.0e-2).  The grown
    handle has tail poses and tail cones (grown()).  Yardstick: the plain gs_optimize(1) increment and the chi2 behind it, GPU against oracle, same graph and
    estimates; LM may be 4x that; floor 1e-8 of the largest increment (1e-9 random graph), 1e-9 for chi2.  Damping improves cond(H):
    LM is expected at or under the plain figure.  A growth needs variant 3: the grown case runs there only.
    The accept / reject decision is compared where the checker's margin is >= 1e-3: lambda = 1e-12 and 1e-5 max diag (asserted, margins
    0.6 - 0.94).  At 1e3 max diag the step is tiny by construction (margins 5e-5 .. 2e-4 on these graphs, measured with the checker): there
    the increment is compared, and chi_new / the estimates when the trial was accepted; the decision is not.
    Measured on an MI355X (profiles/lm_gpu_suite.txt), increment error plain / LM at lambda = 1e-12, 1e-5, 1e3 max diag:
      50/30 v3 8.0e-14 / 3.1e-14 4.1e-14 1.4e-13      1000/200 v3 8.3e-11 / 1.1e-10 8.3e-14 5.6e-13     10k/2k v3 9.1e-7 / 6.4e-7 9.8e-13 4.5e-12
      random v3 1.8e-14 / 7.3e-15 8.2e-15 3.7e-16     grown v3 1.1e-10 / 1.2e-10 7.8e-14 5.6e-13        track400 K16 v3 1.4e-11 / 1.3e-11 2.4e-14 8.6e-14
    (variant 4 alike: 10k/2k 1.5e-6 / 4.8e-8 1.0e-12 4.5e-12; the grown row: a closed-lap tail without cones, before grown() took an
    open stretch — the figures of the stretch with tail cones, and of 1e1 max diag on every graph — at most 4.6e-12, all accepted —,
    are in profiles/lm_gpu_suite.txt; on that stretch the 1e-12 case is 2.0e-10 against a plain 4.2e-11, 4.8x: two solves of an undamped,
    ill-conditioned system, both far under the 1e-8 floor that decides there).  With a lambda that matters LM is 2 - 6 orders under the plain figure;
    at 1e-12 max diag the system is the undamped one to rounding and the two figures are the same size (1.35x at most, 1000/200 v3),
    far inside 4x.  chi_old at most 1.4e-15, chi_new at most 1.5e-11 (10k/2k, lambda 1e-12: behind the 6.4e-7 increment), lambda_0 exact
    or 1 ulp.  All 33 trials were accepted on GPU and checker alike.
    n255 / n256 / n257 (and -gather: linearize_gather = 1): bench graphs with N + M = 255, 256, 257 vertices from their own start, the
    sizes at which the vertex-parallel kernels go from one workgroup with an idle thread to exactly one to a second one whose only
    thread is a landmark (test_lm_cpu.boundary_start).  Checker margins there: 0.69 .. 0.75 at 1e-12 and 1e-5 max diag, 1.2e-2 ..
    1.7e-2 at 1e1, 1.4e-4 .. 1.8e-4 at 1e3.  Measured on an MI355X (profiles/trial_scaffold_gpu_suite.txt): plain increment 1.3e-13 ..
    1.9e-13 fused, 2.2e-12 .. 3.4e-12 gather; LM increment at most 1.7e-13 fused and 3.4e-12 gather (1e-12 max diag, the undamped system
    to rounding), chi_new at most 4.1e-15, lambda_0 exact; all 24 trials accepted on both sides."""
    name, _, path = name.partition("-")
    kw = dict(factor_variant=variant, **({"linearize_gather": 1} if path == "gather" else {}))
    g0 = graph_of(pkg, bench_graphs, frontend, name)
    A, g = handle_of(pkg, g0, name, **kw)
    og = make_oracle_graph(po, g); og.build_system(); og.apply_update(og.solve_ldlt(1)); dp_o, dl_o = og.delta()
    done, st = A.optimize(1); assert done == 1
    dp, dl = A.export_delta(); sc = max(np.abs(dp_o).max(), np.abs(dl_o).max())
    y_inc = max(np.abs(dp - dp_o).max(), np.abs(dl - dl_o).max()) / sc
    y_chi = abs(A.chi2() - og.chi2()) / og.chi2()
    A.close()
    floor = 1e-9 if name == "random" else 1e-8
    tol_inc, tol_chi = max(4 * y_inc, floor), max(4 * y_chi, 1e-9)
    md = lm_ref.max_diag(po, g, g["pose_est"], g["lm_est"])
    if name == "track400_K16":
        assert st.n_big_fronts > 0 and st.max_front > 63
    for f in (1e-12, None, 1e1, 1e3):
        lam = 1e-5 * md if f is None else f * md
        t = lm_ref.trial(po, g, g["pose_est"], g["lm_est"], lam)
        margin = abs(t["chi_old"] - t["chi_new"]) / t["chi_old"]
        G, _ = handle_of(pkg, g0, name, **kw)
        done, st, info = G.optimize_lm(1, max_trials=1, **({} if f is None else {"initial_lambda": lam}))
        dp, dl = G.export_delta(); sc = max(np.abs(t["dpose"]).max(), np.abs(t["dlm"]).max())
        e_inc = max(np.abs(dp - t["dpose"]).max(), np.abs(dl - t["dlm"]).max()) / sc
        e_lam = abs(info["lambda_initial"] - lam) / lam
        e_old = abs(info["chi2"][0] - t["chi_old"]) / t["chi_old"]
        e_new = abs(st.chi2_final - t["chi_new"]) / t["chi_new"] if done == 1 else float("nan")
        print("%s%s v%d lambda %.3e (%s max diag): plain increment %.2e chi2 %.2e | LM increment %.2e lambda %.2e chi_old %.2e chi_new %.2e | rho %+.4f margin %.2e accepted %d"
              % (name, " " + path if path else "", variant, lam, "1e-5" if f is None else "%g" % f, y_inc, y_chi, e_inc, e_lam, e_old, e_new, t["rho"], margin, done))
        assert e_inc <= tol_inc and e_lam <= 1e-11 and e_old <= 1e-9
        assert info["trials"] == 1 and info["rejected"] == 1 - done and info["terminated"] == 1 - done
        if f != 1e3:
            assert margin >= lm_ref.MIN_MARGIN and done == (1 if t["rho"] > 0 else 0)
        if done == 1:
            assert e_new <= tol_chi
            assert rel(G.poses(), t["P"]) <= max(4 * y_inc, 1e-9) and rel(G.landmarks(), t["L"]) <= max(4 * y_inc, 1e-9)
        else:
            assert np.array_equal(G.poses(), g["pose_est"]) and np.array_equal(G.landmarks(), g["lm_est"])
        G.close()


# ---------------------------------------------------------------- 3. the default lambda_0
@pytest.mark.parametrize("how", ["fused", "gather", "grown", "grown-max-on-a-tail-pose"])
def test_default_initial_lambda_is_tau_times_the_largest_diagonal_entry(pkg, po, bench_graphs, how):
    """lambda_0 = tau * max_j |H_jj| over the free scalars of the oracle's H, relative 1e-11; tau = 1e-5 and 3e-3.  On a grown plan also
    with the information of the observation edges of the last tail pose scaled by 1e4, so that the largest entry is read from the tail
    arena t_Hpp_diag (asserted on the oracle's blocks).  (The same with a tail CONE does not put the maximum there: the theta-theta entry
    of every pose that sees the cone grows by range^2 times as much — checked with the oracle; the tail-cone branch of k_lm_maxdiag is
    run by the grown cases, its value is not what decides them.)
    Measured on an MI355X: equal to the last bit on the fused, gather and grown paths (0.00027634600145705519 at tau = 1e-5) and with the
    maximum on a tail pose (1.1608738689425482)."""
    g0 = bench_graphs(1000, 200)[1]
    if how.startswith("grown-max"):
        base, tail, full = split_for_growth(g0, GROWN_H, GROWN_KEEP)
        g0 = dict(g0, pl_info=np.array(g0["pl_info"], dtype=np.float64, copy=True).reshape(-1, 4), pp_info=np.array(g0["pp_info"], dtype=np.float64, copy=True).reshape(-1, 9))
        g0["pl_info"][g0["pl_p"] == GROWN_KEEP - 1] *= 1e4
    for tau in (1e-5, 3e-3):
        G, g = grown(pkg, g0) if how.startswith("grown") else (fresh(pkg, g0, linearize_gather=int(how == "gather")), g0)
        md = lm_ref.max_diag(po, g, g["pose_est"], g["lm_est"])
        if how.startswith("grown-max"):
            B = make_oracle_graph(po, g).linearize_blocks()
            assert np.abs(B["Hpp_diag"][-1]).max() == md
        done, st, info = G.optimize_lm(1, tau=tau)
        print("%s tau %g: lambda_0 %.17g, tau max diag %.17g, rel %.2e" % (how, tau, info["lambda_initial"], tau * md, abs(info["lambda_initial"] - tau * md) / (tau * md)))
        assert abs(info["lambda_initial"] - tau * md) <= 1e-11 * tau * md and info["lambda"][0] == info["lambda_initial"]
        G.close()


# ---------------------------------------------------------------- 4. / 7. rejection trajectories
def trajectory(pkg, po, g, P1, L1, kernels, want_trials, label, make=None):
    """make(graph at the start) -> handle; default: a fresh handle on the whole graph"""
    gs = dict(g, pose_est=P1, lm_est=L1)
    mk = (lambda pkg_, g_: make(g_)) if make is not None else fresh
    r = lm_ref.run(po, g, 6, kernels=kernels, initial_lambda=REJECTION_LAMBDA0, poses=P1, lms=L1)
    assert r["n_trials"].tolist() == want_trials and all(t["margin"] >= lm_ref.MIN_MARGIN for t in r["trials"])
    # yardstick: plain gs_optimize(6) (with the same kernels) from the same start against the oracle
    A = mk(pkg, gs)
    for kind, k in kernels.items():
        A.set_robust_kernel(kind, *k)
    done, st = A.optimize(6); assert done == 6
    if kernels:
        Po, Lo, chi_o, _ = rr.irls(po, g, kernels, 6, make_oracle_graph, poses=P1, lms=L1); chi_end = rr.robust_chi2(g, Po, Lo, kernels)
    else:
        og = make_oracle_graph(po, gs); og.optimize(6, ordering=1); Po, Lo, chi_end = og.poses(), og.landmarks(), og.chi2()
    y_est = max(rel(A.poses(), Po), rel(A.landmarks(), Lo)); y_chi = abs(st.chi2_final - chi_end) / chi_end
    A.close()
    tol_est, tol_chi = max(4 * y_est, 1e-9), max(4 * y_chi, 4 * y_est, 1e-9)
    G = mk(pkg, gs)
    for kind, k in kernels.items():
        G.set_robust_kernel(kind, *k)
    done, st, info = G.optimize_lm(6, initial_lambda=REJECTION_LAMBDA0)
    e_chi = float(np.abs(info["chi2"] / r["chi2"] - 1).max()); e_lam = float(np.abs(info["lambda"] / r["lam"] - 1).max())
    e_est = max(rel(G.poses(), r["P"]), rel(G.landmarks(), r["L"])); e_fin = abs(st.chi2_final - r["chi2_final"]) / r["chi2_final"]
    print("%s: trials GPU %s checker %s, rejected %d / %d, min margin %.2e\n  plain(6) estimates %.2e chi2 %.2e | LM chi2[] %.2e lambda[] %.2e estimates %.2e chi2_final %.2e lambda_final %.6e / %.6e"
          % (label, info["n_trials"].tolist(), r["n_trials"].tolist(), info["rejected"], r["rejected"], r["min_margin"], y_est, y_chi, e_chi, e_lam, e_est, e_fin,
             info["lambda_final"], r["lambda_final"]))
    print("  chi2[] " + " ".join("%.8g" % v for v in info["chi2"]) + " -> %.8g" % st.chi2_final)
    print("  lambda[] " + " ".join("%.6e" % v for v in info["lambda"]))
    assert done == 6 and info["iterations"] == 6 and info["terminated"] == 0 and st.iterations == 6
    assert info["n_trials"].tolist() == r["n_trials"].tolist()
    assert info["rejected"] == r["rejected"] and info["trials"] == len(r["trials"])
    assert e_chi <= tol_chi and e_lam <= tol_chi and e_fin <= tol_chi and e_est <= tol_est
    assert abs(st.chi2_initial - r["chi2"][0]) <= 1e-9 * r["chi2"][0] and abs(info["lambda_final"] / r["lambda_final"] - 1) <= tol_chi
    G.close()


@pytest.mark.parametrize("seed", [1, 2])
def test_rejection_trajectory_matches_the_checker(pkg, po, bench_graphs, seed):
    """The CPU-established case (test_lm_cpu.py): from x1 with initial_lambda 1e-12, 6 iterations; n_trials exactly the checker's
    ([8,1,1,1,1,1] / [1,7,1,1,1,1]), rejected / trials agree, lambda[it], chi2[it] and the estimates the checker's.  Yardstick:
    plain gs_optimize(6) from the same start.
    Measured on an MI355X (profiles/lm_gpu_suite.txt), plain estimates / chi2 | LM chi2[] lambda[] estimates chi2_final:
      seed 1: 1.2e-11 / 5.9e-13 | 4.3e-14 0 7.6e-14 4.2e-15; trials [8,1,1,1,1,1], 7 rejected, both sides
      seed 2: 2.1e-11 / 7.2e-13 | 1.4e-11 1.4e-11 2.1e-11 6.4e-13; trials [1,7,1,1,1,1], 6 rejected, both sides"""
    g, _, _, P1, L1, _, _ = starts(po, bench_graphs, seed)
    trajectory(pkg, po, g, P1, L1, {}, REJECTION_TRIALS[seed], "seed %d" % seed)


def test_robust_rejection_trajectory_matches_the_checker(pkg, po, bench_graphs):
    """Huber on the observation edges (delta = median sqrt(s) at x1) + LM on the CPU-established case; yardstick plain gs_optimize
    with the same kernel against robust_ref.irls.
    Measured on an MI355X: plain estimates 1.7e-11, chi2 2.0e-12 | LM chi2[] 6.6e-13, lambda[] 4.3e-13, estimates 9.3e-13, chi2_final
    8.0e-14; trials [8,1,1,1,1,1], 7 rejected, both sides."""
    g, P1, L1, k = robust_case(po, bench_graphs)
    trajectory(pkg, po, g, P1, L1, k, ROBUST_TRIALS, "huber delta %.4f" % k["observation"][1])


def test_rejection_trajectory_on_the_gather_path(pkg, po, bench_graphs):
    """The seed-1 trajectory with linearize_gather = 1: k_lm_scale reads b_lm, k_lm_damp writes Hll_diag; rho, lambda[] and the decisions
    of 13 trials depend on both.
    Measured on an MI355X: trials [8, 1, 1, 1, 1, 1] on both sides; plain estimates 3.4e-10, chi2 6.2e-11 | LM chi2[] 2.0e-12, lambda[]
    0, estimates 3.8e-12, chi2_final 1.5e-14."""
    g, _, _, P1, L1, _, _ = starts(po, bench_graphs, 1)
    trajectory(pkg, po, g, P1, L1, {}, REJECTION_TRIALS[1], "seed 1 gather", make=lambda gs: fresh(pkg, gs, linearize_gather=1))


_grown_start = {}


def grown_start(po, bench_graphs):
    """the open stretch grown() uses (600 poses / 128 cones of bench 1000 / 200) as a graph of its own, and x0 = its oracle optimum
    perturbed(seed 1, 5.0, 10.0).  The checker from x0 with initial_lambda 1e-12: trials [1, 8, 1, 1, 1, 1], smallest margin 0.17."""
    if not _grown_start:
        from test_robust_cpu import perturbed
        _, _, full = split_for_growth(bench_graphs(1000, 200)[1], GROWN_H, GROWN_KEEP)
        og = make_oracle_graph(po, full); og.optimize(10, ordering=1)
        _grown_start["x"] = (full,) + tuple(perturbed(dict(full, pose_est=og.poses(), lm_est=og.landmarks()), 1, 5.0, 10.0))
    return _grown_start["x"]


def grown_at(pkg, gs):
    """a grown handle (tail poses and tail cones) holding graph gs, a 600-pose stretch, at gs's estimates"""
    G, full = grown(pkg, gs, keep=None)
    assert np.array_equal(G.poses(), gs["pose_est"]) and np.array_equal(G.landmarks(), gs["lm_est"])
    return G


def test_rejection_trajectory_on_a_grown_plan(pkg, po, bench_graphs):
    """Six iterations with seven rejected trials on a plan with a tail of 6 poses and 2 cones: the tail arenas are damped (t_Hpp_diag,
    t_Hll_diag), their b enters the scale sum (t_b_pose, t_b_lm), and every rejection restores the tail vertices.  n_trials, lambda[],
    chi2[] and the estimates against the checker; yardstick plain gs_optimize(6) on a grown handle from the same start.
    Measured on an MI355X: trials [1, 8, 1, 1, 1, 1] on both sides, 7 rejected; plain estimates 4.8e-9, chi2 2.1e-8 (an open stretch is
    worse conditioned, and undamped Gauss-Newton from x0 passes through its two rises) | LM chi2[] 4.5e-11, lambda[] 1.7e-11, estimates
    3.5e-11, chi2_final 2.8e-12."""
    full, P0, L0 = grown_start(po, bench_graphs)
    trajectory(pkg, po, full, P0, L0, {}, [1, 8, 1, 1, 1, 1], "grown 600/128", make=lambda gs: grown_at(pkg, gs))


def test_terminate_on_a_grown_plan_keeps_the_tail_vertices_bit_identical(pkg, po, bench_graphs):
    """max_trials = 3 from the same start: the checker accepts iteration 0 and rejects three trials of iteration 1.  The call returns 1 with
    terminated = 1 and leaves every vertex, tail poses and tail cones included, with the bits a one-iteration call leaves (the same
    launches up to there); a call whose only trial is rejected (zero pivot injected) leaves the start's bits.
    Measured on an MI355X: so (returned 1, n_trials [1, 3], rejected 3, every vertex bit-identical)."""
    full, P0, L0 = grown_start(po, bench_graphs)
    gs = dict(full, pose_est=P0, lm_est=L0)
    r = lm_ref.run(po, full, 6, initial_lambda=REJECTION_LAMBDA0, max_trials=3, poses=P0, lms=L0)
    assert r["terminated"] and r["n_trials"].tolist() == [1, 3] and all(t["margin"] >= lm_ref.MIN_MARGIN for t in r["trials"])
    A = grown_at(pkg, gs); da, sa, ia = A.optimize_lm(1, initial_lambda=REJECTION_LAMBDA0)
    G = grown_at(pkg, gs); done, st, info = G.optimize_lm(6, initial_lambda=REJECTION_LAMBDA0, max_trials=3)
    print("grown terminate: returned %d terminated %d n_trials %s rejected %d; tail poses %s" % (done, info["terminated"], info["n_trials"].tolist(), info["rejected"],
          np.array_equal(G.poses()[-GROWN_H:], A.poses()[-GROWN_H:])))
    assert da == 1 and done == 1 and info["terminated"] == 1 and info["n_trials"].tolist() == [1, 3] and info["rejected"] == 3
    assert np.array_equal(G.poses(), A.poses()) and np.array_equal(G.landmarks(), A.landmarks()) and st.chi2_final == sa.chi2_final
    assert not np.array_equal(G.poses()[-GROWN_H:], P0[-GROWN_H:]) and not np.array_equal(G.landmarks()[-2:], L0[-2:])     # (the accepted step did move the tail)
    A.close(); G.close()
    Z = grown_at(pkg, gs); Z.optimize(0); Z.debug_fail_at_iteration(1, 1)
    done, st, info = Z.optimize_lm(4, max_trials=1)
    assert done == 0 and info["terminated"] == 1 and info["rejected"] == 1 and st.numeric_failure == 0
    assert np.array_equal(Z.poses(), P0) and np.array_equal(Z.landmarks(), L0)
    done, st = Z.optimize(2); assert done == 2 and st.numeric_failure == 0
    Z.close()


# ---------------------------------------------------------------- 5. terminate
def test_terminate_leaves_the_estimates_bit_identical(pkg, po, bench_graphs):
    """max_trials = 3 from x1 (seed 1), initial_lambda 1e-12: the checker rejects all three (rho -0.232 each).  The call returns 0 with
    terminated = 1, rejected = 3, poses and landmarks bit-identical to those before the call.
    Measured on an MI355X: so; lambda[0] = 8e-12 (1e-12 * 2 * 4), chi2 63935.07089 on both sides."""
    g, _, _, P1, L1, _, _ = starts(po, bench_graphs, 1)
    r = lm_ref.run(po, g, 6, initial_lambda=REJECTION_LAMBDA0, max_trials=3, poses=P1, lms=L1)
    assert r["terminated"] and r["rejected"] == 3 and all(t["margin"] >= lm_ref.MIN_MARGIN for t in r["trials"])
    G = fresh(pkg, dict(g, pose_est=P1, lm_est=L1))
    P_before, L_before = G.poses(), G.landmarks()
    done, st, info = G.optimize_lm(6, initial_lambda=REJECTION_LAMBDA0, max_trials=3)
    print("terminate: returned %d, terminated %d, rejected %d, trials %d, n_trials %s, lambda[] %s, chi2 %.10g (checker %.10g)"
          % (done, info["terminated"], info["rejected"], info["trials"], info["n_trials"].tolist(), info["lambda"].tolist(), st.chi2_final, r["chi2_final"]))
    assert done == 0 and info["terminated"] == 1 and info["rejected"] == 3 and info["trials"] == 3 and info["iterations"] == 0
    assert info["n_trials"].tolist() == [3] and info["lambda"][0] == 8e-12
    assert np.array_equal(G.poses(), P_before) and np.array_equal(G.landmarks(), L_before)
    assert np.array_equal(P_before, P1) and np.array_equal(L_before, L1)
    assert st.chi2_initial == st.chi2_final and abs(st.chi2_final - r["chi2_final"]) <= 1e-9 * r["chi2_final"]
    assert abs(G.chi2() - st.chi2_final) <= 1e-12 * st.chi2_final
    G.close()


@pytest.mark.parametrize("total", sorted(BOUNDARY))
def test_terminate_at_the_workgroup_boundary_leaves_the_estimates_bit_identical(pkg, po, bench_graphs, total):
    """The test above at N + M = 255, 256, 257 from test_lm_cpu.boundary_start: one workgroup of the vertex-parallel kernels with an
    idle last thread, exactly one, and a second one whose only thread is a landmark (two scale partials, the second from a single
    thread; the restore of the last landmark is that workgroup's).  The checker rejects all three trials (rho -0.148 / -0.688 / -0.239,
    margins 0.14 / 0.60 / 0.23: asserted here again, test_lm_cpu.py asserts them without a GPU); the call returns 0 with terminated = 1,
    rejected = 3 and every pose and landmark holds the bits from before the call.
    Measured on an MI355X: so at all three sizes; lambda[0] = 8e-12, chi2 12834.73073 / 10548.07652 / 12691.96237 on both sides."""
    g, P1, L1 = boundary_start(po, bench_graphs, total)
    r = boundary_terminate(po, g, P1, L1)
    G = fresh(pkg, dict(g, pose_est=P1, lm_est=L1))
    P_before, L_before = G.poses(), G.landmarks()
    done, st, info = G.optimize_lm(6, initial_lambda=REJECTION_LAMBDA0, max_trials=3)
    print("N + M = %d terminate: returned %d, terminated %d, rejected %d, trials %d, n_trials %s, lambda[] %s, chi2 %.10g (checker %.10g, rho %.4f)"
          % (total, done, info["terminated"], info["rejected"], info["trials"], info["n_trials"].tolist(), info["lambda"].tolist(), st.chi2_final, r["chi2_final"], r["trials"][0]["rho"]))
    assert done == 0 and info["terminated"] == 1 and info["rejected"] == 3 and info["trials"] == 3 and info["iterations"] == 0
    assert info["n_trials"].tolist() == [3] and info["lambda"][0] == 8e-12
    assert np.array_equal(G.poses(), P_before) and np.array_equal(G.landmarks(), L_before)
    assert np.array_equal(P_before, P1) and np.array_equal(L_before, L1)
    assert st.chi2_initial == st.chi2_final and abs(st.chi2_final - r["chi2_final"]) <= 1e-9 * r["chi2_final"]
    G.close()


def test_zero_pivot_with_a_second_workgroup_of_one_landmark_is_a_rejection(pkg, po, bench_graphs):
    """N + M = 257, a zero pivot injected into the only trial (gs_debug_fail_at_iteration(1, 1), as in the tests above and below;
    max_trials = 1): the call returns 0 with rejected = 1, terminated = 1 and numeric_failure = 0, and leaves the start's bits in every
    vertex, the landmark of the second workgroup included; a following optimize(2) runs clean."""
    g, P1, L1 = boundary_start(po, bench_graphs, 257)
    Z = fresh(pkg, dict(g, pose_est=P1, lm_est=L1)); Z.optimize(0); Z.debug_fail_at_iteration(1, 1)
    done, st, info = Z.optimize_lm(4, max_trials=1)
    print("N + M = 257 zero pivot: returned %d terminated %d rejected %d numeric_failure %d first_failure %d" % (done, info["terminated"], info["rejected"], st.numeric_failure, st.first_failure))
    assert done == 0 and info["terminated"] == 1 and info["rejected"] == 1 and st.numeric_failure == 0
    assert np.array_equal(Z.poses(), P1) and np.array_equal(Z.landmarks(), L1)
    done, st = Z.optimize(2); assert done == 2 and st.numeric_failure == 0
    Z.close()


# ---------------------------------------------------------------- 6. monotone where Gauss-Newton is not
def test_monotone_where_gauss_newton_is_not(pkg, po, bench_graphs):
    """From x0 (seed 1): Gauss-Newton's chi2 rises twice (CPU test); the accepted chi2[] of LM is non-increasing over 10 iterations.
    The end: below GN's value after 10 gs_optimize iterations from the same start, or — when the checker's own final value is not
    below the oracle's GN value — within the test-2 tolerance of the checker's.  Which applies is decided by the checker, on the CPU.
    Measured: the checker's LM ends at 1398.0584, the oracle's Gauss-Newton at 1385.8053 (it recovers after its two rises), so the
    second claim applies; GPU 527345 46638.921 21895.293 4350.6152 2245.1653 1966.3225 1663.3628 1553.4715 1527.1337 1416.8433 ->
    1398.0584, the checker's to the digits shown; plain yardstick 7.3e-12."""
    g, P0, L0, _, _, chi_gn, gn_final = starts(po, bench_graphs, 1)
    r = lm_ref.run(po, g, 10, poses=P0, lms=L0)
    assert r["rejected"] == 0 and all(t["margin"] >= lm_ref.MIN_MARGIN for t in r["trials"])
    gs = dict(g, pose_est=P0, lm_est=L0)
    A = fresh(pkg, gs); done, stA = A.optimize(10); assert done == 10
    og = make_oracle_graph(po, gs); og.optimize(10, ordering=1)
    y = max(rel(A.poses(), og.poses()), rel(A.landmarks(), og.landmarks()), abs(stA.chi2_final - gn_final) / gn_final); A.close()
    G = fresh(pkg, gs); done, st, info = G.optimize_lm(10)
    seq = np.r_[info["chi2"], st.chi2_final]
    below = r["chi2_final"] < gn_final
    print("LM chi2[] %s\nGN (GPU) after 10: %.8g, oracle %.8g; LM final %.8g, checker %.8g; claim: %s; plain yardstick %.2e"
          % (" ".join("%.8g" % v for v in seq), stA.chi2_final, gn_final, st.chi2_final, r["chi2_final"], "below GN" if below else "the checker's value", y))
    assert done == 10 and info["rejected"] == 0 and np.all(np.diff(seq) <= 0)
    if below:
        assert st.chi2_final < stA.chi2_final
    else:
        assert abs(st.chi2_final - r["chi2_final"]) <= max(4 * y, 1e-9) * r["chi2_final"]
    G.close()


# ---------------------------------------------------------------- 8. launch modes
def test_launch_modes_and_repeated_calls_are_bit_identical(pkg, po, bench_graphs):
    """Whole-tree launches against tree = 0 (one launch per level), and a fresh handle against a second call on the same handle after
    the estimates were set back to the start: the same bits in the estimates and in every figure of gs_lm_info."""
    g, _, _, P1, L1, _, _ = starts(po, bench_graphs, 1)
    gs = dict(g, pose_est=P1, lm_est=L1)
    def run(G):
        done, st, info = G.optimize_lm(6, initial_lambda=REJECTION_LAMBDA0)
        return done, st.chi2_final, info, G.poses(), G.landmarks()
    A = fresh(pkg, gs); a = run(A)
    B = fresh(pkg, gs, debug=dict(tree=0)); b = run(B); B.close()
    set_start(A, P1, L1); c = run(A); A.close()
    for label, o in (("tree=0", b), ("second call", c)):
        same = (o[0] == a[0] and o[1] == a[1] and np.array_equal(o[3], a[3]) and np.array_equal(o[4], a[4]) and
                all(np.array_equal(o[2][k], a[2][k]) for k in a[2]))
        print("%s: accepted %d n_trials %s chi2_final %.17g bit-identical %s" % (label, o[0], o[2]["n_trials"].tolist(), o[1], same))
        assert same
    assert a[2]["n_trials"].tolist() == REJECTION_TRIALS[1]


# ---------------------------------------------------------------- 9. no residue
def test_no_residue_on_the_handle(pkg, po, bench_graphs):
    """After optimize_lm: gs_optimize(10) equals a fresh handle's from the same estimates bit for bit; iterate + synchronize report
    nothing; the marginal getters return GS_ERR_NOT_INITIALIZED until recomputed; gs_chi2 equals the call's final chi2 (1e-9)."""
    g, _, _, P1, L1, _, _ = starts(po, bench_graphs, 1)
    G = fresh(pkg, dict(g, pose_est=P1, lm_est=L1))
    G.compute_marginals(); G.pose_covariances()
    done, st, info = G.optimize_lm(3, initial_lambda=REJECTION_LAMBDA0)
    assert done == 3 and info["rejected"] == 7
    with pytest.raises(pkg.binding.GsError) as e:
        G.pose_covariances()
    assert e.value.code == -6
    chi = G.chi2()
    print("chi2 after the call %.17g, info %.17g, rel %.2e" % (chi, st.chi2_final, abs(chi - st.chi2_final) / chi))
    assert abs(chi - st.chi2_final) <= 1e-9 * chi
    P, L = G.poses(), G.landmarks()
    F = fresh(pkg, dict(g, pose_est=P, lm_est=L))
    d1, s1 = G.optimize(10); d2, s2 = F.optimize(10)
    assert d1 == d2 == 10 and s1.numeric_failure == 0 and s1.first_failure == 0
    assert np.array_equal(G.poses(), F.poses()) and np.array_equal(G.landmarks(), F.landmarks()) and s1.chi2_final == s2.chi2_final
    assert G.iterate() == 1 and F.iterate() == 1
    G.synchronize(); F.synchronize()                                 # (raises if a failure, stop or LM flag were left behind)
    G.sync_estimates(); F.sync_estimates()
    assert np.array_equal(G.poses(), F.poses()) and np.array_equal(G.landmarks(), F.landmarks())
    G.compute_marginals(); G.pose_covariances()
    # a terminated call leaves nothing behind either
    T = fresh(pkg, dict(g, pose_est=P1, lm_est=L1)); T.optimize_lm(6, initial_lambda=REJECTION_LAMBDA0, max_trials=2)
    U = fresh(pkg, dict(g, pose_est=P1, lm_est=L1))
    T.optimize(4); U.optimize(4)
    assert np.array_equal(T.poses(), U.poses()) and np.array_equal(T.landmarks(), U.landmarks())
    for H in (G, F, T, U):
        H.close()


# ---------------------------------------------------------------- 10. a zero pivot is a rejected trial
def test_zero_pivot_in_a_trial_is_a_rejection(pkg, po, bench_graphs):
    """gs_debug_fail_at_iteration arms code 1 on the first solve of the call (the sanctioned fault injection; no singular H is built):
    the call goes on, its first trial is counted as rejected, and the result is the checker's when the checker is told to reject that
    trial.  From x0 (seed 1) with default parameters: the checker runs [2, 1, 1, 1] trials.
    Measured on an MI355X: [2, 1, 1, 1], one rejection, estimates 1.8e-15, lambda[] 7.3e-14 (plain yardstick 1.3e-10)."""
    g, P0, L0, _, _, _, _ = starts(po, bench_graphs, 1)
    r = lm_ref.run(po, g, 4, poses=P0, lms=L0, force_reject=(0,))
    assert all(t["margin"] >= lm_ref.MIN_MARGIN for t in r["trials"])
    gs = dict(g, pose_est=P0, lm_est=L0)
    A = fresh(pkg, gs); A.optimize(4); og = make_oracle_graph(po, gs); og.optimize(4, ordering=1)
    y = max(rel(A.poses(), og.poses()), rel(A.landmarks(), og.landmarks())); A.close()
    G = fresh(pkg, gs); G.initialize_optimization()
    G.debug_fail_at_iteration(1, 1)
    done, st, info = G.optimize_lm(4)
    e_est = max(rel(G.poses(), r["P"]), rel(G.landmarks(), r["L"])); e_lam = float(np.abs(info["lambda"] / r["lam"] - 1).max())
    print("zero pivot: accepted %d n_trials %s (checker %s) rejected %d first_failure %d numeric_failure %d | estimates %.2e lambda[] %.2e (plain yardstick %.2e)"
          % (done, info["n_trials"].tolist(), r["n_trials"].tolist(), info["rejected"], st.first_failure, st.numeric_failure, e_est, e_lam, y))
    assert done == 4 and info["terminated"] == 0 and info["n_trials"].tolist() == r["n_trials"].tolist() and info["n_trials"][0] == 2
    assert info["rejected"] == r["rejected"] == 1 and st.numeric_failure == 0
    assert info["lambda"][0] == 2 * info["lambda_initial"]
    assert e_est <= max(4 * y, 1e-9) and e_lam <= max(4 * y, 1e-9)
    done, st = G.optimize(2); assert done == 2 and st.numeric_failure == 0
    G.close()


# ---------------------------------------------------------------- 11. a flag timeout inside an LM call
def test_flag_timeout_falls_back_to_level_launches_and_finishes(pkg, bench_graphs):
    """The branch gs_optimize_lm shares with gs_optimize: gs_debug_fail_at_iteration arms code 2 (a whole-tree launch gave up on a front's
    flag; the hook sets the status word, nothing stalls) on the first trial.  The call falls back to one launch per level, runs the trial
    again and finishes: three accepted iterations, and — the launch modes being bit-identical — the estimates of an uninjected handle."""
    _, g = bench_graphs(1000, 200)
    A = fresh(pkg, g); da, sa, _ = A.optimize_lm(3)
    G = fresh(pkg, g); G.initialize_optimization()
    G.debug_fail_at_iteration(1, 2)
    done, st, info = G.optimize_lm(3)
    print("LM through a flag timeout: accepted %d (uninjected %d) first_failure %d fell_back %d numeric_failure %d n_trials %s"
          % (done, da, st.first_failure, st.fell_back, st.numeric_failure, info["n_trials"].tolist()))
    assert st.first_failure == 2 and st.fell_back == 1 and st.numeric_failure == 0
    assert done == 3 and da == 3 and sa.fell_back == 0 and sa.first_failure == 0
    assert np.array_equal(G.poses(), A.poses()) and np.array_equal(G.landmarks(), A.landmarks())
    A.close(); G.close()
