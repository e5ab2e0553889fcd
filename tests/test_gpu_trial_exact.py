"""The step control of gs_optimize_dogleg and gs_optimize_lm (csrc/gs_dogleg.hip, csrc/gs_lm.hip, the readers and reductions of
csrc/gs_trial_dev.hpp) against the exact reference tests/trial_exact_ref.py, from what the handle itself exports — no oracle solve, no
tolerance that follows cond(H).  Every trial runs on a fresh handle with max_trials = 1 and one iteration.

Cases (test_trial_exact_cpu.CASES; its census shows that they reach every path and that the bounds can fail): every case of
lin_shapes.CASES at its forced lane count, one run per family of side_shapes.RUNS on the fused and the gather path, five grown plans of
tail_shapes.py, the graphs with N + M = 255, 256, 257 on both paths, and the 600-pose stretch of bench 1000 / 200 grown by 6 poses and 2
cones (728 vertices: three workgroups, the last one partly filled and ending in the tail cones).  Four shape graphs of the 56 have a
singular H (free landmarks nothing observes: test_trial_exact_cpu.DROPPED, with the reason) and are left out: 64 cases run.

Dogleg, per case: a GN handle (initial_delta = 1e4) whose export_delta is held to exact_ref's backward error omega <= 64 (f_max + 2) u
against its own export_system, with the perturbed-increment counter-check; then delta = 0.5 (|h_gn| + |h_sd|) (DL), |h_sd| (1 + 1e-3)
(DL where delta^2 - ss cancels) and 0.5 |h_sd| (SD), the norms from the reference on the GN handle's export: the export is bit-identical to
the GN handle's, step_kind the reference's, every scalar of export_delta within its bound of the reference's h_dl (computed from this
H and b and the GN handle's h_gn bits), fixed rows exactly 0, | |h_dl| - delta | within its bound, and the verdict and delta_final what
the rho rebuilt from the handle's own chi_old, chi_new and the exact gain of its own H, b and h_dl says: 3 sqrt(hh) within its bound,
0.5 delta or delta exactly.  gs_export_delta is k_update's copy of xe, which the blend kernel has overwritten with h_dl, and a rejection
restores the estimates only: it is the applied step after a rejected trial too.  What a rejected trial does not leave behind is chi_new
(gs_stats.chi2_final stays at the accepted point), so its rho is not rebuilt: it must halve delta exactly and leave every estimate's bits.
LM, per case, initial_lambda = 0.01 and 1e-12 max |H_jj|: lambda placement bit for bit (fl(H_jj + lambda) on every free diagonal scalar
of a pose, a gather-path landmark, a tail pose, a tail cone; within 2 k u (H_jj + lambda) on a fused-path base landmark, k its observation
edges — an upper bound of its slots), every other entry bit-identical to the undamped export of a second handle (a grown handle is
linearised as it stands: with one more gs_initialize_optimization in front of gs_linearize the entries that hold tail terms came out one
ulp away from the trial's, on all six grown cases, in entries lambda does not touch), omega of the damped solve, lambda_final against the reference's update from the handle's own dx, b, lambda, chi_old, chi_new; lambda_0 = tau max |H_jj| bit
for bit (within the slot bound where the maximum sits on a fused-path landmark), and the two variants of test_trial_exact_cpu.variant.
Near the thresholds (test_trial_exact_cpu.NEAR_*): four dogleg trials with rho 1e-5 .. 1e-4 beside 0.75 and 0.25, all decided, both sides
of both thresholds taken on the device; LM trials in the cubic window and in both clips, and a rejected one.

Every test prints its worst err / bound before it asserts (-s); the printed run is profiles/trial_exact_gpu_suite.txt.
Measured on an MI355X (that file), 133 tests, worst err / bound per class over the 64 cases: h_dl 0.025 (DL in the middle), 0.007 (DL beside
|h_sd|), 0.002 (SD); | |h_dl| - delta | 0.014; delta_final = 3 sqrt(hh) 0.015; omega at most 12.95 u of 3712 u (GN handles and damped solves
alike, 192 solves; the perturbed increment 3e6 u and more); lambda on the poses, the gather-path landmarks and the tail vertices bit for
bit in all 128 damped trials; on fused-path landmarks 0.497 — one ulp of H_jj on a landmark with two observation edges, where the bound
is 4 u (H_jj + lambda): the granularity of fp64, not a loose count —; lambda_0 bit for bit in all 64 cases and in the "fixed" variant,
0.000 of the slot bound in the "wide" one; lambda_final 0.002 in the cubic window (rho 0.8839) and bit for bit in both clips (126 of the
per-case trials end in the 1/3 clip, 2 in the 2/3 clip).  The four near-threshold dogleg trials: rho - 0.75 = +5.03e-5 / -5.40e-5 with a
bound of 7.4e-14, rho - 0.25 = +9.68e-5 / -4.58e-5 with 3.9e-14; grow, keep, keep, halve as the rebuilt rho says.
Comparisons left undecided: none — step kind 0, verdict 0, delta_final branch 0, clip 0 over the per-case trials, and 0 among the
near-threshold and bisected trials, where a tie would fail the test.  No per-case trial was rejected on the device; the rejected trials
are the Gauss-Newton trial and the lambda = 1e-12 trial from the near-threshold start."""
import numpy as np
import pytest

import exact_ref as xr
import hmul_ref as hr
import lin_shapes as ls
import side_shapes as ss
import tail_shapes as ts
import trial_exact_ref as tx
from plan_exec import Plan
from test_gpu_exact import check_omega
from test_trial_exact_cpu import CASES, DROPPED, GROWN_H, GROWN_KEEP, NEAR_DELTA, NEAR_LAMBDA, VARIANT_BASE, deltas_of, near_start, variant
from test_lm_cpu import BOUNDARY

pytestmark = pytest.mark.gpu
U = tx.U
DIAG3, DIAG2 = tx.DIAG3, tx.DIAG2
UNDECIDED = {"kind": 0, "verdict": 0, "delta": 0, "clip": 0}       # comparisons left unjudged over the run (printed by the last test)
WORST = {}


def note(k, v):
    WORST[k] = max(WORST.get(k, 0.0), float(v))


def handle(pkg, frontend, bench_graphs, fam, name, path):
    """(fresh handle of the case, the graph it holds, (first tail pose, first tail cone) or (None, None), gather path forced)"""
    if fam == "lin":
        g, _, _ = ls.graph(name); G = pkg.Graph(device=0, **ls.handle_kw(name)); G.load_bench_graph(g)
        return G, g, (None, None), False
    if fam == "side":
        G = ss.load(pkg.Graph(device=0, **ss.handle_kw(name, path)), name)
        return G, ss.case(name)["g"], (None, None), path == "gather"
    if fam == "tail":
        from test_gpu_tail_exact import grown
        base = ts.graph(name, pkg, frontend)[0]; G, full, _ = grown(pkg, frontend, name)
        return G, full, (len(base["pose_est"]), len(base["lm_est"])), False
    if fam == "boundary":
        g = bench_graphs(*BOUNDARY[int(name[1:])][:2])[1]; G = pkg.Graph(device=0, linearize_gather=int(path)); G.load_bench_graph(g)
        return G, g, (None, None), bool(path)
    from conftest import split_for_growth
    from test_gpu_lm import grown
    base = split_for_growth(bench_graphs(1000, 200)[1], GROWN_H, GROWN_KEEP)[0]
    G, full = grown(pkg, bench_graphs(1000, 200)[1], GROWN_H, GROWN_KEEP)
    return G, full, (len(base["pose_est"]), len(base["lm_est"])), False


def plan_of(G):
    P = Plan(G.plan_export()); fmax = int((P.npiv + P.nbnd).max())
    return P, fmax, 64 * (fmax + 2)


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


def assert_bits(got, want, tag):
    """bit for bit, naming the first entries that differ"""
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d entries differ, first %s" % (tag, len(bad), "; ".join("%s got %.17g want %.17g" % (tuple(i), got[tuple(i)], want[tuple(i)]) for i in bad[:6])))


def judge(S, g, G, delta, done, st, info, h, P0, L0, tag, must_decide=False):
    """the verdict and delta_final of a dogleg trial against the rho rebuilt from the handle's own numbers; returns the rebuilt record"""
    assert info["trials"] == 1 and info["delta"][0] == delta and info["rejected"] == 1 - done
    if done == 0:                                                    # chi_new is not exported: rho <= 0 < 0.25, delta halves, nothing moved
        assert not must_decide
        assert info["delta_final"] == 0.5 * delta and np.array_equal(G.poses(), P0) and np.array_equal(G.landmarks(), L0), tag
        return None
    r = tx.gain_of_step(S, h, delta, info["chi2"][0], st.chi2_final)
    if not r["accept_decided"]:
        assert not must_decide; UNDECIDED["verdict"] += 1
    else:
        assert r["accept"], (tag, float(r["rho"].value))
    if r["rho_decided"] and r["max_decided"]:
        q = tx.err_over_bound(info["delta_final"], r["delta_next"]); note("delta_final (3 sqrt(hh))", q)
        assert q <= 1.0, (tag, r["branch"], info["delta_final"], float(r["delta_next"].value), r["delta_next"].bound)
        if r["delta_next"].bound > 0:
            assert tx.err_over_bound(info["delta_final"] * (1 + 1e-9), r["delta_next"]) > 1.0
    else:
        assert not must_decide; UNDECIDED["delta"] += 1
    return r


# ---------------------------------------------------------------- dogleg, per case
@pytest.mark.parametrize("fam,name,path", [c for c in CASES if c[:2] not in DROPPED])
def test_dogleg_trials(pkg, frontend, bench_graphs, fam, name, path):
    tag = "%s %s%s" % (fam, name, "" if path is None else " %s" % path)
    G, g, tail, _ = handle(pkg, frontend, bench_graphs, fam, name, path)
    P0, L0 = G.poses(), G.landmarks()
    done, st, info = G.optimize_dogleg(1, initial_delta=1e4, max_trials=1)
    B0 = G.export_system(); dp, dl = G.export_delta()
    P, fmax, C = plan_of(G)
    N, M = len(B0["Hpp_diag"]), len(B0["Hll_diag"]); fp, fl = hr.masks(g, N, M)
    check_omega(xr.BlockSystem(B0, g, P.pose_gidx, P.lm_gidx), dp, dl, C, "%s GN f_max %d" % (tag, fmax))
    assert not dp[~fp].any() and not dl[~fl].any()
    S = tx.System.from_blocks(B0, g); h_gn = S.pack(dp, dl)
    r0, deltas = deltas_of(S, h_gn)
    assert r0["kind"] == tx.GN and r0["kind_decided"] and info["step_kind"].tolist() == [tx.GN]
    judge(S, g, G, 1e4, done, st, info, h_gn, P0, L0, tag + " GN")
    G.close()
    line = []
    for label, kind, delta in deltas[1:]:
        H, _, _, _ = handle(pkg, frontend, bench_graphs, fam, name, path)
        done, st, info = H.optimize_dogleg(1, initial_delta=delta, max_trials=1)
        assert same_bits(H.export_system(), B0), label
        r = tx.dogleg(S, h_gn, delta)
        if r["kind_decided"]:
            assert r["kind"] == kind and info["step_kind"].tolist() == [kind], (tag, label, info["step_kind"])
        else:
            UNDECIDED["kind"] += 1
        hp, hl = H.export_delta()
        assert not hp[~fp].any() and not hl[~fl].any()
        h = S.pack(hp, hl)
        w, n = tx.check_vector(h, r, "%s %s" % (tag, label)); note("h_dl %s" % label, w)
        k = int(np.argmax(np.abs(h))); hb = h.copy(); hb[k] *= 1 + 1e-9       # the counter-check: the largest scalar off by 1e-9 must show
        assert abs(float(tx.mpf(float(hb[k])) - r["h"][k])) > r["e_h"][k], (tag, label)
        nv = tx.norm_of_step(h, r["e_h"]); qn = abs(float(nv.value - tx.mpf(float(delta)))) / nv.bound; note("| |h_dl| - delta |", qn)
        assert qn <= 1.0, (tag, label, float(nv.value), delta, nv.bound)
        assert abs(float(nv.value) * 1e-9) > nv.bound
        jr = judge(S, g, H, delta, done, st, info, h, P0, L0, "%s %s" % (tag, label))
        line.append("%s delta %.6g h_dl %.3f of %d |h|-delta %.3f%s" % (label, delta, w, n, qn, " rho %+.4f delta_final %.6g (%s)" % (float(jr["rho"].value), info["delta_final"], jr["branch"]) if jr else " REJECTED"))
        H.close()
    print("%s: n %d |h_gn| %.4g |h_sd| %.4g | worst err / bound: %s" % (tag, S.nf, float(r0["gn"].value), float(r0["sd"].value), "; ".join(line)))


def test_dogleg_near_the_rho_thresholds(pkg, po, bench_graphs):
    """the four deltas of test_trial_exact_cpu.NEAR_DELTA from its start: every verdict and every delta_final branch is decided and is the
    one the rebuilt rho names; both sides of 0.75 and of 0.25 are taken on the device"""
    g, P1, L1 = near_start(po, bench_graphs); gs = dict(g, pose_est=P1, lm_est=L1)
    taken = {}
    for key, delta in NEAR_DELTA.items():
        G = pkg.Graph(device=0); G.load_bench_graph(gs)
        done, st, info = G.optimize_dogleg(1, initial_delta=delta, max_trials=1)
        S = tx.System.from_blocks(G.export_system(), g); h = S.pack(*G.export_delta())
        assert done == 1 and info["step_kind"].tolist() == [tx.DL]
        r = judge(S, g, G, delta, done, st, info, h, P1, L1, "near " + key, must_decide=True)
        gap = float(r["rho"].value) - float(key[:-1])
        print("near %s: delta %.17g rho - %s = %+.3e (bound %.2e) branch %s delta_final %.17g" % (key, delta, key[:-1], gap, r["rho"].bound, r["branch"], info["delta_final"]))
        assert 1e-6 < abs(gap) < 1e-3 and (gap > 0) == (key[-1] == "+")
        taken[key] = r["branch"]; G.close()
    assert taken == {"0.75+": "grow", "0.75-": "keep", "0.25+": "keep", "0.25-": "halve"}
    # from the same start the full Gauss-Newton step is rejected (the checker's rho -0.448): delta halves, every estimate keeps its bits
    G = pkg.Graph(device=0); G.load_bench_graph(gs)
    done, st, info = G.optimize_dogleg(1, initial_delta=1e4, max_trials=1)
    S = tx.System.from_blocks(G.export_system(), g); h = S.pack(*G.export_delta())
    r = tx.dogleg(S, h, 1e4)
    print("near GN: returned %d terminated %d kind %s delta_final %.6g |h_gn| %.6g" % (done, info["terminated"], info["step_kind"].tolist(), info["delta_final"], float(r["gn"].value)))
    assert done == 0 and info["terminated"] == 1 and r["kind"] == tx.GN and r["kind_decided"] and info["step_kind"].tolist() == [tx.GN]
    assert judge(S, g, G, 1e4, done, st, info, h, P1, L1, "near GN") is None
    G.close()


# ---------------------------------------------------------------- LM, per case
def lm_trial(pkg, frontend, bench_graphs, fam, name, path, U0, md, f, tag):
    """one damped trial at lambda = f max |H_jj|: placement, the untouched entries, omega, scale / rho / update"""
    lam = f * md
    H, g, tail, gather = handle(pkg, frontend, bench_graphs, fam, name, path)
    P0, L0 = H.poses(), H.landmarks()
    done, st, info = H.optimize_lm(1, initial_lambda=lam, max_trials=1)
    assert info["trials"] == 1 and info["lambda_initial"] == lam
    D = H.export_system(); dp, dl = H.export_delta(); P, fmax, C = plan_of(H)
    N, M = len(D["Hpp_diag"]), len(D["Hll_diag"]); fp, fl = hr.masks(g, N, M)
    fused = (not gather) and P.ell_R <= ls.LIN_R; Mb = tail[1] if tail[1] is not None else M
    # placement
    want_p = U0["Hpp_diag"].copy(); want_p[np.ix_(fp, DIAG3)] += lam
    assert_bits(D["Hpp_diag"], want_p, "%s lambda %.17g: a pose's block (tail poses included)" % (tag, lam))
    want_l = U0["Hll_diag"].copy(); want_l[np.ix_(fl, DIAG2)] += lam
    exact_l = np.ones(M, dtype=bool)
    if fused:
        exact_l[:Mb] = False
    assert_bits(D["Hll_diag"][exact_l], want_l[exact_l], "%s lambda %.17g: a landmark's block (gather path / tail cones)" % (tag, lam))
    assert_bits(D["Hll_diag"][:, (1, 2)], U0["Hll_diag"][:, (1, 2)], tag + ": a landmark's off-diagonal entry"); assert_bits(D["Hll_diag"][~fl], U0["Hll_diag"][~fl], tag + ": a fixed landmark's block")
    qs = 0.0
    if fused:
        sb = tx.slot_bound(g, M, U0["Hll_diag"][:, DIAG2], lam); e = np.abs(D["Hll_diag"][:, DIAG2] - want_l[:, DIAG2])
        m = fl[:, None] & (sb > 0) & ~exact_l[:, None]
        qs = float((e[m] / sb[m]).max()) if m.any() else 0.0; note("lambda on a fused-path landmark", qs)
        assert qs <= 1.0, tag
        assert np.all(lam > 2 * sb[m]) or f < 1e-6                   # (the larger lambda stands far above the bound: one put in the wrong slot entry would show)
    for k in ("Hpp_off", "Hpl", "b_pose", "b_lm"):
        assert_bits(D[k], U0[k], "%s %s" % (tag, k))
    # the damped solve
    check_omega(xr.BlockSystem(D, g, P.pose_gidx, P.lm_gidx), dp, dl, C, "%s lambda %.3g f_max %d" % (tag, lam, fmax))
    assert not dp[~fp].any() and not dl[~fl].any()
    # scale, rho, the update
    free = np.concatenate([np.repeat(fp, 3), np.repeat(fl, 2)])
    dx = np.concatenate([dp.reshape(-1), dl.reshape(-1)]); b = np.concatenate([D["b_pose"].reshape(-1), D["b_lm"].reshape(-1)])
    if done == 1:
        r = tx.lm(dx, b, lam, info["chi2"][0], st.chi2_final, free)
        if r["accept_decided"]:
            assert r["accept"], tag
        else:
            UNDECIDED["verdict"] += 1
        if r["clip_decided"]:
            q = tx.err_over_bound(info["lambda_final"], r["lambda_next"]); note("lambda_final (%s)" % r["clip"], q)
            assert q <= 1.0, (tag, r["clip"], info["lambda_final"], float(r["lambda_next"].value))
        else:
            UNDECIDED["clip"] += 1
        line = "rho %+.5f %s lambda_final %.6g" % (float(r["rho"].value), r["clip"], info["lambda_final"])
    else:
        assert info["lambda_final"] == 2.0 * lam and np.array_equal(H.poses(), P0) and np.array_equal(H.landmarks(), L0), tag
        line = "REJECTED lambda_final = 2 lambda"
    H.close()
    return "lambda %.3g: %s path, slots %.3f, %s" % (lam, "fused" if fused else "gather", qs, line)


def undamped(pkg, frontend, bench_graphs, fam, name, path):
    G, g, tail, gather = handle(pkg, frontend, bench_graphs, fam, name, path)
    if tail[0] is None:
        G.initialize_optimization()
    else:                                                            # (a grown handle is planned already; the export below must be the grown plan's)
        assert G.plan_growths() > 0
    G.linearize(); U0 = G.export_system(); P, _, _ = plan_of(G)
    assert (G.plan_growths() > 0) == (tail[0] is not None)
    G.close()
    return U0, g, tail, (not gather) and P.ell_R <= ls.LIN_R


def check_lambda0(info, U0, g, tail, fused, tau, tag):
    md, where = tx.max_diag(U0, g); M = len(U0["Hll_diag"]); Mb = tail[1] if tail[1] is not None else M
    on_slots = fused and where[0] == "landmark" and where[1] < Mb
    if on_slots:
        bound = tau * float(tx.slot_bound(g, M, np.full((M, 2), md), 0.0)[where[1], 0]) + U * tau * md
        q = abs(info["lambda_initial"] - tau * md) / bound; note("lambda_0 on a fused-path landmark", q)
        assert q <= 1.0, (tag, info["lambda_initial"], tau * md)
    else:
        assert info["lambda_initial"] == tau * md, (tag, info["lambda_initial"], tau * md, where)
    assert info["lambda"][0] == info["lambda_initial"]
    return "lambda_0 %.17g = tau max |H_jj| on %s %d (%s)" % (info["lambda_initial"], where[0], where[1], "within the slot bound" if on_slots else "bit for bit")


@pytest.mark.parametrize("fam,name,path", [c for c in CASES if c[:2] not in DROPPED])
def test_lm_trials(pkg, frontend, bench_graphs, fam, name, path):
    tag = "%s %s%s" % (fam, name, "" if path is None else " %s" % path)
    U0, g, tail, fused = undamped(pkg, frontend, bench_graphs, fam, name, path)
    md, where = tx.max_diag(U0, g)
    lines = [lm_trial(pkg, frontend, bench_graphs, fam, name, path, U0, md, f, tag) for f in (0.01, 1e-12)]
    H, _, _, _ = handle(pkg, frontend, bench_graphs, fam, name, path)
    done, st, info = H.optimize_lm(1, max_trials=1)
    lines.append(check_lambda0(info, U0, g, tail, fused, 1e-5, tag)); H.close()
    print("%s: %s" % (tag, " | ".join(lines)))


@pytest.mark.parametrize("which", ["fixed", "wide"])
def test_lambda0_variants(pkg, which):
    """the largest diagonal entry on a fixed vertex is ignored; on a fused-path landmark that three wave tiles see it is found"""
    g, _, notes = variant(which); g0, _, _ = ls.graph(VARIANT_BASE)
    out = []
    for gg in (g0, g):
        G = pkg.Graph(device=0, **ls.handle_kw(VARIANT_BASE)); G.load_bench_graph(gg); G.initialize_optimization(); G.linearize()
        U0 = G.export_system(); P, _, _ = plan_of(G); G.close()
        assert P.ell_R <= ls.LIN_R
        H = pkg.Graph(device=0, **ls.handle_kw(VARIANT_BASE)); H.load_bench_graph(gg)
        done, st, info = H.optimize_lm(1, max_trials=1, tau=3e-3); H.close()
        out.append((U0, info, tx.max_diag(U0, gg)))
        print("variant %s: %s" % (which, check_lambda0(info, U0, gg, (None, None), True, 3e-3, which)))
    (Ua, ia, ma), (Ub, ib, mb) = out
    if which == "fixed":
        assert ma == mb and ia["lambda_initial"] == ib["lambda_initial"]
    else:
        assert mb[1] == ("landmark", notes["wide"]) and mb[0] > 100 * ma[0] and ib["lambda_initial"] > 100 * ia["lambda_initial"]


def test_lm_near_the_clips(pkg, po, bench_graphs):
    """test_trial_exact_cpu.NEAR_LAMBDA from its start: lambda_final within its bound of the cubic update where it depends on rho (and a
    1e-9 error would show), bit for bit lambda * (2.0 / 3.0) and lambda * (1.0 / 3.0) in the clips, 2 lambda and the start's bits after a
    rejection; every one decided"""
    g, P1, L1 = near_start(po, bench_graphs); gs = dict(g, pose_est=P1, lm_est=L1)
    fp, fl = hr.masks(g, len(P1), len(L1)); free = np.concatenate([np.repeat(fp, 3), np.repeat(fl, 2)])
    for key, lam in NEAR_LAMBDA.items():
        G = pkg.Graph(device=0); G.load_bench_graph(gs)
        done, st, info = G.optimize_lm(1, initial_lambda=lam, max_trials=1)
        D = G.export_system(); dp, dl = G.export_delta()
        dx = np.concatenate([dp.reshape(-1), dl.reshape(-1)]); b = np.concatenate([D["b_pose"].reshape(-1), D["b_lm"].reshape(-1)])
        if key == "rejected":
            assert done == 0 and info["lambda_final"] == 2.0 * lam and np.array_equal(G.poses(), P1) and np.array_equal(G.landmarks(), L1)
            print("near LM %s: lambda %.3g rejected, lambda_final %.17g" % (key, lam, info["lambda_final"]))
        else:
            assert done == 1
            r = tx.lm(dx, b, lam, info["chi2"][0], st.chi2_final, free)
            q = tx.err_over_bound(info["lambda_final"], r["lambda_next"]); note("lambda_final near (%s)" % key, q)
            print("near LM %s: lambda %.3g rho %.6f (bound %.2e) scale bound / scale %.2e lambda_final %.17g err / bound %.3f" % (
                key, lam, float(r["rho"].value), r["rho"].bound, r["scale"].bound / float(r["scale"].value), info["lambda_final"], q))
            assert r["accept_decided"] and r["clip_decided"] and r["clip"] == key and q <= 1.0
            if key == "cubic":
                assert 0.86 < float(r["rho"].value) < 0.92 and tx.err_over_bound(info["lambda_final"] * (1 + 1e-9), r["lambda_next"]) > 1.0
            else:
                assert info["lambda_final"] == lam * ((2.0 / 3.0) if key == "2/3" else (1.0 / 3.0))
        G.close()


def test_zz_summary():
    """the figures of the run: worst err / bound per class, comparisons left undecided"""
    print("worst err / bound per class: " + "; ".join("%s %.3f" % kv for kv in sorted(WORST.items())))
    print("undecided comparisons: " + ", ".join("%s %d" % kv for kv in UNDECIDED.items()))
