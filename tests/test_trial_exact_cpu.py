"""The exact reference of the step control (trial_exact_ref.py) without a GPU: pinned against the numpy checkers, a census of every case
test_gpu_trial_exact.py runs, the proof that its bounds can fail, and the near-threshold inputs of that file, found here by bisection.

1. trial_exact_ref.dogleg / lm against dogleg_ref.blend / trial and lm_ref.trial on the oracle's system (bench 50 / 30, the random graph,
   lin_shapes t2_k4): the checkers are one fp64 evaluation of the same rule, so every value of theirs lies within the reference's bound.
2. Census of CASES: the oracle solves the system, |h_sd| < |h_gn| strictly, the deltas of the GPU file reach GN, DL, DL and SD with
   decided comparisons, and every result class times (1 + 1e-9) violates its bound wherever 1e-9 of the value exceeds twice the bound
   (printed: how many scalars of h_dl that covers; asserted: one at least on a base vertex, a tail vertex, a neighbour of a fixed vertex
   and a vertex of the last workgroup of 256, wherever the case has such a vertex and the step is not the Gauss-Newton one).
3. NEAR: bench 50 / 30 at its oracle optimum perturbed(seed 6, 5.0, 10.0) after one oracle Gauss-Newton step — from there the full
   Gauss-Newton step is rejected (rho -0.448).  Bisection of initial_delta gives trials with rho 1e-5 .. 1e-4 above and below 0.75 and 0.25;
   of initial_lambda an accepted LM trial with rho in (0.86, 0.92), where lambda_final depends on rho, and one each in the 2/3 and 1/3
   clips.  The values are constants below; the tests run the bisection again and assert that the constants still sit in their windows."""
import numpy as np
import pytest

import dogleg_ref as dr
import lin_shapes as ls
import lm_ref
import prior_ref as pr
import side_shapes as ss
import tail_shapes as ts
import trial_exact_ref as tx
from conftest import make_oracle_graph, random_graph, split_for_growth
from test_lm_cpu import BOUNDARY
from test_robust_cpu import perturbed

U = tx.U
GROWN_H, GROWN_KEEP = 6, 600                                        # test_gpu_lm.grown(): 600 poses + 128 cones = 728 vertices, three workgroups, tail cones last
SIDE_RUNS = [("wrap", 1), ("wrap", "gather"), ("priors", 8), ("priors", "gather"), ("cauchy", 4), ("cauchy", "gather"), ("mixed", 2), ("mixed", "gather"),
             ("launch255", 0), ("launch257", 0), ("launch257", "gather")]     # polar edges, priors, robust weights, an inactive edge, the launch boundary
TAIL = ("tail_mixed", "tail_mixed_t8", "tail_two_steps", "tail_wide", "tail_robust")
CASES = [("lin", n, None) for n in ls.CASES] + [("side", n, p) for n, p in SIDE_RUNS] + [("tail", n, None) for n in TAIL] + \
        [("boundary", "n%d" % t, gather) for t in sorted(BOUNDARY) for gather in (0, 1)] + [("grown", "bench600", None)]
SINGULAR = "H is singular (free landmarks without an observation edge): no Gauss-Newton step exists and the fused path leaves such a landmark undamped; left out of the GPU file"
DROPPED = {("lin", n): SINGULAR for n in ("n_lt_tile", "robust_t1_r1", "t1_groups", "t1_r1")}      # 4 of 56 graphs
GRAPHS = sorted({(f, n) for f, n, _ in CASES})

# the near-threshold inputs (the tests of part 3 find them again by bisection)
NEAR_SEED = 6
NEAR_DELTA = {"0.75+": 25.772634566888943, "0.75-": 25.777244643727666, "0.25+": 45.10806517463901, "0.25-": 45.11267525147773}
NEAR_LAMBDA = {"cubic": 0.6, "2/3": 0.1, "1/3": 10.0, "rejected": 1e-12}      # the checker's rho: 0.883, 0.758, 0.977, -0.448
WINDOW = (1e-5, 1e-4)

_models = {}


def model_of(po, pkg, frontend, bench_graphs, fam, name):
    """(dogleg_ref.Model, graph dict, first tail pose or None, first tail cone or None) of a case: what the GPU file's handle holds"""
    if (fam, name) not in _models:
        tail = (None, None)
        if fam == "lin":
            g, kernels, _ = ls.graph(name); m = dr.Model(po, g, kernels)
        elif fam == "side":
            c = ss.case(name); g = c["g"]; m = dr.Model(po, g, c["kernels"], c["polar"], c["pri"], c["off"])
        elif fam == "tail":
            base, _, g, kernels = ts.graph(name, pkg, frontend); m = dr.Model(po, g, kernels); tail = (len(base["pose_est"]), len(base["lm_est"]))
        elif fam == "boundary":
            g = bench_graphs(*BOUNDARY[int(name[1:])][:2])[1]; m = dr.Model(po, g)
        else:
            base, _, g = split_for_growth(bench_graphs(1000, 200)[1], GROWN_H, GROWN_KEEP); m = dr.Model(po, g); tail = (len(base["pose_est"]), len(base["lm_est"]))
        _models[fam, name] = (m, g) + tail
    return _models[fam, name]


def cpu_system(m, g, P=None, L=None):
    """(System over the vertices of g, h_gn packed, chi2) from the oracle at (P, L)"""
    P = np.asarray(g["pose_est"] if P is None else P, dtype=np.float64); L = np.asarray(g["lm_est"] if L is None else L, dtype=np.float64)
    og, n, colptr, rowind, values, b = m.system(P, L)
    B = pr.strip(og.linearize_blocks(), g)
    x = lm_ref._solve(m.po, n, colptr, rowind, values, b)
    S = tx.System.from_blocks(B, g)
    _, _, dp, dl = m.step(og, x)
    return S, S.pack(dp, dl), m.chi2(P, L), x, (n, colptr, rowind, values, b)


def deltas_of(S, h_gn):
    """the four deltas of the GPU file from the reference's norms: GN, DL in the middle, DL where delta^2 - ss cancels, SD"""
    r = tx.dogleg(S, h_gn, 1e4)
    gn, sd = float(r["gn"].value), float(r["sd"].value)
    return r, [("GN", tx.GN, 1e4), ("DL-mid", tx.DL, 0.5 * (gn + sd)), ("DL-edge", tx.DL, sd * (1 + 1e-3)), ("SD", tx.SD, 0.5 * sd)]


# ---------------------------------------------------------------- 1. the reference pinned
def _small(po, bench_graphs, which):
    if which == "bench50":
        return bench_graphs(50, 30)[1], None
    if which == "random":
        return random_graph(7), None
    g, kernels, _ = ls.graph("t2_k4")
    return g, kernels


@pytest.mark.parametrize("which", ["bench50", "random", "t2_k4"])
def test_reference_agrees_with_the_dogleg_checker(po, bench_graphs, which):
    g, kernels = _small(po, bench_graphs, which)
    m = dr.Model(po, g, kernels)
    pt = dr.Point(m, np.asarray(g["pose_est"], dtype=np.float64), np.asarray(g["lm_est"], dtype=np.float64))
    S = tx.System.from_ccs(pt.n, pt.colptr, pt.rowind, pt.values, pt.b)
    _, deltas = deltas_of(S, pt.h_gn)
    worst = {}
    def see(k, got, val):
        q = tx.err_over_bound(got, val); worst[k] = max(worst.get(k, 0.0), q)
        assert q <= 1.0, (k, got, float(val.value), val.bound)
        assert abs(got - float(val.value)) <= 64 * U * abs(got) + val.bound
    for label, kind, delta in deltas:
        t = dr.trial(m, pt, delta)
        r = tx.dogleg(S, pt.h_gn, delta, t["chi_old"], t["chi_new"])
        h, k2, gn, sd, _ = dr.blend(pt.h_gn, pt.h_sd, delta)
        assert r["kind"] == kind == k2 == t["kind"] and r["kind_decided"], label
        see("alpha", dr.alpha_of(pt.b, dr.sym_mul(pt.n, pt.colptr, pt.rowind, pt.values, pt.b)), r["alpha"])
        see("|h_gn|", gn, r["gn"]); see("|h_sd|", sd, r["sd"])
        w, _ = tx.check_vector(h, r, "%s %s" % (which, label)); worst["h_dl"] = max(worst.get("h_dl", 0.0), w)
        if kind == tx.DL:
            a = pt.h_gn - pt.h_sd; c = float(pt.h_sd @ a); q = float(a @ a); mm = delta * delta - sd * sd; disc = np.sqrt(c * c + q * mm)
            see("beta", (-c + disc) / q if c <= 0 else mm / (c + disc), r["beta"])
            assert abs(float(r["beta_neg"] - r["beta_pos"])) <= 1e-40 * abs(float(r["beta"].value)) + 1e-50 or not r["cc_decided"] or abs(float(r["beta_neg"] / r["beta_pos"] - 1)) < 1e-30
        see("hh", t["hdl"] ** 2, r["hh"]); see("gain", t["gain"], r["gain"]); see("rho", t["rho"], r["rho"]); see("delta_next", t["delta_next"], r["delta_next"])
        assert t["accepted"] == r["accept"] and r["accept_decided"]
    print("%s: worst err / bound of the numpy checker: %s" % (which, " ".join("%s %.3f" % kv for kv in worst.items())))


@pytest.mark.parametrize("which", ["bench50", "random", "t2_k4"])
def test_reference_agrees_with_the_lm_checker(po, bench_graphs, which):
    g, kernels = _small(po, bench_graphs, which)
    P, L = np.asarray(g["pose_est"], dtype=np.float64), np.asarray(g["lm_est"], dtype=np.float64)
    m = dr.Model(po, g, kernels)
    B = m.system(P, L)[0].linearize_blocks()
    md, where = tx.max_diag(B, g)
    assert md == lm_ref.max_diag(po, g, P, L, kernels)
    free = tx.System.from_blocks(B, g).free; worst = 0.0
    for f in (1e-12, 1e-5, 1e-2, 1e1):
        t = lm_ref.trial(po, g, P, L, f * md, kernels)
        r = tx.lm(np.concatenate([t["dpose"].reshape(-1), t["dlm"].reshape(-1)]), np.concatenate([B["b_pose"].reshape(-1), B["b_lm"].reshape(-1)]), f * md, t["chi_old"], t["chi_new"], free)
        qs, qr = tx.err_over_bound(t["scale"], r["scale"]), tx.err_over_bound(t["rho"], r["rho"]); worst = max(worst, qs, qr)
        assert qs <= 1.0 and qr <= 1.0, (f, qs, qr)
        if r["accept"]:
            a = 2.0 * t["rho"] - 1.0; want = f * md * max(1.0 / 3.0, min(1.0 - a * a * a, 2.0 / 3.0))
            assert tx.err_over_bound(want, r["lambda_next"]) <= 1.0 or not r["clip_decided"], (f, want, float(r["lambda_next"].value), r["clip"])
    print("%s: max |H_jj| %.6g on %s %d; worst err / bound of the numpy checker (scale, rho) %.3f" % ((which, md) + where + (worst,)))


def test_the_lambda_update_and_its_clips():
    """the three branches of the update at rho where they are decided, and the rejected one"""
    for rho, clip in ((0.5, "2/3"), (0.84, "2/3"), (0.89, "cubic"), (0.94, "1/3"), (1.2, "1/3")):
        v, which, decided = tx.lm_update(3.0, tx.Val(tx.mpf(rho), 1e-15))
        assert which == clip and decided, (rho, which)
        a = 2.0 * rho - 1.0; want = 3.0 * max(1.0 / 3.0, min(1.0 - a * a * a, 2.0 / 3.0))
        assert abs(want - float(v.value)) <= v.bound + 4 * U * want
        if clip != "cubic":
            assert v.bound == 0.0 and float(v.value) == want
        else:
            assert tx.err_over_bound(want * (1 + 1e-9), v) > 1.0
    _, _, decided = tx.lm_update(3.0, tx.Val(tx.mpf(0.5 * (1 + (1.0 / 3.0) ** (1.0 / 3.0))), 1e-12))
    assert not decided


# ---------------------------------------------------------------- 2. census
def vertex_kinds(S, g, tail):
    """{kind: mask over S's scalars}: base, tail, neighbour of a fixed vertex, the last workgroup of 256 vertices"""
    N, M = S.shape; sc = lambda mp_, ml_: np.concatenate([np.repeat(mp_, 3), np.repeat(ml_, 2)]) & S.free
    Nb, Mb = (tail[0], tail[1]) if tail[0] is not None else (N, M)
    out = {"base": sc(np.arange(N) < Nb, np.arange(M) < Mb)}
    if tail[0] is not None:
        out["tail"] = sc(np.arange(N) >= Nb, np.arange(M) >= Mb)
    nbp, nbl = np.zeros(N, dtype=bool), np.zeros(M, dtype=bool)
    fxp, fxl = set(int(i) for i in g["fixed_poses"]), set(int(i) for i in g["fixed_landmarks"])
    for i, j in zip(g["pp_i"], g["pp_j"]):
        if int(i) in fxp: nbp[j] = True
        if int(j) in fxp: nbp[i] = True
    for p, l in zip(g["pl_p"], g["pl_l"]):
        if int(p) in fxp: nbl[l] = True
        if int(l) in fxl: nbp[p] = True
    out["fixed neighbour"] = sc(nbp, nbl)
    v = np.arange(N + M); last = v >= 256 * ((N + M - 1) // 256)
    out["last workgroup"] = sc(last[:N], last[N:])
    return out


def covered(val):
    """the can-fail check of one Val: where 1e-9 of the value exceeds twice the bound the perturbed value must violate the bound"""
    v = float(val.value)
    if 1e-9 * abs(v) <= 2 * val.bound:
        return False
    assert tx.err_over_bound(v * (1 + 1e-9), val) > 1.0
    return True


@pytest.mark.parametrize("fam,name", GRAPHS)
def test_census(po, pkg, frontend, bench_graphs, fam, name):
    m, g, tN, tM = model_of(po, pkg, frontend, bench_graphs, fam, name)
    seen = np.zeros(len(g["lm_est"]), dtype=bool); seen[np.asarray(g["pl_l"], dtype=np.int64)] = True; seen[np.asarray(g["fixed_landmarks"], dtype=np.int64)] = True
    assert ((fam, name) in DROPPED) == (not seen.all()) and len(DROPPED) <= len(CASES) // 10      # singular by structure: the same verdict with any solver
    if (fam, name) in DROPPED:
        print("%s %s dropped: %d free landmarks without an observation edge, %s" % (fam, name, int((~seen).sum()), DROPPED[fam, name]))
        return
    S, h_gn, chi, x, _ = cpu_system(m, g)
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(h_gn))
    r0, deltas = deltas_of(S, h_gn)
    assert r0["alpha_decided"] and float(r0["sd"].value) < float(r0["gn"].value) and float(r0["gn"].value) < 1e4
    kinds = vertex_kinds(S, g, (tN, tM)); line = []
    for label, kind, delta in deltas:
        r = tx.dogleg(S, h_gn, delta, chi, 0.5 * chi)
        assert r["kind"] == kind and r["kind_decided"], (label, tx.KINDS[r["kind"]])
        classes = ["alpha", "hh", "gain"] + (["beta"] if kind == tx.DL else [])
        cov = {k: covered(r[k]) for k in classes}
        if label != "DL-edge":                                       # (beside |h_sd| the difference delta^2 - ss cancels: beta is less determined there, by design of the case)
            assert all(cov.values()), (label, cov)
        if kind != tx.GN:
            hit = (1e-9 * np.abs(r["h_f"]) > 2 * r["e_h"]) & S.free
            for i in np.flatnonzero(hit)[:: max(1, int(hit.sum()) // 8)]:
                assert abs(r["h_f"][i] * 1e-9) > r["e_h"][i]
            line.append("%s %d / %d scalars of h_dl" % (label, hit.sum(), S.nf))
            if label == "DL-mid":
                for kname, mask in kinds.items():
                    assert not mask.any() or (hit & mask).any(), (label, kname)
    # LM: scale, rho and the update from the oracle's damped step
    B = pr.strip(m.system(np.asarray(g["pose_est"], dtype=np.float64), np.asarray(g["lm_est"], dtype=np.float64))[0].linearize_blocks(), g)
    md, where = tx.max_diag(B, g)
    rl = tx.lm(h_gn, S.b, 1e-12 * md, chi, 0.5 * chi, S.free)
    assert covered(rl["scale"])
    up, which, _ = tx.lm_update(0.01 * md, tx.Val(tx.mpf(0.89), 0.89 * (2 * U + rl["scale"].bound / float(rl["scale"].value))))
    assert which == "cubic" and covered(up)
    print("%s %s: n %d |h_gn| %.4g |h_sd| %.4g max |H_jj| on %s %d; covered: %s" % (fam, name, S.nf, float(r0["gn"].value), float(r0["sd"].value), where[0], where[1], "; ".join(line)))


# ---------------------------------------------------------------- the two lambda_0 variants
VARIANT_BASE = "t1_tiles3"                                         # T = 1, 134 poses: the landmark `wide` is seen from three wave tiles, three lm_part slots


def variant(which):
    """(graph, kernels, notes) of lin_shapes' VARIANT_BASE with one vertex's information scaled.
    "fixed": the edge between the fixed pose and the fixed landmark times 1e8 — whatever a kernel sums for a fixed vertex, no free scalar changes;
    "wide": every edge of the landmark three wave tiles see gets 1e8 d d^T added, d the unit line of sight in the pose frame — the pose's
    theta-theta entry sees nothing of it (its Jacobian column is perpendicular to d) and the landmark's block collects all three edges"""
    g0, kernels, notes = ls.graph(VARIANT_BASE)
    g = {k: np.array(v, copy=True) for k, v in g0.items()}; g["pl_info"] = g["pl_info"].reshape(-1, 4)
    if which == "fixed":
        k = np.flatnonzero(np.isin(g["pl_p"], g["fixed_poses"]) & np.isin(g["pl_l"], g["fixed_landmarks"])); assert len(k) >= 1
        g["pl_info"][k] *= 1e8
    else:
        for k in np.flatnonzero(g["pl_l"] == notes["wide"]):
            x, y, th = g["pose_est"][g["pl_p"][k]]; dx, dy = g["lm_est"][notes["wide"]] - (x, y)
            d = np.array([np.cos(th) * dx + np.sin(th) * dy, -np.sin(th) * dx + np.cos(th) * dy]); d /= np.linalg.norm(d)
            g["pl_info"][k] += 1e8 * np.outer(d, d).reshape(4)
    return g, kernels, notes


def test_variants_put_the_largest_diagonal_where_they_say(po):
    g0, _, notes = ls.graph(VARIANT_BASE)
    md0, where0 = tx.max_diag(make_oracle_graph(po, g0).linearize_blocks(), g0)
    gf, _, _ = variant("fixed"); Bf = make_oracle_graph(po, gf).linearize_blocks()
    assert tx.max_diag(Bf, gf) == (md0, where0)                     # nothing free changed
    gw, _, _ = variant("wide"); mdw, where = tx.max_diag(make_oracle_graph(po, gw).linearize_blocks(), gw)
    print("largest free diagonal: base %.6g on %s %d; 'wide' %.6g on %s %d (seen from poses %s)" % ((md0,) + where0 + (mdw,) + where + (notes["wide_poses"],)))
    assert where == ("landmark", notes["wide"]) and mdw > 100 * md0 and len(notes["wide_poses"]) == 3


# ---------------------------------------------------------------- 3. the near-threshold inputs
_near = {}


def near_start(po, bench_graphs):
    """(graph, x1 poses, x1 landmarks): bench 50 / 30, oracle optimum, perturbed(NEAR_SEED, 5.0, 10.0), one oracle Gauss-Newton step"""
    if not _near:
        g = bench_graphs(50, 30)[1]
        og = make_oracle_graph(po, g); done, _, _ = og.optimize(10, ordering=1); assert done == 10
        P0, L0 = perturbed(dict(g, pose_est=og.poses(), lm_est=og.landmarks()), NEAR_SEED, 5.0, 10.0)
        o1 = make_oracle_graph(po, dict(g, pose_est=P0, lm_est=L0)); o1.optimize(1, ordering=1)
        _near["x"] = (g, o1.poses(), o1.landmarks())
    return _near["x"]


def bisect(f, lo, hi, target, window):
    """x between lo and hi with f(x) - target inside `window` (f - target changes sign between lo and hi)"""
    c = 0.5 * (window[0] + window[1]); flo = f(lo) - target - c
    assert flo * (f(hi) - target - c) < 0
    for _ in range(200):
        mid = 0.5 * (lo + hi); fm = f(mid) - target
        if window[0] < fm < window[1]:
            return mid, fm
        if (fm - c) * flo > 0:
            lo = mid
        else:
            hi = mid
    raise AssertionError("no point inside the window")


def test_near_threshold_deltas(po, bench_graphs):
    g, P1, L1 = near_start(po, bench_graphs)
    m = dr.Model(po, g); pt = dr.Point(m, P1, L1)
    rho = lambda d: dr.trial(m, pt, d)["rho"]
    t = dr.trial(m, pt, 1e4)
    assert t["kind"] == dr.GN and not t["accepted"] and t["rho"] < -0.1
    gn = float(np.linalg.norm(pt.h_gn))
    for key in NEAR_DELTA:
        target = float(key[:-1]); win = WINDOW if key[-1] == "+" else (-WINDOW[1], -WINDOW[0])
        lo, hi = (0.3 * gn, 0.6 * gn) if target == 0.75 else (0.5 * gn, 0.8 * gn)
        d, off = bisect(rho, lo, hi, target, win)
        have = rho(NEAR_DELTA[key]) - target
        print("rho %s: bisection gives initial_delta %.17g (rho - %.2f = %+.3e); recorded %.17g (%+.3e)" % (key, d, target, off, NEAR_DELTA[key], have))
        assert win[0] < have < win[1]
        assert dr.trial(m, pt, NEAR_DELTA[key])["kind"] == dr.DL


def test_near_threshold_lambdas(po, bench_graphs):
    g, P1, L1 = near_start(po, bench_graphs)
    rho = lambda lam: lm_ref.trial(po, g, P1, L1, lam)["rho"]
    lam, off = bisect(rho, 1e-3, 1e3, 0.89, (-0.02, 0.02))
    r = {k: rho(v) for k, v in NEAR_LAMBDA.items()}
    print("LM: bisection gives initial_lambda %.6g (rho %.4f); recorded: %s" % (lam, 0.89 + off, " ".join("%s %.10g rho %.5f" % (k, NEAR_LAMBDA[k], v) for k, v in r.items())))
    assert 0.86 < r["cubic"] < 0.92 and 0 < r["2/3"] < 0.84 and r["1/3"] > 0.94 and r["rejected"] < -0.1
