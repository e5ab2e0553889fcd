"""The side-pass cases, their exact reference and their bound, checked without a GPU.

  census        every case of tests/side_shapes.py reaches what it names — both wrap branches, the axis points with both signs of zero, the
                ranges, r == 0 exactly — evaluated in numpy in the device's operation order and from the reference's unwrapped angles; the
                host-only plan has the forced T and the R the case counts on; the listed vertices lie on each side of 256;
  soundness     plain fp64 evaluations stay inside C(n) u S of tests/side_exact_ref.py on every entry of every case: the CPU oracle on the
                carriers plus polar_ref.contributions / prior_ref.contributions, polar_ref.edge_s, prior_ref.chi2_each, and the CPU oracle
                on the cartesianised, augmented graph (with the one magnitude that route adds:
                side_exact_ref.exact(cartesian_route)); r, beta and J_d in the device's operation order land within their counted share;
  two-sided     a reference with one polar term, or one prior term, off by 1e-9 does not pass;
  planted bugs  three defects the norm-wise tolerance of test_gpu_polar.py (1e-11 of the array's largest entry) passes on `near_far` and
                the bound refuses.
"""
import numpy as np
import pytest

from conftest import make_oracle_graph
import lin_exact_ref as lx
import polar_ref as plr
import prior_ref as pr
import robust_ref as rr
import side_exact_ref as sx
import side_shapes as ss
from plan_exec import Plan
from test_lin_exact_cpu import tile_groups

ALL = list(ss.CASES)
PLAIN_NEAR = [n for n in ss.POLAR + ss.PRIOR if n not in ("far", "cauchy", "huber", "priors_far")]


def parts(c):
    g = c["g"]
    return g, c["polar"], c["pri"], c["kernels"], c["off"], g["pose_est"], g["lm_est"]


def polar_terms(g, pol, P, L, bug=None):
    """polar_ref.terms, or the same with a planted defect: bug = (kind, polar-set positions)"""
    t = plr.terms(g, pol, P, L)
    if bug is None:
        return t
    kind, where = bug
    Jd = t["Jd"].copy(); e = t["e"].copy(); d = t["d"]
    for n in where:
        r2 = d[n, 0] ** 2 + d[n, 1] ** 2
        if kind == "sign":
            Jd[n, 1, 0] = -Jd[n, 1, 0]
        elif kind == "one_over_r":
            Jd[n, 1, 0] = -d[n, 1] / np.sqrt(r2)
        elif kind == "no_wrap":
            e[n, 1] = np.arctan2(d[n, 1], d[n, 0]) - pol["z"][n, 1]
    th = np.asarray(P)[np.asarray(g["pl_p"])[pol["idx"]], 2]; c, s = np.cos(th), np.sin(th)
    Rt = np.stack([np.stack([c, s], 1), np.stack([-s, c], 1)], 1)
    B = np.einsum("nij,njk->nik", Jd, Rt)
    A = np.concatenate([-B, np.stack([np.zeros(len(d)), np.where(t["ok"], -1.0, 0.0)], 1)[:, :, None]], axis=2)
    return dict(t, e=e, A=A, B=B, Jd=Jd, s=np.einsum("ni,nij,nj->n", e, pol["W"], e))


def polar_contributions(g, pol, P, L, kernels, off, bug=None):
    """polar_ref.contributions and polar_ref.edge_s over polar_terms (the same sums, in the same order), so that a defect can be planted"""
    kernel = (kernels or {}).get("observation", rr.NONE)
    t = polar_terms(g, pol, P, L, bug)
    N, M, Epl = len(P), len(L), len(g["pl_p"])
    fp = np.zeros(N, dtype=bool); fp[np.asarray(g["fixed_poses"], dtype=np.int64)] = True
    fl = np.zeros(M, dtype=bool); fl[np.asarray(g["fixed_landmarks"], dtype=np.int64)] = True
    out = dict(Hpp_diag=np.zeros((N, 9)), Hll_diag=np.zeros((M, 4)), Hpl=np.zeros((Epl, 6)), b_pose=np.zeros((N, 3)), b_lm=np.zeros((M, 2)), chi2=0.0)
    w = rr.weight(kernel, t["s"]); rho = rr.rho(kernel, t["s"]); off = set(int(k) for k in off)
    for n, k in enumerate(pol["idx"]):
        if not t["ok"][n] or int(k) in off:
            continue
        p, l = int(g["pl_p"][k]), int(g["pl_l"][k]); A, B, W, e = t["A"][n], t["B"][n], w[n] * pol["W"][n], t["e"][n]
        if not (fp[p] and fl[l]): out["chi2"] += float(rho[n])
        if not fp[p]: out["Hpp_diag"][p] += (A.T @ W @ A).reshape(9); out["b_pose"][p] -= A.T @ W @ e
        if not fl[l]: out["Hll_diag"][l] += (B.T @ W @ B).reshape(4); out["b_lm"][l] -= B.T @ W @ e
        if not fp[p] and not fl[l]: out["Hpl"][k] = (A.T @ W @ B).reshape(6)
    s = rr.edge_s(g, P, L)[1].copy(); s[pol["idx"]] = t["s"]
    return out, s


def numpy_side(po, c, bug=None):
    """a plain fp64 evaluation of everything the reference describes: (blocks, chi2, s_pl, w_pl, prior s of both kinds)"""
    g, pol, pri, kernels, off, P, L = parts(c)
    gc = plr.carriers(g, pol)
    og = make_oracle_graph(po, rr.reweighted(gc, P, L, kernels) if kernels else gc)
    blocks = {k: np.array(v, dtype=np.float64, copy=True) for k, v in og.linearize_blocks().items()}
    chi2 = rr.robust_chi2(gc, P, L, kernels) if kernels else og.chi2()
    add, s_pl = polar_contributions(g, pol, P, L, kernels, off, bug)
    for k in ("Hpp_diag", "Hll_diag", "Hpl", "b_pose", "b_lm"):
        blocks[k] = blocks[k].reshape(add[k].shape) + add[k]
    Hp, bp, Hl, bl, chi_p = pr.contributions(g, pri, P, L)
    blocks["Hpp_diag"] += Hp; blocks["b_pose"] += bp; blocks["Hll_diag"] += Hl; blocks["b_lm"] += bl
    w = rr.weight((kernels or {}).get("observation", rr.NONE), s_pl); w[list(off)] = 0.0
    return blocks, chi2 + add["chi2"] + chi_p, s_pl, w, pr.chi2_each(pri, P, L)


def oracle_side(po, c):
    """the CPU oracle on the cartesianised graph, augmented by the prior edges"""
    g, pol, pri, kernels, off, P, L = parts(c)
    gc = plr.cartesianised(g, pol, P, L, off)
    gw = rr.reweighted(gc, P, L, kernels) if kernels else gc
    og = make_oracle_graph(po, pr.augment(gw, pri))
    chi2 = rr.robust_chi2(gc, P, L, kernels) + sum(map(np.sum, pr.chi2_each(pri, P, L))) if kernels else og.chi2()
    return pr.strip(og.linearize_blocks(), g), chi2


def line(tag, worst):
    print("%-26s err / (u S): %s" % (tag, " ".join("%s %.2f" % kv for kv in worst.items())))


# ---------------------------------------------------------------- census
@pytest.mark.parametrize("name,path", [r for r in ss.RUNS if r[1] != "gather"])
def test_census_of_the_plan(pkg, name, path):
    c = ss.case(name); g = c["g"]
    G = pkg.Graph(device=-2, debug=dict(ell_lanes=int(path))); ss.load(G, name); G.plan_build_host()
    P = Plan(G.plan_export())
    assert G.num_polar_edges() == len(c["polar"]["idx"]) and G.n_pose_priors == len(c["pri"]["pose"]) and G.n_landmark_priors == len(c["pri"]["lm"])
    G.close()
    kmax = int(np.bincount(g["pl_p"]).max()); T = int(path) or 8
    assert (P.ell_T, P.ell_R) == (T, -(-kmax // T))
    assert kmax == dict(ring=25, near_far=6, priors_groups=4, wrap=4).get(name, 3)
    fused = P.ell_R <= ss.ls.LIN_R
    assert fused == (not (name == "ring" and T < 8 or name == "near_far" and T == 1)), "which lane counts run the fused kernel"
    if name in ss.PRIOR:
        ng = tile_groups(P, g, len(g["pose_est"]))
        F = int(g["fixed_landmarks"][0]); PW = 64 // T
        big = int(np.argmax(ng)) if name == "priors_groups" else 0               # (T = 1: the first tile, 64 poses; T = 8: a tile of 8 poses with 32)
        in_tile = set(int(l) for l in g["pl_l"][g["pl_p"] // PW == big])
        assert any(l != F and l in in_tile for l, _, _ in c["pri"]["lm"]), "a landmark prior on a landmark of that tile"
        assert ng[big] > 25 if name == "priors_groups" else max(ng) <= 12, ng


def test_census_ring():
    c = ss.case("ring"); g = c["g"]; nt = c["notes"]
    assert tuple(g["pose_est"][nt["ring_pose"]]) == (2.0, 0.0, 0.0) and np.signbit(g["pose_est"][nt["ring_pose"], 2])
    d = np.array([ss.device_d(*g["pose_est"][nt["ring_pose"]], *g["lm_est"][l]) for l in nt["ring_lms"]])
    dx, dy = d[:, 0], d[:, 1]
    assert ((dy == 0) & (dx > 0)).any() and ((dx == 0) & (dy > 0)).any() and ((dx == 0) & (dy < 0)).any()
    neg = (dy == 0) & (dx < 0)
    assert (neg & np.signbit(dy)).sum() == 1 and (neg & ~np.signbit(dy)).sum() == 1, "the negative x-axis with dy = -0 and dy = +0"
    beta = np.arctan2(dy, dx)
    assert (beta == np.pi).any() and (beta == -np.pi).any()
    assert np.all(np.abs(np.hypot(dx, dy)[:24] - 3.0) < 0.2) and np.allclose(np.sort(np.rad2deg(beta[:24]) % 360), np.arange(24) * 15.0, atol=4.0)
    assert sum(float(v).is_integer() for v in d[:24].reshape(-1)) >= 16, "integer offsets where the angle allows"
    assert abs(g["pose_est"][nt["second_pose"], 2]) > 0.5
    X = ss.reference("ring"); at = {int(k): n for n, k in enumerate(c["polar"]["idx"])}
    assert sum(X.polar[at[e]]["geo"]["on_negative_axis"] for e in nt["ring_edges"]) == 2


def test_census_wrap():
    c = ss.case("wrap"); g = c["g"]; pol = c["polar"]; X = ss.reference("wrap")
    at = {int(k): n for n, k in enumerate(pol["idx"])}
    a = np.array([float(X.polar[at[e]]["unwrapped"]) for e in c["notes"]["wrap_edges"]])
    for want in (6.0, -6.0, np.pi - 1e-5, -(np.pi - 1e-5), np.pi + 1e-5, -(np.pi + 1e-5), 0.0, 2 * np.pi):
        assert (np.abs(a - want) < 1e-9).any(), want
    assert ((a > np.pi) & (a < 2 * np.pi)).sum() >= 2 and ((a < -np.pi) & (a > -2 * np.pi)).sum() >= 2
    # the device's own expression, in numpy: both branches of normalize_theta (gs_edge_dev.hpp) are taken, and the 2 pi edge gives exactly 0
    t = plr.terms(g, pol, g["pose_est"], g["lm_est"])
    raw = np.arctan2(t["d"][:, 1], t["d"][:, 0]) - pol["z"][:, 1]
    mine = np.array([at[e] for e in c["notes"]["wrap_edges"]])
    assert (raw[mine] >= np.pi).sum() >= 3 and (raw[mine] < -np.pi).sum() >= 2
    assert raw[mine[-1]] == 2 * np.pi and t["e"][mine[-1], 1] == 0.0 and pol["model"][mine[-1]] == ss.BO
    assert raw[mine[6]] == 0.0


def test_census_near_far_zero_mixed():
    c = ss.case("near_far"); X = ss.reference("near_far"); nt = c["notes"]
    at = {int(k): n for n, k in enumerate(c["polar"]["idx"])}
    r = np.array([float(X.polar[at[e]]["geo"]["r"]) for e in nt["nf_edges"]])
    assert np.allclose(r, ss.RANGES + ss.RANGES, rtol=1e-9)
    assert np.all(c["g"]["pl_p"][nt["nf_edges"][:5]] == nt["nf_pose"]) and np.all(c["g"]["pl_l"][nt["nf_edges"][5:]] == nt["nf_cone"])
    J = np.array([[abs(float(v)) for row in X.polar[at[e]]["geo"]["Jd"] for v in row] for e in nt["nf_edges"]])
    assert J.max() / J[J > 0].min() >= 1e10, J.max() / J[J > 0].min()
    assert X.polar[at[nt["nf_weak"]]]["wrapped"]
    c = ss.case("zero"); X = ss.reference("zero"); nt = c["notes"]; g = c["g"]
    at = {int(k): n for n, k in enumerate(c["polar"]["idx"])}
    d = ss.device_d(*g["pose_est"][nt["zero_pose"]], *g["lm_est"][nt["zero_lm"]])
    assert d == (0.0, 0.0) and X.polar[at[nt["zero_edge"]]] is None
    assert not X.S["Hpl"].reshape(-1, 6)[nt["zero_edge"]].any() and X.S_s_pl[nt["zero_edge"]] == 0 and X.s_pl[nt["zero_edge"]] == 0
    assert all(X.S["Hpl"].reshape(-1, 6)[e].all() and X.s_pl[e] > 0 for e in nt["zero_others"])
    c = ss.case("mixed"); X = ss.reference("mixed"); m = c["notes"]["mixed"]; g = c["g"]
    tags = lambda e: X.tags["Hpl"].get(6 * e, [])
    assert tags(m["full"]) == [None, "polar"] and tags(m["bearing"]) == [None, "polar"] and tags(m["pair"][0]) == [None, "polar"] and tags(m["pair"][2]) == [None]
    for e in (m["fixed_pose"], m["fixed_lm"], m["both_fixed"], m["inactive"]):
        assert tags(e) == ([None] if e == m["inactive"] else []) and not X.S["Hpl"].reshape(-1, 6)[e].any() and X.s_pl[e] > 0
    assert g["pl_p"][m["both_fixed"]] == 0 and g["pl_l"][m["both_fixed"]] == g["fixed_landmarks"][0] and c["off"] == [m["inactive"]]
    assert X.w_pl[m["inactive"]] == 0 and len(set(zip(g["pl_p"][m["pair"]], g["pl_l"][m["pair"]]))) == 1
    la = int(g["pl_l"][m["full"]])                        # seen from the free pose 8 (counted), the fixed pose 0 (counted), pose 16 (inactive)
    assert X.tags["Hll_diag"][4 * la].count("polar") == 2
    W = c["polar"]["W"][[int(np.flatnonzero(c["polar"]["idx"] == m["full"])[0])]][0]
    assert W[0, 1] != 0 and np.linalg.eigvalsh(W).min() > 0


def test_census_far_robust_priors_launch():
    assert np.abs(ss.case("far")["g"]["pose_est"][:, :2]).min() > 2.9e4 and np.abs(ss.case("priors_far")["g"]["lm_est"]).min() > 2.9e4
    for name in ("cauchy", "huber"):
        c = ss.case(name); X = ss.reference(name); kname, delta = c["kernels"]["observation"]
        s = np.array([float(X.s_pl[k]) for k in c["polar"]["idx"]])
        assert kname == name and (s > delta ** 2).sum() >= 5 and (s < delta ** 2).sum() >= 5, "polar edges on both sides of delta^2"
        assert X.robust and X.L["Hpl"].max() == sx.L_POLAR_ROBUST
    c = ss.case("priors"); X = ss.reference("priors"); nt = c["notes"]; g = c["g"]
    un = {int(p): float(t["unwrapped"]) for (p, _, _, _), t in zip(c["pri"]["pose"], X.priors["pose"])}
    assert un[nt["wrap_priors"][0]] > np.pi and un[nt["wrap_priors"][1]] < -np.pi
    turned = [t for (p, _, _, _), t in zip(c["pri"]["pose"], X.priors["pose"]) if p == nt["turned_pose"]][0]
    assert g["pose_est"][nt["turned_pose"], 2] > np.pi and turned["wraps"] == 1 and abs(float(turned["e"][2])) < 0.1
    poses = [p for p, _, _, _ in c["pri"]["pose"]]; lms = [l for l, _, _ in c["pri"]["lm"]]
    assert poses.count(14) == 3 and any(x for p, _, _, x in c["pri"]["pose"] if p == 14) and 0 in poses and int(g["fixed_landmarks"][0]) in lms
    assert max(lms.count(l) for l in lms) == 2 and any(x for _, _, _, x in c["pri"]["pose"])
    ev = [np.linalg.eigvalsh(W) for _, _, W, x in c["pri"]["pose"] if not x]
    assert max(e.max() / e.min() for e in ev) > 1e5, "a full 3 x 3 Omega with weak and strong directions"
    assert not X.n["Hpp_diag"].reshape(-1, 9)[0].any(), "the prior on the fixed pose stays out"
    for name, count in (("launch255", 255), ("launch257", 257)):
        c = ss.case(name); g = c["g"]; F = int(g["fixed_landmarks"][0])
        n_pv = len(set(int(p) for p in g["pl_p"][c["polar"]["idx"]]) - {0})
        n_pri = len({p for p, _, _, _ in c["pri"]["pose"]} - {0}) + len({l for l, _, _ in c["pri"]["lm"]} - {F})
        assert n_pv == count and n_pri == count
    assert len(ss.case("launch255")["g"]["pl_p"]) == len(ss.case("launch257")["g"]["pl_p"])


# ---------------------------------------------------------------- soundness
@pytest.mark.parametrize("name", ALL)
def test_plain_fp64_evaluations_stay_inside_the_bound(po, name):
    c = ss.case(name); X = ss.reference(name)
    blocks, chi2, s_pl, w, (s_pose, s_lm) = numpy_side(po, c)
    s_pp = rr.edge_s(c["g"], c["g"]["pose_est"], c["g"]["lm_est"])[0]
    worst = lx.check(X, blocks, chi2, s_pp, s_pl, tag=name + " numpy")
    worst.update(sx.check_side(X, w, s_pose, s_lm, tag=name + " numpy"))
    line(name + " numpy", worst)
    ob, ochi = oracle_side(po, c)
    line(name + " oracle", lx.check(ss.reference(name, cartesian_route=True), ob, ochi, tag=name + " oracle"))


def test_r_beta_and_jd_in_the_device_order_land_within_their_share():
    """numpy, the device's operation order: the worst err / (u S) of r, beta and the four J_d entries over ranges 1e-3 .. 25 m, at the origin
    and at the 4e4 offset, lands at 0.6 .. 1.3 — S is no idle factor, and a plain evaluation uses a tenth of the counted L (r 10, beta 13,
    J_d 11).  The worst of 405 ranges per offset: 0.67 .. 1.04 at the origin, 0.75 .. 0.99 at the offset; the worst of a sample grows with
    its size (60 ranges: 0.51 for dx / r, below the window; 1500: up to 1.23)"""
    rng = np.random.default_rng(5)
    for off in ((0.0, 0.0), ss.ls.FAR):
        worst = np.zeros(6)
        for r in np.concatenate([[1e-3, 1e-2, 0.1, 1.0, 25.0], 10 ** rng.uniform(-3, 1.39, 400)]):
            th, b = rng.uniform(-3, 3, 2); px, py = off[0] + rng.uniform(-5, 5), off[1] + rng.uniform(-5, 5)
            lx_, ly_ = px + r * np.cos(th + b), py + r * np.sin(th + b)
            dx, dy = ss.device_d(px, py, th, lx_, ly_); r2 = dx * dx + dy * dy; rr_ = np.sqrt(r2)
            got = [rr_, np.arctan2(dy, dx), dx / rr_, dy / rr_, -dy / r2, dx / r2]
            if 7 * lx.U * 4 * max(abs(px), abs(py), 1) / rr_ > 1e-3:
                continue                                       # (the reference refuses: d is not determined against r)
            geo = sx.polar_geometry([lx.mpf(float(v)) for v in (px, py, th)], [lx.mpf(float(lx_)), lx.mpf(float(ly_))])
            ex = [geo["r"], geo["beta"]] + [v for row in geo["Jd"] for v in row]; S = [geo["S_r"], geo["S_beta"]] + [v for row in geo["S_Jd"] for v in row]
            worst = np.maximum(worst, [float(abs(lx.mpf(float(a)) - e) / (lx.U * s)) for a, e, s in zip(got, ex, S)])
        print("offset %s: worst err / (u S) of r, beta, J_d: %s" % (off, np.round(worst, 2)))
        assert np.all(worst <= 1.3) and np.all(worst >= 0.6), worst


# ---------------------------------------------------------------- two-sided
@pytest.mark.parametrize("name", ss.POLAR + ss.PRIOR)
def test_a_side_term_off_by_1e_9_breaks_the_bound(po, name):
    c = ss.case(name); X = ss.reference(name)
    blocks, chi2, _, _, _ = numpy_side(po, c)
    near = name in PLAIN_NEAR
    for side, arrays in (("polar", ("Hpl", "Hll_diag", "Hpp_diag", "b_pose", "b_lm")), ("prior", ("Hll_diag", "Hpp_diag", "b_pose", "b_lm"))):
        if side == "prior" and name not in ss.PRIOR:
            continue
        moved = lx.check_can_fail(X, blocks, chi2, tag=name, side=side)
        print("%-14s %-5s perturbed: %s" % (name, side, " ".join("%s %s" % (k, "-" if v is None else "%.3g%s" % (v[1], "*" if v[3] else "")) for k, v in moved.items())))
        assert "Hpp_off" not in moved
        # at kilometre coordinates d~ / r is 1e4 .. 1e5, so 2 C u S of a polar term is 1e-9 of it and more almost everywhere, and a robust
        # weight leaves b less determined than 1e-9 (lin_exact_ref.assert_two_sided): there the perturbation must show in H_pp and H_pl
        for k in arrays[:3] if near or name in ("cauchy", "huber") else ("Hpp_diag",) + (("Hpl",) if side == "polar" else ()):
            assert moved[k] is not None, (name, side, k)
        if near:
            assert all(moved[k] is not None for k in arrays), (name, side, moved)


def test_a_wrong_reference_fails_as_a_whole():
    """the perturbation inside the reference itself (side_exact_ref.exact(perturb=...)): one polar edge, one pose prior, one landmark prior"""
    c = ss.case("priors"); g, pol, pri, kernels, off, P, L = parts(c)
    X = ss.reference("priors"); blocks = {k: np.array([float(v) for v in X.val[k]]) for k in lx.ARRAYS}
    lx.check(X, blocks, float(X.chi2), tag="the rounded reference")
    for what in (("polar", 5), ("pose prior", 2), ("landmark prior", 1)):
        Xp = sx.exact(g, pol, pri, kernels, off, perturb=(what, 1e-9))
        with pytest.raises(AssertionError):
            lx.check(Xp, blocks, tag=str(what))


# ---------------------------------------------------------------- bugs the norm-wise tolerance passes
def old_bar(po, c, blocks, chi2, s_pl):
    """test_gpu_polar.py's bars against the oracle on the cartesianised graph: 1e-11 of each array's largest entry, chi2 1e-9, s 1e-11"""
    g, pol, pri, kernels, off, P, L = parts(c)
    ref = plr.oracle_at(po, g, pol, P, L).linearize_blocks(); chi_o = plr.chi2_at(po, g, pol, P, L); s_ref = plr.edge_s(g, pol, P, L)
    rel = lambda a, b: float(np.abs(np.asarray(a).reshape(-1) - np.asarray(b).reshape(-1)).max() / np.abs(b).max())
    figs = {k: rel(blocks[k], ref[k]) for k in ref}
    return all(v < 1e-11 for v in figs.values()) and abs(chi2 - chi_o) <= 1e-9 * chi_o and rel(s_pl, s_ref) < 1e-11, figs


@pytest.mark.parametrize("kind", ["sign", "no_wrap", "one_over_r"])
def test_planted_bugs_pass_the_old_tolerance_and_fail_the_bound(po, kind):
    """a J_d entry with the wrong sign on the 20 m edges only; a skipped wrap; 1 / r in place of 1 / r^2 at one edge (the last two on the
    wrapped 20 m edge of weight 1e-10)"""
    c = ss.case("near_far"); X = ss.reference("near_far"); nt = c["notes"]
    at = {int(k): n for n, k in enumerate(c["polar"]["idx"])}
    where = [at[e] for e in nt["nf_20m"]] if kind == "sign" else [at[nt["nf_weak"]]]
    good = numpy_side(po, c)
    assert old_bar(po, c, good[0], good[1], good[2])[0]
    lx.check(X, good[0], good[1], None, good[2], tag="near_far")
    blocks, chi2, s_pl, _, _ = numpy_side(po, c, bug=(kind, where))
    assert any(not np.array_equal(blocks[k], good[0][k]) for k in blocks)
    ok, figs = old_bar(po, c, blocks, chi2, s_pl)
    print("%s: the old bar sees %s" % (kind, " ".join("%s %.1e" % kv for kv in figs.items())))
    assert ok, figs
    with pytest.raises(AssertionError):
        lx.check(X, blocks, chi2, None, s_pl, tag="near_far with " + kind)
