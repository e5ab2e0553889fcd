"""GPU tests of the two side passes, entry by entry: the prior edges (k_prior_pass) and the polar observation edges (k_polar_pose, k_polar_lm,
k_polar_edge_chi2), at every forced lane count of the linearisation they run behind and on the gather kernels.

Every case of tests/side_shapes.py (the census in test_side_exact_cpu.py proves what each one reaches) is linearised on a handle with the
forced gs_debug_options.ell_lanes, then with linearize_gather = 1, and every entry of the six arrays of gs_export_system, gs_chi2, the s and
the weight of gs_get_edge_chi2 and the values of gs_get_prior_chi2 are held to
        |got - exact| <= C(n) u S,      C(n) = 2 (L + n),      u = 2^-53
against the mpmath reference of tests/side_exact_ref.py (L: 34 / 71 for the linearisation's own terms, 20 for a prior, 38 for a polar edge,
81 with a robust weight; the count is in that module's docstring).  An entry with S = 0 — r == 0, an inactive edge, a fixed endpoint, the
H_pl row of an edge with a fixed end — must be exactly zero.  A reference with one polar term, or one prior term, off by 1e-9 must fail the
same bound.  An iteration of gs_optimize is held to the bound before and after its update; a grown plan in all of it: the export of the grown
handle (tail arenas included), per-edge s, per-prior values, chi2.

Measured on an MI355X, worst err / (u S) per case over its paths (T = 1, 2, 4, 8 and gather; priors T = 1, 8, gather); C(n) is at least 42
for an entry that holds only prior terms, 78 with a polar term, 164 with a robust polar term.  The fused and the gather path differ in
H_ll and H_pl in the second digit at most; chi2 and the per-edge values sit far below 1 because S of a quadratic form is e~^T |W| e~:
  case                    Hpp_diag   Hll_diag    Hpp_off        Hpl     b_pose       b_lm       chi2       s_pp       s_pl       w_pl prior_pose   prior_lm
  ring                        3.51       1.72       2.95       2.22       0.73       0.47       0.00       0.59       0.01       0.00          -          -
  wrap                        2.30       1.64       3.05       2.08       0.81       0.44       0.00       0.02       0.23       0.00          -          -
  near_far                    2.28       1.92       3.02       1.96       0.78       0.34       0.00       0.11       0.01       0.00          -          -
  zero                        3.16       1.81       2.97       1.96       0.68       0.45       0.00       0.01       0.00       0.00          -          -
  mixed                       2.27       1.27       2.95       1.86       0.58       0.46       0.00       0.01       0.01       0.00          -          -
  far                         3.12       0.78       3.29       2.14       0.48       0.29       0.00       0.00       0.00       0.00          -          -
  cauchy                      2.79       0.25       3.63       0.46       0.59       0.00       0.00       0.02       0.36       0.62          -          -
  huber                       2.13       0.80       3.63       1.98       0.59       0.39       0.00       0.02       0.36       0.47          -          -
  priors                      2.71       1.98       2.87       2.51       0.66       0.07       0.00       0.05       0.31       0.00       0.03       0.00
  priors_groups               2.18       2.16       2.91       2.44       0.79       0.97       0.00       0.02       0.05       0.00       0.03       0.00
  priors_far                  2.67       1.60       3.53       2.44       0.52       0.03       0.00       0.00       0.00       0.00       0.00       0.00
  launch255                   3.02       1.93       3.78       2.37       0.57       0.45       0.00       0.01       0.01       0.00       0.01       0.00
  launch257                   3.02       1.93       3.78       2.37       0.57       0.45       0.00       0.01       0.01       0.00       0.01       0.00
  wrap after update           3.03       1.69       3.58       2.46       0.56       0.28       0.00       0.01       0.24       0.00          -          -
  near_far after update       2.98       1.69       2.86       2.33       0.66       0.35       0.00       0.04       0.53       0.00          -          -
  priors after update         2.50       0.75       3.04       2.10       0.57       0.13       0.00       0.01       0.04       0.00       0.04       0.07
  grown plan                  0.59       1.02       3.01       1.65       0.36       0.27       0.00       0.01       0.00       0.00       0.00       0.00
(the `iteration` lines equal their case's: the exported system of gs_optimize(1) is the linearisation at the start).  No entry of any case
exceeded its bound; nothing under csrc/ needed a change.
"""
import numpy as np
import pytest

import lin_exact_ref as lx
import polar_ref as plr
import prior_ref as pr
import side_exact_ref as sx
import side_shapes as ss
from tail_exact_ref import perturbed_fails

pytestmark = pytest.mark.gpu
NEAR = [n for n in ss.POLAR + ss.PRIOR if n not in ("far", "cauchy", "huber", "priors_far")]


def fresh(pkg, name, path):
    G = pkg.Graph(device=0, **ss.handle_kw(name, path))
    return ss.load(G, name)


def sides_of(c):
    """the passes whose terms a case's reference must hold"""
    return [side for side, n in (("polar", len(c["polar"]["idx"])), ("prior", len(c["pri"]["pose"]) + len(c["pri"]["lm"]))) if n]


def hold(G, X, tag, sides, two_sided="near", system=True):
    """the handle's last linearisation, its chi2, per-edge s and weight and per-prior values against the reference X, both ways.
    two_sided: where a term of each of `sides` off by 1e-9 must show — "near": in every array that pass writes; "H": in H_pp, H_ll and H_pl
    (a robust weight leaves b less determined); "some": in H_pp (kilometre coordinates, or estimates an update chose: see
    test_side_exact_cpu.py).  system = False: chi2 and the per-edge values alone."""
    blocks = G.export_system() if system else None
    s_pl, w_pl = G.edge_chi2("observation")
    chi2 = G.chi2(); s_pp = G.edge_chi2("odometry")[0]
    pri = (G.prior_chi2("pose"), G.prior_chi2("landmark")) if G.n_pose_priors + G.n_landmark_priors else (np.zeros(0), np.zeros(0))
    worst = lx.check(X, blocks, chi2, s_pp, s_pl, tag=tag)
    worst.update(sx.check_side(X, w_pl, pri[0], pri[1], tag=tag))
    out = "%-30s err / (u S): %s" % (tag, " ".join("%s %.2f" % kv for kv in worst.items()))
    for side in sides if system else ():
        moved = lx.check_can_fail(X, blocks, chi2, tag=tag, side=side)
        arrays = ("Hpp_diag", "Hll_diag", "b_pose", "b_lm") + (("Hpl",) if side == "polar" else ())
        assert set(arrays) <= set(moved), (tag, side, "the reference holds no term of this pass in", set(arrays) - set(moved))
        out += " | %s perturbed: %s" % (side, " ".join("%s %s" % (k, "-" if v is None else "%.3g%s" % (v[1], "*" if v[3] else "")) for k, v in moved.items()))
        need = arrays if two_sided == "near" else [k for k in arrays if k[0] == "H"] if two_sided == "H" else ("Hpp_diag",)
        assert all(moved[k] is not None for k in need), (tag, side, moved)
    print(out)
    return worst


def two_sided_of(name):
    return "near" if name in NEAR else "H" if name in ("cauchy", "huber") + ss.LAUNCH else "some"


@pytest.mark.parametrize("name,path", ss.RUNS)
def test_side_passes_entry_by_entry(pkg, name, path):
    G = fresh(pkg, name, path)
    G.initialize_optimization(); G.linearize()
    hold(G, ss.reference(name), "%s %s" % (name, "gather" if path == "gather" else "T=%d" % path), sides_of(ss.case(name)), two_sided_of(name))
    G.close()


@pytest.mark.parametrize("name,path", [("wrap", 2), ("near_far", 4), ("priors", 1)])
def test_an_iteration_runs_the_side_passes_before_and_after_its_update(pkg, name, path):
    """gs_optimize(1): the exported system is that iteration's and meets the bound at the estimates before the update; gs_linearize afterwards
    meets it at the new ones"""
    c = ss.case(name); g = c["g"]
    G = fresh(pkg, name, path)
    done, st = G.optimize(1)
    assert done == 1 and st.numeric_failure == 0
    X = ss.reference(name)
    worst = lx.check(X, G.export_system(), tag=name + " iteration")
    print("%-30s err / (u S): %s" % (name + " iteration", " ".join("%s %.2f" % kv for kv in worst.items())))
    poses, lms = G.poses(), G.landmarks()
    assert max(np.abs(poses - g["pose_est"]).max(), np.abs(lms - g["lm_est"]).max()) > 1e-3
    G.linearize()
    hold(G, sx.exact(g, c["polar"], c["pri"], c["kernels"], c["off"], poses, lms), name + " after update", sides_of(c), "some")
    G.close()


def test_a_grown_plan_keeps_the_per_edge_values_and_chi2(pkg):
    """a plan grown by three keyframes with the ring and the wrap geometry on tail vertices: the six arrays of the grown handle's export
    (polar blocks in place of tail edges' blocks in t_Hpl, priors on tail vertices), per-edge s, gs_get_prior_chi2 and gs_chi2 meet the bound;
    gs_chi2 (inside hold) changes nothing of the system: the export behind it is bit for bit the one before"""
    base, tail, full, pol, pri = ss.growth_case()
    Eb, Nb, Mb = len(base["pl_p"]), len(base["pose_est"]), len(base["lm_est"])
    G = pkg.Graph(device=0); plr.load(G, base, plr.subset(pol, pol["idx"] < Eb)); G.initialize_optimization()
    G.add_poses(np.arange(Nb, Nb + len(tail["pose_est"])), tail["pose_est"]); G.add_landmarks(Mb + np.arange(len(tail["lm_est"])), tail["lm_est"])
    G.add_odometry_edges(tail["pp_i"], tail["pp_j"], tail["pp_z"], tail["pp_info"])
    plr.add_edges(G, full, pol, first=Eb); pr.add_to(G, pri)
    G.initialize_optimization()
    assert G.plan_growths() > 0, G.growth_refusal()
    pp, ll = full["pl_p"][pol["idx"]], full["pl_l"][pol["idx"]]
    assert ((pp >= Nb) & (ll < Mb)).any() and ((pp >= Nb) & (ll >= Mb)).any() and any(p >= Nb for p, _, _, _ in pri["pose"]) and any(l >= Mb for l, _, _ in pri["lm"])
    G.linearize()
    X = sx.exact(full, pol, pri)
    hold(G, X, "grown plan", ["polar", "prior"], two_sided="H")
    tail_polar = pol["idx"][pol["idx"] >= Eb]
    assert len(tail_polar) and X.n["Hpl"].reshape(-1, 6)[tail_polar].any(), "polar blocks on tail edges"
    # ... and with the perturbed term on the TAIL: a polar term of a tail edge must show in every array that pass writes, at a tail pose, a
    # tail cone and a tail edge's own block (the tail arenas); a prior term on a tail pose in H_pp.  (The priors on tail cones carry 0.02 of an
    # edge's information and the residuals of a prior are small: 1e-9 of those terms is below 2 C u S in H_ll and in b, which the reference alone
    # decides — perturbed_fails returns None there, and that is not asserted either way.)
    S = G.export_system(); N, M, E = len(full["pose_est"]), len(full["lm_est"]), len(full["pl_p"])
    rows = dict(Hpp_diag=range(Nb, N), b_pose=range(Nb, N), Hll_diag=range(Mb, M), b_lm=range(Mb, M), Hpl=range(Eb, E))
    shown = {}
    for side, arrays in (("polar", ("Hpp_diag", "Hll_diag", "Hpl", "b_pose", "b_lm")), ("prior", ("Hpp_diag",))):
        for arr in arrays:
            w = lx.WIDTH[arr]
            tagged = lambda r, j: any(j < len(X.tags[arr].get(r * w + q, ())) and X.tags[arr][r * w + q][j] == side for q in range(w))
            shown[side, arr] = perturbed_fails(X, S, arr, rows[arr], tagged, "grown plan, tail")
            assert shown[side, arr] is not None, (side, arr, "1e-9 of a tail term of this pass can show nowhere")
    print("grown plan, a tail term off by 1e-9: " + " ".join("%s %s %.3g" % (k[0], k[1], v[1]) for k, v in shown.items()))
    before = G.export_system(); G.chi2(); after = G.export_system()
    assert all(np.array_equal(before[k], after[k]) for k in lx.ARRAYS)
    assert G.plan_growths() > 0 and G.growth_refusal() == ""
    G.close()


@pytest.mark.parametrize("path", [1, 8, "gather"])
def test_without_polar_edges_and_priors_the_system_keeps_its_bits(pkg, path):
    """the carriers alone (what the graph is with every polar edge and prior removed): a handle that had priors and dropped them, and was
    given empty polar calls, exports the bits of a handle that never saw either.  Neither handle launches a side pass, so this shows
    that gs_clear_priors and empty polar calls leave no residue in the tables, the plan or the launches; it is a stand-in for a comparison
    with an earlier build's bits, which a test cannot hold"""
    c = ss.case("mixed"); gc = plr.carriers(c["g"], c["polar"])
    kw = ss.handle_kw("mixed", path)
    A = pkg.Graph(device=0, **kw); A.load_bench_graph(gc)
    B = pkg.Graph(device=0, **kw); B.load_bench_graph(gc)
    pr.add_to(B, ss.case("priors")["pri"]); B.clear_priors()
    B.add_range_bearing_edges([], [], np.zeros((0, 2)), np.zeros((0, 4))); B.add_bearing_edges([], [], np.zeros(0), np.zeros(0))
    out = []
    for H in (A, B):
        H.initialize_optimization(); H.linearize(); out.append((H.export_system(), H.chi2()))
    assert all(np.array_equal(out[0][0][k], out[1][0][k]) for k in lx.ARRAYS) and out[0][1] == out[1][1]
    assert B.num_polar_edges() == 0 and B.n_pose_priors == 0
    A.close(); B.close()


@pytest.mark.parametrize("path", [1, 8, "gather"])
def test_a_polar_edge_switched_off_and_on_restores_every_bit(pkg, path):
    c = ss.case("mixed"); m = c["notes"]["mixed"]
    G = fresh(pkg, "mixed", path)
    G.initialize_optimization(); G.linearize(); S0 = G.export_system(); chi0 = G.chi2()
    for k in (m["full"], m["pair"][1]):
        G.set_edge_active("observation", int(k), False)
    G.linearize(); S1 = G.export_system()
    assert not np.array_equal(S1["Hpp_diag"], S0["Hpp_diag"]) and not S1["Hpl"][m["full"]].any() and S0["Hpl"][m["full"]].all()
    for k in (m["full"], m["pair"][1]):
        G.set_edge_active("observation", int(k), True)
    G.linearize(); S2 = G.export_system()
    assert all(np.array_equal(S2[k], S0[k]) for k in lx.ARRAYS) and G.chi2() == chi0
    assert not G.edges_active("observation")[m["inactive"]]
    G.close()
