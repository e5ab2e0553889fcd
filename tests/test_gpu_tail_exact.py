"""GPU tests of a GROWN plan's linearisation, entry by entry: k_linearize_tail, the tail arenas, and the two read-modify-write paths from the
tail into base storage (an old cone's first partial-sum slot, an old pose's H_pp / b), through gs_export_system on the grown handle.

Every case of tests/tail_shapes.py (the census in test_tail_exact_cpu.py proves what each one reaches) is built as a base, grown by its
keyframes, linearised, and every entry of the six exported arrays, gs_chi2 and the per-edge s of gs_get_edge_chi2 are held to
        |got - exact| <= C(n) u S,      C(n) = 2 (34 + n), with a robust kernel 2 (71 + n),      u = 2^-53
against the mpmath linearisation of the FULL graph (tests/lin_exact_ref.py; n counts every edge, base and tail, summed into the entry;
S = 0: exactly zero).  The reference must fail the same bound with one term off by 1e-9 (lin_exact_ref.check_can_fail / assert_two_sided)
and with one TAIL edge's term off by 1e-9 in every array the tail writes or adds to — a tail edge's own H_pl / H_pp_off block, the diagonal
block and rhs of a tail pose and a tail cone, and those of the old poses and the old cone that receive tail shares by read-modify-write
(tail_exact_ref.check_can_fail_in_the_tail).  A second gs_linearize must export the same bits (the += into lm_part and Hpp_diag does not
accumulate); gs_chi2 alone on a fresh grown handle (launch_chi2_only's grown branch: the gather kernel and k_chi2_tail) meets the bound and
changes nothing of the system; an iteration of gs_optimize is held before and after its update; inactive tail edges leave exact zeros; gs_multiply_hessian agrees with the exported columns.

Measured worst err / (u S) per case and array on an MI355X, beside the CPU oracle's on the same graphs: profiles/tail_exact_gpu_suite.txt
and profiles/tail_exact_cpu_census.txt (the table below is taken from them).
  case                           Hpp_diag Hll_diag  Hpp_off      Hpl   b_pose     b_lm     chi2     s_pp     s_pl
  tail_min                           3.45     2.07     3.85     2.33     0.66     0.39     0.00     0.00     0.00
    CPU oracle, same graph           3.98     2.07     3.63     2.95     0.66     0.39     0.00     0.00     0.00
  tail_mixed                         3.45     2.07     3.85     2.33     0.66     0.74     0.00     0.00     0.00
    CPU oracle, same graph           3.98     2.07     3.63     2.95     0.66     0.74     0.00     0.00     0.00
  tail_mixed_t8                      4.17     2.21     3.38     2.37     0.65     0.31     0.00     0.00     0.00
    CPU oracle, same graph           4.17     2.36     3.56     2.92     0.65     0.31     0.00     0.00     0.00
  tail_two_steps                     2.84     2.12     2.74     1.98     0.62     0.69     0.00     0.04     0.03
    CPU oracle, same graph           4.03     2.12     4.12     2.56     0.62     0.69     0.00     0.05     0.03
  tail_wide                          3.38     2.00     2.77     2.66     0.53     0.56     0.00     0.01     0.01
    CPU oracle, same graph           4.70     2.51     2.98     2.88     0.53     0.56     0.00     0.01     0.01
  tail_far                           3.11     1.77     3.05     2.02     0.87     0.31     0.00     0.00     0.00
    CPU oracle, same graph           3.11     2.80     3.12     2.39     0.87     0.35     0.00     0.00     0.00
  tail_robust                        1.90     0.62     3.70     1.74     0.41     0.00     0.00     0.04     0.05
    CPU oracle, same graph           1.75     0.62     3.70     1.74     0.41     0.00     0.00     0.03     0.05
  tail_wg                            4.60     1.81     3.53     2.92     0.51     0.38     0.00     0.00     0.02
    CPU oracle, same graph           6.18     5.59     3.20     3.27     0.51     0.60     0.00     0.00     0.02
  tail_mixed iteration               3.45     2.07     3.85     2.33     0.66     0.74        -        -        -
  tail_mixed after update            3.08     1.50     3.70     2.16     0.69     0.51     0.00     0.00     0.00
  tail_mixed_t8 iteration            4.17     2.21     3.38     2.37     0.65     0.31        -        -        -
  tail_mixed_t8 after update         2.56     1.58     3.01     2.12     0.53     0.38     0.00     0.00     0.00
  tail_wg iteration                  4.60     1.81     3.53     2.92     0.51     0.38        -        -        -
  tail_wg after update               3.03     1.28     3.20     3.06     0.61     0.20     0.00     0.00     0.02
  tail_mixed, 1 + 1 tail edges off     3.45     2.07     3.85     2.33     0.66     0.74     0.00     0.00     0.00
(C(n) is at least 70, with the robust kernels 144.  No entry of any case exceeded its bound.  chi2 and the per-edge s sit far below 1 because
S of a quadratic form is e~^T |W| e~.  A tail edge's term off by 1e-9 broke the bound in every array the tail writes or adds to — a tail
edge's own block, a tail pose, a tail cone, the old poses and the old cone with tail shares — in every case: 175 u S at the least (tail_two_steps,
H_pp of the last old pose, C = 84), 8.7e6 u S at the most; the run log has every figure, "-" where the reference says 1e-9 of a b term cannot show.)
"""
import numpy as np
import pytest

import edge_mask_ref as em
import hmul_ref as hr
import lin_exact_ref as lx
import tail_shapes as ts
from conftest import append_tail
from tail_exact_ref import check_can_fail_in_the_tail, exact, show

pytestmark = pytest.mark.gpu


def grown(pkg, frontend, name, graph=None):
    """a handle that holds the case's base, has planned it, and has absorbed the tail step by step; (handle, full graph, kernels).
    graph: (base, tail) with other information matrices (the same structure)"""
    base, tail, full, kernels = ts.graph(name, pkg, frontend)
    if graph is not None:
        base, tail = graph
    G = pkg.Graph(device=0, **ts.handle_kw(name)); G.load_bench_graph(base); G.initialize_optimization()
    assert G.plan_growths() == 0
    for k, step in enumerate(ts.CASES[name]["steps"]):
        append_tail(G, tail, step); G.initialize_optimization()
        assert G.plan_growths() == k + 1 and G.growth_refusal() == "", (name, k, G.growth_refusal())
    assert G.n_poses == len(full["pose_est"]) and G.n_landmarks == len(full["lm_est"]) and G.n_pp == len(full["pp_i"]) and G.n_pl == len(full["pl_p"])
    return G, full, kernels


def hold(G, X, name, tag, with_chi2=True, blocks=None, fitted=False):
    """the handle's last linearisation, its chi2 and its per-edge s against the reference X, both ways, the tail's own terms included"""
    blocks = G.export_system() if blocks is None else blocks
    chi2 = G.chi2() if with_chi2 else None
    s_pp = G.edge_chi2("odometry")[0] if with_chi2 else None; s_pl = G.edge_chi2("observation")[0] if with_chi2 else None
    worst = lx.check(X, blocks, chi2, s_pp, s_pl, tag=tag)
    moved = lx.check_can_fail(X, blocks, chi2, tag=tag)
    c = ts.CASES[name]
    lx.assert_two_sided(moved, far=c["far"], robust=c["robust"], tag=tag)
    tailed = check_can_fail_in_the_tail(X, blocks, name, tag, fitted=fitted)
    print("%-30s err / (u S): %s | a tail term off by 1e-9: %s" % (tag, " ".join("%s %.2f" % kv for kv in worst.items()),
          show(tailed)))
    return blocks


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in lx.ARRAYS)


@pytest.mark.parametrize("name", list(ts.CASES))
def test_grown_plan_entry_by_entry(pkg, frontend, name):
    """base, gs_initialize_optimization, the tail, gs_initialize_optimization again (the plan grew), gs_linearize: all six arrays, chi2 and
    the per-edge s; a second gs_linearize exports the same bits"""
    G, full, _ = grown(pkg, frontend, name)
    G.linearize()
    first = hold(G, exact(name), name, name)
    base = ts._built[name][0]
    F = [int(l) for l in full["fixed_landmarks"]]
    tail_fixed = np.flatnonzero((np.arange(len(full["pl_p"])) >= len(base["pl_p"])) & np.isin(full["pl_l"], F))
    assert not first["Hpl"][tail_fixed].any() and not first["Hll_diag"][F].any() and not first["b_lm"][F].any()
    if ts.CASES[name]["recipe"] == "mixed":
        assert len(tail_fixed) == 1
    G.linearize()
    assert same_bits(G.export_system(), first), "a second pass accumulated into base storage"
    G.close()


@pytest.mark.parametrize("name", list(ts.CASES))
def test_chi2_alone_on_a_fresh_grown_handle(pkg, frontend, name):
    """gs_chi2 as the first call after the growth step (launch_chi2_only with tN > 0: the gather kernel over the base, k_chi2_tail over the
    tail): the value meets the bound; behind a linearisation it changes no bit of the exported system.  There is no export directly behind
    the lone gs_chi2: that pass writes nothing of H or b, so on a handle that has not linearised since the growth step the tail arenas hold
    nothing yet (gs_multiply_hessian refuses such a handle) — what gs_chi2 must NOT do to a system is what can be held, and is"""
    G, full, _ = grown(pkg, frontend, name)
    chi2 = G.chi2(); X = exact(name)
    worst = lx.check(X, None, chi2, tag=name + " chi2 alone")
    G.linearize(); blocks = G.export_system()
    lin_chi2 = G.chi2()
    assert same_bits(G.export_system(), blocks), "gs_chi2 wrote into the system of a grown plan"
    lx.check(X, blocks, lin_chi2, tag=name + " chi2 behind a linearisation")
    print("%-30s err / (u S): chi2 %.3g, behind gs_linearize %.3g" % (name + " chi2 alone", worst["chi2"],
          float(abs(lx.mpf(lin_chi2) - X.chi2)) / (lx.U * X.chi2_S)))
    G.close()


@pytest.mark.parametrize("name", list(ts.MIXED) + ["tail_wg"])
def test_an_iteration_on_a_grown_plan_before_and_after_its_update(pkg, frontend, name):
    """gs_optimize(1): the exported system is that iteration's, at the estimates before the update; gs_linearize afterwards meets the bound at
    the new ones — the tail poses' cos / sin and the tail vertices' estimates are k_update's"""
    G, full, kernels = grown(pkg, frontend, name)
    done, st = G.optimize(1)
    assert done == 1 and st.numeric_failure == 0 and G.plan_growths() == len(ts.CASES[name]["steps"])
    hold(G, exact(name), name, name + " iteration", with_chi2=False)
    poses, lms = G.poses(), G.landmarks()
    N0 = len(ts._built[name][0]["pose_est"])
    assert np.abs(poses[N0:] - full["pose_est"][N0:]).max() > 1e-3, "the tail estimates did not move"
    G.linearize()
    hold(G, lx.linearize(full, kernels, poses, lms), name, name + " after update", fitted=True)
    G.close()


@pytest.mark.parametrize("name", ["tail_mixed_t8", "tail_wg"])
def test_a_fresh_handle_of_the_whole_graph_agrees_with_the_grown_one(pkg, frontend, name):
    """the full structure phase on the same graph: its export meets the same reference, and the two exports differ by at most twice the
    bound at every entry (exact zeros where S = 0) — what test_gpu_exact's growth test cross-checks at 1 000 poses to the parity floor"""
    G, full, _ = grown(pkg, frontend, name); G.linearize(); own = G.export_system(); G.close()
    F = pkg.Graph(device=0, **ts.handle_kw(name)); F.load_bench_graph(full); F.initialize_optimization(); F.linearize()
    other = F.export_system(); assert F.plan_growths() == 0
    F.close()
    X = exact(name); lx.check(X, other, tag=name + " fresh"); worst = 0.0
    for k in lx.ARRAYS:
        d = np.abs(own[k] - other[k]).reshape(-1); tol = 2 * X.bound(k) * lx.U * X.S[k]
        assert np.all(d <= tol), (k, int(np.argmax(d - tol)))
        worst = max(worst, float((d[tol > 0] / tol[tol > 0]).max()))
    print("%-30s grown against fresh: worst |difference| / (2 C u S) %.4f" % (name, worst))


def test_inactive_tail_edges_leave_exact_zeros_and_the_sums_without_them(pkg, frontend):
    """tail_mixed with one tail observation edge (on the old cone three tail poses see) and one tail odometry edge (to the old pose 30)
    inactive: their blocks are exactly zero, every sum is the reference's on the graph WITHOUT them (edge_mask_ref.without)"""
    name = "tail_mixed"
    base, tail, full, _ = ts.graph(name, pkg, frontend)
    Epp0, Epl0 = len(base["pp_i"]), len(base["pl_p"])
    a_pp = np.ones(len(full["pp_i"]), bool); a_pl = np.ones(len(full["pl_p"]), bool)
    k_pp = Epp0 + int(np.flatnonzero(np.minimum(full["pp_i"][Epp0:], full["pp_j"][Epp0:]) == ts.OLD_POSE)[0])
    k_pl = Epl0 + int(np.flatnonzero(full["pl_l"][Epl0:] == ts.A)[1])
    a_pp[k_pp] = False; a_pl[k_pl] = False
    assert em.isolated_vertex(full, a_pp, a_pl) is None
    G, _, _ = grown(pkg, frontend, name)
    G.set_edges_active("odometry", [k_pp]); G.set_edges_active("observation", [k_pl])
    G.linearize()
    S = G.export_system(); chi2 = G.chi2()
    assert G.plan_growths() == 1 and not S["Hpl"][k_pl].any() and not S["Hpp_off"][k_pp].any()
    X = lx.linearize(em.without(full, a_pp, a_pl))
    kept = dict(S, Hpl=S["Hpl"][a_pl], Hpp_off=S["Hpp_off"][a_pp])
    s_pp = G.edge_chi2("odometry")[0][a_pp]; s_pl = G.edge_chi2("observation")[0][a_pl]
    worst = lx.check(X, kept, chi2, s_pp, s_pl, tag="tail mask")
    moved = lx.check_can_fail(X, kept, chi2, tag="tail mask"); lx.assert_two_sided(moved, far=False, tag="tail mask")
    full_ref = exact(name)                                          # the unmasked reference must NOT fit: the two edges carry weight
    with pytest.raises(AssertionError):
        lx.check(full_ref, S, tag="tail mask against the unmasked reference")
    print("%-30s err / (u S): %s" % ("tail_mixed, 1 + 1 tail edges off", " ".join("%s %.2f" % kv for kv in worst.items())))
    G.close()


def test_the_product_is_the_exported_blocks_column_by_column(pkg, frontend):
    """tail_mixed: unit vectors on the last tail pose, a tail cone, the old pose that got a tail odometry share and the old cone that got
    three tail shares — gs_multiply_hessian equals the exported blocks' column within hmul_ref's rounding bound, no block term"""
    name = "tail_mixed"
    G, full, _ = grown(pkg, frontend, name)
    G.linearize(); B = G.export_system()
    N, M = len(full["pose_est"]), len(full["lm_est"]); worst = 0.0
    for kind, i, comps in (("pose", N - 1, 3), ("landmark", M - 1, 2), ("pose", ts.OLD_POSE, 3), ("landmark", ts.A, 2)):
        for c in range(comps):
            vp, vl = np.zeros((N, 3)), np.zeros((M, 2)); (vp if kind == "pose" else vl)[i, c] = 1.0
            yp, yl = G.multiply_hessian(vp, vl)
            assert yp.any() or yl.any()
            worst = max(worst, hr.check(yp, yl, B, full, vp, vl))
    rng = np.random.default_rng(11); vp, vl = rng.normal(size=(N, 3)), rng.normal(size=(M, 2))
    worst = max(worst, hr.check(*G.multiply_hessian(vp, vl), B, full, vp, vl))
    print("tail_mixed product against its own export: worst err / bound %.3f" % worst)
    assert worst <= 1.0
    G.close()
