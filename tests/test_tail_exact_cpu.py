"""The grown-plan cases, their reference and their bound, checked without a GPU.

  census      every case of tests/tail_shapes.py is grown on the host as test_plan_host.py grows its graphs: the plan must absorb every step
              (plan_growths() counts them, the refusal text stays empty) and each property the case is named for is counted from the graph and
              from plan_export(); a case that cannot reach one fails here instead of silently testing less;
  soundness   the unchanged CPU oracle (orc_linearize_blocks on the FULL graph; the robust case on robust_ref's re-weighted graph) stays
              inside C(n) u S of tests/lin_exact_ref.py on every entry, and a reference with one TAIL term off by 1e-9 does not, in every array the
              tail writes or adds to (tests/tail_exact_ref.py) — the reference and the bound are usable on these graphs before a GPU sees them.

tail_wide, what the planner admitted: the base (lin_shapes.make, 70 poses, 196 landmarks, every pose four observations) has a root of 41
scalars.  fits() in gs_plan.cpp lets the root grow to max(63, root_f0 + 24) = 65 scalars, i.e. by 8 poses without a tail cone (9 poses, or 7
poses and two cones: "a front would exceed 159 scalars" — the text of the root's limit in a plan that holds workgroup fronts).  Reached:
8 tail poses, 262 tail observation edges (the edge loop e += 256 runs a second round), 195 touched cones (the landmark loop j += 192 runs a
second round), no tail cone (tail_mixed has them).  16 poses are 48 scalars and need a root of at most 15: no base tried has one (the
lin_shapes bases: 41 .. 201, the K = 16 track cut to 60 .. 250 poses: the root is its largest front, 60 .. 80).

The oracle's worst err / (u S) per case and array (the bound's C(n) is at least 70, 144 robust; profiles/tail_exact_cpu_census.txt is this
module's output):
  case               Hpp_diag Hll_diag  Hpp_off      Hpl   b_pose     b_lm     chi2     s_pp     s_pl
  tail_min               3.98     2.07     3.63     2.95     0.66     0.39     0.00     0.00     0.00
  tail_mixed             3.98     2.07     3.63     2.95     0.66     0.74     0.00     0.00     0.00
  tail_mixed_t8          4.17     2.36     3.56     2.92     0.65     0.31     0.00     0.00     0.00
  tail_two_steps         4.03     2.12     4.12     2.56     0.62     0.69     0.00     0.05     0.03
  tail_wide              4.70     2.51     2.98     2.88     0.53     0.56     0.00     0.01     0.01
  tail_far               3.11     2.80     3.12     2.39     0.87     0.35     0.00     0.00     0.00
  tail_robust            1.75     0.62     3.70     1.74     0.41     0.00     0.00     0.03     0.05
  tail_wg                6.18     5.59     3.20     3.27     0.51     0.60     0.00     0.00     0.02
"""
import numpy as np
import pytest

from conftest import append_tail, make_oracle_graph
import lin_exact_ref as lx
import robust_ref as rr
import tail_shapes as ts
from plan_exec import Plan
from tail_exact_ref import check_can_fail_in_the_tail, exact, show

def grown_host_plan(pkg, name):
    base, tail, full, _ = ts._built[name]
    G = pkg.Graph(device=-2, **ts.handle_kw(name)); G.load_bench_graph(base)
    i0 = G.plan_build_host(); P0 = Plan(G.plan_export())
    assert G.plan_growths() == 0
    for k, step in enumerate(ts.CASES[name]["steps"]):
        append_tail(G, tail, step); info = G.plan_build_host()
        assert G.plan_growths() == k + 1 and G.growth_refusal() == "", (name, k, G.growth_refusal())
    P = Plan(G.plan_export()); P.check_invariants(); G.close()
    return P0, P, i0, info


@pytest.mark.parametrize("name", list(ts.CASES))
def test_census(pkg, frontend, name):
    c = ts.CASES[name]; base, tail, full, kernels = ts.graph(name, pkg, frontend)
    N0, M0, Epp0, Epl0 = len(base["pose_est"]), len(base["lm_est"]), len(base["pp_i"]), len(base["pl_p"])
    N, M, Epp, Epl = len(full["pose_est"]), len(full["lm_est"]), len(full["pp_i"]), len(full["pl_p"])
    P0, P, i0, info = grown_host_plan(pkg, name)
    # the plan: same fronts and tree, the tail's vertices behind every older scalar, the tail's edges behind the base layout in insertion order
    assert P.n_fronts == P0.n_fronts and np.array_equal(P.parent, P0.parent)
    assert (P.n_poses, P.n_lms, P.n_pp, P.n_pl) == (N, M, Epp, Epl) and (P0.n_poses, P0.n_lms, P0.n_pp, P0.n_pl) == (N0, M0, Epp0, Epl0)
    assert np.array_equal(P.pose_gidx[:N0], P0.pose_gidx) and np.array_equal(P.lm_gidx[:M0], P0.lm_gidx)
    old_max = max(P0.pose_gidx.max(), P0.lm_gidx.max())
    assert (P.pose_gidx[N0:] > old_max).all() and (P.lm_gidx[M0:] > old_max).all()
    assert np.array_equal(P.ell_ins[P0.ell_len:P0.ell_len + (Epl - Epl0)], np.arange(Epl0, Epl)), "tail observation edges sit behind the layout, in order"
    assert np.array_equal(P.pp_order, np.arange(Epp)) and np.array_equal(P.ell_ins[:P0.ell_len], P0.ell_ins)
    if c["T"]:
        assert P.ell_T == c["T"]
    # the graph: what growth needs
    tpp = np.arange(Epp0, Epp); tpl = np.arange(Epl0, Epl)
    pl_p, pl_l, pp_i, pp_j = full["pl_p"], full["pl_l"], full["pp_i"], full["pp_j"]
    lf = np.zeros(M, dtype=bool); lf[np.asarray(full["fixed_landmarks"], dtype=np.int64)] = True
    pf = np.zeros(N, dtype=bool); pf[np.asarray(full["fixed_poses"], dtype=np.int64)] = True
    assert (pl_p[tpl] >= N0).all() and (np.maximum(pp_i[tpp], pp_j[tpp]) >= N0).all() and (pl_p[:Epl0] < N0).all()
    assert not pf[N0:].any() and not lf[M0:].any()
    assert np.isin(pl_l[tpl][pl_l[tpl] < M0], pl_l[:Epl0]).all(), "every old cone the tail touches has a partial-sum slot"
    seen_by = lambda l: np.unique(pl_p[tpl][pl_l[tpl] == l])
    touched = np.unique(pl_l[tpl][~lf[pl_l[tpl]]])
    nT = N - N0
    if name == "tail_min":
        assert (nT, len(tpp), len(tpl), M - M0) == (1, 1, 1, 0) and pl_l[tpl[0]] < M0 and not lf[pl_l[tpl[0]]]
    if c["recipe"] == "mixed":
        assert nT == 6 and M - M0 == 2
        assert any(len(seen_by(l)) == 2 for l in range(M0, M)), "a tail cone seen by two tail poses"
        three = [l for l in touched if l < M0 and len(seen_by(l)) >= 3]
        assert three and all(np.all(np.diff(np.flatnonzero(pl_l[tpl] == l)) > 0) for l in three), "an old cone seen by three tail poses"
        F = int(full["fixed_landmarks"][0])
        assert F < M0 and ((pl_l[tpl] == F) & (pl_p[tpl] >= N0)).sum() == 1, "the old fixed landmark seen from a tail pose"
        assert len(np.setdiff1d(np.arange(N0, N), pl_p[tpl])) >= 1, "a tail pose with no observation"
        other = np.minimum(pp_i[tpp], pp_j[tpp])
        far_old = (other < N0 - 1) & ~pf[other]
        assert far_old.any() and (np.bincount(np.concatenate([pp_i[tpp], pp_j[tpp]]), minlength=N)[N0:] >= 2).any(), "a second odometry edge to an old pose that is not adjacent"
        assert ((pp_i[tpp] == 0) & pf[0] & (pp_j[tpp] >= N0)).any(), "a tail odometry edge whose older end is the fixed pose 0"
        assert (pp_i[tpp] > pp_j[tpp]).any(), "a tail pose at the i end"
    if name == "tail_two_steps":
        (a0, b0), (a1, b1) = c["steps"]
        in1 = pl_l[tpl][(pl_p[tpl] >= N0 + a0) & (pl_p[tpl] < N0 + b0)]; in2 = pl_l[tpl][(pl_p[tpl] >= N0 + a1) & (pl_p[tpl] < N0 + b1)]
        both = np.intersect1d(in1, in2); both = both[(both < M0) & ~lf[both]]
        assert len(both) >= 1 and len(c["steps"]) == 2, "an old cone observed in both steps"
    if name == "tail_wide":
        assert nT >= 8 and len(tpl) > 64
        assert len(tpl) > 256 and len(touched) > 192 and len(touched) > 64, (len(tpl), len(touched))
        # one pose more is refused by the root's limit: what the module docstring records
        g9 = ts.grow(base, ts.wide_recipe(nT + 1, ts.WIDE_PER_POSE, 0), c["seed"])
        G = pkg.Graph(device=-2, **ts.handle_kw(name)); G.load_bench_graph(g9[0]); G.plan_build_host(); append_tail(G, g9[1]); G.plan_build_host()
        assert G.plan_growths() == 0 and G.growth_refusal() == "a front would exceed 159 scalars"
        G.close()
        f0 = (P0.npiv + P0.nbnd)[-1]
        assert max(63, f0 + 24) - f0 == 3 * nT, "the root holds exactly the poses it may"
    if c["far"]:
        assert np.abs(full["pose_est"][N0:, :2]).min() > 2.9e4 and np.abs(full["lm_est"][M0:]).min() > 2.9e4
    if c["robust"]:
        s_pp, s_pl = rr.edge_s(full, full["pose_est"], full["lm_est"])
        d2 = kernels["odometry"][1] ** 2
        assert kernels["odometry"][0] == "huber" and kernels["observation"][0] == "cauchy"
        assert (s_pp[tpp] > d2).any() and (s_pp[tpp] < d2).any() and (s_pp[:Epp0] > d2).any(), "Huber's outer branch on a tail odometry edge"
        assert s_pl[tpl].max() > 20 * np.median(s_pl) and s_pp[tpp].max() > 20 * np.median(s_pp), "an outlier on a tail edge of each kind"
    if c["wg"]:
        f0, f1 = P0.npiv + P0.nbnd, (P.npiv + P.nbnd)[:P0.n_fronts]
        assert i0.max_front > 63 and ((f0 <= 63) & (f1 >= 64)).any(), "no front crossed from a wave to a workgroup"
        assert nT == 3 and len(c["steps"]) == 3
    print("%-16s tail: %d poses %d cones %d odometry %d observation edges, %d touched cones; fronts %d, largest %d -> %d, root %d -> %d" % (
        name, nT, M - M0, len(tpp), len(tpl), len(touched), P.n_fronts, i0.max_front, info.max_front, (P0.npiv + P0.nbnd)[-1], (P.npiv + P.nbnd)[-1]))


@pytest.mark.parametrize("name", list(ts.CASES))
def test_the_oracle_stays_inside_the_bound_and_a_perturbed_tail_term_does_not(pkg, frontend, po, name):
    base, tail, full, kernels = ts.graph(name, pkg, frontend); X = exact(name)
    gw = rr.reweighted(full, full["pose_est"], full["lm_est"], kernels) if kernels else full
    og = make_oracle_graph(po, gw)
    blocks = og.linearize_blocks()
    chi2 = rr.robust_chi2(full, full["pose_est"], full["lm_est"], kernels) if kernels else og.chi2()
    s_pp, s_pl = rr.edge_s(full, full["pose_est"], full["lm_est"])
    worst = lx.check(X, blocks, chi2, s_pp, s_pl, tag=name)
    moved = lx.check_can_fail(X, blocks, chi2, tag=name)
    lx.assert_two_sided(moved, far=ts.CASES[name]["far"], robust=bool(kernels), tag=name)
    tailed = check_can_fail_in_the_tail(X, blocks, name, name)
    print("%-16s oracle err / (u S): %s | tail term off by 1e-9: %s" % (name, " ".join("%s %.2f" % kv for kv in worst.items()),
          show(tailed)))


@pytest.mark.parametrize("name", ["tail_mixed", "tail_far", "tail_wg"])
def test_the_float64_magnitudes_are_the_references(pkg, frontend, name):
    """lin_exact_ref.magnitudes (numpy, for graphs beyond mpmath's reach: test_gpu_exact's growth test at 1 000 poses) gives the S of the mpmath
    reference to 1e-14 relative and the same n, zeros where it has zeros"""
    _, _, full, _ = ts.graph(name, pkg, frontend)
    X = lx.linearize(full, None) if ts.CASES[name]["robust"] else exact(name)
    S, n = lx.magnitudes(full)
    for k in lx.ARRAYS:
        assert np.array_equal(n[k], X.n[k]) and np.array_equal(S[k] == 0, X.S[k] == 0), k
        assert np.all(np.abs(S[k] - X.S[k]) <= 1e-14 * X.S[k]), k
