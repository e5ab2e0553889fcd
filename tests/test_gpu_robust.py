"""Robust kernels (Huber, Cauchy) on the GPU against the CPU oracle.

The reference for every comparison is robust_ref.py + the unchanged oracle: a robust linearisation at estimates x is the plain
linearisation of the same graph with every information matrix scaled by its edge's weight at x (robust_ref.reweighted), and an
iteration is one oracle iteration of that graph (robust_ref.irls).  test_robust_cpu.py pins robust_ref to the oracle.

Graphs: bench 50/30, 1000/200, 10k/2k and conftest.random_graph, perturbed from their optimum; delta per kind = the median of
sqrt(s) of that kind at the perturbed estimates, so that both Huber branches hold edges (asserted: >= 10 % each).

Tolerances of the parity tests (per-edge values, H / b blocks, increments, estimates): the yardstick is the SAME comparison with no
kernel on the same graph and the same estimates (GPU against oracle), measured inside the test; the robust comparison may be 4x
that, with the bound of the corresponding test in test_gpu_parity.py as the floor (H / b blocks and per-edge values 1e-11 of the
array's largest entry, chi2 1e-10, increments 1e-8 / 1e-9 of the largest increment, estimates 1e-9).  The factor: w inherits the
relative error of s (two more roundings and a square root) and multiplies every block.

Measured on an MI355X, plain / largest robust figure over the kernel configurations (every figure: profiles/robust_gpu_suite.txt;
each test prints its own before it asserts, -s):
  graph      per-edge s        per-edge w   H blocks          b                 chi2              increment        estimates, 10 its
  50/30      1.3e-14           2.7e-14      3.2e-16 / 3.0e-14  2.4e-14 / 4.2e-14  7.9e-16 / 1.2e-15  5.2e-14 / 4.6e-13  3.9e-16 / 4.5e-16
  1000/200   8.6e-14           2.1e-13      1.4e-15 / 2.1e-13  7.8e-14 / 2.0e-13  2.6e-16 / 7.2e-16  2.2e-10 / 1.1e-9   3.0e-15 / 6.5e-15
  10k/2k     1.3e-12           3.3e-12      2.2e-14 / 3.3e-12  1.0e-12 / 3.1e-12  7.4e-15 / 7.7e-15  1.2e-6 / 3.9e-6    1.5e-13 / 3.9e-12
  random     2.0e-16           3.3e-16      3.1e-16 / 4.0e-16  1.7e-16 / 5.2e-16  0 / 2.0e-16        5.9e-15 / 2.9e-15  2.6e-15 / 1.8e-15
(s does not depend on the kernel.  The fused kernel and linearize_gather = 1 give the same figures to the digits shown.)
The robust H blocks exceed 4x the plain figure (w carries the relative error of s into every block, as the issue of this feature
expected) and stay two orders below the 1e-11 floor; the 10k / 2k increment is the one quantity above its floor, plain and robust
alike (cond(H)), and the robust one is within 4x the plain one.
Outliers: parity plain 5e-15, Huber 2.4e-15; landmark RMSE to the clean optimum plain 3.6810 m, Huber 0.8133 m (the oracle's figures).
Slam: map against the IRLS restatement 2.1e-14, against the plain Slam 0.070 m, 35 % of the edges down-weighted."""
import numpy as np
import pytest

import robust_ref as rr
from conftest import append_tail, make_oracle_graph, random_graph, split_for_growth
from test_robust_cpu import OUTLIER_DELTA, OUTLIER_SEED, lm_rmse, outlier_case, perturbed

pytestmark = pytest.mark.gpu
BLOCKS = ("Hpp_diag", "Hll_diag", "Hpp_off", "Hpl", "b_pose", "b_lm")
GRAPHS = ["bench50", "bench1000", "bench10k", "random"]


def rel(a, b):
    s = max(np.abs(b).max(), 1e-300)
    return float(np.abs(a - b).max() / s)


def fresh(pkg, g, debug=None, **kw):
    G = pkg.Graph(device=0, debug=debug, **kw)
    G.load_bench_graph(g)
    return G


def set_kernels(G, kernels):
    for kind in ("odometry", "observation"):
        G.set_robust_kernel(kind, *kernels.get(kind, rr.NONE))


_cases = {}


def case(po, bench_graphs, name):
    """the graph at estimates perturbed from its optimum (oracle, plain iterations), and the median deltas there"""
    if name not in _cases:
        if name == "random":
            g = random_graph(7); its = 10
        else:
            N, M, its = {"bench50": (50, 30, 10), "bench1000": (1000, 200, 10), "bench10k": (10000, 2000, 4)}[name]
            g = bench_graphs(N, M)[1]
        og = make_oracle_graph(po, g); og.optimize(its, ordering=1)
        g = dict(g, pose_est=og.poses(), lm_est=og.landmarks())
        P, L = perturbed(g, 5)
        g = dict(g, pose_est=P, lm_est=L)
        _cases[name] = (g, rr.median_deltas(g, P, L))
    return _cases[name]


def configurations(deltas):
    dpp, dpl = deltas
    return {"huber-observation": {"observation": ("huber", dpl)},
            "huber-odometry": {"odometry": ("huber", dpp)},
            "huber-both": {"odometry": ("huber", dpp), "observation": ("huber", dpl)},
            "cauchy-both": {"odometry": ("cauchy", dpp), "observation": ("cauchy", dpl)},
            "cauchy-odometry+huber-observation": {"odometry": ("cauchy", dpp), "observation": ("huber", dpl)}}


def assert_both_branches(g, kernels):
    s_pp, s_pl = rr.edge_s(g, g["pose_est"], g["lm_est"])
    for kind, s in (("odometry", s_pp), ("observation", s_pl)):
        k = kernels.get(kind, rr.NONE)
        if k[0] == "huber":
            w = rr.weight(k, s)
            assert (w < 1).mean() >= 0.1 and (w == 1).mean() >= 0.1, (kind, (w < 1).mean())


def linearisation_errors(po, G, g, kernels):
    """GPU against oracle at g's estimates with the kernels set on G: per-edge s and w, H / b blocks, chi2"""
    P, L = g["pose_est"], g["lm_est"]
    set_kernels(G, kernels)
    out = {}
    s_ref = dict(zip(("odometry", "observation"), rr.edge_s(g, P, L)))
    for kind in ("odometry", "observation"):
        s, w = G.edge_chi2(kind)
        out["s_" + kind] = rel(s, s_ref[kind])
        out["w_" + kind] = float(np.abs(w - rr.weight(kernels.get(kind, rr.NONE), s_ref[kind])).max())
    G.linearize(); got = G.export_system()
    ref = make_oracle_graph(po, rr.reweighted(g, P, L, kernels)).linearize_blocks()
    for k in BLOCKS:
        out[k] = rel(got[k], ref[k])
    chi = rr.robust_chi2(g, P, L, kernels)
    out["chi2"] = abs(G.chi2() - chi) / chi
    return out


def bound(plain, key):
    floor = 1e-10 if key == "chi2" else 1e-11
    if key.startswith("w_"):                                    # a weight is compared absolutely (w <= 1); its error comes from s
        return max(4 * plain["s_" + key[2:]], floor)
    return max(4 * plain[key], floor)


@pytest.mark.parametrize("gather", [0, 1])
@pytest.mark.parametrize("name", GRAPHS)
def test_edge_values_and_linearisation_match_the_reweighted_oracle(pkg, po, bench_graphs, name, gather):
    """Items 1 and 2: gs_get_edge_chi2 against robust_ref for both kinds and all kernels; gs_linearize + gs_export_system with a kernel
    set against the oracle's plain linearisation of the re-weighted graph; robust chi2 against sum rho.  Fused kernel and
    linearize_gather = 1; kernel on one kind only, on both, different kernels per kind — on ONE handle, the setting changed between
    the calls (no structure phase)."""
    g, deltas = case(po, bench_graphs, name)
    G = fresh(pkg, g, linearize_gather=gather)
    G.initialize_optimization()
    plain = linearisation_errors(po, G, g, {})
    print("\n%s gather=%d plain   %s" % (name, gather, " ".join("%s=%.2g" % kv for kv in plain.items())))
    st0 = G.stats().ms_structure
    for label, kernels in configurations(deltas).items():
        assert_both_branches(g, kernels)
        e = linearisation_errors(po, G, g, kernels)
        print("%s gather=%d %-34s %s" % (name, gather, label, " ".join("%s=%.2g" % kv for kv in e.items())))
        for k, v in e.items():
            assert v <= bound(plain, k), (label, k, v, plain.get(k))
        for kind in ("odometry", "observation"):
            assert G.robust_kernel(kind) == kernels.get(kind, rr.NONE)
    assert G.stats().ms_structure == st0                       # the setter costs no structure phase
    G.close()


@pytest.mark.parametrize("name", GRAPHS)
def test_iterations_match_the_oracle_irls(pkg, po, bench_graphs, name):
    """Item 3: the increment of one iteration against the oracle's solve of the re-weighted graph; ten iterations against
    robust_ref.irls.  Bounds: 4x the plain figures measured here (GPU optimize against oracle optimize on the same graph), floors
    1e-8 (increment, relative to the largest increment) and 1e-9 (estimates).
    Ten iterations on every graph, the 10k / 2k one included: an IRLS converges linearly, and while its steps are still large the
    estimates carry what one solve's error leaves — on the 10k / 2k graph a relative increment error of 1e-6 (GPU against oracle
    1.2e-6 plain, 2.7e-6 Huber; the oracle against itself with its other elimination order 1.0e-6 / 1.1e-6) times |dx| / |x|.
    After THREE iterations that is 1.9e-9 for Huber (max |dx| still 0.68 m) on the GPU and 2.1e-9 between the oracle's two orders,
    against 1.9e-12 plain (converged, max |dx| 5 mm); after ten the oracle's own spread is 1e-12 for every configuration."""
    g, deltas = case(po, bench_graphs, name)
    its = 10
    ordering = 0 if name == "random" else 1

    def run(kernels):
        G = fresh(pkg, g); set_kernels(G, kernels)
        done, st = G.optimize(1); assert done == 1 and st.numeric_failure == 0
        dp, dl = G.export_delta()
        P1, L1, chi1, (dp_o, dl_o) = rr.irls(po, g, kernels, 1, make_oracle_graph, ordering=ordering)
        scale = max(np.abs(dp_o).max(), np.abs(dl_o).max())
        e = {"delta": max(np.abs(dp - dp_o).max(), np.abs(dl - dl_o).max()) / scale,
             "chi2_initial": abs(st.chi2_initial - chi1[0]) / chi1[0]}
        G.close()
        G = fresh(pkg, g); set_kernels(G, kernels)
        done, st = G.optimize(its); assert done == its
        P, L, chi, _ = rr.irls(po, g, kernels, its, make_oracle_graph, ordering=ordering)
        e["estimates"] = max(rel(G.poses(), P), rel(G.landmarks(), L))
        e["chi2_final"] = abs(st.chi2_final - rr.robust_chi2(g, P, L, kernels)) / rr.robust_chi2(g, P, L, kernels)
        G.close()
        return e

    plain = run({})
    print("\n%s plain   %s" % (name, " ".join("%s=%.2g" % kv for kv in plain.items())))
    floors = {"delta": 1e-8, "estimates": 1e-9, "chi2_initial": 1e-9, "chi2_final": 1e-6}
    cfgs = configurations(deltas)
    for label in ("huber-observation", "huber-both", "cauchy-odometry+huber-observation"):
        e = run(cfgs[label])
        print("%s %-34s %s" % (name, label, " ".join("%s=%.2g" % kv for kv in e.items())))
        for k, v in e.items():
            assert v <= max(4 * plain[k], floors[k]), (label, k, v, plain[k])


@pytest.mark.parametrize("name", ["bench50", "bench1000"])
def test_optimize_until_stops_where_the_oracle_irls_stops(pkg, po, bench_graphs, name):
    """Item 3: the stop rule compares sum rho of consecutive linearisation points — it fires in the iteration the oracle IRLS's
    sequence says."""
    g, deltas = case(po, bench_graphs, name)
    kernels = configurations(deltas)["huber-both"]
    tol, cap = 1e-3, 12
    P, L, chi, _ = rr.irls(po, g, kernels, cap, make_oracle_graph)
    want = rr.stop_iteration(chi, tol, cap)
    assert 2 <= want < cap, chi
    # the decision must not hang on rounding: the neighbouring ratios are not within 1 % of the tolerance
    ratios = np.abs(np.diff(chi)) / chi[1:]
    assert np.all(np.abs(ratios[:want] / tol - 1) > 0.01), ratios
    G = fresh(pkg, g); set_kernels(G, kernels)
    done, st = G.optimize_until(cap, tol)
    assert done == want and st.numeric_failure == 0, (done, want)
    Pw, Lw, _, _ = rr.irls(po, g, kernels, want, make_oracle_graph)
    assert max(rel(G.poses(), Pw), rel(G.landmarks(), Lw)) < 1e-9
    G.close()


@pytest.mark.parametrize("name", ["bench1000", "random"])
def test_none_is_the_parent_bit_for_bit(pkg, po, bench_graphs, name):
    """Item 4: GS_ROBUST_NONE on both kinds — explicitly set, and after setting Huber and going back — gives estimates after
    optimize(10) bit-identical to a handle that never called the setter; Huber with delta = 1e150 (w is exactly 1.0, but the ROBUST
    kernel instances run) gives the same H, b and chi2 bit for bit as none: a robust instance that reorders a sum fails here."""
    g, deltas = case(po, bench_graphs, name)
    A = fresh(pkg, g); A.optimize(10)
    B = fresh(pkg, g); set_kernels(B, {}); B.optimize(10)
    Cc = fresh(pkg, g); set_kernels(Cc, configurations(deltas)["huber-both"]); Cc.linearize(); set_kernels(Cc, {}); Cc.optimize(10)
    for X in (B, Cc):
        assert np.array_equal(A.poses(), X.poses()) and np.array_equal(A.landmarks(), X.landmarks())
    big = {"odometry": ("huber", 1e150), "observation": ("huber", 1e150)}
    for gather in (0, 1):
        N_ = fresh(pkg, g, linearize_gather=gather); N_.linearize(); ref = N_.export_system(); chi = N_.chi2()
        H = fresh(pkg, g, linearize_gather=gather); set_kernels(H, big); H.linearize(); got = H.export_system()
        for k in BLOCKS:
            assert np.array_equal(got[k], ref[k]), (gather, k)
        assert H.chi2() == chi
        s, w = H.edge_chi2("observation"); assert np.all(w == 1.0)
        H.optimize(10); N_.optimize(10)
        assert np.array_equal(H.poses(), N_.poses()) and np.array_equal(H.landmarks(), N_.landmarks())
        N_.close(); H.close()
    for X in (A, B, Cc):
        X.close()


def test_growth_with_a_kernel_equals_a_fresh_handle(pkg, po, bench_graphs):
    """Item 5: a handle grown with append_tail and a kernel set against a fresh handle on the full graph; gs_get_edge_chi2 covers
    the tail's edges (k_linearize_tail and the tail branch of k_edge_chi2)."""
    _, g0 = bench_graphs(1000, 200)
    base, tail, full = split_for_growth(g0, 4, keep=600)
    d = 0.05
    kernels = {"odometry": ("cauchy", 0.5), "observation": ("huber", d)}
    G = fresh(pkg, base); set_kernels(G, kernels); G.optimize(2)
    for k in range(4):
        append_tail(G, tail, (k, k + 1))
        G.initialize_optimization(); assert G.plan_growths() == k + 1, G.growth_refusal()
    assert G.robust_kernel("observation") == ("huber", d)
    P, L = G.poses(), G.landmarks()
    at = dict(full, pose_est=P, lm_est=L)
    F = fresh(pkg, at); set_kernels(F, kernels)
    s_ref = dict(zip(("odometry", "observation"), rr.edge_s(full, P, L)))
    for kind in ("odometry", "observation"):
        s, w = G.edge_chi2(kind); sf, wf = F.edge_chi2(kind)
        assert len(s) == len(s_ref[kind]) and rel(s, s_ref[kind]) < 1e-11 and np.abs(w - rr.weight(kernels[kind], s_ref[kind])).max() < 1e-11
        assert rel(s, sf) < 1e-12 and np.abs(w - wf).max() < 1e-12
    n_tail = len(tail["pl_p"])
    s, w = G.edge_chi2("observation"); assert n_tail > 0 and (w[-n_tail:] < 1).any()      # the kernel acts on tail edges
    chi = rr.robust_chi2(full, P, L, kernels)
    assert abs(G.chi2() - chi) <= 1e-10 * chi and abs(F.chi2() - chi) <= 1e-10 * chi
    G.optimize(3); F.optimize(3)
    Pi, Li, _, _ = rr.irls(po, at, kernels, 3, make_oracle_graph)
    assert G.plan_growths() == 4
    assert max(rel(G.poses(), F.poses()), rel(G.landmarks(), F.landmarks())) < 1e-9
    assert max(rel(G.poses(), Pi), rel(G.landmarks(), Li)) < 1e-9
    G.close(); F.close()


@pytest.mark.parametrize("variant", [3, 4])
def test_launch_modes_are_bit_identical_with_a_kernel(pkg, po, bench_graphs, variant):
    """Item 6: whole-tree and per-level launches of factor variants 3 and 4 give bit-identical estimates with a kernel set."""
    g, deltas = case(po, bench_graphs, "bench1000")
    kernels = configurations(deltas)["huber-both"]
    A = fresh(pkg, g, factor_variant=variant); B = fresh(pkg, g, debug=dict(tree=0), factor_variant=variant)
    for X in (A, B):
        set_kernels(X, kernels); done, st = X.optimize(6); assert done == 6 and st.factor_variant == variant
    assert np.array_equal(A.poses(), B.poses()) and np.array_equal(A.landmarks(), B.landmarks())
    P, L, _, _ = rr.irls(po, g, kernels, 6, make_oracle_graph)
    assert max(rel(A.poses(), P), rel(A.landmarks(), L)) < 1e-8
    A.close(); B.close()


def test_marginals_invert_the_weighted_system(pkg, po, bench_graphs):
    """Item 7: gs_compute_marginals with Huber against the marginals of a second handle that holds the re-weighted graph and no
    kernel (tolerance of test_gpu_marginals.py: 1e-8 of a block's largest entry); a gs_set_robust_kernel makes the getters stale."""
    from test_gpu_marginals import REL, blocks_of, rel_err
    g, deltas = case(po, bench_graphs, "bench1000")
    kernels = configurations(deltas)["huber-both"]
    G = fresh(pkg, g); set_kernels(G, kernels); G.compute_marginals()
    W = fresh(pkg, rr.reweighted(g, g["pose_est"], g["lm_est"], kernels)); W.compute_marginals()
    U = fresh(pkg, g); U.compute_marginals()
    differs = False
    for a, b, c in zip(blocks_of(G), blocks_of(W), blocks_of(U)):
        assert rel_err(a, b) < REL
        differs = differs or rel_err(c, b) > 1e-3
    assert differs                                                      # the weights matter on this graph
    G.set_robust_kernel("observation", "huber", 2 * deltas[1])
    for getter in (G.pose_covariances, G.landmark_covariances, G.odometry_edge_covariances, G.observation_edge_covariances):
        with pytest.raises(pkg.binding.GsError) as e:
            getter()
        assert e.value.code == -6
    G.compute_marginals(); G.pose_covariances()
    for X in (G, W, U):
        X.close()


def test_outliers_end_to_end(pkg, po, bench_graphs):
    """Item 8: bench 1000/200 at its clean optimum x*, a seeded 5 % of the observation edges re-targeted to one of the five nearest
    cones at least 3 m from the right one, estimates starting at x*.  (a) parity of the GPU's plain optimize(10) with the oracle's and
    of the GPU's Huber-on-observations optimize(10), delta = 0.1, with robust_ref.irls; (b) GPU Huber landmark RMSE to x* at most half
    the GPU plain RMSE.  Condition for (b), with the oracle alone: test_robust_cpu.py (oracle: plain 3.681 m, Huber 0.813 m)."""
    xP, xL, go, pick = outlier_case(po, bench_graphs, OUTLIER_SEED)
    kernels = {"observation": ("huber", OUTLIER_DELTA)}
    A = fresh(pkg, go); done, _ = A.optimize(10); assert done == 10
    og = make_oracle_graph(po, go); og.optimize(10, ordering=1)
    e_plain = max(rel(A.poses(), og.poses()), rel(A.landmarks(), og.landmarks()))
    B = fresh(pkg, go); set_kernels(B, kernels); done, _ = B.optimize(10); assert done == 10
    P, L, _, _ = rr.irls(po, go, kernels, 10, make_oracle_graph)
    e_huber = max(rel(B.poses(), P), rel(B.landmarks(), L))
    plain, huber = lm_rmse(A.landmarks(), xL), lm_rmse(B.landmarks(), xL)
    print("\noutliers: parity plain %.2g huber %.2g; landmark RMSE to x*: plain %.4f m, Huber %.4f m" % (e_plain, e_huber, plain, huber))
    assert e_plain < 1e-9 and e_huber <= max(4 * e_plain, 1e-9)
    assert huber <= 0.5 * plain
    s, w = B.edge_chi2("observation")
    assert np.median(w[pick]) < 0.5 and np.median(np.delete(w, pick)) == 1.0       # the re-targeted edges are the down-weighted ones
    A.close(); B.close()


def test_slam_mirror_with_a_kernel_in_its_config(pkg, po):
    """Item 9: a Slam created with observation_robust_kernel = huber reports it on gs_slam_graph, runs a lap to loop closure, and
    its map equals the map of the restated reference (tests/ref_slam.py) whose optimizeGraph is robust_ref.irls on the graph the
    restatement has built by then; the kernel acts (the map differs from a plain Slam's)."""
    from ref_slam import RefSlam
    delta = 0.02
    kernels = {"observation": ("huber", delta)}

    class Rec:
        """the oracle graph of RefSlam, recording what is added to it"""
        def __init__(self, og):
            self.og = og; self.pp = []; self.pl = []

        def add_odometry_edges(self, i, j, z, info):
            self.pp.append((int(i[0]), int(j[0]), np.array(z[0], dtype=np.float64), np.array(info[0], dtype=np.float64))); self.og.add_odometry_edges(i, j, z, info)

        def add_observation_edges(self, p, l, z, info):
            self.pl.append((int(p[0]), int(l[0]), np.array(z[0], dtype=np.float64), np.array(info[0], dtype=np.float64))); self.og.add_observation_edges(p, l, z, info)

        def __getattr__(self, k):
            return getattr(self.og, k)

        def as_dict(self):
            return dict(pose_est=self.og.poses(), lm_est=self.og.landmarks(),
                        pp_i=np.array([e[0] for e in self.pp], np.int32), pp_j=np.array([e[1] for e in self.pp], np.int32),
                        pp_z=np.array([e[2] for e in self.pp]), pp_info=np.array([e[3] for e in self.pp]).reshape(-1, 9),
                        pl_p=np.array([e[0] for e in self.pl], np.int32), pl_l=np.array([e[1] for e in self.pl], np.int32),
                        pl_z=np.array([e[2] for e in self.pl]), pl_info=np.array([e[3] for e in self.pl]).reshape(-1, 4),
                        fixed_poses=np.array([0, 1], np.int32), fixed_landmarks=np.array([0, 1], np.int32))

    class RobustRefSlam(RefSlam):
        def __init__(self, **kw):
            super().__init__(**kw); self.g = Rec(self.g); self.acted = None

        def _optimise(self):                                            # optimizeGraph + updateMap with the IRLS in place of optimize()
            self.g.set_fixed_pose(0); self.g.set_fixed_pose(1); self.g.set_fixed_landmark(0); self.g.set_fixed_landmark(1)
            gd = self.g.as_dict()
            self.acted = float((rr.weight(kernels["observation"], rr.edge_s(gd, gd["pose_est"], gd["lm_est"])[1]) < 1).mean())
            P, L, _, _ = rr.irls(po, gd, kernels, self.iterations, make_oracle_graph)
            self.g.set_poses(P); self.g.set_landmarks(L)
            self.optimise_calls += 1
            for c in self.map:
                c[0], c[1] = L[c[3]]

    N, M = 120, 60
    t = pkg.track.generate(N, M)
    S = pkg.Slam(same_cone_threshold=1.2, cone_mapping_threshold=67.0, observation_robust_kernel="huber", observation_robust_delta=delta)
    assert S.graph.robust_kernel("observation") == ("huber", delta) and S.graph.robust_kernel("odometry") == ("none", 1.0)
    U = pkg.Slam(same_cone_threshold=1.2, cone_mapping_threshold=67.0)
    R = RobustRefSlam(same_cone_threshold=1.2, cone_mapping_threshold=67.0)
    for k in range(N):
        S.perform_slam(t["odom_poses"][k], t["obs"][k]); U.perform_slam(t["odom_poses"][k], t["obs"][k]); R.perform(t["odom_poses"][k], t["obs"][k])
        assert S.map_size == len(R.map) and S.loop_closed == R.loop_closing_complete, k
        assert S.graph.n_pl == R.g.n_pl and S.graph.n_pp == R.g.n_pp, k
        if S.loop_closed:
            break
    assert S.loop_closed and U.loop_closed and R.optimise_calls == 1
    assert 0.02 < R.acted < 0.98, R.acted                              # the kernel acts on part of the edges at the point of the optimisation
    xy, ty = S.map(); uxy, _ = U.map()
    Rm = np.array([[c[0], c[1]] for c in R.map])
    print("\nslam: map against the IRLS restatement %.3g, against the plain Slam %.3g, share of down-weighted edges %.2f"
          % (np.abs(xy - Rm).max(), np.abs(xy - uxy).max(), R.acted))
    assert np.abs(xy - Rm).max() < 1e-7                                 # the bound of the existing Slam parity test
    assert np.abs(S.graph.poses() - R.g.poses()).max() < 1e-7
    assert np.abs(xy - uxy).max() > 1e-4
    S.close(); U.close()
