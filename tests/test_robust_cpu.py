"""Robust kernels without a GPU: the numpy checker (robust_ref.py) against the CPU oracle, the kernels' formulas, the C-ABI's
setter / getter / refusals on a host-only handle, and the condition of the GPU outlier test (oracle alone)."""
import ctypes as C

import numpy as np
import pytest

import robust_ref as rr
from conftest import make_oracle_graph, random_graph

OUTLIER_SEED = 1           # seed of the outlier graph (shared with test_gpu_robust.py); fixed here, on the CPU, see the condition below
OUTLIER_DELTA = 0.1


def perturbed(g, seed, sp=0.05, sl=0.1):
    rng = np.random.default_rng(seed)
    P = np.array(g["pose_est"], dtype=np.float64) + rng.normal(0, sp, np.shape(g["pose_est"])) * [1, 1, 0.2]
    L = np.array(g["lm_est"], dtype=np.float64) + rng.normal(0, sl, np.shape(g["lm_est"]))
    return P, L


@pytest.mark.parametrize("which", ["bench50", "bench1000", "random"])
def test_checker_edge_values_sum_to_the_oracle_chi2(po, bench_graphs, which):
    """Pins robust_ref's per-edge s to OracleGraph.chi2() before it is used against the GPU, at the graph's own estimates and at
    perturbed ones.  Bound: relative 1e-12.  Measured (the order of the sums differs, nothing else): at most 1.5e-15 over the three graphs, at
    their own estimates and at perturbed ones."""
    g = random_graph(7) if which == "random" else bench_graphs(*((50, 30) if which == "bench50" else (1000, 200)))[1]
    for P, L in ((g["pose_est"], g["lm_est"]), perturbed(g, 3)):
        gg = dict(g); gg["pose_est"] = np.asarray(P, dtype=np.float64); gg["lm_est"] = np.asarray(L, dtype=np.float64)
        og = make_oracle_graph(po, gg)
        s_pp, s_pl = rr.edge_s(g, P, L); a_pp, a_pl = rr.active(g)
        mine = s_pp[a_pp].sum() + s_pl[a_pl].sum(); ref = og.chi2()
        print("chi2 checker %.17g oracle %.17g rel %.3g" % (mine, ref, abs(mine - ref) / ref))
        assert abs(mine - ref) <= 1e-12 * ref
        assert abs(rr.robust_chi2(g, P, L, {}) - ref) <= 1e-12 * ref
        # the re-weighted graph with no kernel is the graph itself
        rw = rr.reweighted(g, P, L, {})
        assert np.array_equal(rw["pp_info"], np.asarray(g["pp_info"]).reshape(-1, 9)) and np.array_equal(rw["pl_info"], np.asarray(g["pl_info"]).reshape(-1, 4))


@pytest.mark.parametrize("delta", [0.05, 1.0, 7.5])
def test_huber_is_continuous_at_the_threshold(delta):
    d2 = delta * delta; k = ("huber", delta)
    lo, hi = np.nextafter(d2, 0.0), np.nextafter(d2, np.inf)
    for s in (lo, d2, hi):
        assert abs(rr.rho(k, s) - d2) <= 4 * np.finfo(float).eps * d2
        assert abs(rr.weight(k, s) - 1.0) <= 4 * np.finfo(float).eps
    assert rr.weight(k, d2) == 1.0 and rr.rho(k, d2) == d2
    assert rr.weight(("huber", 1e150), 1e6) == 1.0                     # never acts: exactly one
    assert np.all(rr.weight(("none", 1.0), np.array([0.0, 1.0, 1e9])) == 1.0)


@pytest.mark.parametrize("name", ["huber", "cauchy"])
def test_weight_is_the_derivative_of_rho(name):
    delta = 0.3; k = (name, delta)
    s = np.concatenate([np.linspace(0.001, 0.08, 40), np.linspace(0.1, 5.0, 60)])     # both sides of d2 = 0.09, not across it
    h = 1e-6 * s
    num = (rr.rho(k, s + h) - rr.rho(k, s - h)) / (2 * h)
    assert np.abs(num - rr.weight(k, s)).max() < 1e-8
    assert np.all(np.diff(rr.weight(k, s)) <= 0) and np.all(rr.weight(k, s) <= 1.0) and np.all(rr.weight(k, s) > 0)
    assert np.all(rr.rho(k, s) <= s * (1 + 1e-15))


def test_setter_getter_and_refusals_on_a_host_only_handle(pkg):
    b = pkg.binding
    cfg = b.default_config()
    assert C.sizeof(cfg) == cfg.struct_size                             # the Python mirror of gs_config is the library's
    assert (cfg.odometry_robust_kernel, cfg.odometry_robust_delta, cfg.observation_robust_kernel, cfg.observation_robust_delta) == (0, 1.0, 0, 1.0)
    G = pkg.Graph(device=-2)
    assert G.robust_kernel("odometry") == ("none", 1.0) and G.robust_kernel("observation") == ("none", 1.0)
    G.set_robust_kernel("observation", "huber", 0.1); G.set_robust_kernel("odometry", "cauchy", 2.5)
    assert G.robust_kernel("observation") == ("huber", 0.1) and G.robust_kernel("odometry") == ("cauchy", 2.5)
    G.add_poses([0, 1], [[0, 0, 0], [1, 0, 0]]); G.clear()             # the setting belongs to the handle
    assert G.robust_kernel("observation") == ("huber", 0.1) and G.robust_kernel("odometry") == ("cauchy", 2.5)
    bad = [("observation", "huber", 0.0), ("observation", "huber", -1.0), ("observation", "cauchy", float("nan")),
           ("odometry", "huber", float("inf")), (2, "huber", 1.0), (-1, "none", 1.0), ("odometry", 3, 1.0), ("odometry", -1, 1.0)]
    for kind, kernel, delta in bad:
        with pytest.raises(b.GsError) as e:
            G.set_robust_kernel(kind, kernel, delta)
        assert e.value.code == -1, (kind, kernel, delta)
    with pytest.raises(b.GsError) as e:
        G.robust_kernel(5)
    assert e.value.code == -1
    assert G.robust_kernel("observation") == ("huber", 0.1)             # a refused call changes nothing
    G.set_robust_kernel("odometry", "none", float("nan"))               # delta is not looked at for "none"
    assert G.robust_kernel("odometry") == ("none", 1.0)
    with pytest.raises(b.GsError) as e:
        G.edge_chi2("observation")
    assert e.value.code == -4                                           # GS_ERR_NO_DEVICE
    # shards: refused in both orders
    with pytest.raises(b.GsError) as e:
        G.dist_configure(0, 2)
    assert e.value.code == -1 and "robust" in str(e.value)
    G.dist_configure(0, 1)                                              # world 1 is not a shard
    G.set_robust_kernel("observation", "none")
    G.dist_configure(0, 2)
    with pytest.raises(b.GsError) as e:
        G.set_robust_kernel("odometry", "huber", 1.0)
    assert e.value.code == -1 and "shard" in str(e.value)
    G.set_robust_kernel("odometry", "none")                             # none is always accepted
    G.close()
    # gs_create applies the config fields, and refuses bad ones
    G = pkg.Graph(device=-2, observation_robust_kernel="huber", observation_robust_delta=0.05)
    assert G.robust_kernel("observation") == ("huber", 0.05) and G.robust_kernel("odometry") == ("none", 1.0)
    G.close()
    with pytest.raises(b.GsError) as e:
        pkg.Graph(device=-2, odometry_robust_kernel=1, odometry_robust_delta=0.0)
    assert e.value.code == -1
    # an older caller's smaller struct: the defaults
    cfg = b.default_config(device=-2); cfg.observation_robust_kernel = 2; cfg.struct_size = 88
    G = pkg.Graph(cfg=cfg); assert G.robust_kernel("observation") == ("none", 1.0); G.close()
    S = pkg.Slam(device=-2, observation_robust_kernel="cauchy", observation_robust_delta=0.2)
    assert S.graph.robust_kernel("observation") == ("cauchy", 0.2)
    S.close()


def outlier_case(po, bench_graphs, seed=OUTLIER_SEED):
    """(clean optimum poses, landmarks, outlier graph at the clean optimum)"""
    _, g = bench_graphs(1000, 200)
    og = make_oracle_graph(po, g); done, _, _ = og.optimize(10, ordering=1); assert done == 10
    xP, xL = og.poses(), og.landmarks()
    go, pick = rr.outlier_graph(g, xP, xL, seed)
    return xP, xL, go, pick


def lm_rmse(L, xL):
    return float(np.sqrt(((L - xL) ** 2).sum(1).mean()))


def test_outlier_graph_condition_with_the_oracle_alone(po, bench_graphs):
    """Condition of test_gpu_robust.py's outlier test, established here without a GPU: on the bench 1000/200 graph at its clean
    optimum with a seeded 5 % of the observation edges re-targeted (robust_ref.outlier_graph, seed OUTLIER_SEED), ten oracle
    iterations give a Huber (delta = 0.1, observation edges, IRLS) landmark RMSE to the clean optimum of at most 0.3 of the plain
    one.  Measured with the committed generator: seed 1: plain 3.681 m, Huber 0.813 m, ratio 0.221 (seed 0: 2.186 m, 0.520 m, 0.238)."""
    xP, xL, go, pick = outlier_case(po, bench_graphs)
    assert len(pick) == round(0.05 * len(go["pl_p"])) and np.all(np.hypot(*(xL[go["pl_l"][pick]] - xL[bench_graphs(1000, 200)[1]["pl_l"][pick]]).T) >= 3.0)
    og = make_oracle_graph(po, go); done, _, _ = og.optimize(10, ordering=1); assert done == 10
    plain = lm_rmse(og.landmarks(), xL)
    P, L, chi, _ = rr.irls(po, go, {"observation": ("huber", OUTLIER_DELTA)}, 10, make_oracle_graph)
    huber = lm_rmse(L, xL)
    print("oracle landmark RMSE to the clean optimum: plain %.4f m, Huber %.4f m, ratio %.3f" % (plain, huber, huber / plain))
    assert huber <= 0.3 * plain
